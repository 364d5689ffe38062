"""GPU: the pipeline kernel reading a device-built DIR-24-8 table
(DP_OPT_DEVICE_FIB): one small device-resident burst over tables of 65,537 v4
routes gives the same dp_pkt_out_t records and buffer as with the option off."""
import numpy as np
import pytest

from dataplane_amd import GpuPathNf, _abi as A
from dataplane_amd.workload import Workload

pytestmark = pytest.mark.gpu


def test_burst_over_device_built_fib():
    import torch
    w = Workload(2, 4096, seed=23, n_routes_v4=65537, n_acl=300, n_nat=32, tcp_percent=20)
    dev, nf, runs = torch.device("cuda", 0), GpuPathNf(0), []
    try:
        for on in (True, False):
            nf.set_device_fib(on)
            nf.publish(w.tables)
            assert nf.publish_stats()["device_fibs"] == (1 if on else 0)
            db = torch.from_numpy(w.fresh_buf()).to(dev)
            di = torch.from_numpy(w.inp.view(np.uint8)).to(dev)
            do = torch.zeros(w.n * A.PKT_OUT.itemsize, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            nf.process_device(db.data_ptr(), db.numel(), di.data_ptr(), do.data_ptr(), w.n)
            nf.synchronize()
            runs.append((do.cpu().numpy().view(A.PKT_OUT), db.cpu().numpy()))
    finally:
        nf.close()
    (out_on, buf_on), (out_off, buf_off) = runs
    assert np.count_nonzero(out_off["done"] == A.DONE["Delivered"]) > w.n // 4
    assert np.array_equal(out_on, out_off) and np.array_equal(buf_on, buf_off)
