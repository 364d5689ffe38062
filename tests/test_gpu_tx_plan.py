"""GPU: the TX plan (include/dpgpu.h "TX plan") against plain numpy over the
same records: a bucket id per record by the header's rules, a stable argsort,
counts and u64 byte sums.  `order` and every field of `ports` must be equal."""
import numpy as np
import pytest

from dataplane_amd import GpuPathNf, _abi as A
from dataplane_amd.workload import Workload

pytestmark = pytest.mark.gpu
DELIVERED, T = A.DONE["Delivered"], A.TX_PLAN_TILE
# The scan kernel's 16 waves take 16 tile rows a step, 256 tiles a pass of their loops.  70 T + 3: 71 tiles,
# shares of 5 rows, one row for wave 14 and none for wave 15.  300 T + 3: 301 tiles, shares of 19 rows -- a
# full step and one of 3 rows, the sums and bases carried between them -- and 16 rows, one exact step, for wave 15.
SIZES = [1, 63, 64, 65, 257, T - 1, T, T + 1, 2 * T + 65, 70 * T + 3, 300 * T + 3]
DISTS = ["one_port", "none_delivered", "uniform64", "no_ports", "alternating", "big_ifindex", "strays", "odd_done"]
HOST_FORM = {(2 * T + 65, "uniform64"), (65, "strays")}  # also through dp_tx_plan


@pytest.fixture(scope="module")
def nf():
    import torch
    torch.cuda.init()
    n = GpuPathNf(0)
    yield n
    n.close()


def records(n, dist, seed):
    """(A.PKT_OUT records, port list): every field random, done / oif by `dist`."""
    rng = np.random.default_rng(seed)
    out = np.frombuffer(rng.bytes(n * A.PKT_OUT.itemsize), dtype=A.PKT_OUT).copy()  # (len: 0..65535)
    done, pick = DELIVERED, lambda vals: rng.choice(np.array(vals, dtype=np.uint32), n)
    if dist == "one_port":
        oifs, oif = [7, 3, 9, 1, 5], 9
    elif dist == "none_delivered":  # (with oifs of the list: done decides)
        oifs, oif, done = [7, 3, 9], pick([7, 3, 9]), pick([d for d in range(A.DONE_COUNT) if d != DELIVERED])
    elif dist == "uniform64":  # 62 ports and both special buckets, evenly
        oifs, k = list(100 + rng.permutation(62)), rng.integers(0, 64, n)
        done = np.where(k == 63, A.DONE["AclDropped"], DELIVERED)
        oif = np.where(k < 62, np.array(oifs)[np.minimum(k, 61)], np.where(k == 62, 0, oifs[0]))
    elif dist == "no_ports":
        oifs, oif, done = [], pick([0, 1, 2, 3]), pick([DELIVERED, A.DONE["AclDropped"]])
    elif dist == "alternating":
        oifs, oif, done = [42], 42, np.where(np.arange(n) % 2 == 0, DELIVERED, A.DONE["RouteDrop"])
    elif dist == "big_ifindex":  # unsorted
        oifs = [0xffffffff, 2, 0x80000000, 1, 0x7fffffff, 129]
        oif = pick(oifs)
    elif dist == "strays":  # Delivered with no oif or one outside the list: bucket n_ports
        oifs, oif = [10, 20, 30], pick([0, 10, 11, 20, 30, 31, 0xfffffffe])
    elif dist == "odd_done":  # values outside the enum: the last bucket
        oifs, oif, done = [10, 20], pick([10, 20]), pick([DELIVERED, 255, 200, A.DONE_COUNT])
    out["done"], out["oif"] = done, oif
    return out, np.array(oifs, dtype=np.uint32)


def reference(out, oifs):
    nb, delivered = len(oifs), out["done"] == DELIVERED
    bucket = np.where(delivered, nb, nb + 1)
    for b, o in enumerate(oifs):
        bucket[delivered & (out["oif"] == o)] = b
    ports, nbytes = np.zeros(nb + 2, dtype=A.TX_PORT), np.zeros(nb + 2, dtype=np.uint64)
    np.add.at(nbytes, bucket, out["len"].astype(np.uint64))
    ports["oif"][:nb], ports["count"], ports["bytes"] = oifs, np.bincount(bucket, minlength=nb + 2), nbytes
    ports["first"] = np.cumsum(ports["count"]) - ports["count"]
    return np.argsort(bucket, kind="stable").astype(np.uint32), ports


def plan_device(nf, dev_out, n, oifs, stream=None):
    """dp_tx_plan_device over n records at `dev_out`, read back: (order, ports)."""
    import torch
    dev = torch.device("cuda", 0)
    order = torch.zeros(n, dtype=torch.int32, device=dev)
    ports = torch.zeros((len(oifs) + 2) * A.TX_PORT.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    nf.tx_plan_device(dev_out, n, oifs, order.data_ptr(), ports.data_ptr(), stream)
    nf.synchronize()
    return order.cpu().numpy().view(np.uint32), ports.cpu().numpy().view(A.TX_PORT)


def same(got, ref):
    assert np.array_equal(got[1], ref[1])
    assert np.array_equal(got[0], ref[0])


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("n", SIZES)
def test_plan(nf, n, dist):
    import torch
    out, oifs = records(n, dist, seed=n)
    ref = reference(out, oifs)
    assert dist != "uniform64" or n < 64 * 8 or ref[1]["count"].min() > 0
    dev_out = torch.from_numpy(out.view(np.uint8)).to("cuda:0")
    got = plan_device(nf, dev_out.data_ptr(), n, oifs)
    same(got, ref)
    if (n, dist) in HOST_FORM:
        same(nf.tx_plan(out, oifs), got)


def test_after_a_burst_on_its_stream(nf):
    import torch
    dev = torch.device("cuda", 0)
    w = Workload(2, 3000, seed=402, n_routes_v4=3000, n_acl=300, n_nat=24, tcp_percent=25)
    nf.publish(w.tables)
    host = nf.process_arrays(w.fresh_buf(), w.inp, with_meta=False)
    seen = np.unique(host["oif"][(host["done"] == DELIVERED) & (host["oif"] != 0)])
    oifs = seen[::-1][:A.TX_MAX_PORTS][1:]  # descending, and one port's packets left without a port
    db, di = torch.from_numpy(w.fresh_buf()).to(dev), torch.from_numpy(w.inp.view(np.uint8)).to(dev)
    do = torch.zeros(w.n * A.PKT_OUT.itemsize, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    nf.process_device(db.data_ptr(), db.numel(), di.data_ptr(), do.data_ptr(), w.n, stream=stream.cuda_stream)
    got = plan_device(nf, do.data_ptr(), w.n, oifs, stream.cuda_stream)
    out = do.cpu().numpy().view(A.PKT_OUT)
    assert np.array_equal(out, host)
    ref = reference(out, oifs)
    assert len(oifs) >= 1 and ref[1]["count"][len(oifs)] > 0 and ref[1]["count"][0] > 0
    same(got, ref)


def test_einval_and_empty(nf):
    import torch
    out, oifs = records(300, "strays", seed=1)
    do = torch.from_numpy(out.view(np.uint8)).to("cuda:0")
    order = torch.zeros(300, dtype=torch.int32, device="cuda:0")
    ports = torch.full((5 * A.TX_PORT.itemsize,), 0xa5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()

    def rc(dev_out=do.data_ptr(), n=300, oifs=oifs, dev_order=order.data_ptr(), dev_ports=ports.data_ptr()):
        oifs = np.ascontiguousarray(oifs, dtype=np.uint32)
        return nf.lib.dp_tx_plan_device(nf.ctx, dev_out, n, oifs.ctypes.data, len(oifs), dev_order, dev_ports, None)

    assert rc(oifs=np.arange(1, A.TX_MAX_PORTS + 2)) == A.EINVAL
    assert rc(oifs=[10, 0, 30]) == A.EINVAL and rc(oifs=[10, 20, 10]) == A.EINVAL
    assert rc(dev_out=None) == A.EINVAL and rc(dev_order=None) == A.EINVAL and rc(dev_ports=None) == A.EINVAL
    assert rc(dev_out=do.data_ptr() + 8) == A.EINVAL
    assert rc(dev_order=order.data_ptr() + 2) == A.EINVAL and rc(dev_ports=ports.data_ptr() + 4) == A.EINVAL
    with pytest.raises(RuntimeError):
        nf.tx_plan(out, [10, 10])
    # n = 0: the device form writes nothing, the host form fills zero counts
    assert rc(n=0) == 0 and rc(n=0, dev_out=None, dev_order=None, dev_ports=None) == 0
    nf.synchronize()
    assert bool((ports.cpu() == 0xa5).all())
    same(nf.tx_plan(out[:0], oifs), reference(out[:0], oifs))
    assert rc() == 0  # (and the context still plans)
    nf.synchronize()
    assert np.array_equal(order.cpu().numpy().view(np.uint32), reference(out, oifs)[0])
