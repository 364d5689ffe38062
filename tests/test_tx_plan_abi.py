"""The TX plan's record and names (include/dpgpu.h "TX plan"): the numpy mirror
matches the C struct, the library exports the entry points, the ABI version is
unchanged, and dp_mbuf_burst_tx (host only) orders an mbuf array by a plan."""
import numpy as np

from dataplane_amd import _abi as A

NEW = ("dp_tx_plan_device", "dp_tx_plan", "dp_mbuf_burst_tx")


def test_tx_port_layout_and_symbols():
    assert A.TX_PORT.itemsize == A.work_lib().dpw_sizeof(b"dp_tx_port_t") == 24
    assert [A.TX_PORT.fields[f][1] for f in A.TX_PORT.names] == [0, 4, 8, 12, 16]
    assert A.NP_STRUCTS["dp_tx_port_t"] is A.TX_PORT and A.TX_MAX_PORTS == 62
    assert set(NEW) <= set(A.GPU_SYMBOLS)
    lib = A.gpu_lib()
    assert lib.dp_abi_version() == A.ABI_VERSION == 9
    for s in NEW:
        assert hasattr(lib, s), s


def test_mbuf_burst_tx():
    lib = A.gpu_lib()
    mbufs = (0x1000 + 64 * np.arange(9)).astype(np.uint64)  # (never dereferenced)

    def tx(order, n=len(mbufs)):
        order, got = np.array(order, dtype=np.uint32), np.zeros(len(order), dtype=np.uint64)
        return lib.dp_mbuf_burst_tx(mbufs.ctypes.data, n, order.ctypes.data, len(order), got.ctypes.data), got

    perm = np.random.default_rng(3).permutation(len(mbufs))
    rc, got = tx(perm)
    assert rc == 0 and np.array_equal(got, mbufs[perm])
    rc, got = tx(perm[:4])  # a prefix: one port's share
    assert rc == 0 and np.array_equal(got, mbufs[perm[:4]])
    assert tx([0, 9, 1])[0] == A.EINVAL and tx([3], n=3)[0] == A.EINVAL
    assert tx([])[0] == 0 and lib.dp_mbuf_burst_tx(None, 0, None, 0, None) == 0
