"""Packet capture's records and names (include/dpgpu.h "Packet capture"): the
numpy mirrors match the C structs, the library exports the entry points, the
ABI version is unchanged."""
from dataplane_amd import _abi as A

NEW = ("dp_capture_open", "dp_capture_set_filter", "dp_capture_close", "dp_capture_device", "dp_capture_read")


def test_capture_record_layouts():
    lib = A.work_lib()
    assert A.CAP_REC.itemsize == lib.dpw_sizeof(b"dp_cap_rec_t") == 32
    assert A.CAP_FILTER.itemsize == lib.dpw_sizeof(b"dp_capture_filter_t")
    assert [A.CAP_REC.fields[f][1] for f in A.CAP_REC.names] == [0, 8, 12, 16, 18, 20, 21, 22, 24, 28]
    assert [A.CAP_FILTER.fields[f][1] for f in ("done_mask", "src_vni", "src", "dst", "sport_lo", "snaplen")] == \
        [8, 16, 24, 44, 64, 72]


def test_capture_symbols():
    assert set(NEW) <= set(A.GPU_SYMBOLS)
    lib = A.gpu_lib()
    assert lib.dp_abi_version() == A.ABI_VERSION == 9
    for s in NEW:
        assert hasattr(lib, s), s
    assert A.OPT_CAPTURE == 4 and (A.CAP_RX, A.CAP_TX) == (1, 2)
