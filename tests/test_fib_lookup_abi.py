"""The FIB lookup's records and names (include/dpgpu.h "The FIB lookup alone"):
the numpy mirrors match the C structs, the library exports the entry points."""
from dataplane_amd import _abi as A


def test_fib_record_layouts():
    lib = A.work_lib()
    assert A.FIB_KEY.itemsize == lib.dpw_sizeof(b"dp_fib_key_t") == 24
    assert A.FIB_RESULT.itemsize == lib.dpw_sizeof(b"dp_fib_result_t") == 8
    # dp_fib_key_t: vrf_id 0, family 4, pad 5, addr 8; dp_fib_result_t: nh 0, n_entries 4, code 6, pad 7
    assert [A.FIB_KEY.fields[f][1] for f in ("vrf_id", "family", "pad", "addr")] == [0, 4, 5, 8]
    assert [A.FIB_RESULT.fields[f][1] for f in ("nh", "n_entries", "code", "pad")] == [0, 4, 6, 7]
    assert A.FIB_KEY.fields["addr"][0].shape == (16,)


def test_fib_symbols():
    assert {"dp_fib_lookup", "dp_fib_lookup_device"} <= set(A.GPU_SYMBOLS)
    lib = A.gpu_lib()
    assert lib.dp_abi_version() == A.ABI_VERSION == 9
    for s in ("dp_fib_lookup", "dp_fib_lookup_device", "dpd_debug_set_fib_lookup_form"):
        assert hasattr(lib, s), s
