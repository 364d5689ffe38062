"""The device FIB build's names (include/dpgpu.h DP_OPT_DEVICE_FIB, "Publish
statistics"): the option constant, the numpy mirror of dp_publish_stats_t and
the entry point are in the Python mirror, the header and the library; the ABI
version is unchanged."""
import os
import re

from dataplane_amd import _abi as A


def test_option_stats_record_and_symbol():
    hdr = open(os.path.join(A.ROOT, "include", "dpgpu.h")).read()
    assert int(re.search(r"DP_OPT_DEVICE_FIB\s*=\s*(\d+)", hdr).group(1)) == A.OPT_DEVICE_FIB == 5
    assert A.PUBLISH_STATS.itemsize == A.work_lib().dpw_sizeof(b"dp_publish_stats_t") == 80
    assert [A.PUBLISH_STATS.fields[f][1] for f in A.PUBLISH_STATS.names] == [0, 4] + list(range(8, 80, 8))
    assert A.NP_STRUCTS["dp_publish_stats_t"] is A.PUBLISH_STATS
    assert "dp_tables_publish_stats" in A.GPU_SYMBOLS
    lib = A.gpu_lib()
    assert lib.dp_abi_version() == A.ABI_VERSION == 9
    assert hasattr(lib, "dp_tables_publish_stats")
    assert lib.dp_tables_publish_stats(None, None) == A.EINVAL
