"""The device route sort's names (include/dpgpu.h DP_OPT_DEVICE_FIB = 2): the
option's comment documents the mode, and the word of dp_publish_stats_t at
offset 4 is sorted_fibs in the header and in the numpy mirror."""
import os
import re

from dataplane_amd import _abi as A


def test_mode_two_and_sorted_fibs():
    hdr = open(os.path.join(A.ROOT, "include", "dpgpu.h")).read()
    comment = hdr[hdr.index("DP_OPT_CAPTURE = 4"):hdr.index("DP_OPT_DEVICE_FIB = 5")]
    assert re.search(r"\b2: as 1", comment) and "8 B a route" in comment and "sorted_fibs" in comment
    assert "DP_EINVAL" in comment
    assert re.search(r"uint32_t\s+device_fibs;[^;]*\n\s*uint32_t\s+sorted_fibs;", hdr)
    assert A.PUBLISH_STATS.names[:2] == ("device_fibs", "sorted_fibs") and A.PUBLISH_STATS.fields["sorted_fibs"][1] == 4
    assert A.PUBLISH_STATS.itemsize == 80 and A.ABI_VERSION == 9
