"""GPU: a large v4 FIB's routes sorted, deduplicated and listed on the device at
publish (DP_OPT_DEVICE_FIB = 2).  dp_fib_lookup over the image built that way
against the plain longest-prefix match of test_gpu_fib_device_build (the last
insert of a prefix wins), exactly; the same keys answer the same after a
republish in mode 1 and in mode 0; dp_tables_publish_stats says which FIBs the
device sorted, that the image is the same size, and that only 8 B a route
crossed the bus for them.  Beside that test's shapes: one route set in three
insertion orders, a prefix inserted 5,000 times through the whole order (its
duplicates span the sort's tiles), one address at every length (keys that differ
in the length digit alone), a full /24 of 510 long routes next to a /24 holding
one, and an inserted /0 over the implicit one."""
import random

import pytest

from dataplane_amd import GpuPathNf, _abi as A
from dataplane_amd.tables import TablesBuilder as TB
from test_gpu_fib_device_build import N_NH, build, filler, keys_for, reference
from test_gpu_fib_lookup import add_nhs, same, v4

pytestmark = pytest.mark.gpu
OLD = ["nesting", "blocks", "dense", "mixed"]
ORDERS = ["ascending", "descending", "shuffled"]
NEW = ORDERS + ["duplicates", "lengths", "full_block", "user_default"]

def shape(name):
    if name in OLD:
        return build(name)
    tb, extra = TB(), {}
    add_nhs(tb, 5042 if name == "duplicates" else N_NH)
    tb.add_fib(1)
    if name in ORDERS:  # unique prefixes: the filler's /24s, shorter routes over them, longer ones inside
        rs = [(0x14000000 + (i << 8), 24, i * 7919 % N_NH) for i in range(65540)]
        rs += [(0x14000000 + (i << 8), 12 + i % 12, i % N_NH) for i in range(0, 65540, 4096)]
        rs += [(0x14000000 + (i << 8) + 0x80, 25 + i % 8, i % N_NH) for i in range(0, 65540, 500)]
        rs.sort()  # by (address, length): the order the sort must reach
        if name == "descending":
            rs.reverse()
        elif name == "shuffled":
            random.Random(3).shuffle(rs)
        for a, ln, nh in rs:
            tb.add_route(0, v4(a, ln), nh)
        return tb, 1, extra
    if name == "duplicates":
        for i in range(65540):
            tb.add_route(0, v4(0x14000000 + (i << 8), 24), i % N_NH)
            if i % 13 == 0:
                tb.add_route(0, "20.9.0.0/16", i // 13)  # 5,042 times, a next hop each
        return tb, 1, extra
    filler(tb, 0)
    if name == "lengths":
        for ln in range(8, 33):
            tb.add_route(0, v4(0x0b000000, ln), ln)
    elif name == "full_block":
        for ln in range(25, 33):
            for i in range(1 << (ln - 24)):
                tb.add_route(0, v4(0x1e000000 + (i << (32 - ln)), ln), (ln * 3 + i) % N_NH)
        tb.add_route(0, "30.0.1.77/32", 9)
        extra[1, 4] = list(range(0x1e000000, 0x1e000200))
    elif name == "user_default":
        tb.add_route(0, "0.0.0.0/0", 5)
    return tb, 1, extra


@pytest.mark.parametrize("name", OLD + NEW)
def test_device_sorted_fib(name):
    tb, n_dev, extra = shape(name)
    keys = keys_for(tb, extra, random.Random(5))
    want = reference(tb, keys)
    tables, nf, got, st = tb.build(), GpuPathNf(0), {}, {}
    try:
        for mode in (2, 1, 0):
            nf.set_device_fib(mode)
            nf.publish(tables)
            st[mode] = nf.publish_stats()
            got[mode] = nf.fib_lookup(keys)
    finally:
        nf.close()
    same(got[2], want, f"{name}: device-sorted")
    same(got[1], got[2], f"{name}: republished, host-sorted")
    same(got[0], got[2], f"{name}: republished, host-built")
    assert st[2]["sorted_fibs"] == st[2]["device_fibs"] == st[1]["device_fibs"] == n_dev
    assert st[1]["sorted_fibs"] == st[0]["sorted_fibs"] == st[0]["device_fibs"] == 0
    assert st[2]["image_bytes"] == st[1]["image_bytes"] == st[0]["image_bytes"]
    assert st[2]["built_bytes"] == st[1]["built_bytes"]
    # of a device-sorted FIB only its routes cross the bus, 8 B each with the implicit /0
    per_fib = [sum(1 for r in tb.routes if r.fib == f and r.prefix.family == 4) for f in range(len(tb.fibs))]
    routes = sum(n for n in per_fib if n >= 65536)
    assert 0 < int(st[2]["upload_bytes"]) - int(st[2]["image_bytes"] - st[2]["built_bytes"]) <= 8 * (routes + n_dev) + 64 * n_dev


def test_mode_above_two_is_rejected():
    nf = GpuPathNf(0)
    try:
        with pytest.raises(RuntimeError, match=f"rc={A.EINVAL}"):
            nf.set_device_fib(3)
    finally:
        nf.close()
