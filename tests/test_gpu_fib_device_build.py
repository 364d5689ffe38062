"""GPU: DIR-24-8 tables built on the device at publish (DP_OPT_DEVICE_FIB).
dp_fib_lookup over a device-built image against a plain longest-prefix match
written here (per FIB and family a dict per prefix length, longest first, from
the builder's own route list), exactly; dp_tables_publish_stats says the device
built the expected FIBs; the same keys give the same answers after a republish
with the option off."""
import random

import numpy as np
import pytest

from dataplane_amd import GpuPathNf, _abi as A
from dataplane_amd.tables import TablesBuilder as TB
from test_gpu_fib_lookup import add_nhs, keys_of, same, v4, v6

pytestmark = pytest.mark.gpu
TILE, STAGE = A.FIB_BUILD_TILE, A.FIB_BUILD_STAGE  # csrc/dp_fibbuild.h kTile (/24 slots), kStage (routes)
W = {4: 32, 6: 128}
N_NH = 40


def net_of(r):
    return int.from_bytes(bytes(r.prefix.addr[:W[r.prefix.family] // 8]), "big")


def reference(tb, keys):
    fib_of = {f.vrf_id: i for i, f in enumerate(tb.fibs)}
    tabs = {}
    for r in tb.routes:  # (a prefix inserted twice: the last wins)
        w, ln = W[r.prefix.family], r.prefix.len
        tabs.setdefault((r.fib, r.prefix.family), {}).setdefault(ln, {})[net_of(r) >> (w - ln)] = r.nh
    order = {k: sorted(t, reverse=True) for k, t in tabs.items()}
    out = np.zeros(len(keys), dtype=A.FIB_RESULT)
    for i, k in enumerate(keys):
        fam, nh = int(k["family"]), None
        t = (fib_of[int(k["vrf_id"])], fam)
        a = int.from_bytes(k["addr"][:W[fam] // 8].tobytes(), "big")
        for ln in order.get(t, ()):
            nh = tabs[t][ln].get(a >> (W[fam] - ln))
            if nh is not None:
                break
        out[i] = (A.FIB_NO_NH, 0, A.FIB_DEFAULT, 0) if nh is None else (nh, tb.nhs[nh].n_entries, A.FIB_ROUTE, 0)
    return out


def filler(tb, fib, base=0x14000000):
    """65,540 /24s: the FIB takes the DIR-24-8 form."""
    for i in range(65540):
        tb.add_route(fib, v4(base + (i << 8), 24), (i * 7919) % N_NH)


def build(name):
    """(builder, FIBs the device builds, extra key addresses per (vrf, family))."""
    rng, tb, extra = random.Random(sum(map(ord, name))), TB(), {}
    add_nhs(tb, N_NH)
    nh = lambda: rng.randrange(N_NH)  # noqa: E731
    tb.add_fib(1)
    filler(tb, 0)
    if name == "nesting":
        tb.add_route(0, "0.0.0.0/0", 1)
        for p in ("10.0.0.0/8", "10.16.0.0/12", "10.17.0.0/16", "10.17.16.0/20", "10.17.17.0/24",  # a chain
                  "10.32.0.0/12", "10.18.0.0/16", "10.17.32.0/20", "10.17.18.0/24", "10.17.16.0/24",  # siblings
                  "20.0.0.0/9", "20.64.0.0/10", "20.64.0.0/14", "20.65.0.0/16",  # over the filler's /24s
                  "80.0.0.0/24", "80.3.255.0/24", "80.0.0.0/14", "80.3.240.0/20",  # a tile's first and last slot
                  "80.4.0.0/15", "80.7.255.0/24", "80.8.0.0/24",  # starts on a tile's first slot, spans two
                  "192.0.0.0/3", "224.0.0.0/4", "255.255.255.0/24"):  # tiles in which no route starts
            tb.add_route(0, p, nh())
        tb.add_route(0, "10.17.0.0/16", 7), tb.add_route(0, "10.17.0.0/16", 8)  # twice: the last wins
        t0 = 0x50000000 >> 8
        extra[1, 4] = [s << 8 | 5 for s in (t0 - 1, t0, t0 + TILE - 1, t0 + TILE, t0 + 2 * TILE, t0 + 3 * TILE - 1)]
    elif name == "blocks":
        tb.add_route(0, "30.0.0.0/8", 3)
        for ln in range(25, 33):  # the full nest /25 > ... > /32, inside a routed /24
            tb.add_route(0, v4(0x140005ff, ln), ln)
        for p in ("30.1.2.64/26", "30.1.2.80/28",  # a /24 that is no route: the default is the /8
                  "30.1.3.0/25", "30.1.3.255/32",  # the adjacent slot
                  "0.0.0.128/25", "0.0.0.1/32", "255.255.255.255/32", "255.255.255.0/25"):  # slots 0 and 2^24 - 1
            tb.add_route(0, p, nh())
        for i in range(0, 65700, 1100):  # /25-/32 inside routed /24s and just past them
            tb.add_route(0, v4(0x14000000 + (i << 8) + rng.getrandbits(8), 25 + i // 1100 % 8), nh())
    elif name == "dense":
        # more routes start in one tile than it stages: every /24 of a /14 with all their covering
        # /23 ... /14; a second such tile with every third /24 left to its covers
        for base, gaps in ((0x2c400000, False), (0x2c800000, True)):
            n = 0
            for ln in range(14, 25):
                for i in range(1 << (ln - 14)):
                    if not (gaps and ln == 24 and i % 3 == 0):
                        tb.add_route(0, v4(base + (i << (32 - ln)), ln), (ln * 131 + i) % N_NH)
                        n += 1
            assert n > STAGE and base >> 8 & (TILE - 1) == 0
            extra.setdefault((1, 4), []).extend(base + (i << 8) + 9 for i in range(TILE))  # every slot of the tile
    elif name == "mixed":  # two DIR-24-8 FIBs, a small one (host-built direct table + Poptrie), v6
        tb.add_fib(2), tb.add_fib(3)
        filler(tb, 1, 0x28000000)
        for f in (0, 1, 2):
            tb.add_route(f, "10.0.0.0/8", 1 + f), tb.add_route(f, "10.1.2.128/25", 4 + f)
            tb.add_route(f, "10.1.2.129/32", 7 + f), tb.add_route(f, "2001:db8::/32", 10 + f)
            tb.add_route(f, v6(0x20010db8 << 96 | rng.getrandbits(96), 64), nh())
        extra = {(vrf, 6): [0x20010db8 << 96 | rng.getrandbits(96) for _ in range(200)] for vrf in (1, 2, 3)}
    return tb, (2 if name == "mixed" else 1), extra


def keys_for(tb, extra, rng):
    """Per FIB: the first and last address and the two just outside of every long
    route, every route off the filler and a sample of it; uniform random addresses."""
    ks = []
    for f, fib in enumerate(tb.fibs):
        rs = [r for r in tb.routes if r.fib == f and r.prefix.family == 4]
        pick = [r for r in rs if r.prefix.len != 24] + rng.sample(rs, min(len(rs), 3000))
        a = list(extra.get((fib.vrf_id, 4), ()))
        for r in pick:
            last = net_of(r) + (1 << (32 - r.prefix.len)) - 1
            a += [net_of(r), last, net_of(r) - 1, last + 1]
        ks.append(keys_of(fib.vrf_id, 4, a + [rng.getrandbits(32) for _ in range(30000 // len(tb.fibs))]))
        for r in tb.routes:
            if r.fib == f and r.prefix.family == 6:
                extra.setdefault((fib.vrf_id, 6), []).append(net_of(r) + (1 << (128 - r.prefix.len)) - 1)
        if (fib.vrf_id, 6) in extra:
            ks.append(keys_of(fib.vrf_id, 6, extra[fib.vrf_id, 6]))
    return np.concatenate(ks)


@pytest.mark.parametrize("name", ["nesting", "blocks", "dense", "mixed"])
def test_device_built_fib(name):
    tb, n_dev, extra = build(name)
    keys = keys_for(tb, extra, random.Random(5))
    want = reference(tb, keys)
    tables, nf = tb.build(), GpuPathNf(0)
    try:
        nf.set_device_fib(True)
        nf.publish(tables)
        st = nf.publish_stats()
        on = nf.fib_lookup(keys)
        nf.set_device_fib(False)
        nf.publish(tables)
        st_off = nf.publish_stats()
        off = nf.fib_lookup(keys)
    finally:
        nf.close()
    same(on, want, f"{name}: device-built")
    same(off, on, f"{name}: republished host-built")
    direct = n_dev * (4 << 24)
    assert st["device_fibs"] == n_dev and st_off["device_fibs"] == 0 and st_off["built_bytes"] == 0
    assert st["image_bytes"] == st_off["image_bytes"] == st_off["upload_bytes"]
    assert st["built_bytes"] >= direct and st["built_bytes"] % 512 == 0
    # the device-built regions never cross the bus: the rest of the image, and the lists (at most 16 B a
    # short route; 4 B and a 16-byte block record a long one)
    assert 0 < int(st["upload_bytes"]) - int(st["image_bytes"] - st["built_bytes"]) <= 20 * (len(tb.routes) + 3)
