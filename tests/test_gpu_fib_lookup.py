"""GPU: dp_fib_lookup against a plain longest-prefix match written here (per FIB
and family a dict per prefix length, masked from the longest down), built from
the TablesBuilder route list that is published.  Exact equality."""
import ctypes as C
import functools
import ipaddress
import os
import random

import numpy as np
import pytest

from dataplane_amd import _abi as A
from dataplane_amd.tables import TablesBuilder as TB

pytestmark = pytest.mark.gpu
TILE = 1024  # dp_fiblookup.hip kTile
FORMS = {"auto": 0, "direct": 1}  # (a binned form, 2, lost its measurement and was removed)
W = {4: 32, 6: 128}


def keys_of(vrf, fam, addrs):
    """The key builder: one VRF and family, integer addresses."""
    k = np.zeros(len(addrs), dtype=A.FIB_KEY)
    k["vrf_id"], k["family"] = vrf, fam
    nb = 16 if fam == 6 else 4
    raw = b"".join((int(a) % (1 << 8 * nb)).to_bytes(nb, "big") for a in addrs)
    k["addr"][:, :nb] = np.frombuffer(raw, np.uint8).reshape(-1, nb)
    return k


def reference(tb, keys):
    fib_of = {f.vrf_id: i for i, f in enumerate(tb.fibs)}
    tabs = {}
    for r in tb.routes:
        w, ln = W[r.prefix.family], r.prefix.len
        net = int.from_bytes(bytes(r.prefix.addr[:w // 8]), "big")
        tabs.setdefault((r.fib, r.prefix.family), {}).setdefault(ln, {})[net >> (w - ln)] = r.nh
    order = {k: sorted(t, reverse=True) for k, t in tabs.items()}
    out = np.zeros(len(keys), dtype=A.FIB_RESULT)
    for i, k in enumerate(keys):
        fam, nh = int(k["family"]), None
        if fam not in W:
            code = A.FIB_BAD_FAMILY
        elif int(k["vrf_id"]) not in fib_of:
            code = A.FIB_NO_VRF
        else:
            t = (fib_of[int(k["vrf_id"])], fam)
            a = int.from_bytes(k["addr"][:W[fam] // 8].tobytes(), "big")
            for ln in order.get(t, ()):  # longest first: the first hit wins
                nh = tabs[t][ln].get(a >> (W[fam] - ln))
                if nh is not None:
                    break
            code = A.FIB_ROUTE if nh is not None else A.FIB_DEFAULT
        out[i] = (A.FIB_NO_NH, 0, code, 0) if nh is None else (nh, tb.nhs[nh].n_entries, code, 0)
    return out


def edge_keys(tb, rng, n_random):
    """Per FIB and family: every route's first and last address and the two just
    outside, then random addresses, uniform and under a route's top bits."""
    ks = []
    for f, fib in enumerate(tb.fibs):
        for fam in (4, 6):
            a, low = [], 100 if fam == 6 else 10
            for r in tb.routes:
                if r.fib == f and r.prefix.family == fam:
                    net = int.from_bytes(bytes(r.prefix.addr[:W[fam] // 8]), "big")
                    last = net + (1 << (W[fam] - r.prefix.len)) - 1
                    a += [net, last, net - 1, last + 1]
            near = [x >> low << low | rng.getrandbits(low) for x in a[:n_random]]
            ks.append(keys_of(fib.vrf_id, fam, a + near + [rng.getrandbits(W[fam]) for _ in range(n_random)]))
    return np.concatenate(ks)


def add_nhs(tb, n):
    for i in range(n):  # (every 7th an ECMP pair)
        tb.add_nh([[TB.drop()]] * (2 if i % 7 == 3 else 1))


def v4(x, ln, w=32):
    return f"{ipaddress.ip_address(x >> (w - ln) << (w - ln)) if w == 128 else ipaddress.IPv4Address(x >> (w - ln) << (w - ln))}/{ln}"


v6 = functools.partial(v4, w=128)


@functools.lru_cache(maxsize=None)
def case(name):
    """(builder, keys, reference results) of one table form."""
    rng, tb = random.Random(sum(map(ord, name))), TB()
    if name == "poptrie4":  # FIB 0: every length 0-32 (20-bit direct table); FIB 1: <= /16 (16-bit)
        add_nhs(tb, 40)
        tb.add_fib(1), tb.add_fib(2)
        for ln in range(33):
            for _ in range(8):
                tb.add_route(0, v4(rng.getrandbits(32), ln), rng.randrange(40))
                if 1 <= ln <= 16:
                    tb.add_route(1, v4(rng.getrandbits(32), ln), rng.randrange(40))
        for i, p in enumerate(["10.0.0.0/8", "10.1.0.0/16", "10.1.2.0/24", "10.1.2.128/25", "10.1.2.129/32"]):
            tb.add_route(0, p, i)
    elif name in ("dir16", "dir32"):  # > 65,536 routes: DIR-24-8; dir32: next hops past 16 bits
        n_nh = 65535 if name == "dir32" else 30
        add_nhs(tb, n_nh)
        tb.add_fib(1)
        for i in range(65540):
            tb.add_route(0, v4(0x14000000 + (i << 8), 24), (i * 7919) % n_nh)
        for i in range(0, 65700, 1100):  # /25-/32 inside routed /24s and just past them
            tb.add_route(0, v4(0x14000000 + (i << 8) + rng.getrandbits(8), 25 + i // 1100 % 8), rng.randrange(n_nh))
    elif name == "v6":  # routes longer than /16 sharing no prefix: no window
        add_nhs(tb, 20)
        tb.add_fib(1)
        for top in (0x2001, 0x3001, 0xfd00, 0x2a02):
            for ln in (8, 16, 17, 22, 32, 48, 64, 65, 127, 128):
                tb.add_route(0, v6(top << 112 | rng.getrandbits(112), ln), rng.randrange(20))
    elif name == "v6win":  # every route longer than /16 under 2001:db8::/32
        add_nhs(tb, 20)
        tb.add_fib(1)
        tb.add_route(0, "2000::/3", 1)
        for ln in list(range(33, 129, 5)) * 3 + [128, 52, 53]:
            tb.add_route(0, v6(0x20010db8 << 96 | rng.getrandbits(96), ln), rng.randrange(20))
    keys = edge_keys(tb, rng, 2000)
    if name == "v6win":  # below, inside and above the window
        keys = np.concatenate([keys, keys_of(1, 6, [(0x20010db7 + d) << 96 | rng.getrandbits(96)
                                                    for d in (0, 1, 2) for _ in range(300)])])
    return tb, keys, reference(tb, keys)


def lookup(tb, batches, form="auto"):
    from dataplane_amd import GpuPathNf
    lib = A.gpu_lib()
    nf = GpuPathNf(0)
    try:
        lib.dpd_debug_set_fib_lookup_form(FORMS[form])
        nf.publish(tb.build())
        return [nf.fib_lookup(k) for k in batches]
    finally:
        lib.dpd_debug_set_fib_lookup_form(0)
        nf.close()


def same(got, want, what):
    bad = np.nonzero((got["code"] != want["code"]) | (got["nh"] != want["nh"]) | (got["n_entries"] != want["n_entries"]))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} differ, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["poptrie4", "dir16", "dir32", "v6", "v6win"])
def test_table_forms(name, form):
    tb, keys, want = case(name)
    assert {A.FIB_ROUTE, A.FIB_DEFAULT} <= set(want["code"])
    same(lookup(tb, [keys], form)[0], want, f"{name} {form}")


@pytest.mark.parametrize("form", list(FORMS))
def test_batch_sizes_and_runs(form):
    """The tail; a tile of equal keys and one sharing a /24, over a block."""
    tb, keys, want = case("poptrie4")
    sizes = [1, 63, TILE + 1, 2 * TILE + 17]
    for n, got in zip(sizes, lookup(tb, [keys[:n] for n in sizes], form)):
        assert len(got) == n
        same(got, want[:n], f"n={n}")
    tb, _, _ = case("dir16")
    runs = [keys_of(1, 4, [0x14000000 + (1100 << 8) + 77] * TILE),
            keys_of(1, 4, [0x14000000 + (1100 << 8) + i % 256 for i in range(TILE)])]
    for k, got in zip(runs, lookup(tb, runs, form)):
        same(got, reference(tb, k), "runs")


def mixed():
    tb = TB()
    add_nhs(tb, 8)
    for vrf in (1, 2, 3):  # (VRF 3: a FIB with no routes)
        tb.add_fib(vrf)
    tb.add_route(0, "10.0.0.0/8", 1), tb.add_route(1, "10.0.0.0/8", 2)
    tb.add_route(0, "0.0.0.0/0", 3), tb.add_route(0, "10.9.0.0/16", 4), tb.add_route(1, "2001:db8::/32", 5)
    rng = random.Random(7)
    parts = []
    for _ in range(TILE // 4):  # v4 and v6, the VRFs, an unknown VRF and bad families interleaved
        a4, a6 = 0x0a000000 | rng.getrandbits(24), 0x20010db8 << 96 | rng.getrandbits(96)
        parts += [keys_of(1, 4, [a4]), keys_of(2, 6, [a6]), keys_of(2, 4, [a4, rng.getrandbits(32)]),
                  keys_of(3, 4, [a4]), keys_of(3, 6, [a6]), keys_of(99, 4, [a4]), keys_of(1, 4, [rng.getrandbits(32)])]
    keys = np.concatenate(parts)
    keys["family"][5::97] = 0
    keys["family"][11::89] = 5
    return tb, keys


@pytest.mark.parametrize("form", list(FORMS))
def test_mixed_batch_and_input_order(form):
    tb, keys = mixed()
    want = reference(tb, keys)
    perm = np.random.default_rng(3).permutation(len(keys))
    got, shuffled = lookup(tb, [keys, keys[perm]], form)
    same(got, want, "mixed")
    same(shuffled, want[perm], "shuffled")
    assert set(np.unique(got["code"])) == {A.FIB_ROUTE, A.FIB_DEFAULT, A.FIB_NO_VRF, A.FIB_BAD_FAMILY}
    ok = (keys["family"] == 4) | (keys["family"] == 6)
    assert (got["code"][(keys["vrf_id"] == 3) & ok] == A.FIB_DEFAULT).all()  # the FIB with no routes
    assert (got["code"][(keys["vrf_id"] == 1) & (keys["family"] == 4)] == A.FIB_ROUTE).all()  # its /0 is a route
    both = ok & (keys["addr"][:, 0] == 10) & (keys["addr"][:, 1] != 9)
    assert set(got["nh"][both & (keys["vrf_id"] == 1)]) == {1} and set(got["nh"][both & (keys["vrf_id"] == 2)]) == {2}


def test_no_tables_before_a_publish():
    """(Published tables are the device's, shared by a process's contexts: a
    process of its own.)"""
    import subprocess, sys  # noqa: E401
    code = ("import numpy as np\nfrom dataplane_amd import GpuPathNf, _abi as A\nnf = GpuPathNf(0)\n"
            "k, o = np.zeros(4, A.FIB_KEY), np.zeros(4, A.FIB_RESULT)\n"
            "print(nf.lib.dp_fib_lookup(nf.ctx, k.ctypes.data, o.ctypes.data, 4))\nnf.close()\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=A.ROOT, env=dict(os.environ, PYTHONPATH=A.ROOT),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and int(r.stdout.split()[-1]) == A.ENOTABLES, r.stderr


def test_device_entry_point_and_status_codes():
    import torch
    from dataplane_amd import GpuPathNf
    tb, keys = mixed()
    nf = GpuPathNf(0)
    try:
        out = np.zeros(4, dtype=A.FIB_RESULT)
        nf.publish(tb.build())
        assert nf.lib.dp_fib_lookup(nf.ctx, None, None, 0) == 0 and len(nf.fib_lookup(keys[:0])) == 0
        assert nf.lib.dp_fib_lookup(nf.ctx, None, out.ctypes.data, 4) == -22  # DP_EINVAL
        host = nf.fib_lookup(keys)
        # a stream of the test's own, destroyed below (torch's runtime is the process's one)
        hip, raw = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")), C.c_void_p()
        assert hip.hipStreamCreate(C.byref(raw)) == 0
        stream = torch.cuda.ExternalStream(raw.value)
        with torch.cuda.stream(stream):
            dk = torch.from_numpy(keys.view(np.uint8)).cuda()
            do = torch.zeros(len(keys) * A.FIB_RESULT.itemsize, dtype=torch.uint8, device="cuda")
            nf.fib_lookup_device(dk.data_ptr(), do.data_ptr(), len(keys), raw.value)
        stream.synchronize()
        assert hip.hipStreamDestroy(raw) == 0
        assert np.array_equal(do.cpu().numpy().view(A.FIB_RESULT), host)
        probe = keys_of(1, 4, [0x0a090001])
        assert nf.fib_lookup(probe)["nh"][0] == 4
        tb.routes = [r for r in tb.routes if r.nh != 4]  # republish without 10.9.0.0/16
        nf.publish(tb.build())
        assert nf.fib_lookup(probe)["nh"][0] == 1
    finally:
        nf.close()
