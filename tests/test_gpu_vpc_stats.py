"""GPU: per-VPC statistics (the Stats stage, stats/src/dpstats.rs:942-1007)
against a numpy restatement of its rules, over crafted records through
dp_vpc_stats_accumulate_device and over whole bursts with DP_OPT_VPC_STATS."""
import ctypes as C

import numpy as np
import pytest

from dataplane_amd import GpuPathNf, _abi as A
from dataplane_amd.flows import FlowTable
from dataplane_amd.workload import Workload
from oracle.pyoracle import Oracle, OracleFlows

from edgecase import pack_burst
from flowgen import frames_of, install, scenario

pytestmark = pytest.mark.gpu
DELIVERED = A.DONE["Delivered"]
COLS = ("fwd_packets", "fwd_bytes", "drop_packets", "drop_bytes")


@pytest.fixture(scope="module")
def nf():
    import torch
    torch.cuda.init()
    n = GpuPathNf(0)
    yield n
    n.attach_flows(None)
    n.close()


def reference(out, meta):
    """The cells of `out` / `meta` records (any arrays with those fields), sorted."""
    src, dst = meta["src_vni"].astype(np.uint64), meta["dst_vni"].astype(np.uint64)
    ln, drop = out["len"].astype(np.uint64), out["done"] != DELIVERED
    has, pair = src != 0, dst != 0
    ups = [(has & drop, 0 * dst, 2), (has & drop & pair, dst, 2), (has & ~drop & pair, dst, 0)]
    keys = np.concatenate([src[s] << np.uint64(32) | d[s] for s, d, _ in ups])
    cols = np.concatenate([np.full(int(s.sum()), c) for s, _, c in ups])
    u, inv = np.unique(keys, return_inverse=True)
    tab = np.zeros((len(u), 4), dtype=np.uint64)
    np.add.at(tab, (inv, cols), np.uint64(1))
    np.add.at(tab, (inv, cols + 1), np.concatenate([ln[s] for s, _, _ in ups]))
    cells = np.zeros(len(u), dtype=A.VPC_STAT)
    cells["src_vni"], cells["dst_vni"] = u >> np.uint64(32), u & np.uint64(0xffffffff)
    for j, f in enumerate(COLS):
        cells[f] = tab[:, j]
    return cells


def cell_keys(cells):
    return cells["src_vni"].astype(np.uint64) << np.uint64(32) | cells["dst_vni"]


def records(n, keys, seed):
    """n seeded out / meta records: lengths up to 65535, cells of key set `keys`."""
    rng = np.random.default_rng(seed)
    out, meta = np.zeros(n, dtype=A.PKT_OUT), np.zeros(n, dtype=A.PKT_META)
    out["len"] = rng.integers(0, 65536, n)
    out["done"] = DELIVERED
    j = rng.integers(0, 1 << 30, n)
    if keys == "one":          # the whole wave on one cell
        meta["src_vni"], meta["dst_vni"] = 5, 9
    elif keys == "mixed":      # 3 VPCs all-to-all, no source / no destination, every done class
        vnis = np.array([0, 10, 20, 30])
        meta["src_vni"], meta["dst_vni"] = vnis[j % 4], vnis[j // 4 % 4]
        out["done"] = rng.choice(np.r_[np.arange(A.DONE_COUNT), A.DONE_NONE, [DELIVERED] * 30], n)
    elif keys == "spill":      # more distinct cells than a workgroup's LDS table holds
        meta["src_vni"], meta["dst_vni"] = 1 + j % 40, j // 40 % 31
        out["done"] = rng.choice([DELIVERED, DELIVERED, A.DONE["Filtered"]], n)
    else:                      # "over": DP_VPC_STATS_CELLS / 2 + 50 distinct cells
        c = np.arange(n) % (A.VPC_STATS_CELLS // 2 + 50)
        meta["src_vni"], meta["dst_vni"] = 1 + c // 64, 1 + c % 64
    return out, meta


def accumulate(nf, out, meta):
    import torch
    dev = torch.device("cuda", 0)
    do = torch.from_numpy(out.view(np.uint8)).to(dev)
    dm = torch.from_numpy(meta.view(np.uint8)).to(dev)
    torch.cuda.synchronize(dev)
    nf.vpc_stats_accumulate_device(do.data_ptr(), dm.data_ptr(), len(out))
    nf.synchronize()


@pytest.mark.parametrize("keys", ["one", "mixed", "spill", "over"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, 4096, "chunks3"])
def test_crafted_records(nf, n, keys):
    if n == "chunks3":  # a persistent workgroup (one per compute unit, 1024 packets a chunk) takes 3
        import torch
        n = 2 * torch.cuda.get_device_properties(0).multi_processor_count * 1024 + 300
    out, meta = records(n, keys, seed=n)
    nf.vpc_stats(reset=True)
    accumulate(nf, out, meta)
    got, lost = nf.vpc_stats(reset=True)
    ref = reference(out, meta)
    # every reported cell is exact; what is not reported is counted as lost
    assert np.array_equal(got, ref[np.isin(cell_keys(ref), cell_keys(got))])
    assert lost + int(got["fwd_packets"].sum() + got["drop_packets"].sum()) == \
        int(ref["fwd_packets"].sum() + ref["drop_packets"].sum())
    if len(ref) <= A.VPC_STATS_CELLS // 2:
        assert lost == 0 and len(got) == len(ref)
    else:
        assert lost > 0 and len(got) == A.VPC_STATS_CELLS // 2


def test_accumulates_across_calls_reset_and_enospc(nf):
    a, b = records(1000, "mixed", 1), records(777, "spill", 2)
    nf.vpc_stats(reset=True)
    accumulate(nf, *a)
    accumulate(nf, *b)
    ref = reference(np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]))
    n, small = C.c_uint32(0), np.zeros(3, dtype=A.VPC_STAT)
    assert nf.lib.dp_vpc_stats_read(nf.ctx, small.ctypes.data, 3, C.byref(n), None, 1) == A.ENOSPC
    assert n.value == len(ref)             # the needed count; nothing was reset
    assert np.array_equal(nf.vpc_stats()[0], ref)
    assert np.array_equal(nf.vpc_stats(reset=True)[0], ref)
    got, lost = nf.vpc_stats()
    assert len(got) == 0 and lost == 0


def test_reference_mixed_batch(nf):
    """mixed_batch_accumulates (dpstats.rs:1292-1328) and the missing-source case."""
    a, b, c, L = 100, 200, 300, 1000
    rows = [(a, b, DELIVERED)] * 2 + [(a, b, A.DONE["Filtered"])] * 3 + \
        [(a, c, A.DONE["RouteDrop"]), (a, 0, A.DONE["RouteDrop"]), (0, b, DELIVERED), (0, b, A.DONE["Filtered"])]
    out, meta = np.zeros(len(rows), dtype=A.PKT_OUT), np.zeros(len(rows), dtype=A.PKT_META)
    meta["src_vni"], meta["dst_vni"], out["done"] = zip(*rows)
    out["len"] = L
    nf.vpc_stats(reset=True)
    accumulate(nf, out, meta)
    got, lost = nf.vpc_stats(reset=True)
    assert lost == 0
    assert got.tolist() == [(a, 0, 0, 0, 5, 5 * L), (a, b, 2, 2 * L, 3, 3 * L), (a, c, 0, 0, 1, L)]


def device_burst(nf, w, k):
    """The first k packets as a resident burst without a meta array, launched
    on a stream of its own and not waited for; returns what must outlive it."""
    import torch
    dev = torch.device("cuda", 0)
    db = torch.from_numpy(w.fresh_buf()).to(dev)
    di = torch.from_numpy(w.inp[:k].copy().view(np.uint8)).to(dev)
    do = torch.zeros(k * A.PKT_OUT.itemsize, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    nf.process_device(db.data_ptr(), db.numel(), di.data_ptr(), do.data_ptr(), k, None, st.cuda_stream)
    return db, di, do, st


@pytest.mark.parametrize("path", ["meta", "no_meta", "device_no_meta"])
@pytest.mark.parametrize("cfg", [2, 5])
def test_bursts_match_oracle_records(nf, cfg, path):
    """Whole bursts with the option on equal the rules over the oracle's
    records: a host burst with a meta array and without one (its chunks' meta
    records then stay on the device), and two resident bursts without a meta
    array, of growing size on two streams -- the context's meta scratch, grown
    between them, the second ordered behind the first."""
    w = Workload(cfg, 3000, seed=400 + cfg, n_routes_v4=3000, n_routes_v6=2000 if cfg == 5 else 0,
                 n_acl=300, n_nat=24, tcp_percent=25)
    nf.publish(w.tables)
    o_ref = Oracle(w.tables).process(w.fresh_buf(), w.inp)
    parts = [w.n // 3, w.n] if path == "device_no_meta" else [w.n]
    ref = reference(*[np.concatenate([o_ref[:k] for k in parts])] * 2)
    assert len(ref) > 4 and ref["drop_packets"].sum() and ref["fwd_packets"].sum()
    nf.vpc_stats(reset=True)
    nf.set_vpc_stats(True)
    try:
        if path == "device_no_meta":
            alive = [device_burst(nf, w, k) for k in parts]
            got, lost = nf.vpc_stats()  # ordered behind both bursts
            assert lost == 0 and np.array_equal(got, ref)
            del alive
        else:
            nf.process_arrays(w.fresh_buf(), w.inp, with_meta=path == "meta")
    finally:
        nf.set_vpc_stats(False)
    # option off again: a burst leaves the counters alone
    nf.process_arrays(w.fresh_buf(), w.inp)
    got, lost = nf.vpc_stats(reset=True)
    assert lost == 0 and np.array_equal(got, ref)


def test_flows_burst_counts_final_verdicts(nf):
    """The flows variant (tests/flowgen.py scenario): flows invalidated within
    the burst turn verdicts in dp_flow_fixup; the stage runs behind it."""
    w = Workload(2, 6000, seed=1, n_routes_v4=3000, n_acl=400, n_nat=24, tcp_percent=30)
    ora = Oracle(w.tables)
    o0 = ora.process(w.fresh_buf(), w.inp)
    items, burst = scenario(frames_of(w), o0["dst_vni"], genid=1, seed=1, n_flows=600,
                            vnis=sorted(set(int(v) for v in o0["dst_vni"] if v)))
    oft, gft = OracleFlows(), FlowTable(0, 1 << 13)
    install(oft, items), install(gft, items)
    buf, inp = pack_burst([(f, 1, A.IN_SEEDED_OVERLAY, v) for f, v in burst])
    oout = ora.process_flows(buf.copy(), inp, oft)[0]
    assert (oout["done"] != ora.process(buf.copy(), inp)["done"]).any()  # the flows turn verdicts
    nf.publish(w.tables)
    nf.attach_flows(gft)
    nf.vpc_stats(reset=True)
    nf.set_vpc_stats(True)
    try:
        gout = nf.process_arrays(buf.copy(), inp)
    finally:
        nf.set_vpc_stats(False)
        nf.attach_flows(None)
    assert np.array_equal(gout["done"], oout["done"])
    got, lost = nf.vpc_stats(reset=True)
    assert lost == 0 and np.array_equal(got, reference(oout, oout))


def test_option_off_records_nothing(nf):
    w = Workload(2, 2000, seed=7, n_routes_v4=2000, n_acl=100, n_nat=8)
    fresh = GpuPathNf(0)
    fresh.publish(w.tables)
    fresh.process_arrays(w.fresh_buf(), w.inp)
    got, lost = fresh.vpc_stats()
    fresh.close()
    assert len(got) == 0 and lost == 0
