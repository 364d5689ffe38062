"""GPU: frame placement (tests/placement.py) through the HIP path -- frames at
every start residue, packed tightly with random non-zero fill, bit-exact
against the oracle over the whole buffer.  What the host emulation does not
run is exercised here: the wave-cooperative window load and write-back, the
host staging and the shard rebase on spans that do not start at the frame,
and the wave-uniform all-in-window ballot.  A wave runs the all-in-window copy
of process_packet (the one with the single 16-bit LDS accesses) only when all
its frames fit the window at even starts: the bursts of short frames under
the even placements do, which each such test asserts from its in-records
(placement.wave_fit); the edge corpus and the sweep, with frames longer than
the window in every wave, run the general copy."""
import numpy as np
import pytest

from dataplane_amd import GpuPathNf, _abi as A
from dataplane_amd.flows import FlowTable
from dataplane_amd.workload import Workload
from oracle.pyoracle import Oracle, OracleFlows

from flowgen import frames_of, install, scenario
from helpers import common_fields, compare, hist
from placement import PLACEMENTS, Corpus, check_delivered, pack_at, relaid, wave_fit
from test_gpu_flows import _ref_map, run_device

pytestmark = pytest.mark.gpu

DELIVERED = A.DONE["Delivered"]


@pytest.fixture(scope="module")
def nf():
    # torch (plumbing for the device and pinned-memory tests) bundles its own
    # HIP runtime; it must initialise before libdpgpu's runtime claims the device
    import torch
    torch.cuda.init()
    n = GpuPathNf(0)
    yield n
    n.attach_flows(None)
    n.close()


@pytest.fixture(scope="module")
def corpus():
    return Corpus()


def run_arrays(nf, buf, inp, o_ref):
    """process_arrays with meta and stats on a copy of `buf`: (records, buffer)."""
    b = buf.copy()
    stats = np.zeros(A.DONE_COUNT, dtype=np.uint64)
    o = nf.process_arrays(b, inp, stats)
    assert int(stats.sum()) == len(inp)
    assert int(stats[DELIVERED]) == hist(o_ref).get("Delivered", 0)
    return o, b


@pytest.mark.parametrize("place,form", [("mod16", "bv"), ("odd", "list"), ("lone_odd", "bv"),
                                        ("x7", "list")])
def test_gpu_edge_placed(nf, corpus, place, form, cls_form):
    """The edge corpus (malformed / boundary frames, every table branch) under
    each placement; every wave runs the general copy of process_packet."""
    cls_form(A.gpu_lib(), form)
    nf.publish(corpus.tables)
    buf, inp, o_ref, b_ref = corpus.reference("edge", place)
    assert hist(o_ref).get("Delivered", 0) >= 800
    o_dut, b_dut = run_arrays(nf, buf, inp, o_ref)
    compare(o_ref, b_ref, o_dut, b_dut, inp, f"edge {place} {form}")


@pytest.mark.parametrize("place", ["mod16", "x7"])
def test_gpu_sweep_placed(nf, corpus, place):
    """The length sweep: the frame end and the L4 header across the window
    edge at every shift, the checksum ladder on random payload.  Every packet
    is Delivered, and the GPU's own output frames carry checksums that verify
    in plain Python."""
    nf.publish(corpus.tables)
    buf, inp, o_ref, b_ref = corpus.reference("sweep", place)
    assert np.all(o_ref["done"] == DELIVERED), hist(o_ref)
    o_dut, b_dut = run_arrays(nf, buf, inp, o_ref)
    assert np.all(o_dut["done"] == DELIVERED), hist(o_dut)
    n_deliv, checked, bad = check_delivered(o_dut, b_dut, f"gpu sweep {place}")
    assert n_deliv == checked == len(inp) and not bad, "\n".join(bad[:10])
    compare(o_ref, b_ref, o_dut, b_dut, inp, f"sweep {place}")


@pytest.mark.parametrize("place,form", [("even", "bv"), ("even", "list"), ("lone_odd", "bv"),
                                        ("even_lone_odd", "list")])
def test_gpu_short_placed(nf, corpus, place, form, cls_form):
    """The all-in-window copy of process_packet at non-zero shifts, and the
    ballot that chooses it: edge and sweep frames of at most SHORT_MAX bytes.
    At even starts every wave is all-in-window, seven lanes in eight shifted;
    a lone odd lane sends every second wave to the general copy in the same
    launch.  Which waves fit is computed from the in-records and asserted."""
    cls_form(A.gpu_lib(), form)
    nf.publish(corpus.tables)
    buf, inp, o_ref, b_ref = corpus.reference("short", place)
    fit, shifted = wave_fit(inp)
    assert len(fit) > 50
    if place == "even":
        assert fit.all() and (shifted[:-1] == 56).all()
    else:
        assert np.array_equal(fit, np.arange(len(fit)) % 2 == 1)
        assert place == "lone_odd" or (shifted[:-1] >= 55).all()
    assert hist(o_ref).get("Delivered", 0) >= 800
    o_dut, b_dut = run_arrays(nf, buf, inp, o_ref)
    compare(o_ref, b_ref, o_dut, b_dut, inp, f"short {place} {form}")
    n = corpus.n_short_sweep                      # its well-formed part: all Delivered
    n_deliv, checked, bad = check_delivered(o_dut, b_dut, f"gpu short {place}", first=len(inp) - n)
    assert n_deliv == checked == n > 1000 and not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("place", ["mod16", "odd", "even"])
@pytest.mark.parametrize("cfg", [1, 3, 5])
def test_gpu_relaid_workload(nf, cfg, place):
    """Paths without encapsulation, and v6: Workload frames relaid.  C3 brings
    566- and 1514-byte frames with random payload onto odd starts through the
    general serializer; the 60- and 80-byte frames of C1 and C5 at even starts
    run the all-in-window copy and its straight-line serializer in every wave."""
    w = Workload(cfg, 3000, seed=100 + cfg, n_routes_v4=3000, n_routes_v6=1500, n_acl=400,
                 n_nat=48, tcp_percent=25)
    nf.publish(w.tables)
    buf, inp = relaid(w, PLACEMENTS[place], seed=cfg)
    fit, shifted = wave_fit(inp)
    assert fit.all() and (shifted[:-1] == 56).all() if place == "even" and cfg != 3 else not fit.any()
    b_ref = buf.copy()
    o_ref = Oracle(w.tables).process(b_ref, inp)
    o_dut, b_dut = run_arrays(nf, buf, inp, o_ref)
    n_deliv, checked, bad = check_delivered(o_dut, b_dut, f"gpu C{cfg} {place}")
    assert n_deliv > 300 and checked == n_deliv and not bad, "\n".join(bad[:10])
    compare(o_ref, b_ref, o_dut, b_dut, inp, f"C{cfg} relaid {place}")


def test_gpu_edge_placed_without_lds_context(nf, corpus):
    """The same through the units that read the context tables from HBM."""
    lib = A.gpu_lib()
    nf.publish(corpus.tables)
    buf, inp, o_ref, b_ref = corpus.reference("edge", "x7")
    lib.dpf_debug_no_ctx(1)
    try:
        o_dut, b_dut = run_arrays(nf, buf, inp, o_ref)
    finally:
        lib.dpf_debug_no_ctx(0)
    compare(o_ref, b_ref, o_dut, b_dut, inp, "edge x7 without LDS context")


def test_gpu_sweep_device_path(nf, corpus):
    """dp_process_burst_device on torch memory, on a caller stream, with
    dev_meta and dev_stats."""
    import torch
    nf.publish(corpus.tables)
    buf, inp, o_ref, b_ref = corpus.reference("sweep", "x7")
    n = len(inp)
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    db = torch.from_numpy(buf.copy()).to(dev)
    di = torch.from_numpy(inp.view(np.uint8).copy()).to(dev)
    do = torch.zeros(n * A.PKT_OUT.itemsize, dtype=torch.uint8, device=dev)
    dm = torch.zeros(n * A.PKT_META.itemsize, dtype=torch.uint8, device=dev)
    st = torch.zeros(A.DONE_COUNT, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    nf.process_device(db.data_ptr(), db.numel(), di.data_ptr(), do.data_ptr(), n, st.data_ptr(),
                      s.cuda_stream, dev_meta=dm.data_ptr())
    s.synchronize()
    o = A.join_results(do.cpu().numpy().view(A.PKT_OUT), dm.cpu().numpy().view(A.PKT_META))
    compare(o_ref, b_ref, o, db.cpu().numpy(), inp, "sweep x7 device path")
    st = st.cpu().numpy()
    assert int(st.sum()) == n and int(st[DELIVERED]) == n


def test_gpu_edge_host_paths(nf, corpus):
    """dp_process_burst in each host-path mode on pinned buffers, and staged
    on pageable memory: dp_stage_expand / dp_stage_collect and the host
    write-back work on 16-byte spans that do not start at the frame.  Same
    records and bytes each way."""
    import torch
    nf.publish(corpus.tables)
    buf, inp, o_ref, b_ref = corpus.reference("edge", "mod16")
    n = len(inp)

    def pinned(nbytes):
        return torch.empty(nbytes, dtype=torch.uint8).pin_memory().numpy()
    runs = {}
    for mode, m in (("copy", A.HOST_COPY), ("zero_copy", A.HOST_ZERO_COPY), ("auto", A.HOST_AUTO)):
        pb = pinned(buf.nbytes)
        pb[:] = buf
        pi = pinned(inp.nbytes).view(A.PKT_IN)
        pi[:] = inp
        po = pinned(n * A.PKT_OUT.itemsize).view(A.PKT_OUT)
        pm = pinned(n * A.PKT_META.itemsize).view(A.PKT_META)
        nf.set_host_path(m)
        try:
            o = nf.process_arrays(pb, pi, out=po, meta=pm)
        finally:
            nf.set_host_path(A.HOST_AUTO)
        compare(o_ref, b_ref, o, pb, inp, f"edge mod16 host path {mode}")
        runs[mode] = o.copy()
    b = buf.copy()
    o = nf.process_arrays(b, inp.copy())
    compare(o_ref, b_ref, o, b, inp, "edge mod16 pageable (staged)")
    runs["pageable"] = o
    for mode, o in runs.items():
        a, b = common_fields(o, runs["copy"])
        assert np.array_equal(a, b), f"records of {mode} differ from the staged copy's"


def test_gpu_edge_sharded(nf, corpus):
    """dp_process_burst_sharded over three contexts: with tight packing every
    shard after the first is rebased to the previous packet's end, an
    arbitrary and usually odd start."""
    import torch
    ndev = torch.cuda.device_count()
    tp = corpus.tables
    buf, inp, o_ref, b_ref = corpus.reference("edge", "odd")
    nfs = [GpuPathNf(k % ndev) for k in range(3)]
    try:
        for x in nfs:
            x.publish(tp)
        b_dut = buf.copy()
        stats = np.zeros(A.DONE_COUNT, dtype=np.uint64)
        o_dut = GpuPathNf.process_sharded(nfs, b_dut, inp.copy(), stats)
        compare(o_ref, b_ref, o_dut, b_dut, inp, "edge odd sharded")
        assert int(stats.sum()) == len(inp)
        assert int(stats[DELIVERED]) == hist(o_ref).get("Delivered", 0)
    finally:
        for x in nfs:
            x.close()


@pytest.mark.parametrize("place", ["mod16", "even"])
def test_gpu_flows_placed(nf, place):
    """The flows variant of the pipeline on unaligned frames: one scenario of
    tests/test_gpu_flows.py (its harness and flowgen, C2-shaped workload) laid
    out with pack_at in place of pack_burst; outputs, bytes, flow refs
    (matched through the flows they name) and flow states equal the oracle's.
    mod16: every wave runs the general copy; even: the 60-byte frames run the
    all-in-window copy of the flows instantiation in every wave."""
    w = Workload(2, 6000, seed=1, n_routes_v4=3000, n_acl=400, n_nat=24, tcp_percent=30)
    ora = Oracle(w.tables)
    o0 = ora.process(w.fresh_buf(), w.inp)
    items, burst = scenario(frames_of(w), o0["dst_vni"], genid=1, seed=1, n_flows=600,
                            vnis=sorted(set(int(v) for v in o0["dst_vni"] if v)))
    oft, gft = OracleFlows(), FlowTable(0, 1 << 13)
    orefs, grefs = install(oft, items), install(gft, items)
    g2o = _ref_map(grefs, orefs)
    buf, inp = pack_at([(f, 1, A.IN_SEEDED_OVERLAY, v) for f, v in burst], PLACEMENTS[place], seed=7)
    assert len(inp) <= 6600
    fit, shifted = wave_fit(inp)
    assert fit.all() and (shifted[:-1] == 56).all() if place == "even" else not fit.any()
    nf.publish(w.tables)
    nf.attach_flows(gft)
    try:
        obuf, gbuf = buf.copy(), buf.copy()
        oout, oref, ost = ora.process_flows(obuf, inp, oft, stats=True)
        gout, gref, gst = run_device(nf, gbuf, inp, stats=True)
        compare(oout, obuf, gout, gbuf, inp, f"flows {place}")
        mapped = np.array([g2o.get(int(r), A.FLOW_NONE) if int(r) != A.FLOW_NONE else A.FLOW_NONE
                           for r in gref], dtype=np.uint64)
        assert np.array_equal(mapped, oref), f"flow refs differ ({np.count_nonzero(mapped != oref)})"
        assert np.array_equal(gst, ost), "DoneReason histogram"
        assert int((oref != np.uint64(A.FLOW_NONE)).sum()) > 100, "few packets met a flow"
        assert int((oout["acl"] == 6).sum()) > 0, "no packet took the flow-scope reply path"
        gi, oi = gft.get(grefs), oft.get(orefs)
        assert np.array_equal(gi["ref"] == A.FLOW_NONE, oi["ref"] == A.FLOW_NONE)
        live = gi["ref"] != A.FLOW_NONE
        assert np.array_equal(gi["status"][live], oi["status"][live])
    finally:
        nf.attach_flows(None)
        gft.close()
