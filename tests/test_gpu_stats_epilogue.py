"""GPU: the DoneReason histogram of a device-resident burst, through every
non-flow unit and the flows variant: partial counters per launch (a ring of
part slots per context, handed from stream to stream by the in-flight
entries' completion events), summed into the caller's array and left zero.
The checker of every launch is the bincount of the same launch's out records,
which the parity tests pin to the oracle: integer counts, compared exactly.
(The file is named after a histogram epilogue inside the pipeline kernel that
was measured and not kept, DESIGN.md section 8: the sum is still
dp_stats_reduce.  Only the two-streams test probes what changed with it, the
part slots' hand-over; the others are regression cover that the earlier code
passes too.)"""
import numpy as np
import pytest

from dataplane_amd import GpuPathNf, _abi as A
from dataplane_amd.flows import FlowTable
from dataplane_amd.workload import Workload

pytestmark = pytest.mark.gpu

N = 20000
# one lane, a partial wave, a wave, a partial workgroup of either unit size
# (128 / 256 work-items), one and several workgroups, and more than 256 waves
# (the partial slots wrap)
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000, N]


@pytest.fixture(scope="module")
def nf():
    import torch
    torch.cuda.init()
    n = GpuPathNf(0)
    yield n
    n.attach_flows(None)
    n.close()


@pytest.fixture(scope="module")
def workloads():
    """C2- and C5-shaped bursts with small tables (C5: the v4 / v6 mix)."""
    return {2: Workload(2, N, seed=61, n_routes_v4=2000, n_acl=200, n_nat=32),
            5: Workload(5, N, seed=65, n_routes_v4=2000, n_routes_v6=2000, n_acl=200, n_nat=32)}


class Burst:
    """A workload resident on the device: launches of its first n packets,
    each on a pristine copy of the burst buffer with out records of its own."""

    def __init__(self, w):
        import torch
        self.torch, self.w = torch, w
        self.dev = torch.device("cuda", 0)
        self.pristine = torch.from_numpy(w.buf).to(self.dev)
        self.inp = torch.from_numpy(w.inp.view(np.uint8).copy()).to(self.dev)
        self.keep = []

    def stats(self):
        return self.torch.zeros(A.DONE_COUNT, dtype=self.torch.int64, device=self.dev)

    def prepare(self, n, meta=False):
        """Buffers of one launch (allocated and filled on the default stream:
        synchronise before a launch on another stream reads them)."""
        t = self.torch
        b = self.pristine.clone()
        o = t.full((n * A.PKT_OUT.itemsize,), 0xEE, dtype=t.uint8, device=self.dev)
        m = t.zeros(n * A.PKT_META.itemsize, dtype=t.uint8, device=self.dev) if meta else None
        self.keep.append((b, o, m))
        return b, o, m

    def launch(self, nf, bufs, n, st, stream=None):
        b, o, m = bufs
        nf.process_device(b.data_ptr(), b.numel(), self.inp.data_ptr(), o.data_ptr(), n,
                          st.data_ptr() if st is not None else None, stream,
                          dev_meta=m.data_ptr() if m is not None else None)
        return o


def counts(o):
    """The DoneReason bincount of a launch's out records."""
    done = o.cpu().numpy().view(A.PKT_OUT)["done"]
    assert done.max() < A.DONE_COUNT
    return np.bincount(done, minlength=A.DONE_COUNT).astype(np.uint64)


def host(st):
    return st.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("meta", [False, True], ids=["out", "out+meta"])
@pytest.mark.parametrize("no_ctx", [False, True], ids=["lds-context", "hbm-context"])
@pytest.mark.parametrize("cfg", [2, 5])
def test_histogram_equals_bincount(nf, workloads, cfg, no_ctx, meta):
    """Every size through every non-flow unit: C2 (parts 1 / 2, 256 work-items
    per workgroup), C5 (parts 7 / 8: v6 windows), and with the context tables
    read from HBM (dpf_debug_no_ctx: parts 11 / 12 and 13 / 14, 128
    work-items), without and with meta records."""
    import torch
    lib = A.gpu_lib()
    w = workloads[cfg]
    nf.publish(w.tables)
    d = Burst(w)
    lib.dpf_debug_no_ctx(1 if no_ctx else 0)
    try:
        runs = []
        for n in SIZES:
            st = d.stats()
            bufs = d.prepare(n, meta)
            torch.cuda.synchronize()
            runs.append((n, st, d.launch(nf, bufs, n, st)))
        nf.synchronize()
    finally:
        lib.dpf_debug_no_ctx(0)
    for n, st, o in runs:
        got = host(st)
        assert int(got.sum()) == n, f"n={n}: {got}"
        assert np.array_equal(got, counts(o)), f"n={n}"
    assert int(host(runs[-1][1])[A.DONE["Delivered"]]) > 0


def test_accumulates_and_resets_itself(nf, workloads):
    """stats is `+=`: five launches on one stream into one array give five
    bincounts (more launches than part slots: each slot is met again with its
    partials back at zero); a launch without a histogram in between
    changes nothing; a zeroed array afterwards holds exactly one bincount."""
    import torch
    w = workloads[2]
    nf.publish(w.tables)
    d = Burst(w)
    s = torch.cuda.Stream(d.dev)
    st = d.stats()
    five = [d.prepare(N) for _ in range(5)]
    quiet, after = d.prepare(1000), d.prepare(257)
    torch.cuda.synchronize()
    outs = [d.launch(nf, five[k], N, st, s.cuda_stream) for k in range(2)]
    d.launch(nf, quiet, 1000, None, s.cuda_stream)
    outs += [d.launch(nf, five[k], N, st, s.cuda_stream) for k in range(2, 5)]
    s.synchronize()
    one = counts(outs[0])
    for o in outs[1:]:
        assert np.array_equal(counts(o), one)
    assert np.array_equal(host(st), 5 * one)
    with torch.cuda.stream(s):
        st.zero_()
    o = d.launch(nf, after, 257, st, s.cuda_stream)
    s.synchronize()
    assert np.array_equal(host(st), counts(o)) and int(host(st).sum()) == 257


def test_two_streams_share_no_partials(nf, workloads):
    """Eight launches of one context on two streams in the order 0 1 1 0 1 0
    0 1, a histogram and a burst size per stream.  The context has four part
    slots, so launch k + 4 takes the slot of launch k, every time on the other
    stream; both streams are kept busy by fills queued in front, so launch k
    is still in flight then and the later launch has to wait for it
    (dpd_debug_part_waits counts exactly those four waits).  Each array is its
    own launches' sum."""
    import torch
    lib = A.gpu_lib()
    w = workloads[2]
    nf.publish(w.tables)
    d = Burst(w)
    streams = [torch.cuda.Stream(d.dev), torch.cuda.Stream(d.dev)]
    order = [0, 1, 1, 0, 1, 0, 0, 1]
    sizes = [N, 1000]
    sts = [d.stats(), d.stats()]
    bufs = [d.prepare(sizes[q]) for q in order]
    filler = [torch.empty(1 << 30, dtype=torch.uint8, device=d.dev) for _ in streams]
    torch.cuda.synchronize()
    waits = lib.dpd_debug_part_waits()
    for q, s in enumerate(streams):
        with torch.cuda.stream(s):
            for k in range(32):
                filler[q].fill_(k)
    outs = [d.launch(nf, bufs[k], sizes[q], sts[q], streams[q].cuda_stream) for k, q in enumerate(order)]
    waits = lib.dpd_debug_part_waits() - waits
    for s in streams:
        s.synchronize()
    assert waits == 4, f"{waits} launches waited for a slot's launch on the other stream"
    for q in range(2):
        want = sum(counts(outs[k]) for k in range(8) if order[k] == q)
        assert int(want.sum()) == 4 * sizes[q]
        assert np.array_equal(host(sts[q]), want), f"stream {q}"


def test_two_contexts_on_one_device(nf, workloads):
    """Interleaved launches of two contexts of one device, each on its own
    stream with its own histogram."""
    import torch
    w = workloads[2]
    nf2 = GpuPathNf(0)
    try:
        nf.publish(w.tables)
        nf2.publish(w.tables)
        d = Burst(w)
        ctxs, sizes = [nf, nf2], [N, 255]
        sts = [d.stats(), d.stats()]
        bufs = [d.prepare(sizes[k % 2]) for k in range(6)]
        torch.cuda.synchronize()
        outs = [d.launch(ctxs[k % 2], bufs[k], sizes[k % 2], sts[k % 2]) for k in range(6)]
        nf.synchronize()
        nf2.synchronize()
        for q in range(2):
            want = sum(counts(outs[k]) for k in range(q, 6, 2))
            assert np.array_equal(host(sts[q]), want), f"context {q}"
    finally:
        nf2.close()


def test_flows_variant_keeps_its_sum(nf, workloads):
    """With a flow table attached the partials are fed by the first pass and
    the replays and summed once by the reduce kernel: the histogram of one
    burst still sums to n and equals the bincount."""
    import torch
    w = workloads[2]
    nf.publish(w.tables)
    d = Burst(w)
    ft = FlowTable(0, 1 << 12)
    nf.attach_flows(ft)
    try:
        st = d.stats()
        bufs = d.prepare(N, meta=True)
        torch.cuda.synchronize()
        o = d.launch(nf, bufs, N, st)
        nf.synchronize()
    finally:
        nf.attach_flows(None)
        ft.close()
    assert int(host(st).sum()) == N
    assert np.array_equal(host(st), counts(o))
