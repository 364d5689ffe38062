"""GPU: dp_flow_snapshot (the filtered, ordered scan of the flow table) against
the test's own bookkeeping: the flows it left in the table, filtered by the
restatement of tests/test_flow_snapshot_filter.py, with the infos
dp_flow_lookup gives.  Bit-exact, `ref` and `related` included."""
import functools

import numpy as np
import pytest

from dataplane_amd import _abi as A
from dataplane_amd.flows import FlowTable, flow_filter, flow_key, make_flow

from edgecase import pack_burst
from golden import masqkat, pfkat
from test_flow_snapshot_filter import CASES, T, py_match, seeded_flows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    # (torch's HIP runtime initialises before libdpgpu's claims the device)
    import torch
    torch.cuda.init()


def home_slot(key, mask):
    """dp_flow.h fkey_hash of a FLOW_KEY record, as a slot."""
    w = np.frombuffer(key.tobytes(), "<u4").tolist()
    w[2] = (w[2] & 0xffff) << 16 | w[2] >> 16
    h = 0x9e3779b97f4a7c15
    for x in w:
        h = ((h ^ x) * 0xff51afd7ed558ccd) & (2 ** 64 - 1)
        h ^= h >> 32
    h = (h * 0xc4ceb9fe1a85ec53) & (2 ** 64 - 1)
    return (h ^ h >> 29) & mask


def by_key(entries):
    kb = np.ascontiguousarray(entries["key"]).view(np.uint8).reshape(len(entries), A.FLOW_KEY.itemsize)
    return entries[np.lexsort(kb.T[::-1])]


def expected(ft, keys):
    """FLOW_ENTRY records of stored keys, from dp_flow_lookup."""
    e = np.zeros(len(keys), A.FLOW_ENTRY)
    e["key"], e["info"] = keys, ft.lookup(keys)
    assert (e["info"]["ref"] != A.FLOW_NONE).all()
    e["slot"] = e["info"]["ref"] & 0xffffffff
    return by_key(e)


def select(filt, entries):
    return entries[[py_match(filt, e["key"], e["info"]) for e in entries]] if len(entries) else entries


@functools.lru_cache(maxsize=None)
def world(slots):
    """A table about 40 % full of mixed flows, some paired, with flows in its
    first and last slot; then a sweep, tombstones, replacements and
    invalidations.  Returns the table and what it must hold."""
    ft = FlowTable(0, slots)
    keys, infos = seeded_flows(slots * 2 // 5, slots, nat=False)
    # two more whose home is the first and the last slot, stored first and never expiring
    probe, ends = flow_key(9, "10.1.2.3", "10.1.2.12", A.FLOW_UDP, 1, 53), []
    for s in (0, slots - 1):
        while home_slot(probe, slots - 1) != s:
            probe["sport"] += 1
        ends.append(make_flow(probe, 3, 0, 1))
        probe["sport"] += 1
    fl = np.zeros(len(keys), A.FLOW)
    for j in range(len(keys)):
        fl[j] = make_flow(keys[j], int(infos[j]["dst_vni"]), int(infos[j]["flags"]), int(infos[j]["genid"]),
                          int(infos[j]["expires_at"]))
    fl = np.concatenate([np.array(ends, A.FLOW), fl])
    ft.insert(fl[:2])
    ft.insert(fl[2:len(fl) - 40])
    for j in range(len(fl) - 40, len(fl), 2):  # pairs: exactly one initiator
        a, b = fl[j].copy(), fl[j + 1].copy()
        a["flags"], b["flags"] = a["flags"] | A.FLOW_INITIATOR, b["flags"] & 6
        ft.insert_pair(a, b)
    gone = fl["expires_at"] < T
    assert ft.sweep(T - 1) == gone.sum()            # Expired flows leave
    keep = np.flatnonzero(~gone)
    ft.remove(fl["key"][keep[5::10]])               # tombstones (never the two ends)
    keep = np.delete(keep, np.s_[5::10])
    again = fl[keep[3::50]].copy()                  # replacements
    again["genid"] = 5
    ft.insert(again)
    ft.invalidate(ft.lookup(fl["key"][keep[4::60]])["ref"])
    want = expected(ft, fl["key"][keep])
    assert {0, slots - 1} <= set(want["slot"].tolist())
    return ft, want


@pytest.mark.parametrize("slots", [1 << 10, 1 << 12])
def test_everything_and_counts(slots):
    ft, want = world(slots)
    got = ft.snapshot()
    assert (np.diff(got["slot"].astype(np.int64)) > 0).all()
    assert by_key(got).tobytes() == want.tobytes()
    ln, active = ft.count()
    assert ft.count_matching(None) == ln == len(want)
    assert ft.count_matching(flow_filter(status=A.FLOW_ACTIVE)) == active < ln
    empty = FlowTable(0, 64)
    assert len(empty.snapshot()) == 0 and empty.snapshot_page(None, 0, 8)[1:] == (64, 0)
    with pytest.raises(RuntimeError):
        empty.snapshot_page(None, 65, 1)


@pytest.mark.parametrize("name", CASES)
def test_clauses_on_the_device(name):
    ft, want = world(1 << 12)
    filt = flow_filter(**CASES[name])
    sel = select(filt, want)
    got = ft.snapshot(filt)
    assert by_key(got).tobytes() == sel.tobytes()
    assert ft.count_matching(filt) == len(sel)
    assert (len(sel) == 0) == (name == "nothing" or name.startswith("nat"))


@pytest.mark.parametrize("cap", [1, 63, 64, 65, -1, 0, -2], ids=lambda c: f"cap{c}")
def test_cursor_and_capacity(cap):
    ft, want = world(1 << 12)
    filt = flow_filter(family=6, genid_lt=5)
    whole = ft.snapshot(filt)
    assert len(whole) == len(select(filt, want)) > 130
    cap = cap if cap > 0 else len(whole) + cap + 1     # matches - 1, matches, matches + 1
    pages, cursor = [], 0
    while cursor < ft.slots:
        done = sum(len(p) for p in pages)
        page, cursor, matched = ft.snapshot_page(filt, cursor, cap)
        assert matched == len(whole) - done and len(page) == min(cap, matched)
        assert page.tobytes() == whole[done:done + cap].tobytes()
        assert cursor == (ft.slots if matched <= cap else int(page["slot"][-1]) + 1)
        pages.append(page)
    assert np.concatenate(pages).tobytes() == whole.tobytes()
    # from a cursor inside a 64-slot bitmap word: nothing before it
    mid = next(int(s) for s in whole["slot"] if s % 64 not in (0, 63) and s > 1024)
    page, cursor, matched = ft.snapshot_page(filt, mid, len(whole))
    assert page.tobytes() == whole[whole["slot"] >= mid].tobytes() and cursor == ft.slots


def test_device_form_equals_host_form():
    import torch
    ft, want = world(1 << 12)
    buf = torch.zeros((len(want) + 1) * A.FLOW_ENTRY.itemsize, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for off in (0, 8):  # records on even and on odd 8-byte units
        n, cursor, matched = ft.snapshot_page(None, 0, len(want), device_ptr=buf.data_ptr() + off)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()[off:off + n * A.FLOW_ENTRY.itemsize].view(A.FLOW_ENTRY)
        assert n == matched == len(want) and cursor == ft.slots
        assert got.tobytes() == ft.snapshot().tobytes()


@pytest.mark.parametrize("kind", ["portfw", "masq"])
def test_nat_clauses(kind):
    """One burst that creates a NAT pair; the NAT clauses over its two flows."""
    r = pfkat.GpuRunner()
    if kind == "portfw":
        r.publish(pfkat.world(pfkat.base_rules())())
        pkt = pfkat.tcp_fwd(pfkat.SYN)
    else:
        r.publish(masqkat.world("2vpcs", 1, masqkat.PEERS["2vpcs"]))
        pkt = masqkat.tcp_masq(pfkat.SYN)
    r.set_clock(pfkat.SEC)
    res = r.burst(*pack_burst([(pkt.frame, 1, A.IN_SEEDED_OVERLAY, pkt.vni)]))
    assert A.DONE_NAMES[res[0]["done"]] == "Delivered"
    ft = r.ft
    pair = ft.snapshot()
    assert len(pair) == 2 and by_key(pair).tobytes() == expected(ft, pair["key"]).tobytes()
    assert set(pair["info"]["related"]) == set(pair["info"]["ref"])
    cls = A.FLOW_NAT_PF if kind == "portfw" else A.FLOW_NAT_MASQ
    assert ft.snapshot(flow_filter(nat=cls)).tobytes() == pair.tobytes()
    assert len(ft.snapshot(flow_filter(nat=cls ^ 3))) == 0
    owners = ft.snapshot(flow_filter(nat=A.FLOW_NAT_MASQ_ALLOC))
    assert owners.tobytes() == pair[pair["info"]["masq_alloc"] == 1].tobytes()
    assert len(owners) == (kind == "masq") and all(owners["info"]["masq"] == A.PF_SRC_NAT)
    for e in pair:  # the flows that carry this flow's tuple, and none beside its address
        ip = int.from_bytes(bytes(e["info"]["pf_ip"][:4]), "big")
        filt = flow_filter(nat_ip=f"{ip >> 24}.{ip >> 16 & 255}.{ip >> 8 & 255}.{ip & 255}/32",
                           nat_port=int(e["info"]["pf_port"]))
        sel = select(filt, pair)
        assert len(sel) >= 1 and ft.snapshot(filt).tobytes() == sel.tobytes()
        beside = flow_filter(nat_ip=f"{(ip ^ 1) >> 24}.{(ip ^ 1) >> 16 & 255}.{(ip ^ 1) >> 8 & 255}.{(ip ^ 1) & 255}/32")
        assert len(select(beside, pair)) == ft.count_matching(beside) == 0
    r.close()
