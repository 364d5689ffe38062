"""CPU: frame placement (tests/placement.py) -- the kernel's per-packet code
compiled for the host against the oracle on frames at every start residue,
packed tightly with random fill, and the oracle's serialized frames against
plain-Python RFC 1071 checksums.  The emulation decides per packet whether a
frame lies in its window; the wave-level choice is the GPU suite's."""
import numpy as np
import pytest

from dataplane_amd import _abi as A
from dataplane_amd.workload import Workload
from oracle.pyoracle import Oracle
import pyemu

from helpers import compare, hist
from placement import (PLACEMENTS, SHORT_MAX, Corpus, check_delivered, pack_at, relaid,
                       verify_checksums, wave_fit)

DELIVERED = A.DONE["Delivered"]


@pytest.fixture(scope="module")
def corpus():
    return Corpus()


def test_pack_at_layout(corpus):
    """The packer itself: residues, tight packing, headroom, no zero fill."""
    edge = corpus.frames("edge")[:700]
    for name, res in PLACEMENTS.items():
        buf, inp = pack_at(edge, res, seed=3)
        off, ln = inp["off"].astype(np.int64), inp["len"].astype(np.int64)
        assert np.array_equal(off % 16, [res(i) for i in range(len(inp))]), name
        gap = off[1:] - (off[:-1] + ln[:-1])
        assert gap.min() >= A.HEADROOM and gap.max() < A.HEADROOM + 16 and off[0] >= A.HEADROOM
        assert len(buf) % 16 == 0 and 0 <= len(buf) - (off[-1] + ln[-1]) < 16
        fill = np.ones(len(buf), bool)
        for o, l, (fr, *_) in zip(off, ln, edge):
            assert bytes(buf[o:o + l]) == fr
            fill[o:o + l] = False
        assert buf[fill].min() >= 1
    assert {PLACEMENTS["odd"](i) for i in range(64)} == {1, 3, 5, 7, 9, 11, 13, 15}
    assert {PLACEMENTS["x7"](i) for i in range(16)} == set(range(16))
    assert {PLACEMENTS["even"](i) for i in range(8)} == {0, 2, 4, 6, 8, 10, 12, 14}
    assert [i for i in range(256) if PLACEMENTS["lone_odd"](i)] == [17, 145]
    assert [i for i in range(256) if PLACEMENTS["even_lone_odd"](i) & 1] == [17, 145]


def test_wave_fit_of_the_bursts(corpus):
    """Which copy of process_packet the waves of each burst run on the GPU:
    the edge corpus and the sweep hold frames longer than the window in every
    wave (general copy only); the short burst at even starts runs the
    all-in-window copy in every wave, at non-zero shifts; with a lone odd
    lane both kinds of wave alternate."""
    for name, place in (("edge", "mod16"), ("edge", "lone_odd"), ("sweep", "mod16"), ("sweep", "x7")):
        assert not wave_fit(corpus.reference(name, place)[1])[0].any(), (name, place)
    short = corpus.frames("short")
    assert len(short) > 3000 and max(len(f) for f, *_ in short) == SHORT_MAX
    fit, shifted = wave_fit(corpus.reference("short", "even")[1])
    assert len(fit) > 50 and fit.all() and (shifted[:-1] == 56).all()
    for place, shift_min in (("lone_odd", 0), ("even_lone_odd", 55)):
        fit, shifted = wave_fit(corpus.reference("short", place)[1])
        assert np.array_equal(fit, np.arange(len(fit)) % 2 == 1), place
        assert (shifted[:-1] >= shift_min).all()
    # the ballot's two terms, each alone
    inp = np.zeros(64, dtype=A.PKT_IN)
    inp["off"], inp["len"] = 96 + 14, 82
    assert wave_fit(inp)[0].all()
    inp["len"][5] = 83
    assert not wave_fit(inp)[0].any()
    inp["len"][5], inp["off"][63] = 82, 96 + 13
    assert not wave_fit(inp)[0].any()


def emu_against_reference(corpus, name, place, variant):
    buf, inp, o_ref, b_ref = corpus.reference(name, place)
    if name == "sweep":
        assert np.all(o_ref["done"] == DELIVERED), hist(o_ref)
    else:
        assert hist(o_ref).get("Delivered", 0) >= 800
    b_dut = buf.copy()
    o_dut = pyemu.process(corpus.tables, b_dut, inp, variant=variant)
    compare(o_ref, b_ref, o_dut, b_dut, inp, f"{name} {place} {variant}")


@pytest.mark.parametrize("variant", ["", "w32"])
@pytest.mark.parametrize("place", ["mod16", "odd", "lone_odd", "x7"])
def test_edge_placed_emu_matches_oracle(corpus, place, variant):
    emu_against_reference(corpus, "edge", place, variant)


@pytest.mark.parametrize("variant", ["", "w32"])
@pytest.mark.parametrize("place", ["mod16", "x7"])
def test_sweep_emu_matches_oracle(corpus, place, variant):
    emu_against_reference(corpus, "sweep", place, variant)


@pytest.mark.parametrize("variant", ["", "w32"])
@pytest.mark.parametrize("place", ["even", "lone_odd", "even_lone_odd"])
def test_short_placed_emu_matches_oracle(corpus, place, variant):
    """The guard of the GPU's all-in-window bursts (frames of at most
    SHORT_MAX bytes)."""
    emu_against_reference(corpus, "short", place, variant)
    _, _, o_ref, b_ref = corpus.reference("short", place)
    n = corpus.n_short_sweep                      # its well-formed part: all Delivered
    n_deliv, checked, bad = check_delivered(o_ref, b_ref, f"short {place}", first=len(o_ref) - n)
    assert n_deliv == checked == n > 1000 and not bad, "\n".join(bad[:10])


@pytest.mark.parametrize("place", ["mod16", "x7"])
def test_sweep_oracle_checksums(corpus, place):
    """The oracle delivers every frame of the sweep, encapsulated, many of
    them NAT-rewritten, and every checksum it wrote verifies in plain Python."""
    buf, inp, o_ref, b_ref = corpus.reference("sweep", place)
    assert np.all(o_ref["done"] == DELIVERED), hist(o_ref)
    assert np.all(o_ref["len"] == inp["len"] + 50), "VXLAN over IPv4 in front of every frame"
    nat = A.META["NATTED_SRC"] | A.META["NATTED_DST"]
    assert np.count_nonzero(o_ref["meta_flags"] & nat) > len(inp) // 2
    _, checked, bad = check_delivered(o_ref, b_ref, f"sweep {place}")
    assert checked == len(inp) and not bad, "\n".join(bad[:10])


def test_verify_checksums_sees_errors(corpus):
    """The checker itself: a flipped payload byte, a flipped address byte and
    a swapped pair of payload bytes at odd / even positions are all caught."""
    f = next(fr for fr, *_ in corpus.frames("sweep") if len(fr) > 80)
    assert verify_checksums(f) == []
    assert verify_checksums(f[:-1] + bytes([f[-1] ^ 1])) != []
    assert len(verify_checksums(f[:27] + bytes([f[27] ^ 0x10]) + f[28:])) == 2
    a, b = len(f) - 3, len(f) - 2
    if f[a] != f[b]:
        g = bytearray(f)
        g[a], g[b] = f[b], f[a]
        assert verify_checksums(bytes(g)) != []
    assert verify_checksums(b"\0" * 12 + b"\x08\x06" + bytes(28)) is None

@pytest.fixture(scope="module")
def relaid_ref():
    """(workload, buf, inp, oracle records, oracle buffer) of a relaid
    Workload, once per (cfg, place)."""
    cache = {}

    def get(cfg, place):
        if (cfg, place) not in cache:
            w = Workload(cfg, 3000, seed=100 + cfg, n_routes_v4=3000, n_routes_v6=1500, n_acl=400,
                         n_nat=48, tcp_percent=25)
            buf, inp = relaid(w, PLACEMENTS[place], seed=cfg)
            b_ref = buf.copy()
            o_ref = Oracle(w.tables).process(b_ref, inp)
            cache[cfg, place] = w, buf, inp, o_ref, b_ref
        return cache[cfg, place]
    return get


@pytest.mark.parametrize("variant", ["", "w32"])
@pytest.mark.parametrize("place", ["mod16", "odd", "even"])
@pytest.mark.parametrize("cfg", [1, 3, 5])
def test_relaid_workload_oracle_checksums(relaid_ref, cfg, place, variant):
    """Workload frames (no encapsulation; IMIX lengths on C3, v6 on C5) relaid:
    emulation against the oracle, and the oracle's own checksums verified in
    plain Python."""
    w, buf, inp, o_ref, b_ref = relaid_ref(cfg, place)
    b_dut = buf.copy()
    o_dut = pyemu.process(w.tables, b_dut, inp, variant=variant)
    compare(o_ref, b_ref, o_dut, b_dut, inp, f"C{cfg} relaid {place} {variant}")
    n_deliv, checked, bad = check_delivered(o_ref, b_ref, f"C{cfg}")
    assert n_deliv > 300 and checked == n_deliv and not bad, "\n".join(bad[:10])
