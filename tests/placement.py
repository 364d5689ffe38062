"""Frame placement for the parity tests: frames at any byte of the burst buffer.

dpgpu.h lets a frame start anywhere (dp_pkt_in_t.off is any offset with
DP_HEADROOM bytes in front; only the buffer base is 16-byte aligned), and the
pipeline kernel has code that depends on the start residue off & 15: the LDS
window shift, the wave's all-in-window ballot, 16-bit fields split between LDS
and HBM at the window edge, sum_frame's head / tail masks and its byte swap
for sums that start on an odd address, the write-back range.

``pack_at`` lays frames out at chosen residues, packed tightly, with every
byte that is not frame data random and non-zero, so a wrong write-back into
headroom or a gap shows in helpers.compare.  ``wave_fit`` evaluates the
kernel's all-in-window ballot on a burst's in-records, so a test can assert
which copy of process_packet its waves run: only a burst of short frames at
even starts ("short" under "even") reaches the all-in-window copy at a
non-zero shift.  ``length_sweep`` moves the end of
the frame and the L4 header across the window edge and walks sum_frame's
128 / 64 / 16 / 4-byte ladder on random payload.  ``verify_checksums`` checks
a serialized frame's checksums in plain Python, independent of the oracle.
"""
from __future__ import annotations

import random
import struct
import zlib

import numpy as np

from dataplane_amd import _abi as A
from oracle.pyoracle import Oracle
import pktgen as P
from edgecase import (FAST_PORTS, FAST_V4_DST, FAST_V4_SRC, edge_frames, edge_tables,
                      pack_burst)

# residue (frame start mod 16) of packet i; in the non-replay kernels a wave
# is 64 consecutive packets
PLACEMENTS = {
    "mod16": lambda i: i % 16,                              # every residue
    "odd": lambda i: (2 * i + 1) % 16,                      # only odd starts
    # one odd lane in every second wave: on a burst of short frames those
    # waves take the general copy of process_packet and the waves between the
    # all-in-window copy, in one launch (wave_fit says which; a burst with
    # frames longer than the window has no all-in-window wave at all)
    "lone_odd": lambda i: 9 if i % 128 == 17 else 0,
    "x7": lambda i: (7 * i) % 16,                           # a second mixing
    # only even starts: with frames of at most SHORT_MAX bytes every wave runs
    # the all-in-window copy, seven lanes in eight at a non-zero shift
    "even": lambda i: 2 * (i % 8),
    # the two together: all-in-window waves at non-zero shifts and general
    # waves in one launch
    "even_lone_odd": lambda i: 9 if i % 128 == 17 else 2 * (i % 8),
}

WIN = 96            # the kernel's LDS header window (DP_WIN)
SHORT_MAX = 80      # 14 (the largest even residue) + SHORT_MAX <= WIN


def wave_fit(inp):
    """The kernel's wave-uniform all_fit predicate from the in-records, per
    wave of 64 consecutive packets: (fit, shifted) -- fit[w]: every frame of
    wave w lies inside its window at an even address, so the wave runs the
    all-in-window copy of process_packet; shifted[w]: its lanes with a
    non-zero start residue."""
    off, ln = inp["off"].astype(np.int64), inp["len"].astype(np.int64)
    starts = np.arange(0, len(inp), 64)
    unfit = ((off & 15) + ln > WIN) | ((off & 1) == 1)
    return np.add.reduceat(unfit, starts) == 0, np.add.reduceat((off & 15) != 0, starts)


def pack_at(frames, residue_of, seed: int):
    """Lay `frames` ((frame, iif, flags, src_vni) tuples) out tightly: frame i
    starts at the lowest offset >= the previous frame's end + DP_HEADROOM that
    is congruent to residue_of(i) mod 16.  Every byte outside the frames
    (headroom, gaps, tail) is seeded random in 1..255.  Returns (buf, inp)."""
    offs, end = [], 0
    for i, (fr, *_) in enumerate(frames):
        lo = end + A.HEADROOM
        off = lo + (residue_of(i) - lo) % 16
        offs.append(off)
        end = off + len(fr)
    buf = np.random.default_rng(seed).integers(1, 256, size=(end + 15) & ~15, dtype=np.uint8)
    inp = np.zeros(len(frames), dtype=A.PKT_IN)
    for i, (fr, iif, flags, svni) in enumerate(frames):
        buf[offs[i]:offs[i] + len(fr)] = np.frombuffer(fr, dtype=np.uint8)
        inp[i] = (offs[i], len(fr), flags, iif, svni)
    return buf, inp


def relaid(w, residue_of, seed: int = 1):
    """The frames of a Workload packed through pack_at."""
    frames = [(bytes(w.buf[int(r["off"]):int(r["off"]) + int(r["len"])]), int(r["iif"]),
               int(r["flags"]), int(r["src_vni"])) for r in w.inp]
    return pack_at(frames, residue_of, seed)


# --------------------------------------------------------------------------
# length sweep

def _overlay_frame(tup, payload: bytes) -> tuple:
    src, dst, proto, sp, dp, vni = tup
    ps = P.pseudo4(src, dst, proto, (8 if proto == 17 else 20) + len(payload))
    body = P.udp(sp, dp, payload, ps) if proto == 17 else P.tcp(sp, dp, payload, ps)
    ip = P.ipv4(src, dst, proto, len(body), ttl=64)
    f = P.l2("02:00:00:00:aa:01", "02:00:00:00:bb:01", 0x0800) + ip + body
    return (f, 1, A.IN_SEEDED_OVERLAY, vni)


# payload lengths 0..130: the frame end and the L4 header cross window
# positions 80..111 at every shift.  Each (length, protocol) fills 16
# consecutive packet indices, which take all 16 residues under any placement
# that permutes the residues over 16 consecutive indices (mod16, x7).
SWEEP_SHORT = list(range(0, 131))
# the checksum ladder past the window (128 / 64 / 16 / 4-byte steps and tails)
# on random data, in blocks of five lengths laid out twice, five indices
# apart: residues r and r + 5 under mod16 (r and r + 3 under x7), the two
# copies with the two protocols.  1461..1463 fill the last block (every tail
# length mod 4 at a large size).
SWEEP_LONG = list(range(131, 300)) + [300 + 13 * k for k in range(95)] + [1460, 1464, 8950,
                                                                         1461, 1462, 1463]


def length_sweep(tables, seed: int = 5):
    """Valid overlay frames of VPCs 1010 / 1011 (edge_tables(); `tables` its
    built form), UDP and TCP over IPv4 with every payload byte random, over
    the payload lengths of SWEEP_SHORT and SWEEP_LONG.  Only (src, dst, proto,
    sport, dport, vni) tuples the oracle delivers for a 10-byte payload are
    used; the caller asserts that the oracle delivers every frame."""
    cand = [(s, d, p, sp, dp, v) for s in FAST_V4_SRC for d in FAST_V4_DST for p in (17, 6)
            for sp in FAST_PORTS[:3] for dp in FAST_PORTS[:3] for v in (1010, 1011)]
    buf, inp = pack_burst([_overlay_frame(t, bytes(range(10))) for t in cand])
    out = Oracle(tables).process(buf, inp)
    ok = {17: [], 6: []}
    for t, o in zip(cand, out):
        if o["done"] == A.DONE["Delivered"]:
            ok[t[2]].append(t)
    assert len(ok[17]) > 100 and len(ok[6]) > 100, "edge tables deliver too few tuples"
    r = random.Random(seed)
    turn = {17: 0, 6: 0}

    def frame(n, proto):
        turn[proto] += 1
        return _overlay_frame(ok[proto][turn[proto] % len(ok[proto])], r.randbytes(n))
    frames = []
    for n in SWEEP_SHORT:
        for proto in (17, 6):
            frames += [frame(n, proto) for _ in range(16)]
    assert len(SWEEP_LONG) % 5 == 0
    for b in range(0, len(SWEEP_LONG), 5):
        blk = SWEEP_LONG[b:b + 5]
        frames += [frame(n, (17, 6)[(b + k) % 2]) for k, n in enumerate(blk)]
        frames += [frame(n, (6, 17)[(b + k) % 2]) for k, n in enumerate(blk)]
    return frames


class Corpus:
    """The placement tests' bursts over edge_tables(), and their oracle runs:
    one instance per test module (a module-scoped fixture), every burst and
    every reference built on first use and then read-only.
    "edge": edge_frames(6000, 31); "sweep": length_sweep; "short": the frames
    of at most SHORT_MAX bytes of the edge corpus, then those of the sweep
    (the last n_short_sweep packets)."""

    def __init__(self):
        self.builder = edge_tables()
        self.tables = self.builder.build()
        self._frames, self._ref = {}, {}

    def frames(self, name: str):
        if name not in self._frames:
            if name == "edge":
                fr = edge_frames(6000, 31)
            elif name == "sweep":
                fr = length_sweep(self.tables)
            elif name == "short":
                fr = [f for f in self.frames("edge") + self.frames("sweep") if len(f[0]) <= SHORT_MAX]
            else:
                raise KeyError(name)
            self._frames[name] = fr
        return self._frames[name]

    @property
    def n_short_sweep(self) -> int:
        return sum(len(f) <= SHORT_MAX for f, *_ in self.frames("sweep"))

    def reference(self, name: str, place: str):
        """(buf, inp, oracle records, oracle buffer) of burst `name` under
        PLACEMENTS[place]."""
        if (name, place) not in self._ref:
            buf, inp = pack_at(self.frames(name), PLACEMENTS[place],
                               seed=zlib.crc32(f"{name}/{place}".encode()))
            b_ref = buf.copy()
            o_ref = Oracle(self.tables).process(b_ref, inp)
            for a in (buf, inp, o_ref, b_ref):
                a.flags.writeable = False
            self._ref[name, place] = buf, inp, o_ref, b_ref
        return self._ref[name, place]


# --------------------------------------------------------------------------
# RFC 1071 in plain Python

def _ones(*parts: bytes) -> int:
    """The folded one's-complement sum of the parts (each padded to 16 bits)."""
    return ~P.csum_fold(sum(P.sum16(p) for p in parts)) & 0xFFFF


def verify_checksums(frame: bytes):
    """Checks a serialized frame's checksums: a VXLAN outer stack (Ethernet,
    IPv4 or IPv6, UDP to port 4789, VXLAN) is skipped after its IPv4 header
    checksum; on the innermost IPv4 / IPv6 + UDP / TCP the IPv4 header must
    sum to 0xFFFF, and the L4 segment with its pseudo header must sum to
    0xFFFF.  Returns the list of failures (empty: all good), or None when the
    frame has no such innermost stack to check."""
    bad = []
    o = 0
    for depth in range(2):
        if len(frame) < o + 14:
            return None
        et = struct.unpack_from("!H", frame, o + 12)[0]
        o += 14
        while et in (0x8100, 0x88A8) and len(frame) >= o + 4:
            et = struct.unpack_from("!H", frame, o + 2)[0]
            o += 4
        if et == 0x0800:
            if len(frame) < o + 20:
                return None
            hl = (frame[o] & 0xF) * 4
            tl = struct.unpack_from("!H", frame, o + 2)[0]
            frag = struct.unpack_from("!H", frame, o + 6)[0] & 0x3FFF
            if hl < 20 or tl < hl or len(frame) < o + tl:
                return None
            if _ones(frame[o:o + hl]) != 0xFFFF:
                bad.append(f"IPv4 header checksum at {o}")
            proto, l4, l4len = frame[o + 9], o + hl, tl - hl
            pseudo = lambda: P.pseudo4(frame[o + 12:o + 16], frame[o + 16:o + 20], proto, l4len)  # noqa: E731
            if frag:
                return bad or None
        elif et == 0x86DD:
            if len(frame) < o + 40:
                return None
            proto, l4, l4len = frame[o + 6], o + 40, struct.unpack_from("!H", frame, o + 4)[0]
            if len(frame) < l4 + l4len:
                return None
            pseudo = lambda: P.pseudo6(frame[o + 8:o + 24], frame[o + 24:o + 40], proto, l4len)  # noqa: E731
        else:
            return None
        if proto == 17 and l4len >= 16 and depth == 0 and struct.unpack_from("!H", frame, l4 + 2)[0] == 4789:
            o = l4 + 16                                   # UDP + VXLAN; the inner Ethernet frame
            continue
        if proto == 17 and l4len >= 8:
            if et == 0x0800 and frame[l4 + 6:l4 + 8] == b"\0\0":
                return bad or None                        # no UDP checksum
        elif not (proto == 6 and l4len >= 20):
            return bad or None
        if _ones(pseudo(), frame[l4:l4 + l4len]) != 0xFFFF:
            bad.append(f"{'UDP' if proto == 17 else 'TCP'} checksum at {l4}")
        return bad
    return None


def check_delivered(out, buf, label: str = "", first: int = 0):
    """verify_checksums over every Delivered frame of a run, from packet
    `first` on: (Delivered, frames with an innermost stack that was checked,
    failures).  Meant for well-formed input: the edge corpus is malformed on
    purpose, and there the reference keeps or computes checksums RFC 1071 does
    not accept (a TCP segment summed to the end of a padded buffer; reserved
    TCP bits cleared under an encapsulation that leaves the inner checksum
    alone), which the comparison with the oracle pins instead."""
    checked, bad = 0, []
    deliv = first + np.nonzero(out["done"][first:] == A.DONE["Delivered"])[0]
    for i in deliv:
        o, n = int(out[i]["off"]), int(out[i]["len"])
        v = verify_checksums(bytes(buf[o:o + n]))
        if v is not None:
            checked += 1
            bad += [f"{label} packet {i}: {m}" for m in v]
    return len(deliv), checked, bad
