"""GPU: packet capture (include/dpgpu.h "Packet capture", the reference's
PacketDumper) against a plain Python restatement of its parse, filter and
packing rules over the same buffer and records: records, bytes, matched and
lost must be equal."""
import ctypes as C
import ipaddress
import struct

import numpy as np
import pytest

from dataplane_amd import GpuPathNf, _abi as A
from dataplane_amd.workload import Workload

pytestmark = pytest.mark.gpu
DELIVERED = A.DONE["Delivered"]
BIG = 1 << 23  # a capture buffer nothing here fills


@pytest.fixture(scope="module")
def nf():
    import torch
    torch.cuda.init()
    n = GpuPathNf(0)
    yield n
    n.close()


def be16(b, p):
    return b[p] << 8 | b[p + 1]


def view(fr):
    """(classes, family, src, dst, ports) of a frame: the filter's parse."""
    L, cls, fam, src, dst, ports, proto, l4 = len(fr), 0, 0, None, None, None, None, 0
    if L < 14:
        return cls, fam, src, dst, ports
    et, p = be16(fr, 12), 14
    for _ in range(2):
        if et in (0x8100, 0x88a8) and p + 4 <= L:
            et, p = be16(fr, p + 2), p + 4
    if et == 0x0800 and p + 20 <= L:
        ihl = fr[p] & 15
        if ihl >= 5 and p + 4 * ihl <= L:
            fam, src, dst, l4 = 4, fr[p + 12:p + 16], fr[p + 16:p + 20], p + 4 * ihl
            proto = None if be16(fr, p + 6) & 0x1fff else fr[p + 9]
    elif et == 0x86dd and p + 40 <= L:
        fam, src, dst, l4, proto = 6, fr[p + 8:p + 24], fr[p + 24:p + 40], p + 40, fr[p + 6]
        for _ in range(3):
            if proto in (0, 43, 60):
                if l4 + 2 > L:
                    proto = None
                    break
                proto, l4 = fr[l4], l4 + (fr[l4 + 1] + 1) * 8
            elif proto == 44:
                if l4 + 8 > L or be16(fr, l4 + 2) & 0xfff8:
                    proto = None
                    break
                proto, l4 = fr[l4], l4 + 8
            else:
                break
    cls |= A.CAPC_ICMP4 if (fam, proto) == (4, 1) else A.CAPC_ICMP6 if (fam, proto) == (6, 58) else 0
    if proto in (6, 17):
        cls |= A.CAPC_UDP if proto == 17 else A.CAPC_TCP
        if l4 + 4 <= L:
            ports = be16(fr, l4), be16(fr, l4 + 2)
            if proto == 17 and 4789 in ports:
                cls |= A.CAPC_VXLAN
    return cls, fam, src, dst, ports


def selects(f, fr, done, sv, dv):
    cls, fam, src, dst, ports = view(fr) if fr is not None else (0, 0, None, None, None)

    def inside(pfx, addr):
        bits = 32 if pfx["family"] == 4 else 128
        sh = bits - int(pfx["len"])
        return fam == pfx["family"] and \
            int.from_bytes(addr, "big") >> sh == int.from_bytes(bytes(pfx["addr"][:bits // 8]), "big") >> sh

    c = int(f["clauses"])
    return not (
        (c & A.CAPF_L4 and not cls & int(f["l4_mask"])) or (c & A.CAPF_SRC and not inside(f["src"], src)) or
        (c & A.CAPF_DST and not inside(f["dst"], dst)) or
        (c & A.CAPF_SPORT and not (ports and f["sport_lo"] <= ports[0] <= f["sport_hi"])) or
        (c & A.CAPF_DPORT and not (ports and f["dport_lo"] <= ports[1] <= f["dport_hi"])) or
        (c & A.CAPF_DONE and not (done < 64 and int(f["done_mask"]) >> done & 1)) or
        (c & A.CAPF_SRC_VNI and sv != f["src_vni"]) or (c & A.CAPF_DST_VNI and dv != f["dst_vni"]))


def reference(tap, buf, recs, meta, f, max_records, max_bytes, prior=None):
    """One launch by the header's rules, appended to `prior`: (records, bytes, matched, lost, burst)."""
    out, data, matched, lost, burst = prior or ([], bytearray(), 0, 0, 0)
    out, data, full, tx = list(out), bytearray(data), False, tap == A.CAP_TX
    for i, r in enumerate(recs):
        off, ln, done = int(r["off"]), int(r["len"]), int(r["done"]) if tx else A.DONE_NONE
        has = (done == DELIVERED if tx else off >= A.HEADROOM) and (off + ln + 15) & ~15 <= len(buf)
        sv, dv = (int(meta[i]["src_vni"]), int(meta[i]["dst_vni"])) if tx and meta is not None else (0, 0)
        if not selects(f, bytes(buf[off:off + ln]) if has else None, done, sv, dv):
            continue
        matched += 1
        caplen = min(ln, int(f["snaplen"]) or ln) if has else 0
        size = (caplen + 15) & ~15
        full = full or len(out) >= max_records or len(data) + size > max_bytes // 16 * 16
        if full:
            lost += 1
            continue
        out.append((len(data), burst, i, ln, caplen, tap, done, 0, sv, dv))
        data += bytes(buf[off:off + caplen]) + bytes(size - caplen)
    return out, data, matched, lost, burst + 1


def same(got, ref):
    recs, data, matched, lost = got
    assert (matched, lost) == (ref[2], ref[3])
    assert np.array_equal(recs, np.array(ref[0], dtype=A.CAP_REC))
    assert bytes(data) == bytes(ref[1])


def flt(l4=0, src=None, dst=None, sport=None, dport=None, done=None, src_vni=None, dst_vni=None, snaplen=0):
    """An A.CAP_FILTER record; a clause is set by giving its value."""
    f = np.zeros((), dtype=A.CAP_FILTER)
    f["l4_mask"], f["snaplen"], f["src_vni"], f["dst_vni"] = l4, snaplen, src_vni or 0, dst_vni or 0
    f["done_mask"] = sum(1 << A.DONE[d] for d in done or ())
    for name, p in (("src", src), ("dst", dst)):
        if p:
            net = ipaddress.ip_network(p)
            raw = net.network_address.packed
            f[name]["family"], f[name]["len"], f[name]["addr"][:len(raw)] = net.version, net.prefixlen, list(raw)
    for name, r in (("sport", sport), ("dport", dport)):
        if r:
            f[name + "_lo"], f[name + "_hi"] = r
    given = (l4, src, dst, sport, dport, done, src_vni, dst_vni)
    f["clauses"] = sum(1 << b for b, v in enumerate(given) if v)
    return f


# -- frames ------------------------------------------------------------------
def eth(et, payload, tags=()):
    return bytes(12) + b"".join(struct.pack(">HH", t, 7) for t in tags) + struct.pack(">H", et) + payload


def ip4(proto, payload, src="10.1.127.255", dst="10.2.0.1", ihl=5, frag=0):
    return struct.pack(">BBHHHBBH", 0x40 | ihl, 0, 4 * ihl + len(payload), 1, frag, 64, proto, 0) + \
        ipaddress.ip_address(src).packed + ipaddress.ip_address(dst).packed + bytes(4 * ihl - 20) + payload


def ip6(nh, payload, exts=(), src="2001:db8::1", dst="2001:db8::2", frag=0):
    kinds = list(exts) + [nh]
    chain = b"".join(struct.pack(">BBHI", kinds[i + 1], 0, frag, 0) if k == 44 else
                     bytes([kinds[i + 1], i & 1]) + bytes(6 + 8 * (i & 1)) for i, k in enumerate(exts))
    return struct.pack(">IHBB", 6 << 28, len(chain) + len(payload), kinds[0], 64) + \
        ipaddress.ip_address(src).packed + ipaddress.ip_address(dst).packed + chain + payload


def l4(sport, dport):
    return struct.pack(">HHHH", sport, dport, 16, 0) + bytes(8)


def pack(frames):
    """Frames into a burst buffer, frame i starting at residue i mod 16."""
    inp, cur = np.zeros(len(frames), dtype=A.PKT_IN), 0
    for i, fr in enumerate(frames):
        inp[i]["off"], inp[i]["len"] = ((cur + A.HEADROOM + 15) & ~15) + i % 16, len(fr)
        cur = int(inp[i]["off"]) + len(fr)
    buf = np.zeros((cur + 15) & ~15, dtype=np.uint8)
    for r, fr in zip(inp, frames):
        buf[r["off"]:r["off"] + r["len"]] = np.frombuffer(fr, dtype=np.uint8)
    return buf, inp


UDP = eth(0x0800, ip4(17, l4(1000, 53)))
FRAMES = {
    "v4_udp": UDP, "v4_tcp": eth(0x0800, ip4(6, l4(2000, 80), src="10.1.128.0", dst="10.2.0.2")),
    "v4_icmp": eth(0x0800, ip4(1, bytes(8))), "v6_udp": eth(0x86dd, ip6(17, l4(999, 2001))),
    "v6_udp_e1": eth(0x86dd, ip6(17, l4(1500, 81), exts=(0,), src="2001:db8::3")),
    "v6_udp_e3": eth(0x86dd, ip6(17, l4(2001, 52), exts=(0, 43, 60))),
    "v6_udp_e4": eth(0x86dd, ip6(17, l4(1000, 53), exts=(0, 43, 60, 0))),
    "v6_icmp6": eth(0x86dd, ip6(58, bytes(8))), "v4_frag": eth(0x0800, ip4(17, l4(1000, 53), frag=5)),
    "v6_frag0": eth(0x86dd, ip6(17, l4(1000, 53), exts=(44,))),
    "v6_frag": eth(0x86dd, ip6(17, l4(1000, 53), exts=(44,), frag=8)),
    "vlan1": eth(0x0800, ip4(17, l4(1000, 53)), tags=(0x8100,)),
    "vlan2": eth(0x0800, ip4(17, l4(1000, 53)), tags=(0x88a8, 0x8100)),
    "vlan3": eth(0x0800, ip4(17, l4(1000, 53)), tags=(0x88a8, 0x8100, 0x8100)),
    "ihl6": eth(0x0800, ip4(17, l4(1000, 53), ihl=6)), "vx_src": eth(0x0800, ip4(17, l4(4789, 9))),
    "vx_dst": eth(0x86dd, ip6(17, l4(9, 4789))), "arp": eth(0x0806, bytes(28)), "eth14": eth(0x0800, b""),
    "cut_ip": UDP[:24], "cut_ports": UDP[:36],
}
UDPS = {"v4_udp", "v6_udp", "v6_udp_e1", "v6_udp_e3", "v6_frag0", "vlan1", "vlan2", "ihl6", "vx_src", "vx_dst",
        "cut_ports"}
FILTERS = {  # name -> (filter, the frames it must select where that is written out by hand, else None)
    "any_traffic": (flt(), set(FRAMES)), "udp_only": (flt(l4=A.CAPC_UDP), UDPS),
    "vxlan_only": (flt(l4=A.CAPC_VXLAN), {"vx_src", "vx_dst"}),
    "vxlan_or_icmp": (flt(l4=A.CAPC_VXLAN | A.CAPC_ICMP4), {"vx_src", "vx_dst", "v4_icmp"}),
    "icmp_only": (flt(l4=A.CAPC_ICMP4), {"v4_icmp"}), "tcp": (flt(l4=A.CAPC_TCP), {"v4_tcp"}),
    "icmp6": (flt(l4=A.CAPC_ICMP6), {"v6_icmp6"}), "src4_0": (flt(src="0.0.0.0/0"), None),
    "src4_17": (flt(src="10.1.0.0/17"), None), "dst4_32": (flt(dst="10.2.0.2/32"), {"v4_tcp"}),
    "src6_0": (flt(src="::/0"), None), "src6_17": (flt(src="2001:8000::/17"), set()),
    "dst6_128": (flt(dst="2001:db8::2/128"), None), "src6_128": (flt(src="2001:db8::3/128"), {"v6_udp_e1"}),
    "sport": (flt(sport=(1000, 2000)), None), "dport": (flt(dport=(53, 80)), None),
    "four": (flt(l4=A.CAPC_UDP, src="10.1.0.0/17", sport=(1000, 1000), dport=(53, 53)),
             {"v4_udp", "vlan1", "vlan2", "ihl6"}),
}


def capture(nf, tap, buf, recs, meta, f, max_records=BIG // 32, max_bytes=BIG, launches=1, read=True):
    """`launches` launches of dp_capture_device into a fresh buffer (kept open with read=False)."""
    import torch
    dev = torch.device("cuda", 0)
    db, dr = torch.from_numpy(buf).to(dev), torch.from_numpy(recs.view(np.uint8)).to(dev)
    dm = torch.from_numpy(meta.view(np.uint8)).to(dev) if meta is not None else None
    torch.cuda.synchronize(dev)
    nf.capture_open(f, max_records, max_bytes)
    try:
        for _ in range(launches):
            nf.capture_device(tap, db.data_ptr(), db.numel(), dr.data_ptr(), dm.data_ptr() if dm is not None else None,
                              len(recs))
        return nf.capture_read() if read else None
    finally:
        if read:
            nf.capture_close()


@pytest.mark.parametrize("name", FILTERS)
def test_filter_truth_table(nf, name):
    f, expect = FILTERS[name]
    buf, inp = pack(list(FRAMES.values()))
    ref = reference(A.CAP_RX, buf, inp, None, f, BIG, BIG)
    if expect is not None:
        assert {list(FRAMES)[r[2]] for r in ref[0]} == expect
    assert name in ("any_traffic", "src6_17") or 0 < ref[2] < len(FRAMES)
    same(capture(nf, A.CAP_RX, buf, inp, None, f), ref)


def mix(n, pattern, seed):
    """n seeded frames of the packing lengths; the wanted ones carry destination port 7777."""
    rng = np.random.default_rng(seed)
    want = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "third": np.arange(n) % 3 == 0,
            "first": np.arange(n) == 0, "last": np.arange(n) == n - 1}[pattern]
    lens = rng.choice([14, 60, 64, 65, 590, 1514], n)
    if pattern != "all":  # (a 14-byte frame has no ports to be wanted by)
        lens[want & (lens == 14)] = 60
    body = rng.integers(0, 256, 1514, dtype=np.uint8).tobytes()
    frames = [(eth(0x0800, ip4(17, l4(5, 7777 if w else 5))) + body)[:L] for w, L in zip(want, lens)]
    return pack(frames)


# (n, snaplen, pattern): every value of each axis, not the product
PACKING = [(1, 0, "all"), (63, 1, "third"), (64, 16, "first"), (65, 17, "last"), (1023, 96, "none"),
           (1024, 2000, "all"), (1025, 0, "third"), (3 * 1024 + 17, 17, "all"), (3 * 1024 + 17, 96, "last"),
           (3 * 1024 + 17, 0, "third")]


@pytest.mark.parametrize("n,snap,pattern", PACKING)
def test_packing(nf, n, snap, pattern):
    buf, inp = mix(n, pattern, seed=n)
    f = flt(snaplen=snap) if pattern == "all" else flt(dport=(7777, 7777), snaplen=snap)
    same(capture(nf, A.CAP_RX, buf, inp, None, f), reference(A.CAP_RX, buf, inp, None, f, BIG, BIG))


@pytest.mark.parametrize("limit", ["records", "unit_short", "exact"])
def test_capacity_cut(nf, limit):
    n, k = 2 * 1024 + 300, 1500  # record k lies in the second tile
    buf, inp = mix(n, "all", seed=3)
    end = int(np.cumsum((inp["len"].astype(np.int64) + 15) // 16 * 16)[k])
    max_records, max_bytes = {"records": (k, BIG), "unit_short": (n, end - 16), "exact": (n, end)}[limit]
    ref = reference(A.CAP_RX, buf, inp, None, flt(), max_records, max_bytes)
    assert len(ref[0]) == (k + 1 if limit == "exact" else k) and ref[3] == n - len(ref[0])
    same(capture(nf, A.CAP_RX, buf, inp, None, flt(), max_records, max_bytes), ref)


def test_appends_enospc_reset_and_einval(nf):
    buf, inp = mix(700, "third", seed=5)
    f, ref = flt(dport=(7777, 7777), snaplen=96), None
    for _ in range(3):
        ref = reference(A.CAP_RX, buf, inp, None, f, BIG, BIG, ref)
    assert [r[1] for r in ref[0]][::len(ref[0]) // 3] == [0, 1, 2]
    capture(nf, A.CAP_RX, buf, inp, None, f, launches=3, read=False)
    try:
        nr, nb, small = C.c_uint32(0), C.c_uint64(0), np.zeros(3, dtype=A.CAP_REC)
        data = np.zeros(BIG, dtype=np.uint8)
        assert nf.lib.dp_capture_read(nf.ctx, small.ctypes.data, 3, data.ctypes.data, BIG, C.byref(nr), C.byref(nb),
                                      None, None, 1) == A.ENOSPC
        assert (nr.value, nb.value) == (len(ref[0]), len(ref[1]))  # the needed counts; nothing was reset
        same(nf.capture_read(reset=True), ref)
        same(nf.capture_read(), ([], b"", 0, 0))
        # the next launch is burst 0 again; a filter the tap cannot run is refused at launch
        import torch
        db, dr = torch.from_numpy(buf).cuda(), torch.from_numpy(inp.view(np.uint8)).cuda()
        torch.cuda.synchronize()
        args = (db.data_ptr(), db.numel(), dr.data_ptr(), None, len(inp), None)
        nf.capture_device(A.CAP_RX, *args)
        same(nf.capture_read(), reference(A.CAP_RX, buf, inp, None, f, BIG, BIG))
        nf.set_capture_filter(flt(done=["AclDropped"]))
        assert nf.lib.dp_capture_device(nf.ctx, A.CAP_RX, *args) == A.EINVAL
        nf.set_capture_filter(flt(src_vni=7))
        assert nf.lib.dp_capture_device(nf.ctx, A.CAP_TX, *args) == A.EINVAL  # a VNI clause without meta
    finally:
        nf.capture_close()


def path_burst(nf, w, taps, f):
    """The image's burst through process_device with `taps`; the buffer before
    and after, the records, and what the capture holds."""
    import torch
    dev, before = torch.device("cuda", 0), w.fresh_buf()
    db, di = torch.from_numpy(before).to(dev), torch.from_numpy(w.inp.view(np.uint8)).to(dev)
    do = torch.zeros(w.n * A.PKT_OUT.itemsize, dtype=torch.uint8, device=dev)
    dm = torch.zeros(w.n * A.PKT_META.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    nf.set_capture(taps)
    try:
        nf.process_device(db.data_ptr(), db.numel(), di.data_ptr(), do.data_ptr(), w.n, dev_meta=dm.data_ptr())
        got = nf.capture_read(reset=True) if f is not None else None
    finally:
        nf.set_capture(0)
    nf.synchronize()
    return before, db.cpu().numpy(), do.cpu().numpy().view(A.PKT_OUT), dm.cpu().numpy().view(A.PKT_META), got


@pytest.mark.parametrize("cfg", [2, 4, 5])  # (4: the VXLAN image, where vxlan_only has something to select)
def test_through_the_path(nf, cfg):
    filters = [flt(l4=A.CAPC_VXLAN), None, flt(snaplen=64)]
    w = Workload(cfg, 3000, seed=400 + cfg, n_routes_v4=3000, n_routes_v6=2000 if cfg == 5 else 0, n_acl=300,
                 n_nat=24, tcp_percent=25)
    nf.publish(w.tables)
    nf.capture_open(flt(), BIG // 32, BIG)
    try:
        # option 0: the burst records nothing
        before, after, out, meta, _ = path_burst(nf, w, 0, None)
        same(nf.capture_read(), ([], b"", 0, 0))
        dropped = meta["src_vni"][np.isin(out["done"], [A.DONE["AclDropped"], A.DONE["Filtered"]])]
        vni = int(dropped[0]) if len(dropped) else None
        filters[1] = flt(done=["AclDropped", "Filtered"], src_vni=vni)
        for f in filters:
            nf.set_capture_filter(f)
            got = path_burst(nf, w, A.CAP_TX, f)[4]
            ref = reference(A.CAP_TX, after, out, meta, f, BIG, BIG)
            assert ref[2] > 0 or (f is filters[0] and cfg != 4)
            same(got, ref)
        # both taps: the RX records (the frames as received) precede the TX records of the burst
        nf.set_capture_filter(filters[2])
        got = path_burst(nf, w, A.CAP_RX | A.CAP_TX, filters[2])[4]
        ref = reference(A.CAP_TX, after, out, meta, filters[2], BIG, BIG,
                        reference(A.CAP_RX, before, w.inp, None, filters[2], BIG, BIG))
        assert list(got[0]["tap"]) == [A.CAP_RX] * w.n + [A.CAP_TX] * w.n
        same(got, ref)
    finally:
        nf.capture_close()
    # no capture open: the option alone launches and records nothing
    path_burst(nf, w, A.CAP_TX, None)
    nf.capture_open(None, 16, 4096)
    same(nf.capture_read(), ([], b"", 0, 0))
    nf.capture_close()
