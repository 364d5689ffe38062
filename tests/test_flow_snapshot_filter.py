"""The flow-table snapshot's filter (include/dpgpu.h "Flow-table snapshot") on
the host: dp_flow_filter_match against a plain restatement of each clause
(addresses as Python ints, prefixes by shifting) over seeded flows of both
families; the invalid filters; the records' sizes.  No GPU."""
import ipaddress

import numpy as np
import pytest

from dataplane_amd import _abi as A
from dataplane_amd.flows import NEVER, filter_match, flow_filter, flow_key

T = 5_000_000_000  # the EXPIRES_LE edge
V4, V6 = int(ipaddress.ip_address("10.1.2.3")), int(ipaddress.ip_address("2001:db8:1:2:3:4:5:6"))
NAT4, NAT6 = int(ipaddress.ip_address("70.71.72.73")), int(ipaddress.ip_address("2a00::77"))
PORTS = [1, 2, 1000, 1001, 65535]


def _inside(p, fam, addr) -> bool:
    if int(p["family"]) != fam:
        return False
    w = 32 if fam == 4 else 128
    a = int.from_bytes(bytes(addr[:w // 8]), "big")
    n = int.from_bytes(bytes(p["addr"][:w // 8]), "big")
    return a >> (w - int(p["len"])) == n >> (w - int(p["len"]))


def py_match(f, k, i) -> bool:
    """The filter's clauses restated over a FLOW_KEY / FLOW_INFO record."""
    has_pf, has_mq = int(i["pf"]) != 0, int(i["masq"]) != 0
    nat = has_pf * 1 | has_mq * 2 | (has_mq and int(i["masq_alloc"]) != 0) * 4
    fam, flags = int(k["family"]), int(i["flags"])
    tests = dict(
        SRC_VNI=lambda: k["src_vni"] == f["src_vni"], DST_VNI=lambda: i["dst_vni"] == f["dst_vni"],
        FAMILY=lambda: fam == f["family"], KIND=lambda: (int(f["kind_mask"]) >> int(k["kind"])) & 1,
        SRC=lambda: _inside(f["src"], fam, k["src"]), DST=lambda: _inside(f["dst"], fam, k["dst"]),
        SPORT=lambda: f["sport_lo"] <= k["sport"] <= f["sport_hi"],
        DPORT=lambda: f["dport_lo"] <= k["dport"] <= f["dport_hi"],
        STATUS=lambda: (int(f["status_mask"]) >> int(i["status"])) & 1,
        FLAGS_ALL=lambda: flags & int(f["flags_all"]) == int(f["flags_all"]),
        FLAGS_NONE=lambda: flags & int(f["flags_none"]) == 0,
        GENID_LT=lambda: i["genid"] < f["genid"], GENID_EQ=lambda: i["genid"] == f["genid"],
        EXPIRES_LE=lambda: i["expires_at"] <= f["expires_at"], NAT=lambda: nat & int(f["nat_mask"]),
        NAT_IP=lambda: nat and _inside(f["nat_ip"], int(i["pf_family"]), i["pf_ip"]),
        NAT_PORT=lambda: nat and f["nat_port_lo"] <= i["pf_port"] <= f["nat_port_hi"])
    return all(bool(t()) for n, t in tests.items() if int(f["clauses"]) & A.FLOWF[n])


def _near(rng, base, bits):
    """`base` with up to two bits flipped: every prefix length has addresses on both sides."""
    for _ in range(int(rng.integers(0, 3))):
        base ^= 1 << int(rng.integers(0, bits))
    return ipaddress.ip_address(base) if bits == 128 else ipaddress.IPv4Address(base)


def seeded_flows(n, seed, nat=True):
    """n distinct valid keys and an info each (status, flags, NAT state when `nat`)."""
    rng = np.random.default_rng(seed)
    keys, infos, seen = np.zeros(n, A.FLOW_KEY), np.zeros(n, A.FLOW_INFO), set()
    j = 0
    while j < n:
        v6 = bool(rng.integers(0, 2))
        kind = int(rng.integers(1, 5))
        sport = int(rng.choice(PORTS)) if kind < 4 else 0
        dport = int(rng.choice(PORTS)) if kind < 3 else 0
        k = flow_key(int(rng.choice([0, 7, 9])), _near(rng, V6 if v6 else V4, 128 if v6 else 32),
                     _near(rng, V6 + 9 if v6 else V4 + 9, 128 if v6 else 32), kind, sport, dport)
        if k.tobytes() in seen:
            continue
        seen.add(k.tobytes())
        i = infos[j]
        i["dst_vni"], i["flags"], i["genid"] = rng.choice([3, 4]), rng.integers(0, 8), rng.integers(0, 6)
        i["expires_at"] = rng.choice([T - 1, T, T + 1, NEVER])
        state = int(rng.integers(0, 4)) if nat else 0  # none, port forwarding, masquerade, + allocation
        i["status"] = rng.integers(0, 4)
        if state:
            i["pf" if state == 1 else "masq"], i["masq_alloc"] = rng.integers(1, 3), state == 3
            fam6 = bool(rng.integers(0, 2))
            i["pf_family"], i["pf_port"] = 6 if fam6 else 4, rng.choice(PORTS)
            ip = _near(rng, NAT6 if fam6 else NAT4, 128 if fam6 else 32).packed
            i["pf_ip"] = np.frombuffer(ip + bytes(16 - len(ip)), np.uint8)
        keys[j] = k
        j += 1
    return keys, infos


CASES = {"none": {}, "src_vni": dict(src_vni=7), "src_vni_none": dict(src_vni=0), "dst_vni": dict(dst_vni=4),
         "family4": dict(family=4), "family6": dict(family=6), "kind": dict(kind=[A.FLOW_TCP, A.FLOW_ICMP_QUERY]),
         "sport": dict(sport=(2, 1000)), "sport_one": dict(sport=65535), "dport": dict(dport=(1001, 65535)),
         "status": dict(status=[A.FLOW_CANCELLED, A.FLOW_DETACHED]), "status_active": dict(status=A.FLOW_ACTIVE),
         "flags_all": dict(flags_all=3), "flags_none": dict(flags_none=5),
         "genid_lt": dict(genid_lt=3), "genid_eq": dict(genid_eq=3), "expires_le": dict(expires_le=T),
         "nat_pf": dict(nat=A.FLOW_NAT_PF), "nat_alloc": dict(nat=A.FLOW_NAT_MASQ_ALLOC),
         "nat_masq_pf": dict(nat=A.FLOW_NAT_PF | A.FLOW_NAT_MASQ), "nat_port": dict(nat_port=(2, 1000)),
         "nat_ip4": dict(nat_ip=f"{ipaddress.ip_address(NAT4)}/31"), "nat_ip6": dict(nat_ip=f"{ipaddress.ip_address(NAT6)}/127"),
         "and_first": dict(family=4, kind=A.FLOW_TCP, dport=(2, 1001), flags_none=4, dst=f"{ipaddress.ip_address(V4 + 9)}/30"),
         "and_both": dict(src=f"{ipaddress.ip_address(V6)}/64", dst_vni=3, genid_lt=4, expires_le=T + 1),
         "nothing": dict(src_vni=7, family=6, src="10.0.0.0/8")}
CASES.update({f"src6_{n}": dict(src=f"{ipaddress.ip_address(V6)}/{n}") for n in (0, 1, 31, 32, 33, 127, 128)})
CASES.update({f"dst4_{n}": dict(dst=f"{ipaddress.ip_address(V4 + 9)}/{n}") for n in (0, 1, 31, 32)})
FLOWS = seeded_flows(400, 1)


@pytest.mark.parametrize("name", CASES)
def test_filter_match_against_restatement(name):
    f = flow_filter(**CASES[name])
    want = [py_match(f, k, i) for k, i in zip(*FLOWS)]
    got = [filter_match(f, k, i) for k, i in zip(*FLOWS)]
    assert got == want
    # the seeded set exercises both outcomes of every clause
    assert any(want) != (name == "nothing") and all(want) == (name == "none")


def test_no_filter_and_unset_fields():
    k, i = FLOWS[0][:1], FLOWS[1][:1]
    assert A.gpu_lib().dp_flow_filter_match(None, k.ctypes.data, i.ctypes.data) == 1
    f = flow_filter(family=int(k["family"][0]))
    f["src"]["family"], f["sport_lo"] = 9, 7  # fields of clauses that are not set
    assert filter_match(f, k, i)


@pytest.mark.parametrize("edit", [
    dict(clauses=1 << 17), dict(clauses=A.FLOWF["SRC"], src=(5, 8)), dict(clauses=A.FLOWF["DST"], dst=(4, 33)),
    dict(clauses=A.FLOWF["SRC"], src=(6, 129)), dict(clauses=A.FLOWF["NAT_IP"], nat_ip=(0, 0)),
    dict(clauses=A.FLOWF["SPORT"], sport_lo=2, sport_hi=1), dict(clauses=A.FLOWF["DPORT"], dport_lo=2, dport_hi=1),
    dict(clauses=A.FLOWF["NAT_PORT"], nat_port_lo=2, nat_port_hi=1)], ids=lambda e: "-".join(list(e)[1:]) or "clause")
def test_invalid_filters(edit):
    f = flow_filter()
    for name, v in edit.items():
        if isinstance(v, tuple):
            f[name]["family"], f[name]["len"] = v
        else:
            f[name] = v
    k, i = FLOWS[0][:1], FLOWS[1][:1]
    assert A.gpu_lib().dp_flow_filter_match(f.ctypes.data, k.ctypes.data, i.ctypes.data) == A.EINVAL
    assert A.gpu_lib().dp_flow_filter_match(None, None, i.ctypes.data) == A.EINVAL


def test_snapshot_record_layouts():
    lib = A.work_lib()
    assert A.FLOW_FILTER.itemsize == lib.dpw_sizeof(b"dp_flow_filter_t") == 112
    assert A.FLOW_ENTRY.itemsize == lib.dpw_sizeof(b"dp_flow_entry_t") == 136
    assert [A.FLOW_ENTRY.fields[n][1] for n in A.FLOW_ENTRY.names] == [0, 44, 48]
    assert [A.FLOW_FILTER.fields[n][1] for n in ("family", "flags_all", "sport_lo", "src", "nat_ip", "genid")] == \
        [12, 16, 24, 36, 76, 96]
    assert {"dp_flow_filter_match", "dp_flow_snapshot", "dp_flow_snapshot_device"} <= set(A.GPU_SYMBOLS)
    assert A.gpu_lib().dp_abi_version() == A.ABI_VERSION == 9
