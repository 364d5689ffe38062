/* SPDX-License-Identifier: Apache-2.0
 *
 * dpgpu.h -- C ABI of the MI355X (gfx950) per-burst packet path.
 *
 * This is the drop-in boundary for the reference's packet hot loop
 * (githedgehog/dataplane).  The reference composes the path from NetworkFunction
 * stages (pipeline/src/static_nf.rs:12-32) assembled in
 * dataplane/src/packet_processor/mod.rs:130-145:
 *
 *   Ingress -> IP-Forward-1 -> IcmpErrorHandler -> FlowLookup -> FlowFilter ->
 *   AclFilter -> StaticNat -> PortForwarder -> Masquerade -> IP-Forward-2 -> Egress
 *
 * followed by Packet::serialize (net/src/packet/mod.rs:363-374).  One call of
 * dp_process_burst*() runs that whole block for a burst, on the GPU.  The
 * FlowTable FlowLookup and IcmpErrorHandler consult is a device flow table
 * attached to the context (dp_ctx_attach_flow_table; none attached = an
 * empty table).  PortForwarder runs on the GPU over the
 * port-forwarding rules of the tables (dp_portfw_rule_t) and creates its flow
 * pairs in the attached flow table; Masquerade runs on the GPU over the
 * masquerade exposes (dp_masq_expose_t) with its port allocator as device
 * state of the attached flow table.  AclFilter's classifier is also callable
 * alone (dp_acl_classify: the batch Lookup of acl/src/dpdk/lookup.rs).
 *
 * A Rust `GpuPathNf: NetworkFunction` materialises the burst
 * exactly like FlowFilter::process does (flow-filter/src/lib.rs:357-362),
 * stages the frames + metadata into the buffers below, calls this ABI and
 * applies the returned DoneReason / metadata to each Packet.
 *
 * Conventions
 *  - Every function returns 0 on success or a negative errno value.  Per-packet
 *    failures are never status codes: they are DoneReason values in dp_pkt_out_t
 *    (net/src/packet/meta.rs:84-119).  A whole-burst failure marks every packet
 *    DP_DONE_INTERNAL_FAILURE, as the reference stages do for unreadable tables
 *    (dataplane/src/packet_processor/ipforward.rs:89-98).
 *  - Addresses, MACs and prefixes are in network byte order.
 *  - The library never retains caller memory past a call.
 *  - A context is used by one thread (one dp-worker); dp_tables_publish may be
 *    called from another thread (mgmt) and only swaps a pointer for bursts
 *    that start after it returns (left-right / ArcSwap semantics,
 *    routing/src/fib/fibtype.rs:323-392, flow-filter/src/context/mod.rs:40-90).
 */
#ifndef DPGPU_H
#define DPGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPGPU_ABI_VERSION 9u

/* Bytes every frame must have in front of it (its own scratch, owned by the
 * packet).  Output headers are written in place into this headroom: VXLAN
 * encap over an IPv6 underlay grows the frame by at most 14+40+8+8 = 70 B.
 * Mirrors TestBuffer's 96 B headroom (net/src/buffer/test_buffer.rs:45-50). */
#define DP_HEADROOM 96u

/* ------------------------------------------------------------------------ */
/* DoneReason, in the reference's declaration order (u8 ordinals),           */
/* net/src/packet/meta.rs:84-119.                                            */
/* ------------------------------------------------------------------------ */
enum dp_done_reason {
    DP_DONE_INTERNAL_FAILURE = 0,
    DP_DONE_INTERFACE_UNKNOWN = 1,
    DP_DONE_INTERFACE_DETACHED = 2,
    DP_DONE_INTERFACE_ADM_DOWN = 3,
    DP_DONE_INTERFACE_OPER_DOWN = 4,
    DP_DONE_INTERFACE_UNSUPPORTED = 5,
    DP_DONE_NOT_ETHERNET = 6,
    DP_DONE_UNHANDLED = 7,
    DP_DONE_MAC_NOT_FOR_US = 8,
    DP_DONE_INVALID_DST_MAC = 9,
    DP_DONE_MISSING_ETHER_TYPE = 10,
    DP_DONE_NOT_IP = 11,
    DP_DONE_ROUTE_FAILURE = 12,
    DP_DONE_ROUTE_DROP = 13,
    DP_DONE_HOP_LIMIT_EXCEEDED = 14,
    DP_DONE_MISS_L2_RESOLUTION = 15,
    DP_DONE_VXLAN_DECAP_FAILURE = 16,
    DP_DONE_VXLAN_ENCAP_FAILURE = 17,
    DP_DONE_FILTERED = 18,
    DP_DONE_ACL_DROPPED = 19,
    DP_DONE_NAT_OUT_OF_RESOURCES = 20,
    DP_DONE_FLOW_CAPACITY_EXCEEDED = 21,
    DP_DONE_NAT_UNSUPPORTED_PROTO = 22,
    DP_DONE_NAT_FAILURE = 23,
    DP_DONE_NAT_NOT_PORT_FORWARDED = 24,
    DP_DONE_MALFORMED = 25,
    DP_DONE_UNROUTABLE = 26,
    DP_DONE_INVALID_CHECKSUM = 27,
    DP_DONE_ICMP_ERROR_INCOMPLETE = 28,
    DP_DONE_INTERNAL_DROP = 29,
    DP_DONE_LOCAL = 30,
    DP_DONE_DELIVERED = 31,
    DP_DONE_DEPARSE_ERROR = 32,
    DP_DONE_NO_HEAD_ROOM = 33,
    DP_DONE_COUNT = 34,
    /* "not done": only ever seen if a stage sequence leaves a packet pending,
     * which the router pipeline never does (Egress always decides). */
    DP_DONE_NONE = 255
};

/* PacketMeta flags, bit-identical to MetaFlags (net/src/packet/meta.rs:121-136). */
enum dp_meta_flag {
    DP_META_INITIALIZED = 1u << 0,
    DP_META_IS_L2_BCAST = 1u << 1,
    DP_META_NATTED_SRC = 1u << 2,
    DP_META_NATTED_DST = 1u << 3,
    DP_META_REFR_CHKSUM = 1u << 4,
    DP_META_KEEP = 1u << 5,
    DP_META_IS_OVERLAY = 1u << 6,
    DP_META_REQ_MASQUERADE = 1u << 7,
    DP_META_REQ_PORT_FORWARDING = 1u << 8,
    DP_META_REQ_STATIC_NAT_SRC = 1u << 9,
    DP_META_REQ_STATIC_NAT_DST = 1u << 10
};

/* ------------------------------------------------------------------------ */
/* Burst descriptors (SoA-friendly fixed-size records, 16 B in / 32 B out).  */
/* ------------------------------------------------------------------------ */

/* dp_pkt_in_t.flags */
enum dp_in_flag {
    /* Harness idiom of nat/src/static_nat/test.rs:285-296 and
     * flow-filter tests: the frame is the INNER frame of a VXLAN packet that
     * IP-Forward-1 has already decapsulated.  src_vni is the VNI it arrived
     * on; Ingress and IP-Forward-1 are skipped and the metadata is set exactly
     * as packet_exec_instruction_local sets it after a successful decap
     * (dataplane/src/packet_processor/ipforward.rs:140-161): src_vpcd=VNI,
     * vrf=fib(VNI).id, IS_OVERLAY; an unregistered VNI gives Unroutable. */
    DP_IN_SEEDED_OVERLAY = 1u << 0
};

typedef struct dp_pkt_in {
    uint32_t off;      /* frame start inside the burst buffer; >= DP_HEADROOM
                          bytes in front of it belong to this packet */
    uint16_t len;      /* frame length (mbuf data_len, FCS stripped) */
    uint16_t flags;    /* enum dp_in_flag */
    uint32_t iif;      /* PacketMeta.iif, set by the driver */
    uint32_t src_vni;  /* only with DP_IN_SEEDED_OVERLAY */
} dp_pkt_in_t;

/* What the driver needs to transmit or drop a packet (16 B, always written). */
typedef struct dp_pkt_out {
    uint32_t off;        /* serialized frame start (only valid if Delivered) */
    uint16_t len;        /* serialized frame length (only valid if Delivered) */
    uint8_t done;        /* enum dp_done_reason */
    uint8_t acl;         /* 0: ACL not consulted, 1: allow (rule), 2: deny (rule),
                            3: allow (peering default), 4: deny (peering default),
                            5: allow (no ACL for peering), 6: allow (reply of a
                            flow a Flow-scope rule allowed; acl_rule = that rule) */
    uint32_t oif;        /* PacketMeta.oif (0 if None) */
    uint16_t meta_flags; /* enum dp_meta_flag (MetaFlags, 11 bits) */
    uint16_t pad;
} dp_pkt_out_t;

/* dp_pkt_meta_t.pm_flags: which Option<> fields of PacketMeta are Some */
enum dp_pm_flag {
    DP_PM_HAS_VRF = 1u << 0,   /* vrf */
    DP_PM_HAS_NH = 1u << 1,    /* nh_addr */
    DP_PM_HAS_DSCP = 1u << 2   /* dscp and ecn (set together, ipforward.rs:143-148) */
};

/* The rest of PacketMeta (net/src/packet/meta.rs:138-154), 48 B, written
 * only when the caller passes a meta array: the fields a CPU stage kept
 * after the GPU block (PacketStatsNF, a dumper) would read.  The per-VPC
 * Stats stage reads src_vni / dst_vni on the device (DP_OPT_VPC_STATS below)
 * and needs no meta array on the host. */
typedef struct dp_pkt_meta {
    uint32_t dst_vni;    /* PacketMeta.dst_vpcd VNI (0 if None) */
    uint32_t src_vni;    /* PacketMeta.src_vpcd VNI (0 if None) */
    uint32_t fib_entry;  /* index of the last FibEntry executed (UINT32_MAX: none) */
    uint32_t acl_rule;   /* index of the matching ACL rule in its table (UINT32_MAX: none) */
    uint32_t vrf;        /* PacketMeta.vrf (DP_PM_HAS_VRF) */
    uint8_t pm_flags;    /* enum dp_pm_flag */
    uint8_t dscp;        /* PacketMeta.dscp (DP_PM_HAS_DSCP) */
    uint8_t ecn;         /* PacketMeta.ecn (DP_PM_HAS_DSCP) */
    uint8_t nh_family;   /* 4 / 6 (DP_PM_HAS_NH) */
    uint8_t nh_addr[16]; /* PacketMeta.nh_addr, network order (v4: first 4 bytes) */
    uint64_t flow_ref;   /* PacketMeta.flow_info as a flow-table ref (DP_FLOW_NONE: None) */
} dp_pkt_meta_t;

/* ------------------------------------------------------------------------ */
/* Table descriptors: host arrays lowered from the reference's structures.  */
/* ------------------------------------------------------------------------ */

typedef struct dp_ipaddr {
    uint8_t family;  /* 4 or 6 (0: none) */
    uint8_t pad[3];
    uint8_t addr[16]; /* v4 uses addr[0..4] */
} dp_ipaddr_t;

typedef struct dp_prefix {
    uint8_t family;  /* 4 or 6 */
    uint8_t len;     /* prefix length; host bits must be zero
                        (lpm/src/prefix/ip.rs:148-165) */
    uint8_t pad[2];
    uint8_t addr[16];
} dp_prefix_t;

/* FIB: routing/src/fib/fibtype.rs:54-61.  One per VRF. */
enum dp_fib_flag {
    DP_FIB_VTEP_HAS_IP = 1u << 0,
    DP_FIB_VTEP_HAS_MAC = 1u << 1
};
typedef struct dp_fib {
    uint32_t vrf_id;        /* FibKey::Id */
    uint32_t flags;         /* enum dp_fib_flag */
    dp_ipaddr_t vtep_ip;    /* Vtep (routing/src/evpn/vtep.rs:11-14) */
    uint8_t vtep_mac[6];
    uint8_t pad[2];
} dp_fib_t;

/* FibTable VNI registration (routing/src/fib/fibtable.rs:46-56). */
typedef struct dp_vni_fib {
    uint32_t vni;
    uint32_t fib;           /* index into fibs[] */
} dp_vni_fib_t;

/* PktInstruction (routing/src/fib/fibobjects.rs:258-264). */
enum dp_instr_kind {
    DP_INSTR_DROP = 0,
    DP_INSTR_LOCAL = 1,
    DP_INSTR_ENCAP_VXLAN = 2,
    DP_INSTR_EGRESS = 3
};
enum dp_instr_flag {
    DP_INSTR_HAS_IFINDEX = 1u << 0, /* EgressObject.ifindex is Some */
    DP_INSTR_HAS_ADDR = 1u << 1,    /* EgressObject.address is Some */
    DP_INSTR_HAS_DMAC = 1u << 2     /* VxlanEncapsulation.dmac is Some */
};
typedef struct dp_instr {
    uint32_t kind;          /* enum dp_instr_kind */
    uint32_t flags;         /* enum dp_instr_flag */
    uint32_t ifindex;       /* LOCAL / EGRESS */
    uint32_t vni;           /* ENCAP_VXLAN */
    dp_ipaddr_t addr;       /* EGRESS next-hop / ENCAP_VXLAN remote */
    uint8_t mac[6];         /* ENCAP_VXLAN dmac */
    uint8_t pad[2];
} dp_instr_t;

/* FibEntry = ordered instruction list (fibobjects.rs:142-144). */
typedef struct dp_fib_entry {
    uint32_t first_instr;
    uint32_t n_instr;       /* 1..4 */
} dp_fib_entry_t;

/* FibRoute = its FibGroups' entries, flattened in group order
 * (routing/src/fib/fibgroupstore.rs:195-234). */
typedef struct dp_route_nh {
    uint32_t first_entry;
    uint32_t n_entries;     /* >= 1; > 1 selects by packet_hash_ecmp */
} dp_route_nh_t;

typedef struct dp_route {
    dp_prefix_t prefix;
    uint32_t fib;           /* index into fibs[] */
    uint32_t nh;            /* index into route_nhs[] */
} dp_route_t;

/* Interface table (routing/src/interfaces/interface.rs). */
enum dp_if_state { DP_IF_UNKNOWN = 0, DP_IF_DOWN = 1, DP_IF_UP = 2 };
enum dp_if_type { DP_IFT_UNKNOWN = 0, DP_IFT_ETHERNET = 1, DP_IFT_DOT1Q = 2,
                  DP_IFT_LOOPBACK = 3, DP_IFT_VXLAN = 4 };
enum dp_if_attach { DP_ATTACH_NONE = 0, DP_ATTACH_VRF = 1, DP_ATTACH_BRIDGE = 2 };
typedef struct dp_iface {
    uint32_t ifindex;
    uint8_t admin_state;    /* enum dp_if_state */
    uint8_t oper_state;     /* enum dp_if_state */
    uint8_t iftype;         /* enum dp_if_type (Ethernet/Dot1q carry a MAC) */
    uint8_t attach;         /* enum dp_if_attach */
    uint32_t vrf_id;        /* Attachment::Vrf(fibkey) */
    uint8_t mac[6];
    uint8_t pad[2];
} dp_iface_t;

/* Adjacency table, keyed (ifindex, ip) (routing/src/atable/adjacency.rs:51-82). */
typedef struct dp_adjacency {
    dp_ipaddr_t addr;
    uint32_t ifindex;
    uint8_t mac[6];
    uint8_t pad[2];
} dp_adjacency_t;

/* Classifier rule: the union of the reference's three MatchKeys
 *   AclKey    (acl-filter/src/context.rs:168-190)
 *   RemoteKey (flow-filter/src/context/tables.rs:192-207)
 *   LocalKey  (flow-filter/src/context/tables.rs:211-229)
 * with match-action predicate semantics (match-action/src/predicate.rs):
 * proto = Mask, vni_a/vni_b/gate = Exact, src/dst = Prefix, ports = Range
 * (inclusive).  Unused fields are wildcards (prefix len 0, range 0..65535).
 *   ACL:       vni_a=src_vni, vni_b=dst_vni, gate=0
 *   FF remote: vni_a=src_vni, vni_b=GateVni (0 = ungated), src wildcard,
 *              sport wildcard
 *   FF local:  vni_a=src_vni, vni_b=dst_vni, gate=SourceGate, dst wildcard,
 *              dport wildcard */
typedef struct dp_rule {
    uint8_t proto_val;
    uint8_t proto_mask;     /* 0xff exact, 0x00 any */
    uint8_t family;         /* 4 or 6: which table */
    uint8_t gate;
    uint32_t vni_a;
    uint32_t vni_b;
    uint16_t sport_lo, sport_hi;
    uint16_t dport_lo, dport_hi;
    uint32_t priority;      /* flow-filter only: rule_priority(); tables are
                               matched in stable descending-priority order
                               (flow-filter/src/context/tables.rs:373-380);
                               ACL tables match in array order (first match,
                               acl-filter/src/context.rs:447-452) */
    dp_prefix_t src;
    dp_prefix_t dst;
    uint32_t action;        /* ACL: 0 Allow / 1 Deny.  FF remote: dst VNI.
                               FF local: enum dp_nat_mode (source NAT mode). */
    uint32_t action2;       /* FF remote: enum dp_nat_mode (destination NAT).
                               ACL: enum dp_acl_scope */
} dp_rule_t;

enum dp_acl_action { DP_ACL_ALLOW = 0, DP_ACL_DENY = 1 };
/* AclScope (config/src/external/overlay/acl.rs:137-141; Flow is the default):
 * a Flow-scope Allow also admits replies of a flow it allowed
 * (acl-filter/src/lib.rs:110-128). */
enum dp_acl_scope { DP_ACL_SCOPE_FLOW = 0, DP_ACL_SCOPE_PACKET = 1 };
/* NatRequirement (flow-filter/src/lib.rs NatMode = Option<NatRequirement>). */
enum dp_nat_mode { DP_NAT_NONE = 0, DP_NAT_STATIC = 1, DP_NAT_MASQUERADE = 2,
                   DP_NAT_PORT_FORWARDING = 3 };

/* Per-peering ACL default (acl-filter/src/context.rs:564-566). */
typedef struct dp_acl_default {
    uint32_t src_vni;
    uint32_t dst_vni;
    uint32_t action;        /* enum dp_acl_action */
} dp_acl_default_t;

/* Static NAT tables (nat/src/static_nat/setup/tables.rs), NAT44.
 * NatTables: src_vni -> PerVniTable{ dst_nat, src_nat[dst_vni] }. */
enum dp_nat_table_kind { DP_NAT_TABLE_DST = 0, DP_NAT_TABLE_SRC = 1 };
typedef struct dp_nat_table {
    uint32_t kind;          /* enum dp_nat_table_kind */
    uint32_t src_vni;       /* owning PerVniTable */
    uint32_t dst_vni;       /* DP_NAT_TABLE_SRC only: src_nat key */
    uint32_t first_entry;
    uint32_t n_entries;
} dp_nat_table_t;

/* One IpPortPrefixTrie entry: prefix -> NatTableValue. */
typedef struct dp_nat_entry {
    dp_prefix_t prefix;
    uint32_t is_pat;        /* NatTableValue::Pat (else ::Nat) */
    uint32_t first_port_range, n_port_ranges; /* Pat: prefix_port_ranges */
    uint32_t first_range, n_ranges;           /* ranges_tree, sorted by key */
    uint32_t pad;
    uint64_t size;          /* Nat: ip_len(); Pat: size() (ips x ports) */
} dp_nat_entry_t;

typedef struct dp_port_range {
    uint16_t lo, hi;        /* inclusive */
} dp_port_range_t;

/* ranges_tree element.  Nat:  key IpRange [orig_lo_ip, orig_hi_ip] ->
 * (target IpRange, offset).  Pat: key IpPortRangeBounds
 * [(orig_lo_ip,orig_lo_port), (orig_hi_ip,orig_hi_port)] ->
 * (IpPortRange{target ip range, target port range}, offset). */
typedef struct dp_nat_range {
    uint8_t orig_lo_ip[4];
    uint8_t orig_hi_ip[4];
    uint16_t orig_lo_port, orig_hi_port;
    uint8_t tgt_lo_ip[4];
    uint8_t tgt_hi_ip[4];
    uint16_t tgt_lo_port, tgt_hi_port;
    uint64_t offset;
} dp_nat_range_t;

/* Port-forwarding rule: PortFwEntry (nat/src/portfw/portfwtable/objects.rs:
 * 30-39, checks of PortFwEntry::new :70-155).  A publish applies the rule set
 * as PortFwTable::update does (:284-300): a rule that `matches` one of the
 * previous generation on the same device (same key, prefixes, port ranges and
 * destination VPC) is that same entry -- flows that refer to it stay valid
 * (their Weak upgrades) and only its timeouts change; rules no longer present
 * are gone; a new rule whose external range overlaps another of the same key
 * and external prefix is skipped (RangeSet overlap error, logged by the
 * reference).  Each entry has an id (dp_flow_info_t.pf_rule), stable while it
 * lives. */
typedef struct dp_portfw_rule {
    uint32_t src_vni;          /* PortFwKey.src_vpcd */
    uint8_t proto;             /* PortFwKey.proto: 6 (TCP) or 17 (UDP) */
    uint8_t pad[3];
    uint32_t dst_vni;          /* dst_vpcd (!= src_vni) */
    uint16_t ext_lo, ext_hi;   /* ext_ports: non-zero, ext_lo <= ext_hi */
    uint16_t int_lo, int_hi;   /* int_ports: same length */
    uint32_t init_timeout_s;   /* 0: PortFwEntry::DEFAULT_INITIAL_TOUT (10 s) */
    uint32_t estab_timeout_s;  /* 0: 30 min (TCP) / 30 s (UDP) */
    dp_prefix_t ext_prefix;    /* external prefix (what the client addresses) */
    dp_prefix_t int_prefix;    /* internal prefix (same family and length) */
} dp_portfw_rule_t;

/* Masquerade (stateful source NAT, nat/src/masquerade/).  One record per
 * masquerade expose of a stateful-NAT peering, in configuration order
 * (MasqueradeConfig::new, nat/src/masquerade/allocator_writer.rs:43-61;
 * gather_exposes, apalloc/setup.rs:95-137): the VPC whose private sources are
 * masqueraded towards the peer VPC, the expose's private prefixes (ips()),
 * its public ranges (as_range, the pools), its idle timeout, and the public
 * tuples the port-forwarding exposes of the same local manifest may claim
 * (claims_for, setup.rs:73-92), which the pools never hand out
 * (apalloc/reserved.rs).  An expose is one address family: its private and
 * public prefixes are all v4 (NAT44) or all v6 (NAT66).  Ports come in
 * bitmap order within a port block and addresses lowest first; the blocks of
 * an address come in index order (MasqueradeConfig::set_randomize(false), the
 * mode the reference's collision test runs, nat/src/masquerade/test.rs:
 * 1399-1406) or, with dp_tables_desc_t.masq_randomize, in a shuffled order
 * (the default, allocator_writer.rs:58; mgmt sets it, proc.rs:541): when an
 * address is put to use, its 256 blocks are permuted (PortAllocator::new,
 * port_alloc.rs:105-113).  The permutation is a function of masq_seed and
 * the address, so the device and any restatement agree:
 *   splitmix64(z): z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *                  z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31
 *   x = masq_seed; for each 32-bit word w of the address as a 128-bit number,
 *   most significant first (v4: three zero words, then the address):
 *   x = splitmix64(x ^ w); perm = 0..255; for i = 255 down to 1:
 *   x = splitmix64(x); swap(perm[i], perm[x % (i + 1)])
 * and block i of the address covers ports [256 perm[i], 256 perm[i] + 255]. */
typedef struct dp_masq_expose {
    uint32_t src_vni;          /* MasqueradePeering.src_vpcd */
    uint32_t dst_vni;          /* MasqueradePeering.dst_vpcd */
    uint32_t idle_timeout_s;   /* expose idle_timeout (0: 120 s, setup.rs:25) */
    uint32_t first_prefix;     /* into masq_prefixes: n_private private prefixes,
                                  then n_public public ones */
    uint16_t n_private, n_public;
    uint32_t first_claim;      /* into masq_claims */
    uint32_t n_claims;
} dp_masq_expose_t;

/* A public (prefix, port range) a port-forwarding expose may claim, and the
 * L4 protocols of its rule (ExposeNat.proto). */
enum dp_masq_proto { DP_MASQ_TCP = 1u << 0, DP_MASQ_UDP = 1u << 1 };
typedef struct dp_masq_claim {
    dp_prefix_t prefix;
    uint16_t lo, hi;           /* inclusive */
    uint32_t protos;           /* enum dp_masq_proto */
} dp_masq_claim_t;

/* Addresses of one allocator region (a disjoint public range of one
 * protocol towards one peer VPC, apalloc/region.rs) that can be in use at
 * once: the region's lowest DP_MASQ_REGION_ADDRS offsets (the reference's
 * u32 offset bitmap, alloc.rs:349-377, bounded for device memory; each
 * address carries 64512 TCP / UDP ports). */
#define DP_MASQ_REGION_ADDRS 4096u
/* Addresses in use at once over one flow table's allocator (each carries its
 * PortAllocator, ~9 KiB of device memory): a new address past this many fails
 * as the region's exhaustion does (NoFreeIp; NoPoolFound when reserving). */
#define DP_MASQ_ADDRS 65536u

typedef struct dp_tables_desc {
    uint32_t abi_version;   /* DPGPU_ABI_VERSION */
    uint32_t pad0;
    int64_t genid;          /* PipelineData.genid (pipeline/src/pipeline.rs:22-42) */

    const dp_fib_t *fibs;            uint32_t n_fibs;
    const dp_vni_fib_t *vni_fibs;    uint32_t n_vni_fibs;
    const dp_route_t *routes;        uint64_t n_routes;
    const dp_route_nh_t *route_nhs;  uint32_t n_route_nhs;
    const dp_fib_entry_t *entries;   uint32_t n_entries;
    const dp_instr_t *instrs;        uint32_t n_instrs;
    const dp_iface_t *ifaces;        uint32_t n_ifaces;
    const dp_adjacency_t *adjs;      uint32_t n_adjs;

    const dp_rule_t *acl_v4;         uint32_t n_acl_v4;
    const dp_rule_t *acl_v6;         uint32_t n_acl_v6;
    const dp_acl_default_t *acl_defaults; uint32_t n_acl_defaults;

    const dp_rule_t *ff_remote_v4;   uint32_t n_ff_remote_v4;
    const dp_rule_t *ff_local_v4;    uint32_t n_ff_local_v4;
    const dp_rule_t *ff_remote_v6;   uint32_t n_ff_remote_v6;
    const dp_rule_t *ff_local_v6;    uint32_t n_ff_local_v6;

    const dp_nat_table_t *nat_tables; uint32_t n_nat_tables;
    const dp_nat_entry_t *nat_entries; uint32_t n_nat_entries;
    const dp_port_range_t *nat_port_ranges; uint32_t n_nat_port_ranges;
    const dp_nat_range_t *nat_ranges; uint32_t n_nat_ranges;

    const dp_portfw_rule_t *portfw;  uint32_t n_portfw;

    /* masquerade (NatAllocatorWriter::update_nat_allocator,
     * allocator_writer.rs:120-154, applied to the attached flow tables) */
    const dp_masq_expose_t *masq;    uint32_t n_masq;
    const dp_prefix_t *masq_prefixes; uint32_t n_masq_prefixes;
    const dp_masq_claim_t *masq_claims; uint32_t n_masq_claims;
    /* MasqueradeConfig identity: two generations with the same non-zero tag
     * are the same configuration (the allocator and its flows are kept, only
     * the generation advances); 0: compared by the exposes and claims above */
    uint64_t masq_config_tag;
    /* MasqueradeConfig::set_randomize (dp_masq_expose_t above): 1 shuffles
     * each address's port blocks by masq_seed; part of the configuration's
     * identity (a change rebuilds the allocators) */
    uint32_t masq_randomize;
    uint32_t pad1;
    uint64_t masq_seed;
} dp_tables_desc_t;

/* ------------------------------------------------------------------------ */
/* Errors (negative errno).                                                  */
/* ------------------------------------------------------------------------ */
#define DP_OK 0
#define DP_EINVAL (-22)
#define DP_ENOMEM (-12)
#define DP_ENODEV (-19)
#define DP_ENOTSUP (-95)   /* a table form the path does not support */
#define DP_EIO (-5)        /* HIP runtime failure */
#define DP_ENOTABLES (-61) /* no tables published yet (ENODATA) */
#define DP_ENOSPC (-28)    /* the caller's array is too small */

/* ------------------------------------------------------------------------ */
/* Entry points.                                                             */
/* ------------------------------------------------------------------------ */
typedef struct dp_ctx dp_ctx_t;

/* Library / ABI version (for the FFI loader's sanity check). */
uint32_t dp_abi_version(void);

/* One context per worker thread (worker.rs:175 builds one pipeline per
 * worker); owns one HIP stream and the device-side staging scratch.  Tables
 * are shared by all contexts on the same device (refcounted image). */
/* DP_ENOTSUP: the process maps two HIP runtimes (two copies of
 * libamdhip64 / libhsa-runtime64 -- e.g. PyTorch's bundled one loaded after
 * this library's); one runtime per process is required (DESIGN.md §5,
 * INTEGRATION.md §6). */
int dp_ctx_create(int device_ordinal, dp_ctx_t **out);
int dp_ctx_destroy(dp_ctx_t *ctx);

/* Compile the lowered tables into the device image and publish it.
 * Replaces left-right FibWriter publish / NatTablesWriter::update_nat_tables /
 * FlowFilterContextWriter::store / AclFilterContextWriter::store
 *  for every context on the device.  Never blocks a burst
 * beyond a pointer swap; the old image is retired once bursts using it end.
 * The attached flow tables' masquerade allocators follow the new
 * configuration within the call; if one cannot (device memory), the call
 * still publishes the tables, updates every other flow table, and returns the
 * first error -- the failed table tries again at its next burst, and that
 * burst fails whole (DP_DONE_INTERNAL_FAILURE) while it cannot. */
int dp_tables_publish(dp_ctx_t *ctx, const dp_tables_desc_t *tables);

/* Current generation id (PipelineData::genid). */
int64_t dp_tables_genid(const dp_ctx_t *ctx);

/* Host-origin burst: `buf` is caller-owned (pinned for best speed) host
 * memory holding every frame at in[i].off with DP_HEADROOM bytes in front.
 * Frames are rewritten in place; out[i] tells where each serialized frame
 * now starts; `meta` (may be NULL) receives the rest of each PacketMeta.
 * Synchronous.  `stats` (may be NULL) receives DP_DONE_COUNT
 * counters (PacketStatsNF, pipeline/src/sample_nfs.rs:225-273).  On any
 * error (layout violation, HIP failure) every out[i] is
 * DP_DONE_INTERNAL_FAILURE and the negative status is returned. */
int dp_process_burst(dp_ctx_t *ctx, uint8_t *buf, uint64_t buf_bytes,
                     const dp_pkt_in_t *in, dp_pkt_out_t *out, dp_pkt_meta_t *meta,
                     uint32_t n, uint64_t *stats);

/* Device-resident burst: every pointer is device memory; enqueued on
 * `stream` (a hipStream_t; NULL = the context's stream).  Asynchronous.
 * `dev_buf` must be 16-byte aligned and `buf_bytes` must cover every frame
 * end rounded up to 16 bytes (frames are staged with 16-byte loads); a
 * packet violating the layout contract is marked DP_DONE_INTERNAL_FAILURE
 * without touching memory, and a burst that cannot run at all (no tables,
 * misaligned buffer, launch failure) has every dev_out[i] marked
 * DP_DONE_INTERNAL_FAILURE on `stream` besides the negative status.
 * `dev_meta` (may be NULL: the bench path writes only the 16-byte out
 * records) receives the rest of each PacketMeta, flow_info included.
 * `dev_stats` (may be NULL) is accumulated into (DP_DONE_COUNT u64).
 * Bursts of one context may run concurrently on different streams.  The
 * context tells streams apart by their handles (hipStreamPerThread is taken
 * as a different stream every time): a caller that destroys a stream while
 * one of the context's bursts with `dev_stats` is still running on it must
 * not hand the context a new stream before that burst has completed, since
 * the new handle may equal the old one. */
int dp_process_burst_device(dp_ctx_t *ctx, uint8_t *dev_buf, uint64_t buf_bytes,
                            const dp_pkt_in_t *dev_in, dp_pkt_out_t *dev_out,
                            dp_pkt_meta_t *dev_meta, uint32_t n, uint64_t *dev_stats,
                            void *stream);

/* Multi-GPU, host-origin burst: `ctxs` holds one
 * context per device (created by the caller, e.g. one per GPU of the node).
 * The burst -- laid out as for dp_process_burst, with packets in buffer
 * order and non-overlapping slots [off - DP_HEADROOM, off + len) -- is split
 * into n_ctx contiguous shards of whole packets (shard k: packets
 * [k n / n_ctx, (k+1) n / n_ctx)); each shard's byte span is copied to its
 * device with its own hipMemcpyAsync (every GPU has its own PCIe link, no
 * collective), processed there, and copied back.  Packets are independent,
 * so the result equals dp_process_burst on one device bit for bit
 * (tests/test_shard.py).  The analogue of the reference's per-worker fan-out
 * (dataplane/src/drivers/kernel/fanout.rs:49-73, worker.rs:175).
 * With a flow table: every context must be attached to the same one (else
 * DP_EINVAL) -- the reference's one Arc<FlowTable> shared by every worker --
 * and the shards are the workers' bursts, their flows launches run on the
 * table one after the other in shard order (one of the orders the
 * reference's concurrent workers may take): the result equals
 * dp_process_burst of each shard in turn on one context.  A flow table lives
 * on one device, so those contexts are contexts of one GPU.
 * Synchronous; `stats` (may be NULL) receives the summed DoneReason counts.
 * A whole-burst failure marks every packet DP_DONE_INTERNAL_FAILURE. */
int dp_process_burst_sharded(dp_ctx_t *const *ctxs, uint32_t n_ctx, uint8_t *buf,
                             uint64_t buf_bytes, const dp_pkt_in_t *in, dp_pkt_out_t *out,
                             dp_pkt_meta_t *meta, uint32_t n, uint64_t *stats);

/* Wait for the context's stream. */
int dp_ctx_synchronize(dp_ctx_t *ctx);

/* Context options (dp_ctx_set_option). */
enum dp_ctx_option {
    /* How dp_process_burst moves a host-origin burst:
     *   DP_HOST_AUTO      zero-copy when `buf`, `in` and `out` are all pinned,
     *                     device-mapped host memory (hipHostMalloc /
     *                     hipHostRegister) and `buf` is 16-byte aligned with
     *                     every frame end rounded up to 16 inside buf_bytes;
     *                     otherwise staged copies (default);
     *   DP_HOST_COPY      staged copies: each chunk's slot span and records
     *                     H2D, kernel, D2H, chunks overlapped on 3 streams;
     *   DP_HOST_ZERO_COPY zero-copy only: the kernel reads the frames and
     *                     records over PCIe and writes the rewritten header
     *                     spans and records back in place; a burst that does
     *                     not qualify fails with DP_EINVAL. */
    DP_OPT_HOST_PATH = 1,
    /* The flow clock (nanoseconds, the caller's clock -- the unit of
     * dp_flow_t.expires_at and dp_flow_sweep's `now`): Instant::now() for the
     * bursts that follow.  PortForwarder sets the expiry of the flows it
     * creates or refreshes to now + the rule's timeout
     * (flow_state.rs:233-263, flow_info.rs:399-407). */
    DP_OPT_CLOCK = 2,
    /* 1: every burst of the context (dp_process_burst, _device, _sharded,
     * dp_process_mbufs) is accounted into the context's per-VPC statistics
     * ("Per-VPC statistics" below) on the burst's stream, after the last
     * kernel that writes its records.  A burst without a meta array writes
     * its meta records into a context-owned device scratch array instead
     * (nothing more goes to the host); such bursts of one context on
     * different streams run one after the other.  A burst that fails whole
     * records nothing.  Where the records are pinned host memory (the
     * zero-copy host path, dp_process_mbufs) the stage reads them back over
     * PCIe: 16 B a packet, 24 B with a caller's meta array.
     * 0 (default): no launch, no allocation. */
    DP_OPT_VPC_STATS = 3,
    /* A mask of enum dp_cap_tap ("Packet capture" below): while a capture is
     * open, every dp_process_burst_device of the context runs the RX tap on
     * the burst's stream before the path and / or the TX tap after the last
     * kernel that writes the records, behind the Stats stage.  A tap the
     * filter cannot run on (DP_CAPF_DONE or a VNI clause on the RX tap) fails
     * the burst whole with DP_EINVAL; a TX tap with a VNI clause on a burst
     * without a meta array reads the context's meta scratch, as the Stats
     * stage does.  The host-origin entry points (dp_process_burst, _sharded,
     * dp_process_mbufs) ignore the option: their caller has the frames on the
     * host already.  0 (default), or no capture open: no launch, no
     * allocation. */
    DP_OPT_CAPTURE = 4,
    /* 1: dp_tables_publish through this context builds the tables of every
     * v4 FIB that takes the DIR-24-8 form (more than 65,536 v4 routes, next
     * hops below 0xffff) on the device: the host neither fills nor uploads
     * the 64 MiB direct table and the next-hop blocks, it uploads the rest of
     * the image and a compact route list (16 B a route), and two kernels on a
     * stream of the publish's own write the tables in place before the
     * generation is swapped in ("Publish statistics" below reports what ran).
     * The image -- layout and every byte -- is the host-built one, so the
     * lookups do not change; the other table forms, v6 and the classifiers
     * are host-built either way.  The publish takes 16 B a route of device
     * memory more until it returns.  A failure leaves the current generation
     * in place.
     * 2: as 1, and the device also sorts and lists such a FIB's routes (at
     * most 2^26 of them; a larger FIB is built as under 1).  The host neither
     * sorts them nor removes duplicate prefixes: it validates and packs them in
     * insertion order at 8 B a route (address, length, next hop), uploads
     * that, and kernels ahead of the two above sort the records stably by
     * (address, length), keep the last insert of a prefix and write the
     * route lists the build reads, which never leave the device.  The image
     * is still the host-built one byte for byte; the device's block count is
     * checked against the host's before anything is written (DP_EIO, nothing
     * published).  The publish takes at most 37 B a route of device memory
     * more until it returns (the records twice, 0.5 B of histograms, the
     * lists at up to 20 B).  dp_publish_stats_t.sorted_fibs counts these FIBs.
     * 0 (default): the host builds and uploads everything.  Another value is
     * DP_EINVAL. */
    DP_OPT_DEVICE_FIB = 5
};
enum dp_host_path { DP_HOST_AUTO = 0, DP_HOST_COPY = 1, DP_HOST_ZERO_COPY = 2 };
int dp_ctx_set_option(dp_ctx_t *ctx, int option, int64_t value);

/* ------------------------------------------------------------------------ */
/* The ACL classifier alone (the narrower drop-in for A14):   */
/* AclFilter's classification as a batch lookup -- the reference's           */
/* Lookup<K, A> / DpdkAclLookup::lookup_batch (lookup/src/lib.rs:24-38,      */
/* acl/src/dpdk/lookup.rs:112-155), an rte_acl replacement.  Each key is     */
/* matched against the ACL of its (source VPC, destination VPC) peering in   */
/* the published tables: the first rule in rule order whose prefixes, ports  */
/* and protocol hold it, else the peering's default, else Allow              */
/* (acl-filter/src/lib.rs:96-137, acl/src/reference/table.rs:94-101).        */
/* ------------------------------------------------------------------------ */
typedef struct dp_acl_key {
    uint32_t src_vni, dst_vni;  /* the peering */
    uint8_t family;             /* 4 or 6 */
    uint8_t proto;              /* IP next header */
    uint16_t sport, dport;      /* 0 for a protocol without ports */
    uint8_t pad[2];
    uint8_t src[16], dst[16];   /* network byte order; v4 in the first 4 bytes */
} dp_acl_key_t;                 /* 48 B */

typedef struct dp_acl_result {
    uint32_t rule;    /* index of the matching rule in the published acl_v4 / acl_v6,
                         UINT32_MAX when none matched */
    uint8_t action;   /* enum dp_acl_action the key gets */
    uint8_t scope;    /* enum dp_acl_scope of the matching rule (0 without one) */
    uint8_t acl;      /* dp_pkt_out_t.acl's code: 1 / 2 rule allow / deny, 3 / 4 peering
                         default allow / deny, 5 no ACL for the peering; 0: a key of
                         another family than 4 / 6 (not classified) */
    uint8_t pad;
} dp_acl_result_t;    /* 8 B */

/* Classify n keys resident on the context's device into dev_out (stream as in
 * dp_process_burst_device; asynchronous there). */
int dp_acl_classify_device(dp_ctx_t *ctx, const dp_acl_key_t *dev_keys, dp_acl_result_t *dev_out,
                           uint32_t n, void *stream);
/* The same for keys and results in host memory (synchronous). */
int dp_acl_classify(dp_ctx_t *ctx, const dp_acl_key_t *keys, dp_acl_result_t *out, uint32_t n);

/* The reference's own key bytes.  AclKey<Ipv4Addr> / AclKey<Ipv6Addr>
 * (acl-filter/src/context.rs:168-190) as MatchKey::as_key_into writes them
 * (match-action-derive/src/lib.rs:191-206, 341-347): its fields back to back,
 * each big-endian (net/src/fixed_size.rs: NextHeader 1 byte, Vni right-aligned
 * in 4) -- proto, src_vni, dst_vni, src address, dst address, src port, dst
 * port: DP_ACL_MATCH_KEY_V4 (21) or DP_ACL_MATCH_KEY_V6 (45) bytes a key, the
 * key size naming the family.  Keys lie `stride` bytes apart (>= key_size;
 * lookup_batch's arena packs them at its layout's stride, lookup.rs:131-138),
 * so a binding hands over AclKey::as_key() output as it is.
 * dp_acl_key_from_match converts n of them to dp_acl_key_t (host code: no
 * device, no context); dp_acl_classify_match classifies them as
 * dp_acl_classify does.  DP_EINVAL: another key size, stride < key_size. */
#define DP_ACL_MATCH_KEY_V4 21u
#define DP_ACL_MATCH_KEY_V6 45u
int dp_acl_key_from_match(const uint8_t *match, uint32_t key_size, uint32_t stride, uint32_t n,
                          dp_acl_key_t *out);
int dp_acl_classify_match(dp_ctx_t *ctx, const uint8_t *match, uint32_t key_size, uint32_t stride,
                          uint32_t n, dp_acl_result_t *out);

/* ------------------------------------------------------------------------ */
/* The flow-filter classifier alone (the narrower drop-in for */
/* A13): FlowFilterContext::lookup_batch (flow-filter/src/context/tables.rs: */
/* 800-848) over the published ff_remote_* / ff_local_* rules.  Per input,   */
/* stage 1 matches the destination (RemoteKey: proto, src VNI, the GateVni   */
/* dst_vni -- 0 for an ungated lookup --, destination, destination port)     */
/* against the remote rules in priority order; on a hit, stage 2 matches the */
/* source (LocalKey: proto, src VNI, the verdict's VPC, source, source port, */
/* SourceGate) against the local rules (lookup_versioned, :854-915).  The    */
/* outcome is LookupResult (:70-81): Route (the verdict's VPC and NAT mode,  */
/* the source's NAT mode), SourceMiss (the verdict's VPC) or                 */
/* DestinationMiss -- also for an input whose two addresses are of different */
/* families.  Inputs are never reordered.                                   */
/* ------------------------------------------------------------------------ */
typedef struct dp_ff_input {        /* LookupInput (tables.rs:88-97) */
    uint32_t src_vni;               /* src_vpcd */
    uint32_t dst_vni;               /* dst_vpcd: stage 1's GateVni (0: None, an ungated lookup) */
    uint8_t src_family, dst_family; /* 4 or 6 each (IpAddr::V4 / V6) */
    uint8_t proto;                  /* NextHeader */
    uint8_t gate;                   /* SourceGate: 0 Ungated, 1 PortFwdReply */
    uint16_t sport, dport;          /* ports; None is (0, 0) */
    uint8_t pad[4];
    uint8_t src[16], dst[16];       /* network byte order; v4 in the first 4 bytes */
} dp_ff_input_t;                    /* 48 B */

enum dp_ff_outcome { DP_FF_DESTINATION_MISS = 0, DP_FF_SOURCE_MISS = 1, DP_FF_ROUTE = 2 };
typedef struct dp_ff_result {       /* LookupResult */
    uint8_t outcome;                /* enum dp_ff_outcome */
    uint8_t dst_nat;                /* Route: the verdict's NatMode (enum dp_nat_mode) */
    uint8_t src_nat;                /* Route: the source's NatMode */
    uint8_t pad;
    uint32_t dst_vni;               /* Route / SourceMiss: the verdict's dst_vpcd */
} dp_ff_result_t;                   /* 8 B */

/* n inputs resident on the context's device (stream as in
 * dp_process_burst_device; asynchronous there). */
int dp_ff_classify_device(dp_ctx_t *ctx, const dp_ff_input_t *dev_in, dp_ff_result_t *dev_out,
                          uint32_t n, void *stream);
/* The same for inputs and results in host memory (synchronous). */
int dp_ff_classify(dp_ctx_t *ctx, const dp_ff_input_t *in, dp_ff_result_t *out, uint32_t n);

/* The two tables alone over the reference's own key bytes -- what the
 * rte_acl classifiers behind lookup_batch are handed (AnyTable::lookup_batch,
 * tables.rs:313-326; MatchKey::as_key_into's fields back to back, big-endian,
 * match-action-derive/src/lib.rs:191-206):
 *   table DP_FF_REMOTE, RemoteKey<I>: proto 1, src_vni 4, dst_vni (GateVni, 0
 *     None) 4, destination 4 / 16, destination port 2 -- DP_FF_REMOTE_KEY_V4
 *     (15) or DP_FF_REMOTE_KEY_V6 (27) bytes;
 *   table DP_FF_LOCAL, LocalKey<I>: proto 1, src_vni 4, dst_vni 4, source 4 /
 *     16, source port 2, gate (SourceGate) 1 -- DP_FF_LOCAL_KEY_V4 (16) or
 *     DP_FF_LOCAL_KEY_V6 (28) bytes;
 * keys `stride` bytes apart (>= key_size), the key size naming the family.
 * dp_ff_key_from_match converts n of them to dp_ff_input_t (host code: no
 * device, no context; a remote key leaves the source zero, a local key the
 * destination); dp_ff_classify_match runs that table alone: per key
 * DP_FF_ROUTE with the matching rule's action (remote: dst_vni + dst_nat;
 * local: src_nat), else DP_FF_DESTINATION_MISS (remote) / DP_FF_SOURCE_MISS
 * (local).  DP_EINVAL: another table, key size, stride < key_size. */
enum dp_ff_table { DP_FF_REMOTE = 1, DP_FF_LOCAL = 2 };
#define DP_FF_REMOTE_KEY_V4 15u
#define DP_FF_REMOTE_KEY_V6 27u
#define DP_FF_LOCAL_KEY_V4 16u
#define DP_FF_LOCAL_KEY_V6 28u
int dp_ff_key_from_match(int table, const uint8_t *match, uint32_t key_size, uint32_t stride, uint32_t n,
                         dp_ff_input_t *out);
int dp_ff_classify_match(dp_ctx_t *ctx, int table, const uint8_t *match, uint32_t key_size,
                         uint32_t stride, uint32_t n, dp_ff_result_t *out);

/* ------------------------------------------------------------------------ */
/* The FIB lookup alone: the longest prefix match behind IP-Forward as a     */
/* batch lookup -- FibReader::lpm_route / Fib::lpm (routing/src/fib/         */
/* fibtype.rs:239-257, 440-443) over the published routes.  Per key, the FIB */
/* of the key's VRF (FibKey::Id, dp_fib_t.vrf_id) is searched for the        */
/* longest published route covering the address; the result names that       */
/* route's dp_route_nh_t.  A FIB always answers: where no published route    */
/* covers the key, the answer is the FIB's implicit drop default             */
/* (DP_FIB_DEFAULT), never an index; a /0 the caller published is a route    */
/* like any other.  Keys are never reordered: out[i] answers keys[i].        */
/* Declared boundaries: the matched prefix itself (lpm_with_prefix) is not   */
/* reported -- the device tables' leaves hold the next hop alone --, and no  */
/* ECMP entry is chosen (that needs the packet's hash): n_entries says how   */
/* many there are.                                                           */
/* ------------------------------------------------------------------------ */
typedef struct dp_fib_key {
    uint32_t vrf_id;     /* FibKey::Id of the FIB to search (dp_fib_t.vrf_id) */
    uint8_t  family;     /* 4 or 6 */
    uint8_t  pad[3];
    uint8_t  addr[16];   /* network byte order; v4 in the first 4 bytes */
} dp_fib_key_t;          /* 24 B */

enum dp_fib_code {
    DP_FIB_ROUTE = 0,       /* a published route covers the key */
    DP_FIB_DEFAULT = 1,     /* none does: the FIB's implicit drop default */
    DP_FIB_NO_VRF = 2,      /* no published FIB has the key's vrf_id */
    DP_FIB_BAD_FAMILY = 3   /* a family other than 4 / 6 (whatever the vrf_id) */
};
typedef struct dp_fib_result {
    uint32_t nh;         /* index into the published route_nhs[] of the longest matching
                            route; UINT32_MAX when code != DP_FIB_ROUTE */
    uint16_t n_entries;  /* that dp_route_nh_t's n_entries (> 1: ECMP), else 0 */
    uint8_t  code;       /* enum dp_fib_code */
    uint8_t  pad;
} dp_fib_result_t;       /* 8 B */

/* n keys resident on the context's device into dev_out, both 8-byte aligned
 * (DP_EINVAL otherwise; stream as in dp_process_burst_device; asynchronous
 * there).  DP_ENOTABLES before a publish; n = 0 is DP_OK and launches nothing. */
int dp_fib_lookup_device(dp_ctx_t *ctx, const dp_fib_key_t *dev_keys, dp_fib_result_t *dev_out,
                         uint32_t n, void *stream);
/* The same for keys and results in host memory (synchronous; any alignment). */
int dp_fib_lookup(dp_ctx_t *ctx, const dp_fib_key_t *keys, dp_fib_result_t *out, uint32_t n);

/* ------------------------------------------------------------------------ */
/* Flow table: FlowTable                              */
/* (flow-entry/src/flow_table/table.rs:24-330) resident in HBM, consulted by */
/* the FlowLookup stage (nf_lookup.rs:34-55) and by the flow-aware branches  */
/* of IcmpErrorHandler (nat/src/icmp_handler/nf.rs:102-180), FlowFilter      */
/* (flow-filter/src/lib.rs:115-349) and AclFilter (acl-filter/src/lib.rs:    */
/* 62-138) for every context it is attached to.                              */
/*                                                                           */
/* The NAT state of the flow pairs the data path creates is carried:        */
/* port forwarding's (.port_fw_state) and masquerade's (.nat_state, with the */
/* allocation the SrcNat flow owns, released when that flow leaves the table:*/
/* a sweep, a remove, or a replacement -- at the end of the burst that       */
/* replaced it).  Every flow has a destination VPC.                          */
/*                                                                           */
/* Burst semantics are the reference pipeline's: FlowLookup, the flow-filter */
/* bypass decision and IcmpErrorHandler see flow states as they were when    */
/* the burst started; flows invalidated by the flow-filter (a miss, or an    */
/* outdated flow) are seen invalid by every AclFilter of the burst, and a    */
/* packet denied by the ACL invalidates its flows for the packets after it   */
/* (the pipeline runs FlowFilter over the whole burst, then the later stages */
/* packet by packet: flow-filter/src/lib.rs:352-363).                        */
/* ------------------------------------------------------------------------ */
typedef struct dp_flow_table dp_flow_table_t;

/* IpProtoKey variant (net/src/flows/flow_key.rs:360-365).  ICMP error keys
 * (IcmpProtoKey::ErrorMsgData) are never stored: no creator of flows makes
 * them, so dp_flow_insert rejects them and lookups of such keys miss. */
enum dp_flow_kind {
    DP_FLOW_TCP = 1,          /* sport / dport */
    DP_FLOW_UDP = 2,          /* sport / dport */
    DP_FLOW_ICMP_QUERY = 3,   /* IcmpProtoKey::QueryMsgData: sport = identifier, dport = 0 */
    DP_FLOW_ICMP_OTHER = 4    /* IcmpProtoKey::Unsupported: ports 0 */
};
/* FlowStatus (net/src/flows/flow_info.rs:37-49). */
enum dp_flow_status { DP_FLOW_ACTIVE = 0, DP_FLOW_CANCELLED = 1, DP_FLOW_EXPIRED = 2,
                      DP_FLOW_DETACHED = 3 };
/* FlowInfoFlags (flow_info.rs:142-149). */
enum dp_flow_flag { DP_FLOW_INITIATOR = 1u << 0, DP_FLOW_REQ_STATIC_NAT_SRC = 1u << 1,
                    DP_FLOW_REQ_STATIC_NAT_DST = 1u << 2 };

/* FlowKey (flow_key.rs:457-463): src_vpcd (0 = None), addresses of one
 * family (v4 in src[0..4] / dst[0..4], the rest zero), protocol key. */
typedef struct dp_flow_key {
    uint32_t src_vni;
    uint8_t family;           /* 4 or 6 */
    uint8_t kind;             /* enum dp_flow_kind */
    uint16_t pad;
    uint16_t sport, dport;
    uint8_t src[16];
    uint8_t dst[16];
} dp_flow_key_t;

/* A FlowInfo to insert (flow_info.rs:189-199). */
typedef struct dp_flow {
    dp_flow_key_t key;
    uint32_t dst_vni;         /* FlowInfoLocked.dst_vpcd (required, != 0) */
    uint32_t flags;           /* enum dp_flow_flag */
    uint32_t pad;
    int64_t genid;            /* FlowInfo.genid */
    uint64_t expires_at;      /* FlowInfo.expires_at, on the caller's clock */
} dp_flow_t;

/* A flow as stored.  `ref` names one stored FlowInfo (slot + fill tag); a
 * flow replaced or removed from the table no longer matches its ref. */
/* PortFwState.action (nat/src/common/mod.rs:14-19) */
enum dp_pf_action { DP_PF_NONE = 0, DP_PF_DST_NAT = 1, DP_PF_SRC_NAT = 2 };
/* NatFlowStatus (nat/src/common/mod.rs:34-45), shared by the two flows of a
 * port-forwarded pair */
enum dp_nat_flow_status { DP_NFS_ONE_WAY = 0, DP_NFS_TWO_WAY = 1, DP_NFS_ESTABLISHED = 2,
                          DP_NFS_RESET = 3, DP_NFS_C_CLOSING = 4, DP_NFS_S_CLOSING = 5,
                          DP_NFS_C_HALF_CLOSE = 6, DP_NFS_S_HALF_CLOSE = 7,
                          DP_NFS_LAST_ACK = 8, DP_NFS_CLOSED = 9 };
typedef struct dp_flow_info {
    uint64_t ref;             /* DP_FLOW_NONE: not found */
    uint32_t status;          /* enum dp_flow_status */
    uint32_t flags;
    uint32_t dst_vni;
    uint32_t pad;
    int64_t genid;
    uint64_t expires_at;
    uint64_t related;         /* ref of the related flow (FlowInfo.related), DP_FLOW_NONE */
    /* FlowInfoLocked.port_fw_state (nat/src/portfw/flow_state.rs:29-35) */
    uint8_t pf;               /* enum dp_pf_action (DP_PF_NONE: no state) */
    uint8_t pf_status;        /* enum dp_nat_flow_status */
    uint16_t pf_port;         /* use_port */
    uint32_t pf_rule;         /* id of the PortFwEntry its Weak names (dp_portfw_rule_t) */
    uint8_t pf_family;        /* use_ip family */
    uint8_t pad2[7];
    uint8_t pf_ip[16];        /* use_ip */
    /* FlowInfoLocked.nat_state (MasqueradeState, nat/src/masquerade/state.rs:
     * 13-20): action, with the status / use_ip / use_port in pf_status /
     * pf_ip / pf_port (pf_family) */
    uint8_t masq;             /* enum dp_pf_action (DP_PF_NONE: no state) */
    uint8_t masq_alloc;       /* 1: the state owns an allocation (the SrcNat flow) */
    uint16_t pad3;
    uint32_t idle_timeout_s;  /* MasqueradeState.idle_timeout */
} dp_flow_info_t;
#define DP_FLOW_NONE UINT64_MAX

/* dp_flow_insert per-flow results */
#define DP_FLOW_INSERTED 0
#define DP_FLOW_REPLACED 1    /* an existing flow of that key became Detached */
#define DP_EFLOWCAP (-28)     /* FlowTableError::CapacityExceeded (ENOSPC) */

/* `slots`: a power of two; the table holds at most slots / 2 flows.  The
 * capacity (FlowTable::set_capacity) defaults to FlowTable::DEFAULT_CAPACITY
 * (10M, table.rs:65) clamped to slots / 2. */
int dp_flow_table_create(int device_ordinal, uint64_t slots, dp_flow_table_t **out);
int dp_flow_table_destroy(dp_flow_table_t *ft);
int dp_flow_table_set_capacity(dp_flow_table_t *ft, uint64_t capacity);

/* FlowTable::insert for each flow in order (table.rs:134-260): the flow
 * becomes Active; an existing flow of the same key is Detached and replaced;
 * at capacity a new flow is refused (DP_EFLOWCAP).  `refs` / `results` may
 * be NULL.  Synchronous. */
int dp_flow_insert(dp_flow_table_t *ft, const dp_flow_t *flows, uint32_t n, uint64_t *refs,
                   int32_t *results);
/* FlowInfo::related_pair (flow_info.rs:290-339) then insert of both: exactly
 * one flow must have DP_FLOW_INITIATOR and the keys must differ.  The second
 * is admitted at capacity if the first is in the table and Active
 * (table.rs:221-233).  refs[2] / results[2] may be NULL. */
int dp_flow_insert_pair(dp_flow_table_t *ft, const dp_flow_t *a, const dp_flow_t *b,
                        uint64_t *refs, int32_t *results);
/* FlowTable::lookup (table.rs:267-275). */
int dp_flow_lookup(dp_flow_table_t *ft, const dp_flow_key_t *keys, uint32_t n,
                   dp_flow_info_t *out);
/* Current state of stored flows by ref (status etc.; ref DP_FLOW_NONE in
 * `out` when the ref no longer names a stored flow). */
int dp_flow_get(dp_flow_table_t *ft, const uint64_t *refs, uint32_t n, dp_flow_info_t *out);
/* FlowTable::remove (table.rs:282-295): the flow becomes Detached. */
int dp_flow_remove(dp_flow_table_t *ft, const dp_flow_key_t *keys, uint32_t n,
                   uint32_t *n_removed);
/* FlowInfo::invalidate_pair (flow_info.rs:435-455) / update_status. */
int dp_flow_invalidate(dp_flow_table_t *ft, const uint64_t *refs, uint32_t n);
int dp_flow_set_status(dp_flow_table_t *ft, uint64_t ref, uint32_t status);
/* The flow timers (FlowTable::start_timer, table.rs:160-213) up to `now`:
 * an Active flow with expires_at <= now becomes Expired and leaves the table;
 * a Cancelled or Expired flow leaves the table; a Detached one stays. */
int dp_flow_sweep(dp_flow_table_t *ft, uint64_t now, uint64_t *n_removed);
/* FlowTable::len / active_len (table.rs:297-317). */
int dp_flow_count(dp_flow_table_t *ft, uint64_t *len, uint64_t *active);
/* FlowLookup::new(name, Arc<FlowTable>) for this context's pipeline (and the
 * IcmpErrorHandler's table); NULL detaches (an empty flow table).  The table
 * must live on the context's device and outlive the attachment. */
int dp_ctx_attach_flow_table(dp_ctx_t *ctx, dp_flow_table_t *ft);

/* ------------------------------------------------------------------------ */
/* Flow-table snapshot: FlowTable::for_each_flow_filtered / snapshot(filter) */
/* (flow-entry/src/flow_table/table.rs:319-372) on the device.  A            */
/* declarative filter selects stored flows; the selected flows are written,  */
/* in ascending slot order, as dp_flow_entry_t records: the scan and the     */
/* compaction run in HBM and only the matches cross the bus.  A cursor       */
/* chunks a walk (the chunking table.rs:374-376 asks for).                   */
/*                                                                           */
/* Only stored flows are seen, whatever their FlowStatus (a Detached flow    */
/* that a replacement or a remove took out of the table is not stored).      */
/*                                                                           */
/* Order.  For a given table state the order is deterministic (ascending     */
/* slot), and it carries no meaning -- the reference's DashMap order has     */
/* none either.  A walk over several calls is consistent only if nothing     */
/* modifies the table in between (inserts, removes, sweeps, flows bursts);   */
/* between the calls the table is free.                                      */
/* ------------------------------------------------------------------------ */
enum dp_flowf {
    DP_FLOWF_SRC_VNI = 1u << 0,     /* key.src_vni == src_vni (0: None) */
    DP_FLOWF_DST_VNI = 1u << 1,     /* info.dst_vni == dst_vni */
    DP_FLOWF_FAMILY = 1u << 2,      /* key.family == family (4 / 6) */
    DP_FLOWF_KIND = 1u << 3,        /* bit key.kind of kind_mask (enum dp_flow_kind) */
    DP_FLOWF_SRC = 1u << 4,         /* key.src inside `src`; a prefix of the other family is false */
    DP_FLOWF_DST = 1u << 5,         /* key.dst inside `dst` */
    DP_FLOWF_SPORT = 1u << 6,       /* sport_lo <= key.sport <= sport_hi, whatever the kind (an ICMP */
    DP_FLOWF_DPORT = 1u << 7,       /*   query's identifier sits in sport); likewise key.dport */
    DP_FLOWF_STATUS = 1u << 8,      /* bit info.status of status_mask (enum dp_flow_status) */
    DP_FLOWF_FLAGS_ALL = 1u << 9,   /* (info.flags & flags_all) == flags_all (enum dp_flow_flag) */
    DP_FLOWF_FLAGS_NONE = 1u << 10, /* (info.flags & flags_none) == 0 */
    DP_FLOWF_GENID_LT = 1u << 11,   /* info.genid < genid ("what is stale") */
    DP_FLOWF_GENID_EQ = 1u << 12,   /* info.genid == genid */
    DP_FLOWF_EXPIRES_LE = 1u << 13, /* info.expires_at <= expires_at */
    DP_FLOWF_NAT = 1u << 14,        /* the flow is in a class of nat_mask (enum dp_flow_nat) */
    DP_FLOWF_NAT_IP = 1u << 15,     /* use_ip (info.pf_ip / pf_family) of the flow's port-forwarding or */
    DP_FLOWF_NAT_PORT = 1u << 16    /*   masquerade state inside nat_ip; use_port (info.pf_port) in
                                         [nat_port_lo, nat_port_hi]; false for a flow with neither state */
};
/* NAT classes (not exclusive): info.pf != DP_PF_NONE; info.masq != DP_PF_NONE;
 * info.masq != DP_PF_NONE with info.masq_alloc */
enum dp_flow_nat { DP_FLOW_NAT_PF = 1, DP_FLOW_NAT_MASQ = 2, DP_FLOW_NAT_MASQ_ALLOC = 4 };

/* Every set clause must hold; clauses == 0 selects every stored flow.  The
 * fields of a clause that is not set are ignored.  A prefix's host bits are
 * ignored.  112 bytes, no implicit padding. */
typedef struct dp_flow_filter {
    uint32_t clauses;            /* enum dp_flowf */
    uint32_t src_vni, dst_vni;
    uint8_t family;
    uint8_t kind_mask;           /* 1 << kind */
    uint8_t status_mask;         /* 1 << status */
    uint8_t nat_mask;            /* enum dp_flow_nat */
    uint32_t flags_all, flags_none;
    uint16_t sport_lo, sport_hi, dport_lo, dport_hi;   /* inclusive */
    uint16_t nat_port_lo, nat_port_hi;
    dp_prefix_t src, dst, nat_ip;
    int64_t genid;               /* GENID_LT and GENID_EQ share it */
    uint64_t expires_at;
} dp_flow_filter_t;              /* 112 B */

/* One selected flow: its key, the slot it sits in (informational: the low
 * half of info.ref) and its dp_flow_info_t exactly as dp_flow_lookup of that
 * key fills it.  136 bytes, 8-byte aligned. */
typedef struct dp_flow_entry {
    dp_flow_key_t key;
    uint32_t slot;
    dp_flow_info_t info;
} dp_flow_entry_t;               /* 136 B */
#ifdef __cplusplus
static_assert(sizeof(dp_flow_filter_t) == 112 && sizeof(dp_flow_entry_t) == 136, "snapshot ABI");
#else
_Static_assert(sizeof(dp_flow_filter_t) == 112 && sizeof(dp_flow_entry_t) == 136, "snapshot ABI");
#endif

/* The filter's predicate on the host, and its specification: 1 the flow
 * (key, info) is selected, 0 it is not; needs no device.  `filter` NULL
 * selects every flow.  DP_EINVAL: key or info NULL, an unknown clause, a set
 * prefix clause whose family is not 4 / 6 or whose length exceeds it, a set
 * range clause with lo > hi. */
int dp_flow_filter_match(const dp_flow_filter_t *filter, const dp_flow_key_t *key,
                         const dp_flow_info_t *info);

/* The stored flows `filter` selects (NULL: all), scanning from slot `*cursor`
 * (0 starts a walk; `cursor` NULL: from 0, nothing reported; above the slot
 * count: DP_EINVAL).  `entries[0 .. *n_entries)` receive the first
 * min(cap, matches from the cursor on) matches in ascending slot order --
 * always an exact prefix.  On return `*cursor` is the slot after the last
 * entry returned, or the slot count when the call reached the end (every
 * match from the starting cursor on was returned): page by calling again
 * until it equals the slot count (`slots` of dp_flow_table_create).  With
 * cap 0 and matches left, `*cursor` is unchanged.  `matched` (may be NULL)
 * receives the matches from the starting cursor to the end of the table,
 * whatever `cap`; `entries` NULL with cap 0 is a count-only call
 * (dp_flow_count generalised).  `n_entries` may be NULL.  Synchronous, in the
 * table's order like the other management calls.  DP_EINVAL also for an
 * invalid filter (dp_flow_filter_match) and for cap > 0 with `entries`
 * NULL. */
int dp_flow_snapshot(dp_flow_table_t *ft, const dp_flow_filter_t *filter, uint64_t *cursor,
                     dp_flow_entry_t *entries, uint32_t cap, uint32_t *n_entries,
                     uint64_t *matched);
/* The same with `entries` in device memory (the table's device, 8-byte
 * aligned); they are written when the call returns. */
int dp_flow_snapshot_device(dp_flow_table_t *ft, const dp_flow_filter_t *filter, uint64_t *cursor,
                            dp_flow_entry_t *dev_entries, uint32_t cap, uint32_t *n_entries,
                            uint64_t *matched);


/* ------------------------------------------------------------------------ */
/* DPDK rx / tx burst glue: an rx burst of rte_mbufs  */
/* (RxQueue::receive, dpdk/src/queue/rx.rs:178-201) runs through the path in */
/* place in its mempool memory, and every delivered mbuf is left holding its */
/* serialized frame, ready for TxQueue::transmit (dpdk/src/queue/tx.rs:      */
/* 144-160).  The mempool region must be pinned and device-mapped            */
/* (hipHostRegister of the hugepage memzone): the kernel reads and rewrites  */
/* the frames over PCIe, no staging copies (the zero-copy host path).        */
/* Mbuf::raw_data (dpdk/src/mem.rs:502-522): the frame is the first segment, */
/* buf_addr + data_off, data_len bytes.                                      */
/* ------------------------------------------------------------------------ */

/* Byte offsets of the rte_mbuf fields this glue reads and writes; the
 * default is the rte_mbuf_core.h layout of the reference's DPDK (v26.03,
 * npins/sources.json: githedgehog/dpdk@fa7e361) on 64-bit targets. */
typedef struct dp_mbuf_layout {
    uint16_t buf_addr;    /* void *   */
    uint16_t data_off;    /* uint16_t */
    uint16_t nb_segs;     /* uint16_t */
    uint16_t port;        /* uint16_t */
    uint16_t pkt_len;     /* uint32_t */
    uint16_t data_len;    /* uint16_t */
    uint16_t buf_len;     /* uint16_t */
    uint16_t pad;
} dp_mbuf_layout_t;
#define DP_MBUF_LAYOUT_DPDK {0, 16, 20, 22, 36, 40, 54, 0}

/* Burst records for an rx burst: in[i].off = the frame's offset from
 * `pool_base`, .len = data_len, .iif = port_ifindex[port] (the driver's
 * PacketMeta.iif; `port_ifindex` NULL: the port number).  An mbuf whose frame
 * lies outside [pool_base, pool_base + pool_bytes), beyond 4 GiB of it, or
 * with less than DP_HEADROOM bytes of headroom, gets a record the pipeline
 * marks InternalFailure.  Host only (no device call). */
int dp_mbuf_burst_in(const void *pool_base, uint64_t pool_bytes, void *const *mbufs, uint32_t n,
                     const dp_mbuf_layout_t *layout, const uint32_t *port_ifindex,
                     uint32_t n_ports, dp_pkt_in_t *in);
/* Apply a burst's results to its mbufs: a Delivered mbuf's data_off,
 * data_len and pkt_len describe its serialized frame (prepend / trim of the
 * headroom, dpdk/src/mem.rs:547-590); other mbufs are left as received (the
 * caller frees them).  Host only. */
int dp_mbuf_burst_out(void *const *mbufs, uint32_t n, const dp_mbuf_layout_t *layout,
                      const dp_pkt_in_t *in, const dp_pkt_out_t *out);
/* dp_mbuf_burst_in, the pipeline over the mapped mempool region (zero copy),
 * dp_mbuf_burst_out.  `out` (host memory) receives every packet's result
 * (`meta`, may be NULL, the rest of its PacketMeta);
 * the caller transmits the Delivered mbufs on their out[i].oif and frees the
 * others.  Synchronous.  A pool that is not device-mapped fails with
 * DP_EINVAL (every out[i] InternalFailure). */
int dp_process_mbufs(dp_ctx_t *ctx, const void *pool_base, uint64_t pool_bytes,
                     void *const *mbufs, uint32_t n, const dp_mbuf_layout_t *layout,
                     const uint32_t *port_ifindex, uint32_t n_ports, dp_pkt_out_t *out,
                     dp_pkt_meta_t *meta, uint64_t *stats);

/* ------------------------------------------------------------------------ */
/* Per-VPC statistics: the reference's Stats stage (stats/src/dpstats.rs:     */
/* 914-1011, Stats::process :942-1007), the accounting stage after Egress,    */
/* on the device.  Per packet i of a burst, from the records the path wrote:  */
/*   src = meta[i].src_vni, dst = meta[i].dst_vni (0: None),                  */
/*   bytes = out[i].len, drop = out[i].done != DP_DONE_DELIVERED              */
/*   (DP_DONE_NONE and Local count as drops, as the reference counts them);   */
/*   src == 0: nothing; drop: the drop total of src gains (1, bytes) and, if  */
/*   dst != 0, the pair-drop cell (src, dst) too; delivered with dst != 0:    */
/*   the forward cell (src, dst) gains (1, bytes); delivered, dst == 0:       */
/*   nothing.                                                                 */
/* Counters are u64, per context, cumulative across bursts until read with    */
/* reset, and independent of table generations (a publish leaves them).       */
/* Boundary: a delivered packet's out.len is its serialized length (the       */
/* reference's total_len() at the Stats stage); a dropped packet's out.len is */
/* the frame as received (in.len), where the reference counts total_len() at  */
/* the point of the drop (different after a decap or an encap): drop bytes    */
/* are "bytes received".  The reference never rate-smooths drop bytes.        */
/* ------------------------------------------------------------------------ */
typedef struct dp_vpc_stat {
    uint32_t src_vni, dst_vni;  /* dst_vni == 0: src_vni's drop total (fwd_* are 0) */
    uint64_t fwd_packets, fwd_bytes;
    uint64_t drop_packets, drop_bytes;
} dp_vpc_stat_t;                /* 40 B */

/* Slots of the context's device table of cells (open addressing).  At most
 * half of them hold reported cells: the first DP_VPC_STATS_CELLS / 2 distinct
 * cells since the last reset, in claim order.  Every update of a later cell
 * counts its packets into `lost_packets` instead, so a reported cell is
 * always exact. */
#define DP_VPC_STATS_CELLS 4096u

/* The stage alone over n device-resident records (stream as in
 * dp_process_burst_device; asynchronous there), whatever DP_OPT_VPC_STATS is. */
int dp_vpc_stats_accumulate_device(dp_ctx_t *ctx, const dp_pkt_out_t *dev_out,
                                   const dp_pkt_meta_t *dev_meta, uint32_t n, void *stream);
/* Read the cells, sorted by (src_vni, dst_vni), all-zero cells omitted.
 * A call of the context's own thread, like every other (Conventions above):
 * the worker reads on its tick and hands the cells to whoever collects them.
 * Synchronous, ordered after every burst and accumulate call the context has
 * launched (the caller synchronises streams it owns, as for dev_out).
 * `*n_entries` receives the number of cells; with cap too small nothing is
 * copied or reset and the call returns DP_ENOSPC.  `lost_packets` (may be
 * NULL) receives the packets of cells that found no slot.  `reset` != 0
 * clears every counter and lost_packets with the read: the table is copied
 * and then cleared on the context's stream, behind every burst launched so
 * far and before the call returns, so no update falls between the two. */
int dp_vpc_stats_read(dp_ctx_t *ctx, dp_vpc_stat_t *entries, uint32_t cap, uint32_t *n_entries,
                      uint64_t *lost_packets, int reset);

/* ------------------------------------------------------------------------ */
/* Packet capture: the reference's PacketDumper (pipeline/src/sample_nfs.rs: */
/* 41-150), a switchable tap with an optional filter, on the device.  A      */
/* declarative filter selects packets of a device-resident burst; the        */
/* selected packets are appended, in burst order, to a context-owned capture */
/* buffer in device memory: a dp_cap_rec_t each and the frames' bytes packed  */
/* densely in 16-byte units.  The buffer is cumulative across launches until  */
/* read with reset.  enable / disable are DP_OPT_CAPTURE, set_filter is       */
/* dp_capture_set_filter, the sample filters are dp_capture_filter_t values   */
/* (INTEGRATION.md).                                                          */
/*                                                                            */
/* Frame of a packet.  RX tap: in.off / in.len.  TX tap: out.off / out.len    */
/* when out.done == DP_DONE_DELIVERED; a packet that was not delivered has no */
/* frame: its header clauses (L4, SRC, DST, SPORT, DPORT) are false, and if   */
/* the remaining clauses select it, it is recorded with caplen 0 and len =    */
/* out.len ("everything the ACL dropped for VNI 3000").  A frame that         */
/* violates the layout contract of dp_process_burst_device (its end rounded   */
/* up to 16 bytes outside buf_bytes; on the RX tap also off < DP_HEADROOM) is */
/* treated the same way, as no frame, and never read.                         */
/*                                                                            */
/* The filter's view of a frame is a small parse of its own over the          */
/* outermost headers -- not Headers::parse; exact for the frames the          */
/* reference's sample filters tell apart, and this is its boundary:           */
/*   Ethernet: up to two tags (0x8100 / 0x88a8), then IPv4 (0x0800) or IPv6   */
/*     (0x86dd); anything else (a third tag, ARP, a frame cut short) is in no */
/*     class and has no addresses.                                            */
/*   IPv4: IHL >= 5 and the whole header inside the frame (the version nibble */
/*     is not examined); a non-zero fragment offset gives no ports and no     */
/*     class (the addresses stay).                                            */
/*   IPv6: the fixed header inside the frame; at most three extension         */
/*     headers are skipped: kinds 0, 43 and 60 are (len + 1) * 8 bytes, kind  */
/*     44 is 8 bytes and a non-zero fragment offset is handled as for IPv4;   */
/*     an extension header cut by the frame's end, or a fourth one, gives no  */
/*     class.                                                                 */
/*   Classes: UDP (protocol 17), TCP (6), ICMP4 (IPv4, 1), ICMP6 (IPv6, 58),  */
/*     VXLAN (UDP with ports and source or destination port 4789).            */
/*   Ports exist (UDP / TCP) when their four bytes lie inside the frame.      */
/*   A prefix clause of the other family is false.                            */
/*                                                                            */
/* Order and capacity.  Records appear in launch order and, within a launch,  */
/* in packet order.  Record k of a launch is kept if and only if it and every */
/* earlier one fit in both max_records and max_bytes (max_bytes rounded down  */
/* to 16), a record taking caplen rounded up to 16 bytes: what is kept is     */
/* always an exact prefix; `lost` counts the rest, `matched` counts both.     */
/* Bytes past caplen in a record's last 16-byte unit are zero.                */
/* Concurrency.  Capture launches of one context run one after the other,     */
/* whatever their streams (they share the launch scratch and the buffer).     */
/* ------------------------------------------------------------------------ */
enum dp_cap_tap { DP_CAP_RX = 1, DP_CAP_TX = 2 };   /* before / after the path */

/* packet classes (not exclusive): a packet matches DP_CAPF_L4 when it is in any class of l4_mask */
enum dp_cap_class { DP_CAPC_UDP = 1, DP_CAPC_TCP = 2, DP_CAPC_ICMP4 = 4, DP_CAPC_ICMP6 = 8,
                    DP_CAPC_VXLAN = 16 /* UDP with source or destination port 4789 */ };

enum dp_capf { DP_CAPF_L4 = 1, DP_CAPF_SRC = 2, DP_CAPF_DST = 4, DP_CAPF_SPORT = 8, DP_CAPF_DPORT = 16,
               DP_CAPF_DONE = 32, DP_CAPF_SRC_VNI = 64, DP_CAPF_DST_VNI = 128 };

typedef struct dp_capture_filter {
    uint32_t clauses;            /* enum dp_capf: every set clause must hold; 0 = every packet */
    uint32_t l4_mask;            /* enum dp_cap_class */
    uint64_t done_mask;          /* bit d: out.done == d (TX tap only) */
    uint32_t src_vni, dst_vni;   /* meta.src_vni / dst_vni equal (TX tap with a meta array only) */
    dp_prefix_t src, dst;        /* outermost IP source / destination inside the prefix */
    uint16_t sport_lo, sport_hi, dport_lo, dport_hi;   /* inclusive, UDP / TCP only */
    uint32_t snaplen;            /* bytes kept per frame; 0 = the whole frame */
    uint32_t pad;
} dp_capture_filter_t;           /* 80 B */

typedef struct dp_cap_rec {      /* 32 B */
    uint64_t off;                /* into the capture bytes, a multiple of 16 */
    uint32_t burst;              /* capture launches since open / reset, from 0 */
    uint32_t index;              /* the packet's index in that burst */
    uint16_t len, caplen;        /* frame length; bytes stored (min(len, snaplen)) */
    uint8_t tap, done;           /* done: DP_DONE_NONE on the RX tap */
    uint16_t pad;
    uint32_t src_vni, dst_vni;   /* TX tap with a meta array, else 0 */
} dp_cap_rec_t;

/* Open the context's capture: a buffer of max_records records and max_bytes
 * bytes in device memory, empty; `filter` NULL selects every packet.  One
 * capture a context (DP_EINVAL while one is open; also for an unknown clause,
 * or a prefix clause whose family is not 4 / 6 or whose length exceeds it). */
int dp_capture_open(dp_ctx_t *, const dp_capture_filter_t *, uint32_t max_records, uint64_t max_bytes);
/* Another filter for the launches that follow (launches already enqueued
 * keep theirs). */
int dp_capture_set_filter(dp_ctx_t *, const dp_capture_filter_t *);  /* for launches that follow */
/* Waits for the last capture launch and frees the buffer; what was not read
 * is gone. */
int dp_capture_close(dp_ctx_t *);
/* The stage alone over n device-resident records on `stream` (as in
 * dp_process_burst_device; asynchronous there), whatever DP_OPT_CAPTURE is:
 * `dev_buf` 16-byte aligned under the layout contract above, `dev_recs` the
 * burst's dp_pkt_in_t (DP_CAP_RX) or dp_pkt_out_t (DP_CAP_TX) records,
 * 16-byte aligned.  DP_EINVAL: no capture open, another tap, DP_CAPF_DONE or a
 * VNI clause on the RX tap, a VNI clause with dev_meta NULL.  n = 0 is DP_OK
 * and counts no launch. */
int dp_capture_device(dp_ctx_t *, int tap, const uint8_t *dev_buf, uint64_t buf_bytes,
                      const void *dev_recs /* dp_pkt_in_t (RX) or dp_pkt_out_t (TX) */,
                      const dp_pkt_meta_t *dev_meta /* may be NULL */, uint32_t n, void *stream);
/* Read the buffer, like dp_vpc_stats_read: synchronous, ordered behind every
 * burst and capture launch the context has launched.  `*n_recs` / `*n_bytes`
 * receive what the buffer holds, `matched` / `lost` (may be NULL) the packets
 * selected since open / reset and those of them that did not fit.  With
 * rec_cap or byte_cap too small nothing is copied or reset and the call
 * returns DP_ENOSPC (the counts say what is needed).  `reset` != 0 empties the
 * buffer and the counters on the stream after the copy, before the call
 * returns; the next launch's `burst` is 0. */
int dp_capture_read(dp_ctx_t *, dp_cap_rec_t *recs, uint32_t rec_cap, uint8_t *bytes, uint64_t byte_cap,
                    uint32_t *n_recs, uint64_t *n_bytes, uint64_t *matched, uint64_t *lost, int reset);

/* ------------------------------------------------------------------------ */
/* TX plan: what the reference's drivers do with a burst after               */
/* pipeline.process(burst), on the device.  The kernel driver transmits each */
/* Delivered packet on the interface meta.oif names and counts a missing or  */
/* unknown oif as a TX drop (dataplane/src/drivers/kernel/worker.rs:239-251, */
/* tx_packet :549-575); TxQueue::transmit takes the packets of ONE port as   */
/* an array (dpdk/src/queue/tx.rs:141-169).  A TX plan of n out records over */
/* a caller-given list of TX ports oifs[n_ports] is a stable partition of    */
/* the packet indexes 0..n-1 into n_ports + 2 buckets:                       */
/*   bucket b < n_ports: out[i].done == DP_DONE_DELIVERED and                */
/*     out[i].oif == oifs[b] -- the packets TxQueue::transmit of that port   */
/*     gets; the buckets follow the list's order, not the ifindexes';        */
/*   bucket n_ports: Delivered, but oif is 0 (None) or not in the list: the  */
/*     reference's TX drop;                                                  */
/*   bucket n_ports + 1: every other done value (DP_DONE_NONE and values     */
/*     >= DP_DONE_COUNT included): the packets the caller frees.             */
/* Within a bucket the indexes ascend: a flow's packets leave a port in the  */
/* order they arrived.                                                       */
/* order[n] receives the indexes, bucket after bucket; ports[n_ports + 2] a  */
/* dp_tx_port_t per bucket: oif (0 for the two special buckets), first (into */
/* order), count, bytes (the sum of out.len over the bucket);                */
/* ports[b].first + ports[b].count == ports[b + 1].first, and the last       */
/* bucket ends at n.                                                         */
/* oifs is host memory, read during the call and never retained.  DP_EINVAL: */
/* n_ports > DP_TX_MAX_PORTS, a 0 or a duplicate in oifs, a NULL array with  */
/* n > 0, out not 16-byte aligned, order / ports not 4- / 8-byte aligned     */
/* (device form).  n = 0 is DP_OK: the host form fills ports with zero       */
/* counts, the device form launches and writes nothing.  No published tables */
/* are needed.  Plans of one context run one after the other, whatever their */
/* streams (they share the context's launch scratch).                        */
/* ------------------------------------------------------------------------ */
#define DP_TX_MAX_PORTS 62u          /* + 2 special buckets = 64: one wave lane a bucket;
                                        RTE_MAX_ETHPORTS is 32 */
typedef struct dp_tx_port {
    uint32_t oif, first, count, pad;
    uint64_t bytes;
} dp_tx_port_t;                      /* 24 B */

/* Everything but oifs in device memory; enqueued on `stream` as
 * dp_process_burst_device does; asynchronous. */
int dp_tx_plan_device(dp_ctx_t *, const dp_pkt_out_t *dev_out, uint32_t n, const uint32_t *oifs,
                      uint32_t n_ports, uint32_t *dev_order, dp_tx_port_t *dev_ports, void *stream);
/* The same for records, order and ports in host memory; synchronous. */
int dp_tx_plan(dp_ctx_t *, const dp_pkt_out_t *out, uint32_t n, const uint32_t *oifs, uint32_t n_ports,
               uint32_t *order, dp_tx_port_t *ports);
/* Host only, no device: tx_mbufs[k] = mbufs[order[k]] for k < n_order -- with
 * ports[b].first / .count, the arrays rte_eth_tx_burst takes, after
 * dp_mbuf_burst_out.  DP_EINVAL for an order[k] >= n (nothing is promised
 * about tx_mbufs then) or a NULL array with n_order > 0. */
int dp_mbuf_burst_tx(void *const *mbufs, uint32_t n, const uint32_t *order, uint32_t n_order, void **tx_mbufs);

/* ------------------------------------------------------------------------ */
/* Publish statistics: what the context's last successful dp_tables_publish  */
/* did and how long its phases took (host clock, microseconds; the device    */
/* build by HIP events, nanoseconds).  DP_ENOTABLES before the context's     */
/* first successful publish.                                                 */
/* ------------------------------------------------------------------------ */
typedef struct dp_publish_stats {
    uint32_t device_fibs;   /* FIBs whose DIR-24-8 tables the device built (DP_OPT_DEVICE_FIB) */
    uint32_t sorted_fibs;   /* those of them whose route list the device also sorted and listed (mode 2; else 0) */
    uint64_t image_bytes;   /* the image in device memory */
    uint64_t upload_bytes;  /* bytes sent over the bus: the image (less the device-built regions) and the build lists */
    uint64_t built_bytes;   /* bytes the build kernels wrote: direct tables and blocks */
    uint64_t sort_us;       /* FIB routes: sort, duplicate pass, build lists */
    uint64_t paint_us;      /* host-built FIB tables: direct tables, blocks, Poptrie */
    uint64_t compile_us;    /* the rest of the table compile */
    uint64_t upload_us;     /* device allocation and copies */
    uint64_t kernel_ns;     /* the build kernels */
    uint64_t total_us;      /* dp_tables_publish, entry to return */
} dp_publish_stats_t;       /* 80 B */
int dp_tables_publish_stats(const dp_ctx_t *ctx, dp_publish_stats_t *out);

/* Introspection: bytes of the device table image and its parts (for
 * DESIGN.md / bench), and the last HIP error string. */
uint64_t dp_tables_device_bytes(const dp_ctx_t *ctx);
const char *dp_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* DPGPU_H */
