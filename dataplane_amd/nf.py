# SPDX-License-Identifier: Apache-2.0
"""Host-side mirror of the reference's stage API for this path.

The reference drives the path through ``NetworkFunction`` stages
(``pipeline/src/static_nf.rs:12-32``)::

    fn process(&mut self, input: impl Iterator<Item = Packet<Buf>>) -> impl Iterator<Item = Packet<Buf>>
    fn set_data(&mut self, data: Arc<PipelineData>)

``GpuPathNf`` keeps that shape: ``process`` materialises the burst (as
``FlowFilter::process`` does, ``flow-filter/src/lib.rs:357-362``), runs the
whole Ingress..Egress + serialize block on the GPU through the C ABI, applies
the returned DoneReason / metadata to every packet and yields them all
(``KEEP`` semantics: packets are marked, never removed).  ``set_data`` carries
the generation id.  Device-resident bursts go through ``process_device``.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Iterable, Iterator, List, Optional

import numpy as np

from . import _abi as A


@dataclass
class PipelineData:
    """pipeline/src/pipeline.rs:22-42"""
    genid: int = 0


@dataclass
class Packet:
    """A frame plus the PacketMeta fields this path reads and writes."""
    frame: bytes
    iif: int = 1
    src_vni: int = 0            # seeded src_vpcd (harness idiom, DP_IN_SEEDED_OVERLAY)
    seeded_overlay: bool = False
    # results (net/src/packet/meta.rs:138-154)
    done: Optional[str] = None
    meta_flags: int = 0
    oif: Optional[int] = None
    dst_vni: Optional[int] = None
    fib_entry: Optional[int] = None
    acl_rule: Optional[int] = None
    vrf: Optional[int] = None           # PacketMeta.vrf
    nh_addr: Optional[str] = None       # PacketMeta.nh_addr (next-hop IP, text form)
    dscp: Optional[int] = None          # PacketMeta.dscp / .ecn (set by the path when known)
    ecn: Optional[int] = None
    flow_ref: int = 0                   # the packet's attached flow (meta.flow_info), 0 = none

    def is_done(self) -> bool:
        return self.done is not None


class GpuPathNf:
    """One context per worker thread (worker.rs:175); one HIP stream each."""

    def __init__(self, device: int = 0, name: str = "gpu-path"):
        self.name = name
        self.lib = A.gpu_lib()
        h = C.c_void_p()
        A.check(self.lib.dp_ctx_create(device, C.byref(h)), "dp_ctx_create", self.lib)
        self.ctx = h
        self.data = PipelineData()
        self._keep = None

    # -- table publication --------------------------------
    def publish(self, tables_ptr) -> None:
        """Publish lowered tables (a POINTER(TablesDesc)); bursts that start
        after this returns see the new generation."""
        A.check(self.lib.dp_tables_publish(self.ctx, tables_ptr), "dp_tables_publish", self.lib)
        self.data.genid = int(self.lib.dp_tables_genid(self.ctx))

    def set_device_fib(self, on) -> None:
        """dp_ctx_set_option(DP_OPT_DEVICE_FIB): the publishes that follow build
        the DIR-24-8 tables of large v4 FIBs on the device instead of uploading them.
        `on`: a bool, or the option's integer mode (2: the device also sorts and
        lists the routes)."""
        self.set_option(A.OPT_DEVICE_FIB, int(on))

    def publish_stats(self) -> np.ndarray:
        """dp_tables_publish_stats: one A.PUBLISH_STATS record on this context's
        last publish (FIBs built on the device, bytes uploaded, phase times)."""
        st = np.zeros(1, dtype=A.PUBLISH_STATS)
        A.check(self.lib.dp_tables_publish_stats(self.ctx, st.ctypes.data), "dp_tables_publish_stats", self.lib)
        return st[0]

    def set_data(self, data: PipelineData) -> None:
        self.data = data

    # -- NetworkFunction::process -------------------------------------------
    def process(self, packets: Iterable[Packet]) -> Iterator[Packet]:
        burst: List[Packet] = list(packets)
        if not burst:
            return iter(())
        offs, total = [], 0
        for p in burst:
            total += A.HEADROOM
            offs.append(total)
            total = (total + len(p.frame) + 15) & ~15
        buf = np.zeros(total + 16, dtype=np.uint8)
        inp = np.zeros(len(burst), dtype=A.PKT_IN)
        for i, p in enumerate(burst):
            buf[offs[i]:offs[i] + len(p.frame)] = np.frombuffer(p.frame, dtype=np.uint8)
            inp[i] = (offs[i], len(p.frame), A.IN_SEEDED_OVERLAY if p.seeded_overlay else 0,
                      p.iif, p.src_vni)
        out = self.process_arrays(buf, inp)
        for i, p in enumerate(burst):
            r = out[i]
            d = int(r["done"])
            p.done = A.DONE_NAMES[d] if d < A.DONE_COUNT else None
            p.meta_flags = int(r["meta_flags"])
            p.oif = int(r["oif"]) or None
            p.dst_vni = int(r["dst_vni"]) or None
            p.fib_entry = None if r["fib_entry"] == 0xFFFFFFFF else int(r["fib_entry"])
            p.acl_rule = None if r["acl_rule"] == 0xFFFFFFFF else int(r["acl_rule"])
            pm = int(r["pm_flags"])
            p.vrf = int(r["vrf"]) if pm & A.PM_HAS_VRF else None
            p.nh_addr = A.nh_text(r) if pm & A.PM_HAS_NH else None
            p.dscp = int(r["dscp"]) if pm & A.PM_HAS_DSCP else None
            p.ecn = int(r["ecn"]) if pm & A.PM_HAS_DSCP else None
            p.flow_ref = int(r["flow_ref"])
            if d == A.DONE["Delivered"]:
                p.frame = bytes(buf[r["off"]:r["off"] + r["len"]])
        return iter(burst)

    def set_host_path(self, mode: int) -> None:
        """dp_ctx_set_option(DP_OPT_HOST_PATH): A.HOST_AUTO / HOST_COPY / HOST_ZERO_COPY."""
        A.check(self.lib.dp_ctx_set_option(self.ctx, A.OPT_HOST_PATH, mode), "dp_ctx_set_option",
                self.lib)

    def set_option(self, option: int, value: int) -> None:
        """dp_ctx_set_option (A.OPT_HOST_PATH, A.OPT_CLOCK: the flow clock in ns)."""
        A.check(self.lib.dp_ctx_set_option(self.ctx, option, value), "dp_ctx_set_option", self.lib)

    def set_clock(self, now_ns: int) -> None:
        """Instant::now() for the bursts that follow (DP_OPT_CLOCK): the expiry
        port forwarding gives the flows it creates and refreshes."""
        self.set_option(A.OPT_CLOCK, now_ns)

    def process_arrays(self, buf: np.ndarray, inp: np.ndarray,
                       stats: Optional[np.ndarray] = None,
                       out: Optional[np.ndarray] = None,
                       meta: Optional[np.ndarray] = None, with_meta: bool = True) -> np.ndarray:
        """Host-origin burst, in place (dp_process_burst).  Returns PKT_RES
        records (dp_pkt_out_t + dp_pkt_meta_t) -- or, with with_meta=False,
        the dp_pkt_out_t array alone (no meta array passed to the path)."""
        if out is None:
            out = np.zeros(len(inp), dtype=A.PKT_OUT)
        if meta is None and with_meta:
            meta = np.zeros(len(inp), dtype=A.PKT_META)
        sp = stats.ctypes.data if stats is not None else None
        A.check(self.lib.dp_process_burst(self.ctx, buf.ctypes.data, buf.nbytes, inp.ctypes.data,
                                          out.ctypes.data,
                                          meta.ctypes.data if meta is not None else None,
                                          len(inp), sp),
                "dp_process_burst", self.lib)
        return A.join_results(out, meta) if meta is not None else out

    def attach_flows(self, flow_table) -> None:
        """FlowLookup::new(name, flow_table) (flow-entry/src/flow_table/nf_lookup.rs:24-32):
        this context's pipeline consults `flow_table` (a dataplane_amd.flows.FlowTable);
        None detaches it (an empty flow table)."""
        A.check(self.lib.dp_ctx_attach_flow_table(self.ctx, flow_table.h if flow_table else None),
                "dp_ctx_attach_flow_table", self.lib)

    def process_mbufs(self, pool_base: int, pool_bytes: int, mbufs: np.ndarray,
                      port_ifindex: Optional[np.ndarray] = None,
                      stats: Optional[np.ndarray] = None, layout=None) -> np.ndarray:
        """An rx burst of rte_mbufs (addresses in `mbufs`) through the path in
        their pinned, device-mapped mempool region (dp_process_mbufs): the
        delivered mbufs hold their serialized frames, ready for tx."""
        mbufs = np.ascontiguousarray(mbufs, dtype=np.uint64)
        out = np.zeros(len(mbufs), dtype=A.PKT_OUT)
        meta = np.zeros(len(mbufs), dtype=A.PKT_META)
        pif = None if port_ifindex is None else np.ascontiguousarray(port_ifindex, dtype=np.uint32)
        A.check(self.lib.dp_process_mbufs(self.ctx, pool_base, pool_bytes, mbufs.ctypes.data,
                                          len(mbufs), C.byref(layout or A.MBUF_LAYOUT_DPDK),
                                          pif.ctypes.data if pif is not None else None,
                                          len(pif) if pif is not None else 0, out.ctypes.data,
                                          meta.ctypes.data,
                                          stats.ctypes.data if stats is not None else None),
                "dp_process_mbufs", self.lib)
        return A.join_results(out, meta)

    def process_device(self, dev_buf: int, buf_bytes: int, dev_in: int, dev_out: int, n: int,
                       dev_stats: Optional[int] = None, stream: Optional[int] = None,
                       dev_meta: Optional[int] = None) -> None:
        """Device-resident burst (dp_process_burst_device): raw device pointers;
        dev_meta (dp_pkt_meta_t[n]) is optional."""
        A.check(self.lib.dp_process_burst_device(self.ctx, dev_buf, buf_bytes, dev_in, dev_out,
                                                 dev_meta, n, dev_stats, stream),
                "dp_process_burst_device", self.lib)

    @staticmethod
    def process_sharded(nfs: List["GpuPathNf"], buf: np.ndarray, inp: np.ndarray,
                        stats: Optional[np.ndarray] = None) -> np.ndarray:
        """Host-origin burst split over several contexts / GPUs
        (dp_process_burst_sharded): contiguous shards of whole packets, one
        per context, copied and processed concurrently."""
        out = np.zeros(len(inp), dtype=A.PKT_OUT)
        meta = np.zeros(len(inp), dtype=A.PKT_META)
        ctxs = (C.c_void_p * len(nfs))(*[nf.ctx for nf in nfs])
        lib = nfs[0].lib
        sp = stats.ctypes.data if stats is not None else None
        A.check(lib.dp_process_burst_sharded(ctxs, len(nfs), buf.ctypes.data, buf.nbytes,
                                             inp.ctypes.data, out.ctypes.data, meta.ctypes.data,
                                             len(inp), sp),
                "dp_process_burst_sharded", lib)
        return A.join_results(out, meta)

    def synchronize(self) -> None:
        A.check(self.lib.dp_ctx_synchronize(self.ctx), "dp_ctx_synchronize", self.lib)

    def device_table_bytes(self) -> int:
        return int(self.lib.dp_tables_device_bytes(self.ctx))

    def acl_classify(self, keys: np.ndarray) -> np.ndarray:
        """The ACL classifier alone (dp_acl_classify): A.ACL_KEY records ->
        A.ACL_RESULT records (the batch Lookup<K, A> of the reference's
        DpdkAclLookup, acl/src/dpdk/lookup.rs:112-155)."""
        keys = np.ascontiguousarray(np.atleast_1d(keys), dtype=A.ACL_KEY)
        out = np.zeros(len(keys), dtype=A.ACL_RESULT)
        A.check(self.lib.dp_acl_classify(self.ctx, keys.ctypes.data, out.ctypes.data, len(keys)),
                "dp_acl_classify", self.lib)
        return out

    def acl_classify_match(self, match: np.ndarray, key_size: int, stride: int = 0) -> np.ndarray:
        """The same over the reference's own key bytes (dp_acl_classify_match):
        AclKey::as_key() output, key_size 21 (v4) or 45 (v6), keys `stride`
        bytes apart (default: packed)."""
        match = np.ascontiguousarray(match, dtype=np.uint8).reshape(-1)
        stride = stride or key_size
        n = len(match) // stride if len(match) >= key_size else 0
        if n and (n - 1) * stride + key_size > len(match):
            n -= 1
        out = np.zeros(n, dtype=A.ACL_RESULT)
        A.check(self.lib.dp_acl_classify_match(self.ctx, match.ctypes.data, key_size, stride, n,
                                               out.ctypes.data), "dp_acl_classify_match", self.lib)
        return out

    def ff_classify(self, inputs: np.ndarray) -> np.ndarray:
        """The flow-filter classifier alone (dp_ff_classify): A.FF_INPUT
        records (LookupInput) -> A.FF_RESULT records (LookupResult) --
        FlowFilterContext::lookup_batch, flow-filter/src/context/tables.rs:800-848."""
        inputs = np.ascontiguousarray(np.atleast_1d(inputs), dtype=A.FF_INPUT)
        out = np.zeros(len(inputs), dtype=A.FF_RESULT)
        A.check(self.lib.dp_ff_classify(self.ctx, inputs.ctypes.data, out.ctypes.data, len(inputs)),
                "dp_ff_classify", self.lib)
        return out

    def ff_classify_match(self, table: int, match: np.ndarray, key_size: int, stride: int = 0) -> np.ndarray:
        """One table alone over the reference's key bytes (dp_ff_classify_match):
        RemoteKey::as_key() (table A.FF_REMOTE, 15 / 27 bytes) or LocalKey::as_key()
        (A.FF_LOCAL, 16 / 28 bytes), keys `stride` bytes apart (default: packed)."""
        match = np.ascontiguousarray(match, dtype=np.uint8).reshape(-1)
        stride = stride or key_size
        n = len(match) // stride if len(match) >= key_size else 0
        if n and (n - 1) * stride + key_size > len(match):
            n -= 1
        out = np.zeros(n, dtype=A.FF_RESULT)
        A.check(self.lib.dp_ff_classify_match(self.ctx, table, match.ctypes.data, key_size, stride, n,
                                              out.ctypes.data), "dp_ff_classify_match", self.lib)
        return out

    def fib_lookup(self, keys: np.ndarray) -> np.ndarray:
        """The FIB lookup alone (dp_fib_lookup): A.FIB_KEY records -> A.FIB_RESULT
        records in input order -- FibReader::lpm_route per key
        (routing/src/fib/fibtype.rs:440-443)."""
        keys = np.ascontiguousarray(np.atleast_1d(keys), dtype=A.FIB_KEY)
        out = np.zeros(len(keys), dtype=A.FIB_RESULT)
        A.check(self.lib.dp_fib_lookup(self.ctx, keys.ctypes.data, out.ctypes.data, len(keys)),
                "dp_fib_lookup", self.lib)
        return out

    def fib_lookup_device(self, dev_keys: int, dev_out: int, n: int, stream: Optional[int] = None) -> None:
        """n device-resident keys (dp_fib_lookup_device): raw device pointers,
        asynchronous on `stream`."""
        A.check(self.lib.dp_fib_lookup_device(self.ctx, dev_keys, dev_out, n, stream),
                "dp_fib_lookup_device", self.lib)

    # -- per-VPC statistics (the Stats stage, stats/src/dpstats.rs:914-1011) ----
    def set_vpc_stats(self, on: bool) -> None:
        """dp_ctx_set_option(DP_OPT_VPC_STATS): every burst that follows is
        accounted into the context's per-VPC statistics on the device."""
        self.set_option(A.OPT_VPC_STATS, 1 if on else 0)

    def vpc_stats_accumulate_device(self, dev_out: int, dev_meta: int, n: int,
                                    stream: Optional[int] = None) -> None:
        """The stage alone over n device-resident dp_pkt_out_t / dp_pkt_meta_t
        records (dp_vpc_stats_accumulate_device): raw device pointers."""
        A.check(self.lib.dp_vpc_stats_accumulate_device(self.ctx, dev_out, dev_meta, n, stream),
                "dp_vpc_stats_accumulate_device", self.lib)

    def vpc_stats(self, reset: bool = False):
        """(A.VPC_STAT records sorted by (src_vni, dst_vni), lost packets) of
        dp_vpc_stats_read; `reset` clears the counters with the read."""
        cells = np.zeros(A.VPC_STATS_CELLS // 2, dtype=A.VPC_STAT)
        n, lost = C.c_uint32(0), C.c_uint64(0)
        A.check(self.lib.dp_vpc_stats_read(self.ctx, cells.ctypes.data, len(cells), C.byref(n),
                                           C.byref(lost), 1 if reset else 0),
                "dp_vpc_stats_read", self.lib)
        return cells[:n.value].copy(), int(lost.value)

    # -- packet capture (the PacketDumper stage, pipeline/src/sample_nfs.rs:41-150) --
    @staticmethod
    def _filter_ptr(flt):
        if flt is None:
            return None, None
        keep = np.ascontiguousarray(np.atleast_1d(flt), dtype=A.CAP_FILTER)
        return keep, keep.ctypes.data

    def capture_open(self, flt, max_records: int, max_bytes: int) -> None:
        """dp_capture_open: a capture buffer of max_records records and max_bytes
        bytes on the device; `flt` an A.CAP_FILTER record (None: every packet)."""
        keep, ptr = self._filter_ptr(flt)
        A.check(self.lib.dp_capture_open(self.ctx, ptr, max_records, max_bytes), "dp_capture_open", self.lib)
        self._cap = (max_records, max_bytes)

    def set_capture_filter(self, flt) -> None:
        """dp_capture_set_filter: the filter of the launches that follow."""
        keep, ptr = self._filter_ptr(flt)
        A.check(self.lib.dp_capture_set_filter(self.ctx, ptr), "dp_capture_set_filter", self.lib)

    def set_capture(self, taps: int) -> None:
        """dp_ctx_set_option(DP_OPT_CAPTURE): the taps (A.CAP_RX | A.CAP_TX) every
        process_device burst runs while a capture is open; 0 switches them off."""
        self.set_option(A.OPT_CAPTURE, taps)

    def capture_device(self, tap: int, dev_buf: int, buf_bytes: int, dev_recs: int, dev_meta: Optional[int],
                       n: int, stream: Optional[int] = None) -> None:
        """The stage alone over n device-resident records (dp_capture_device):
        raw device pointers; dp_pkt_in_t records for A.CAP_RX, dp_pkt_out_t for A.CAP_TX."""
        A.check(self.lib.dp_capture_device(self.ctx, tap, dev_buf, buf_bytes, dev_recs, dev_meta, n, stream),
                "dp_capture_device", self.lib)

    def capture_read(self, reset: bool = False):
        """(A.CAP_REC records, their bytes as a uint8 array, matched, lost) of
        dp_capture_read; `reset` empties the buffer with the read."""
        max_records, max_bytes = self._cap
        recs, data = np.zeros(max_records, dtype=A.CAP_REC), np.zeros(max_bytes, dtype=np.uint8)
        nr, nb, matched, lost = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        A.check(self.lib.dp_capture_read(self.ctx, recs.ctypes.data, max_records, data.ctypes.data, max_bytes,
                                         C.byref(nr), C.byref(nb), C.byref(matched), C.byref(lost),
                                         1 if reset else 0), "dp_capture_read", self.lib)
        return recs[:nr.value].copy(), data[:nb.value].copy(), int(matched.value), int(lost.value)

    def capture_close(self) -> None:
        A.check(self.lib.dp_capture_close(self.ctx), "dp_capture_close", self.lib)

    # -- TX plan (what the drivers do after pipeline.process: worker.rs:239-251, tx.rs:141-169) --
    def tx_plan(self, out: np.ndarray, oifs):
        """dp_tx_plan over A.PKT_OUT records in host memory: (order, ports) --
        the packet indexes grouped by TX port in the order of `oifs`, then the
        Delivered packets without a port of the list, then the packets to
        free; one A.TX_PORT record per bucket (len(oifs) + 2)."""
        out = np.ascontiguousarray(out, dtype=A.PKT_OUT)
        oifs = np.ascontiguousarray(oifs, dtype=np.uint32).reshape(-1)
        order = np.zeros(len(out), dtype=np.uint32)
        ports = np.zeros(len(oifs) + 2, dtype=A.TX_PORT)
        A.check(self.lib.dp_tx_plan(self.ctx, out.ctypes.data, len(out), oifs.ctypes.data, len(oifs),
                                    order.ctypes.data, ports.ctypes.data), "dp_tx_plan", self.lib)
        return order, ports

    def tx_plan_device(self, dev_out: int, n: int, oifs, dev_order: int, dev_ports: int,
                       stream: Optional[int] = None) -> None:
        """The plan over n device-resident dp_pkt_out_t records (dp_tx_plan_device):
        raw device pointers (dev_order: n u32, dev_ports: len(oifs) + 2
        A.TX_PORT records), asynchronous on `stream`; `oifs` is host memory."""
        oifs = np.ascontiguousarray(oifs, dtype=np.uint32).reshape(-1)
        A.check(self.lib.dp_tx_plan_device(self.ctx, dev_out, n, oifs.ctypes.data, len(oifs), dev_order,
                                           dev_ports, stream), "dp_tx_plan_device", self.lib)

    def close(self) -> None:
        if self.ctx:
            self.lib.dp_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
