// SPDX-License-Identifier: Apache-2.0
//
// Flow-table snapshot (include/dpgpu.h "Flow-table snapshot"):
// FlowTable::for_each_flow_filtered / snapshot(filter)
// (flow-entry/src/flow_table/table.rs:319-372) as a filtered, order-preserving
// compaction of the table's slots on the device, in three launches:
//
//   fl_snap_mark_k   one match bit per slot.  A wave takes 64 consecutive
//                    slots in 4 rounds of 16-byte loads: lane L of round r
//                    loads chunk L & 3 of slot 4 (L >> 2) + r -- 16 whole
//                    64-byte first halves per wave request -- and tests the
//                    clauses of its chunk (dp_flowsnap.h chunk_ok).  A ballot
//                    per round holds the 16 slots' four chunk verdicts side by
//                    side; lane L then reads the verdict of slot L out of
//                    round L & 3's ballot (its own group's four bits all
//                    set), so the wave's next ballot is the 64 slots' bitmap
//                    word in slot order, with no shuffle and no LDS.  The
//                    second half of a slot is read by its lane only if the
//                    slot survived and the filter has a clause there.  Two
//                    bitmap words (8 loads a lane) are in flight at a time.
//   fl_snap_scan_k   one workgroup: exclusive prefix over the tiles' counts,
//                    the total, and the slot of match number cap - 1.
//   fl_snap_emit_k   a wave per non-zero bitmap word: rank = tile prefix +
//                    popcounts of the tile's earlier words + bits below the
//                    lane; lanes with rank < cap write entries[rank].
//
// A tile is the 1024 slots (16 bitmap words) of one workgroup.  The bitmap
// starts at the tile of the cursor; bits before the cursor are clear.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <mutex>

#include "../../include/dpgpu.h"
#include "dp_flows_dev.h"
#include "dp_flowsnap.h"

using dpf::FlowSlot;
using dpfl::kTB;
using dpfs::Filter;

namespace {

constexpr uint32_t kTileWords = 16;                // bitmap words a workgroup (4 waves x 4)
constexpr uint32_t kTileSlots = 64 * kTileWords;   // 1024
constexpr uint32_t kScanTB = 1024;

struct ScanOut {
  unsigned long long total;  // matches from the cursor to the end
  unsigned long long last;   // slot of match number cap - 1 (valid with total >= cap >= 1)
};

__device__ __forceinline__ uint4 ld16(const FlowSlot *s, uint32_t chunk) {
  return *(reinterpret_cast<const uint4 *>(s) + chunk);
}

// `bitmap` / `tile_cnt` are indexed from the cursor's tile.
__global__ void __launch_bounds__(kTB) fl_snap_mark_k(const FlowSlot *slots, uint64_t nslots, uint64_t cursor,
                                                     Filter F, unsigned long long *bitmap, uint32_t *tile_cnt) {
  __shared__ uint32_t wave_cnt[kTB / 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t c = lane & 3u, g = lane >> 2;
  const bool second = (F.clauses & dpfs::kSecondClauses) != 0;
  const bool nat = (F.clauses & (DP_FLOWF_NAT | DP_FLOWF_NAT_IP | DP_FLOWF_NAT_PORT)) != 0;
  // this wave's 4 words, by their index in the bitmap and their first slot
  const uint64_t word0 = (uint64_t)blockIdx.x * kTileWords + wave * 4u;
  const uint64_t slot0 = (cursor / kTileSlots) * kTileSlots + word0 * 64u;
  uint32_t cnt = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; k += 2) {
    // a word past the table is loaded from the table's last 64 slots (the
    // smallest table has 64) and masked off below: every load is in bounds
    // and none waits for a branch
    uint64_t base[2];
    uint4 v[2][4];
#pragma unroll
    for (uint32_t u = 0; u < 2; u++) {
      base[u] = slot0 + (uint64_t)(k + u) * 64u;
      const uint64_t b = base[u] < nslots ? base[u] : nslots - 64u;
#pragma unroll
      for (uint32_t r = 0; r < 4; r++) v[u][r] = ld16(slots + b + 4u * g + r, c);
    }
#pragma unroll
    for (uint32_t u = 0; u < 2; u++) {
      unsigned long long rb[4];
#pragma unroll
      for (uint32_t r = 0; r < 4; r++)
        rb[r] = __ballot(dpfs::chunk_ok(F, c, v[u][r].x, v[u][r].y, v[u][r].z, v[u][r].w));
      // slot `lane` of the word was round c's slot of this lane's group
      const unsigned long long mine = c == 0 ? rb[0] : c == 1 ? rb[1] : c == 2 ? rb[2] : rb[3];
      bool pass = ((mine >> (4u * g)) & 0xfull) == 0xfull;
      // the cursor's word keeps the slots from the cursor on
      unsigned long long live = 0;
      if (base[u] < nslots && base[u] + 64u > cursor) live = base[u] >= cursor ? ~0ull : ~0ull << (cursor - base[u]);
      pass = pass && ((live >> lane) & 1ull);
      if (second && pass) {
        const FlowSlot *s = slots + base[u] + lane;
        uint4 h[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) h[j] = ld16(s, 4u + j);
        const uint32_t hw[16] = {h[0].x, h[0].y, h[0].z, h[0].w, h[1].x, h[1].y, h[1].z, h[1].w,
                                 h[2].x, h[2].y, h[2].z, h[2].w, h[3].x, h[3].y, h[3].z, h[3].w};
        pass = dpfs::second_ok(F, nat ? s->flags : 0u, hw);
      }
      const unsigned long long bits = __ballot(pass);
      if (lane == 0) bitmap[word0 + k + u] = bits;
      cnt += (uint32_t)__popcll(bits);
    }
  }
  if (lane == 0) wave_cnt[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// The exclusive prefix of the tiles' counts (each thread a run of consecutive
// tiles), the total, and the slot of match number want - 1 (`want` >= 1).
__global__ void __launch_bounds__(kScanTB) fl_snap_scan_k(const uint32_t *tile_cnt, uint32_t *tile_pref,
                                                         uint32_t ntiles, const unsigned long long *bitmap,
                                                         uint64_t slot0, uint32_t want, ScanOut *out) {
  __shared__ uint32_t part[kScanTB];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (ntiles + kScanTB - 1) / kScanTB;
  const uint64_t lo = (uint64_t)t * per < ntiles ? (uint64_t)t * per : ntiles;
  const uint64_t hi = lo + per < ntiles ? lo + per : ntiles;
  uint32_t sum = 0;
  for (uint64_t i = lo; i < hi; i++) sum += tile_cnt[i];
  part[t] = sum;
  __syncthreads();
  // Hillis-Steele inclusive scan of the 1024 partial sums
  for (uint32_t d = 1; d < kScanTB; d <<= 1) {
    const uint32_t add = t >= d ? part[t - d] : 0u;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  if (t == kScanTB - 1) out->total = part[t];
  uint32_t p = part[t] - sum;
  for (uint64_t i = lo; i < hi; i++) {
    const uint32_t n = tile_cnt[i];
    tile_pref[i] = p;
    if (want && p < want && want <= p + n) {  // match number want - 1 sits in tile i
      uint32_t rem = want - 1 - p;
      for (uint32_t w = 0; w < kTileWords; w++) {
        unsigned long long b = bitmap[i * kTileWords + w];
        const uint32_t pc = (uint32_t)__popcll(b);
        if (rem >= pc) { rem -= pc; continue; }
        for (; rem; rem--) b &= b - 1;
        out->last = slot0 + (i * kTileWords + w) * 64u + (uint32_t)(__ffsll(b) - 1);
        break;
      }
    }
    p += n;
  }
}

// One wave per bitmap word in [0, nwords).
__global__ void __launch_bounds__(kTB) fl_snap_emit_k(const FlowSlot *slots, uint32_t mask, uint64_t slot0,
                                                     const unsigned long long *bitmap, const uint32_t *tile_pref,
                                                     uint64_t nwords, uint32_t cap, dp_flow_entry_t *out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t w = (uint64_t)blockIdx.x * (kTB / 64) + (threadIdx.x >> 6);
  if (w >= nwords) return;
  const unsigned long long bits = bitmap[w];
  if (!bits) return;
  // matches before this word: the tile's prefix and its earlier words
  const uint64_t tile = w / kTileWords;
  const uint32_t wi = (uint32_t)(w % kTileWords);
  uint32_t before = lane < wi ? (uint32_t)__popcll(bitmap[tile * kTileWords + lane]) : 0u;
#pragma unroll
  for (uint32_t o = 8; o > 0; o >>= 1) before += __shfl_xor(before, o);
  before = __shfl(before, 0) + tile_pref[tile];
  if (before >= cap) return;
  const uint32_t rank = before + (uint32_t)__popcll(bits & ((1ull << lane) - 1ull));
  if (!((bits >> lane) & 1ull) || rank >= cap) return;

  const uint64_t sl = slot0 + w * 64u + lane;
  const FlowSlot *s = slots + sl;
  const uint4 k0 = ld16(s, 0), k1 = ld16(s, 1), k2 = ld16(s, 2);
  dp_flow_info_t o{};
  o.ref = DP_FLOW_NONE;
  o.related = DP_FLOW_NONE;
  dpfl::fill_info(slots, mask, (uint32_t)sl, o);
  // the record as 34 words: the key as dp_flow_key_t lays it out, the slot,
  // the info
  uint32_t e[34];
  e[0] = k0.y;
  e[1] = k0.z & 0xffffu;
  e[2] = (k0.w >> 16) | (k0.w << 16);
  e[3] = k1.x; e[4] = k1.y; e[5] = k1.z; e[6] = k1.w;
  e[7] = k2.x; e[8] = k2.y; e[9] = k2.z; e[10] = k2.w;
  e[11] = (uint32_t)sl;
  __builtin_memcpy(&e[12], &o, sizeof o);
  static_assert(sizeof(dp_flow_key_t) == 44 && sizeof(dp_flow_info_t) == 88 && sizeof(dp_flow_entry_t) == 136 &&
                    offsetof(dp_flow_entry_t, info) == 48,
                "the record's words");
  // 136 bytes, 8-byte aligned: eight 16-byte stores and one of 8 bytes, the
  // short one first where the record starts on an odd 8-byte unit
  char *dst = reinterpret_cast<char *>(out + rank);
  if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
#pragma unroll
    for (uint32_t j = 0; j < 8; j++)
      *reinterpret_cast<uint4 *>(dst + 16 * j) = make_uint4(e[4 * j], e[4 * j + 1], e[4 * j + 2], e[4 * j + 3]);
    *reinterpret_cast<uint2 *>(dst + 128) = make_uint2(e[32], e[33]);
  } else {
    *reinterpret_cast<uint2 *>(dst) = make_uint2(e[0], e[1]);
#pragma unroll
    for (uint32_t j = 0; j < 8; j++)
      *reinterpret_cast<uint4 *>(dst + 8 + 16 * j) =
          make_uint4(e[2 + 4 * j], e[3 + 4 * j], e[4 + 4 * j], e[5 + 4 * j]);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// A prefix as (mask, value) words; `be`: the words are big-endian numbers
// (use_ip), else the address bytes as stored in a key.  false: invalid.
bool compile_prefix(const dp_prefix_t &p, bool be, dpfs::Pfx &o) {
  if ((p.family != 4 && p.family != 6) || p.len > (p.family == 4 ? 32 : 128)) return false;
  uint8_t m[16] = {0}, v[16] = {0};
  for (uint32_t i = 0; i < p.len; i++) m[i >> 3] |= (uint8_t)(0x80u >> (i & 7u));
  for (int i = 0; i < (p.family == 4 ? 4 : 16); i++) v[i] = p.addr[i] & m[i];
  o.fam = p.family;
  for (int j = 0; j < 4; j++) {
    if (be) {
      o.m[j] = (uint32_t)m[4 * j] << 24 | (uint32_t)m[4 * j + 1] << 16 | (uint32_t)m[4 * j + 2] << 8 | m[4 * j + 3];
      o.v[j] = (uint32_t)v[4 * j] << 24 | (uint32_t)v[4 * j + 1] << 16 | (uint32_t)v[4 * j + 2] << 8 | v[4 * j + 3];
    } else {
      memcpy(&o.m[j], m + 4 * j, 4);
      memcpy(&o.v[j], v + 4 * j, 4);
    }
  }
  return true;
}

// dp_flow_filter_t -> the form the predicate reads.  false: invalid.
bool compile_filter(const dp_flow_filter_t *f, Filter &F) {
  F = Filter{};
  if (!f) return true;
  const uint32_t cl = f->clauses;
  if (cl & ~dpfs::kAllClauses) return false;
  F.clauses = cl;
  F.src_vni = f->src_vni;
  F.dst_vni = f->dst_vni;
  F.family = f->family;
  F.kind_mask = f->kind_mask;
  F.status_mask = f->status_mask;
  F.nat_mask = f->nat_mask;
  F.flags_all = f->flags_all;
  F.flags_none = f->flags_none;
  F.sport_lo = f->sport_lo; F.sport_hi = f->sport_hi;
  F.dport_lo = f->dport_lo; F.dport_hi = f->dport_hi;
  F.nport_lo = f->nat_port_lo; F.nport_hi = f->nat_port_hi;
  F.genid = f->genid;
  F.expires_at = f->expires_at;
  if ((cl & DP_FLOWF_SPORT) && f->sport_lo > f->sport_hi) return false;
  if ((cl & DP_FLOWF_DPORT) && f->dport_lo > f->dport_hi) return false;
  if ((cl & DP_FLOWF_NAT_PORT) && f->nat_port_lo > f->nat_port_hi) return false;
  if ((cl & DP_FLOWF_SRC) && !compile_prefix(f->src, false, F.src)) return false;
  if ((cl & DP_FLOWF_DST) && !compile_prefix(f->dst, false, F.dst)) return false;
  if ((cl & DP_FLOWF_NAT_IP) && !compile_prefix(f->nat_ip, true, F.nat)) return false;
  return true;
}

int snapshot(dp_flow_table *ft, const dp_flow_filter_t *filter, uint64_t *cursor, dp_flow_entry_t *entries,
             uint32_t cap, uint32_t *n_entries, uint64_t *matched, bool device) {
  if (!ft) return dpr_fail(DP_EINVAL, "null table");
  if (cap && !entries) return dpr_fail(DP_EINVAL, "entries NULL with cap > 0");
  Filter F;
  if (!compile_filter(filter, F)) return dpr_fail(DP_EINVAL, "invalid flow filter");
  const uint64_t c0 = cursor ? *cursor : 0;
  if (c0 > ft->nslots) return dpr_fail(DP_EINVAL, "cursor beyond the table");
  uint64_t total = 0, next = ft->nslots;
  uint32_t n = 0;
  if (c0 < ft->nslots) {
    std::lock_guard<std::mutex> lk(ft->mu);
    const uint64_t slot0 = c0 / kTileSlots * kTileSlots;  // the bitmap's first slot
    const uint32_t ntiles = (uint32_t)((ft->nslots - slot0 + kTileSlots - 1) / kTileSlots);
    FlowScratch &sw = ft->scr[0], &se = ft->scr[1];
    ScanOut so{0, 0};
    int rc = dpfl::run(ft, "flow snapshot", [&](hipStream_t st) {
      // bitmap | scan result | tile counts | tile prefixes
      const size_t bm_bytes = sizeof(unsigned long long) * kTileWords * (size_t)ntiles;
      char *w = static_cast<char *>(sw.get(bm_bytes + sizeof(ScanOut) + 2 * sizeof(uint32_t) * (size_t)ntiles));
      if (!w) return dpr_fail(DP_ENOMEM, "flow scratch");
      unsigned long long *bm = reinterpret_cast<unsigned long long *>(w);
      ScanOut *dso = reinterpret_cast<ScanOut *>(w + bm_bytes);
      uint32_t *cnt = reinterpret_cast<uint32_t *>(dso + 1), *pref = cnt + ntiles;
      hipLaunchKernelGGL(fl_snap_mark_k, dim3(ntiles), dim3(kTB), 0, st, ft->slots, ft->nslots, c0, F, bm, cnt);
      hipLaunchKernelGGL(fl_snap_scan_k, dim3(1), dim3(kScanTB), 0, st, cnt, pref, ntiles, bm, slot0, cap, dso);
      if (hipMemcpyAsync(&so, dso, sizeof so, hipMemcpyDeviceToHost, st) != hipSuccess)
        return dpr_fail(DP_EIO, "flow snapshot copy");
      hipError_t e = hipStreamSynchronize(st);
      if (e != hipSuccess) return dpr_fail(DP_EIO, "flow snapshot scan", e);
      total = so.total;
      n = total < cap ? (uint32_t)total : cap;
      // the end was reached, or the slot after the last entry
      next = total <= cap ? ft->nslots : cap ? so.last + 1 : c0;
      if (!n) return 0;  // count-only, or nothing matched
      dp_flow_entry_t *de = entries;
      if (!device && !(de = static_cast<dp_flow_entry_t *>(se.get(sizeof(dp_flow_entry_t) * (size_t)n))))
        return dpr_fail(DP_ENOMEM, "flow scratch");
      // the words up to the last entry's
      const uint64_t end = total <= cap ? ft->nslots : so.last + 1;
      const uint64_t nwords = (end - slot0 + 63) / 64;
      hipLaunchKernelGGL(fl_snap_emit_k, dim3((uint32_t)((nwords + kTB / 64 - 1) / (kTB / 64))), dim3(kTB), 0, st,
                         ft->slots, ft->mask, slot0, bm, pref, nwords, cap, de);
      if (!device &&
          hipMemcpyAsync(entries, de, sizeof(dp_flow_entry_t) * (size_t)n, hipMemcpyDeviceToHost, st) != hipSuccess)
        return dpr_fail(DP_EIO, "flow snapshot copy");
      return 0;
    });
    if (rc) return rc;
  }
  if (cursor) *cursor = next;
  if (n_entries) *n_entries = n;
  if (matched) *matched = total;
  return 0;
}

}  // namespace

extern "C" {

int dp_flow_filter_match(const dp_flow_filter_t *filter, const dp_flow_key_t *key, const dp_flow_info_t *info) {
  Filter F;
  if (!key || !info || !compile_filter(filter, F)) return DP_EINVAL;
  // the flow as the words of a slot that stores it
  uint32_t w[32] = {0};
  const dpf::FKey k = dpfl::key_words(*key);
  w[0] = dpf::FS_FULL;
  for (int i = 0; i < 11; i++) w[1 + i] = k.w[i];
  w[12] = info->status;
  w[13] = info->flags & 7u;
  w[14] = info->dst_vni;
  w[15] = dpf::kNoSlot;
  w[18] = (uint32_t)(uint64_t)info->genid;
  w[19] = (uint32_t)((uint64_t)info->genid >> 32);
  w[20] = (uint32_t)info->expires_at;
  w[21] = (uint32_t)(info->expires_at >> 32);
  const uint32_t action = info->pf != DP_PF_NONE ? info->pf : info->masq;
  if (info->pf != DP_PF_NONE) w[13] |= dpf::kFlagPf;
  if (info->masq != DP_PF_NONE) w[13] |= dpf::kFlagMasq;
  if (action != DP_PF_NONE) {
    w[22] = action | (uint32_t)info->pf_status << 8 | (uint32_t)info->pf_port << 16;
    for (int j = 0; j < 4; j++)
      w[24 + j] = (uint32_t)info->pf_ip[4 * j] << 24 | (uint32_t)info->pf_ip[4 * j + 1] << 16 |
                  (uint32_t)info->pf_ip[4 * j + 2] << 8 | info->pf_ip[4 * j + 3];
    w[28] = info->pf_family;
    w[29] = info->masq != DP_PF_NONE && info->masq_alloc ? 1u : 0u;
  }
  return dpfs::slot_ok(F, w) ? 1 : 0;
}

int dp_flow_snapshot(dp_flow_table_t *ft, const dp_flow_filter_t *filter, uint64_t *cursor, dp_flow_entry_t *entries,
                     uint32_t cap, uint32_t *n_entries, uint64_t *matched) {
  return snapshot(ft, filter, cursor, entries, cap, n_entries, matched, false);
}

int dp_flow_snapshot_device(dp_flow_table_t *ft, const dp_flow_filter_t *filter, uint64_t *cursor,
                            dp_flow_entry_t *dev_entries, uint32_t cap, uint32_t *n_entries, uint64_t *matched) {
  return snapshot(ft, filter, cursor, dev_entries, cap, n_entries, matched, true);
}

}  // extern "C"
