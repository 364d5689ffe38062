// SPDX-License-Identifier: Apache-2.0
//
// Filtered packet capture on the device (include/dpgpu.h "Packet capture"): an
// order-preserving compaction of variable-length frames.  The selected
// packets of a burst are appended, in burst order, to the context's capture
// buffer -- a 32-byte record each and their bytes packed in 16-byte units --
// by three launches, none of which waits on another workgroup:
//
//  1. dp_capture_select_k: a workgroup of 256 takes a tile of 1024 packets in
//     four rounds (packet tile*1024 + r*256 + tid in round r, so the record
//     loads coalesce).  A lane loads its four records, then the head of each
//     frame -- five 16-byte loads from the 16-byte boundary at or below the
//     frame's start, which hold the frame's first 64 bytes at any alignment --
//     with all of them in flight before the first parse.  A round's heads go
//     through a lane-private, transposed LDS slab so the parse can index bytes
//     at run-time positions without scratch; bytes past the head (IPv6
//     extension headers, IPv4 options behind two tags) are single global
//     loads.  The filter is a kernel argument (scalar registers).  Out: one
//     select word a packet (match bit + caplen) and the tile's (matches,
//     units), reduced by ballots / a DPP wave sum and one LDS step.
//  2. dp_capture_scan_k: one workgroup scans the tile totals exclusively
//     (wave scans, LDS across the waves, 1024 tiles a trip), starting from the
//     buffer's device-resident counters; finds the first tile that does not
//     fit whole and, with a scan of that tile's select words, the exact record
//     where capacity ends; leaves every tile its bases and kept count and
//     updates the counters.
//  3. dp_capture_copy_k: same tiling.  The tile's select words are scanned in
//     LDS into record slots and unit offsets (a table of at most 1024
//     entries), the kept records are built 256 at a time and leave through
//     LDS as consecutive 16-byte stores, and the bytes are copied by OUTPUT
//     UNIT, not by packet: lane tid takes units tid, tid + 256, ... of the
//     tile, finds the owning record by binary search in the offset table (at
//     most 10 steps), reads 16 source bytes at the frame's true address (two
//     aligned 16-byte loads and a byte funnel, one load when aligned), zeroes
//     what lies past caplen and stores one aligned vector.  Stores are fully
//     coalesced and the work is balanced to a unit however 64-byte and
//     1514-byte frames mix in a wave; tiles past the cut do nothing.
#include <hip/hip_runtime.h>

#include "dp_capture.h"

namespace {

using namespace dpc;
using u64 = unsigned long long;

constexpr uint32_t kHeadChunks = 5;                  // 16-byte loads a frame head
constexpr uint32_t kHeadBytes = 16 * kHeadChunks;    // from the boundary below the frame
constexpr uint32_t kHeadWords = kHeadBytes / 4;
constexpr uint32_t kNoProto = 0xffffffffu;
constexpr uint32_t kScanTpb = 1024;

__device__ __forceinline__ bool frame_inside(uint32_t off, uint32_t len, bool rx, u64 buf_bytes) {
  // the layout contract of dp_process_burst_device (a received frame also
  // owns DP_HEADROOM bytes in front of it)
  return (!rx || off >= DP_HEADROOM) && (((u64)off + len + 15) & ~15ull) <= buf_bytes;
}

template <int kCtrl, int kRowMask>
__device__ __forceinline__ uint32_t dpp_add(uint32_t v) {
  return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, kRowMask, 0xf, false);
}
// Sum of v over the 64 lanes (all active), uniform (VALU only, as the Stats stage's).
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  v = dpp_add<0xb1, 0xf>(v);   // quad_perm:[1,0,3,2]
  v = dpp_add<0x4e, 0xf>(v);   // quad_perm:[2,3,0,1]
  v = dpp_add<0x124, 0xf>(v);  // row_ror:4
  v = dpp_add<0x128, 0xf>(v);  // row_ror:8
  v = dpp_add<0x142, 0xa>(v);  // row_bcast:15 into rows 1, 3
  v = dpp_add<0x143, 0xc>(v);  // row_bcast:31 into rows 2, 3
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// Inclusive scan of v over the workgroup's kWaves waves in thread order (all
// threads call): a wave scan, the waves' totals through `ws`, `total` the sum.
template <uint32_t kWaves>
__device__ __forceinline__ u64 block_scan(u64 v, u64 *ws, u64 &total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const u64 t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  __syncthreads();  // (ws may still be read from the scan before)
  if (lane == 63) ws[wave] = v;
  __syncthreads();
  u64 add = 0, all = 0;
  for (uint32_t w = 0; w < kWaves; w++) {
    const u64 t = ws[w];
    if (w < wave) add += t;
    all += t;
  }
  total = all;
  return v + add;
}

// A frame's head as the parse reads it: the lane's column of the LDS slab
// (word w of the head at lw[w][tid]), `sh` the frame's start inside the first
// chunk, `g` the chunk's address for the bytes past the head.
struct Head {
  const uint32_t (*lw)[kTpb];
  const uint8_t *g;
  uint32_t tid, sh;
  __device__ __forceinline__ uint32_t b8(uint32_t pos) const {
    const uint32_t q = sh + pos;
    if (q < kHeadBytes) return (lw[q >> 2][tid] >> (8 * (q & 3))) & 0xffu;
    return g[q];  // rare: past the head (the caller keeps pos inside the frame)
  }
  __device__ __forceinline__ uint32_t be16(uint32_t pos) const { return b8(pos) << 8 | b8(pos + 1); }
  // four bytes in memory order
  __device__ __forceinline__ uint32_t w32(uint32_t pos) const {
    const uint32_t q = sh + pos;
    if (q + 4 <= kHeadBytes) {
      const uint32_t lo = lw[q >> 2][tid], hi = (q & 3) ? lw[(q >> 2) + 1][tid] : 0u;
      return __builtin_amdgcn_alignbyte(hi, lo, q & 3);
    }
    return b8(pos) | b8(pos + 1) << 8 | b8(pos + 2) << 16 | b8(pos + 3) << 24;
  }
};

__device__ __forceinline__ bool in_prefix(const Head &H, uint32_t pos, uint32_t fam, const uint32_t *pfx,
                                          const uint32_t *mask) {
  const uint32_t words = fam == 4 ? 1u : 4u;
  for (uint32_t i = 0; i < words; i++)
    if (mask[i] && ((H.w32(pos + 4 * i) ^ pfx[i]) & mask[i])) return false;
  return true;
}

// The filter over one packet: the small parse of the outermost headers
// (include/dpgpu.h states its boundary) and the clauses.  `frame`: the packet
// has a frame of L bytes behind H.
__device__ __forceinline__ bool filter_match(const Filter &f, const Head &H, bool frame, uint32_t L, uint32_t done,
                                             uint2 vni) {
  uint32_t cls = 0, fam = 0, src = 0, dst = 0, sport = 0, dport = 0;
  bool ports = false;
  if (frame && L >= 14 && (f.clauses & (DP_CAPF_L4 | DP_CAPF_SRC | DP_CAPF_DST | DP_CAPF_SPORT | DP_CAPF_DPORT))) {
    uint32_t et = H.be16(12), p = 14, proto = kNoProto, l4 = 0;
    for (int t = 0; t < 2; t++)
      if ((et == 0x8100u || et == 0x88a8u) && p + 4 <= L) {
        et = H.be16(p + 2);
        p += 4;
      }
    if (et == 0x0800u && p + 20 <= L) {
      const uint32_t ihl = H.b8(p) & 15u;
      if (ihl >= 5 && p + 4 * ihl <= L) {
        fam = 4, src = p + 12, dst = p + 16, l4 = p + 4 * ihl;
        proto = (H.be16(p + 6) & 0x1fffu) ? kNoProto : H.b8(p + 9);
      }
    } else if (et == 0x86ddu && p + 40 <= L) {
      fam = 6, src = p + 8, dst = p + 24, l4 = p + 40;
      proto = H.b8(p + 6);
      for (int k = 0; k < 3; k++) {
        if (proto == 0 || proto == 43 || proto == 60) {
          if (l4 + 2 > L) { proto = kNoProto; break; }
          proto = H.b8(l4);
          l4 += (H.b8(l4 + 1) + 1) * 8;
        } else if (proto == 44) {
          if (l4 + 8 > L || (H.be16(l4 + 2) & 0xfff8u)) { proto = kNoProto; break; }
          proto = H.b8(l4);
          l4 += 8;
        } else {
          break;
        }
      }
    }
    if (fam == 4 && proto == 1) cls |= DP_CAPC_ICMP4;
    if (fam == 6 && proto == 58) cls |= DP_CAPC_ICMP6;
    if (proto == 17 || proto == 6) {
      cls |= proto == 17 ? DP_CAPC_UDP : DP_CAPC_TCP;
      if (l4 + 4 <= L) {
        ports = true, sport = H.be16(l4), dport = H.be16(l4 + 2);
        if (proto == 17 && (sport == 4789 || dport == 4789)) cls |= DP_CAPC_VXLAN;
      }
    }
  }
  const uint32_t c = f.clauses;
  bool ok = true;
  if (c & DP_CAPF_L4) ok = (cls & f.l4_mask) != 0;
  if (ok && (c & DP_CAPF_SRC)) ok = fam == f.src_fam && in_prefix(H, src, fam, f.src, f.src_mask);
  if (ok && (c & DP_CAPF_DST)) ok = fam == f.dst_fam && in_prefix(H, dst, fam, f.dst, f.dst_mask);
  if (ok && (c & DP_CAPF_SPORT)) ok = ports && sport >= f.sport_lo && sport <= f.sport_hi;
  if (ok && (c & DP_CAPF_DPORT)) ok = ports && dport >= f.dport_lo && dport <= f.dport_hi;
  if (ok && (c & DP_CAPF_DONE)) ok = done < 64 && ((f.done_mask >> done) & 1ull);
  if (ok && (c & DP_CAPF_SRC_VNI)) ok = vni.y == f.src_vni;  // dp_pkt_meta_t: dst_vni, src_vni
  if (ok && (c & DP_CAPF_DST_VNI)) ok = vni.x == f.dst_vni;
  return ok;
}

// A burst record as both taps read it: x = off, y = len | (TX: done << 16).
template <bool TX>
__device__ __forceinline__ void rec_fields(uint4 r, uint32_t &off, uint32_t &len, uint32_t &done) {
  off = r.x;
  len = r.y & 0xffffu;
  done = TX ? (r.y >> 16) & 0xffu : (uint32_t)DP_DONE_NONE;
}

template <bool TX>
__global__ __launch_bounds__(kTpb) void dp_capture_select_k(const uint8_t *__restrict__ buf, u64 buf_bytes,
                                                            const uint4 *__restrict__ recs,
                                                            const dp_pkt_meta_t *__restrict__ meta, uint32_t n,
                                                            const Filter f, uint32_t *__restrict__ sel,
                                                            uint2 *__restrict__ tot) {
  __shared__ uint32_t lw[kHeadWords][kTpb];
  __shared__ uint32_t wm[kTpb / 64], wu[kTpb / 64];
  const uint32_t tid = threadIdx.x;
  const u64 first = (u64)blockIdx.x * kTile;
  const bool want_vni = TX && meta && (f.clauses & (DP_CAPF_SRC_VNI | DP_CAPF_DST_VNI));
  // every load of the lane before the first parse: the records, then the heads
  uint4 rec[4];
  uint2 vni[4];
#pragma unroll
  for (uint32_t r = 0; r < 4; r++) {
    const u64 p = first + r * kTpb + tid;
    rec[r] = make_uint4(0, 0, 0, 0);
    vni[r] = make_uint2(0, 0);
    if (p < n) {
      rec[r] = recs[p];
      if (want_vni) vni[r] = *reinterpret_cast<const uint2 *>(meta + p);
    }
  }
  uint4 h[4][kHeadChunks];
  bool frame[4];
#pragma unroll
  for (uint32_t r = 0; r < 4; r++) {
    uint32_t off, len, done;
    rec_fields<TX>(rec[r], off, len, done);
    frame[r] = first + r * kTpb + tid < n && (!TX || done == DP_DONE_DELIVERED) &&
               frame_inside(off, len, !TX, buf_bytes);
    const u64 a = off & ~15u, end = ((u64)off + len + 15) & ~15ull;
#pragma unroll
    for (uint32_t k = 0; k < kHeadChunks; k++) {
      h[r][k] = make_uint4(0, 0, 0, 0);
      if (frame[r] && a + 16 * k < end) h[r][k] = *reinterpret_cast<const uint4 *>(buf + a + 16 * k);
    }
  }
  uint32_t units = 0, matches = 0;
#pragma unroll
  for (uint32_t r = 0; r < 4; r++) {
    uint32_t off, len, done;
    rec_fields<TX>(rec[r], off, len, done);
    // the lane's own column of the slab: no other lane reads it, so the
    // rounds need no barrier between them
#pragma unroll
    for (uint32_t k = 0; k < kHeadChunks; k++) {
      lw[4 * k + 0][tid] = h[r][k].x;
      lw[4 * k + 1][tid] = h[r][k].y;
      lw[4 * k + 2][tid] = h[r][k].z;
      lw[4 * k + 3][tid] = h[r][k].w;
    }
    const Head H{lw, buf + (off & ~15u), tid, off & 15u};
    const u64 p = first + r * kTpb + tid;
    const bool m = p < n && filter_match(f, H, frame[r], len, done, vni[r]);
    const uint32_t caplen = frame[r] ? (f.snaplen && f.snaplen < len ? f.snaplen : len) : 0u;
    if (p < n) sel[p] = m ? kSelMatch | caplen : 0u;
    matches += (uint32_t)__popcll(__ballot(m));
    units += m ? (caplen + 15) >> 4 : 0u;
  }
  units = wave_sum(units);
  if ((tid & 63) == 0) {
    wm[tid >> 6] = matches;
    wu[tid >> 6] = units;
  }
  __syncthreads();
  if (tid == 0) tot[blockIdx.x] = make_uint2(wm[0] + wm[1] + wm[2] + wm[3], wu[0] + wu[1] + wu[2] + wu[3]);
}

__global__ __launch_bounds__(kScanTpb) void dp_capture_scan_k(const uint2 *__restrict__ tot,
                                                              const uint32_t *__restrict__ sel, uint32_t n,
                                                              uint32_t tiles, State *st, TileBase *__restrict__ base,
                                                              uint32_t max_records, u64 max_units) {
  __shared__ u64 ws[kScanTpb / 64];
  __shared__ uint32_t cut, cut_keep, cut_units;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) cut = 0xffffffffu, cut_keep = 0, cut_units = 0;
  const u64 recs0 = st->n_recs, units0 = st->n_units;
  u64 run_m = 0, run_u = 0;  // matches / units of the tiles before this trip
  for (uint32_t t0 = 0; t0 < tiles; t0 += kScanTpb) {
    const uint32_t t = t0 + tid;
    const uint2 mine = t < tiles ? tot[t] : make_uint2(0, 0);
    u64 all_m, all_u;
    const u64 m1 = block_scan<kScanTpb / 64>(mine.x, ws, all_m), u1 = block_scan<kScanTpb / 64>(mine.y, ws, all_u);
    const u64 rb = recs0 + run_m + m1 - mine.x, ub = units0 + run_u + u1 - mine.y;  // exclusive
    // (sums are monotone: once a tile does not fit whole, no later tile with a match does)
    const bool fits = rb + mine.x <= max_records && ub + mine.y <= max_units;
    if (t < tiles) {
      base[t] = TileBase{ub, (uint32_t)(rb < max_records ? rb : max_records), fits ? mine.x : 0u};
      if (!fits) atomicMin(&cut, t);
    }
    run_m += all_m;
    run_u += all_u;
  }
  __syncthreads();
  u64 kept = run_m, kept_units = run_u;
  const uint32_t ct = cut;
  if (ct != 0xffffffffu) {
    // the first tile that does not fit whole: its exact cut, by packet
    const TileBase b = base[ct];
    const u64 p = (u64)ct * kTile + tid;
    const uint32_t w = p < n ? sel[p] : 0u;
    const uint32_t m = w >> 31, u = m ? ((w & 0xffffu) + 15) >> 4 : 0u;
    u64 all;
    const u64 inc = block_scan<kScanTpb / 64>((u64)m << 32 | u, ws, all);
    const u64 slot = (inc >> 32) - m, ue = (inc & 0xffffffffu);  // this record's slot, its end in units
    if (m && b.rec_base + slot < max_records && b.unit_base + ue <= max_units) {
      atomicMax(&cut_keep, (uint32_t)slot + 1);
      atomicMax(&cut_units, (uint32_t)ue);
    }
    __syncthreads();
    if (tid == 0) base[ct].keep = cut_keep;
    kept = (b.rec_base - recs0) + cut_keep;
    kept_units = (b.unit_base - units0) + cut_units;
  }
  if (tid == 0) {
    st->n_recs = (uint32_t)(recs0 + kept);
    st->n_units = units0 + kept_units;
    st->matched += run_m;
    st->lost += run_m - kept;
    st->cur_burst = st->burst;
    st->burst = st->cur_burst + 1;
  }
}

template <bool TX>
__global__ __launch_bounds__(kTpb) void dp_capture_copy_k(const uint8_t *__restrict__ buf,
                                                          const uint4 *__restrict__ recs,
                                                          const dp_pkt_meta_t *__restrict__ meta, uint32_t n,
                                                          const uint32_t *__restrict__ sel,
                                                          const TileBase *__restrict__ base, const State *st,
                                                          uint4 *__restrict__ out_recs, uint4 *__restrict__ out_bytes) {
  const TileBase tb = base[blockIdx.x];
  const uint32_t K = tb.keep;
  if (K == 0) return;  // no match, or past the cut
  __shared__ __attribute__((aligned(16))) uint32_t lsel[kTile];
  __shared__ uint32_t uoff[kTile + 1];  // slot -> its first unit in the tile
  __shared__ uint32_t soff[kTile];      // slot -> its frame's offset in the burst buffer
  __shared__ uint16_t pidx[kTile];      // slot -> packet of the tile
  __shared__ uint16_t clen[kTile];      // slot -> caplen
  __shared__ uint4 stage[2 * kTpb];     // 256 records on their way out
  __shared__ u64 ws[kTpb / 64];
  const uint32_t tid = threadIdx.x;
  const u64 first = (u64)blockIdx.x * kTile;
#pragma unroll
  for (uint32_t r = 0; r < 4; r++) {
    const u64 p = first + r * kTpb + tid;
    lsel[r * kTpb + tid] = p < n ? sel[p] : 0u;
  }
  __syncthreads();
  // packets 4 tid .. 4 tid + 3: their slots and unit offsets in packet order
  const uint4 w4 = *reinterpret_cast<const uint4 *>(&lsel[4 * tid]);
  const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
  u64 mine = 0;
#pragma unroll
  for (uint32_t i = 0; i < 4; i++)
    if (w[i] >> 31) mine += 1ull << 32 | (((w[i] & 0xffffu) + 15) >> 4);
  u64 all;
  const u64 ex = block_scan<kTpb / 64>(mine, ws, all) - mine;
  uint32_t slot = (uint32_t)(ex >> 32), u0 = (uint32_t)ex;
#pragma unroll
  for (uint32_t i = 0; i < 4; i++)
    if (w[i] >> 31) {
      const uint32_t un = ((w[i] & 0xffffu) + 15) >> 4;
      if (slot < K) {
        pidx[slot] = (uint16_t)(4 * tid + i);
        uoff[slot] = u0;
        if (slot == K - 1) uoff[K] = u0 + un;
      }
      slot++;
      u0 += un;
    }
  __syncthreads();
  // the kept records, 256 at a time through LDS: consecutive 16-byte stores
  const uint32_t burst = st->cur_burst;
  for (uint32_t c0 = 0; c0 < K; c0 += kTpb) {
    const uint32_t j = c0 + tid;
    if (j < K) {
      const uint32_t pi = pidx[j], caplen = lsel[pi] & 0xffffu;
      const u64 p = first + pi;
      uint32_t off, len, done;
      rec_fields<TX>(recs[p], off, len, done);
      uint2 vni = make_uint2(0, 0);
      if (TX && meta) vni = *reinterpret_cast<const uint2 *>(meta + p);
      const u64 boff = (tb.unit_base + uoff[j]) << 4;
      stage[2 * tid] = make_uint4((uint32_t)boff, (uint32_t)(boff >> 32), burst, (uint32_t)p);
      stage[2 * tid + 1] = make_uint4(len | caplen << 16, (TX ? DP_CAP_TX : DP_CAP_RX) | done << 8, vni.y, vni.x);
      soff[j] = off;
      clen[j] = (uint16_t)caplen;
    }
    __syncthreads();
    const uint32_t cnt = 2 * (K - c0 < kTpb ? K - c0 : kTpb);
    for (uint32_t q = tid; q < cnt; q += kTpb) out_recs[2 * ((u64)tb.rec_base + c0) + q] = stage[q];
    __syncthreads();
  }
  // the bytes, by output unit
  const uint32_t U = uoff[K];
  for (uint32_t u = tid; u < U; u += kTpb) {
    uint32_t lo = 0, hi = K;  // the last slot that starts at or before u (empty records start where the next does)
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (uoff[mid] <= u) lo = mid;
      else hi = mid;
    }
    const uint32_t k = u - uoff[lo];
    const int valid = (int)clen[lo] - (int)(16 * k);  // bytes of this unit, >= 1 (16 or more: a whole one)
    const uint8_t *s = buf + soff[lo] + 16 * k;
    const uint32_t sh = (uint32_t)((uintptr_t)s & 15);
    const uint4 *a = reinterpret_cast<const uint4 *>(s - sh);
    const uint4 v0 = a[0];
    uint4 v1 = make_uint4(0, 0, 0, 0);
    if ((int)sh + (valid < 16 ? valid : 16) > 16) v1 = a[1];  // (only where the frame reaches into it)
    const uint32_t x[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    const uint32_t ds = sh >> 2, bs = sh & 3;
    uint32_t y[5], o[4];
#pragma unroll
    for (uint32_t i = 0; i < 5; i++)
      y[i] = ds == 0 ? x[i] : ds == 1 ? x[i + 1] : ds == 2 ? x[i + 2] : x[i + 3 < 8 ? i + 3 : 7];
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {
      const int nb = valid - 4 * (int)i;
      const uint32_t keep = nb >= 4 ? 0xffffffffu : nb <= 0 ? 0u : (1u << (8 * nb)) - 1;
      o[i] = __builtin_amdgcn_alignbyte(y[i + 1], y[i], bs) & keep;
    }
    out_bytes[tb.unit_base + u] = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

__global__ void dp_capture_reset_k(State *st) {
  if (threadIdx.x == 0) *st = State{};
}

}  // namespace

// One capture launch over n records on `stream`: the three kernels.  `scratch`
// holds dpc::scratch_bytes(n); the capture arrays hold max_records records and
// max_units units.  The caller has checked the tap / clause / meta rules.
extern "C" int dpk_capture(int tap, const uint8_t *buf, uint64_t buf_bytes, const void *recs,
                           const dp_pkt_meta_t *meta, uint32_t n, const dpc::Filter *f, void *scratch,
                           void *state, void *out_recs, void *out_bytes, uint32_t max_records,
                           uint64_t max_units, hipStream_t stream) {
  if (n == 0) return 0;
  const uint32_t tiles = (uint32_t)tiles_of(n);
  uint32_t *sel = static_cast<uint32_t *>(scratch);
  uint2 *tot = reinterpret_cast<uint2 *>(static_cast<uint8_t *>(scratch) + (((uint64_t)n * 4 + 15) & ~15ull));
  TileBase *base = reinterpret_cast<TileBase *>(tot + tiles);
  State *st = static_cast<State *>(state);
  const uint4 *r = static_cast<const uint4 *>(recs);
  uint4 *orec = static_cast<uint4 *>(out_recs), *obytes = static_cast<uint4 *>(out_bytes);
  if (tap == DP_CAP_TX)
    hipLaunchKernelGGL(dp_capture_select_k<true>, dim3(tiles), dim3(kTpb), 0, stream, buf, buf_bytes, r, meta, n, *f,
                       sel, tot);
  else
    hipLaunchKernelGGL(dp_capture_select_k<false>, dim3(tiles), dim3(kTpb), 0, stream, buf, buf_bytes, r, meta, n,
                       *f, sel, tot);
  hipLaunchKernelGGL(dp_capture_scan_k, dim3(1), dim3(kScanTpb), 0, stream, tot, sel, n, tiles, st, base, max_records,
                     max_units);
  if (tap == DP_CAP_TX)
    hipLaunchKernelGGL(dp_capture_copy_k<true>, dim3(tiles), dim3(kTpb), 0, stream, buf, r, meta, n, sel, base, st,
                       orec, obytes);
  else
    hipLaunchKernelGGL(dp_capture_copy_k<false>, dim3(tiles), dim3(kTpb), 0, stream, buf, r, meta, n, sel, base, st,
                       orec, obytes);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// Empty the buffer on `stream` (a kernel, so the clear may sit in a captured graph).
extern "C" int dpk_capture_reset(void *state, hipStream_t stream) {
  hipLaunchKernelGGL(dp_capture_reset_k, dim3(1), dim3(64), 0, stream, static_cast<dpc::State *>(state));
  return hipGetLastError() == hipSuccess ? 0 : -5;
}
