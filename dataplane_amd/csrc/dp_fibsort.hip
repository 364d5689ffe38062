// SPDX-License-Identifier: Apache-2.0
//
// The route lists of a device-built v4 FIB made on the device
// (DP_OPT_DEVICE_FIB = 2, include/dpgpu.h): the FIB's routes arrive as 8-byte
// records in insertion order (dp_fibsort.h) and leave as the Short / Long /
// Block lists of dp_fibbuild.h, element for element what the table compiler's
// stable_sort, duplicate pass and stack walk give (dp_tables.cpp
// reserve_dir248).  Integer work for wave 64; every phase is a launch of its
// own on one stream, so no workgroup waits on or spins for another, and no
// loop's trip count depends on the records beyond a fixed bound.
//
//  1. Stable LSD radix sort of the 38-bit key (address, length), five passes
//     (the 6-bit length digit, then the address bytes, low to high), the
//     records ping-ponging between two buffers.  A pass is three launches:
//      - dp_fibsort_hist_k: a workgroup of 256 counts the digits of its tile
//        of 2048 records in LDS and writes them digit-major
//        (hist[digit * tiles + tile]);
//      - dp_fibsort_scan_k: one workgroup of 1024 turns that array into its
//        exclusive prefix sum in place -- position of (digit, tile)'s first
//        record in the output -- carrying a running total from step to step;
//      - dp_fibsort_scatter_k: a wave owns a contiguous 512 records of the
//        tile and takes them 64 at a time in memory order.  Eight ballots over
//        the digit's bits give each lane the mask of lanes holding its digit:
//        its rank among them is the popcount of the lower lanes, the first of
//        them adds the group to the wave's counter of that digit in LDS and
//        broadcasts the old value.  The four waves' counters are then turned
//        into bases (an exclusive scan over the digits, earlier waves first),
//        the records are staged in LDS at base + rank -- the tile sorted by
//        digit, ties in memory order -- and written out in that order, so a
//        digit's records leave as one contiguous run behind the scanned
//        position.  Equal digits keep tile order and then in-tile order: the
//        pass is stable, which is what makes the last insert of a prefix the
//        last of its run.
//  2. dp_fibsort_count_k / dp_fibsort_scan_k: per tile of the sorted records
//     the survivors (the last of each run of equal keys) of length <= 24 and
//     of length 25..32, and the block heads (dp_fibsort.h classify); the scan
//     kernel over the three count arrays laid end to end gives every tile its
//     three list positions and the three totals.
//  3. dp_fibsort_emit_k: a lane takes 8 consecutive records, a workgroup scan
//     of the flags gives each survivor its position: Short{slot, len, nh}
//     (parent left for the next kernel), the Long word, and the Block record's
//     slot and first.  dp_fibsort_parent_k: one lane a short route; for
//     L = len - 1 down to 0 it binary-searches the Short list (sorted by
//     (slot, len)) for the route's address masked to L -- the first hit is the
//     nearest enclosing route, the host's stack top.  At most 24 searches of at
//     most 27 steps, each over the part of the list below the last miss.
//     dp_fibsort_blockcount_k: a block's count is the next block's first (or
//     the long total) minus its own.
//
// Bounds: a scatter's destinations are the scan of the histogram of the very
// records it moves; list positions are the scan of the flags the emit kernel
// recomputes, and are checked against the capacities the host allocated.
#include <hip/hip_runtime.h>

#include "dp_fibsort.h"

namespace {

using namespace dps;
using dpb::Block;
using dpb::Long;
using dpb::Short;

// exclusive prefix of v over the workgroup (waves of 64, at most 16), and the total
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *s_w, uint32_t &total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(incl, d);
    if (lane >= d) incl += t;
  }
  if (lane == 63) s_w[wave] = incl;
  __syncthreads();
  uint32_t before = 0, tot = 0;
  for (uint32_t w = 0; w < nw; w++) {
    const uint32_t x = s_w[w];
    before += w < wave ? x : 0;
    tot += x;
  }
  __syncthreads();  // s_w may be written again
  total = tot;
  return before + incl - v;
}

__global__ __launch_bounds__(kTpb) void dp_fibsort_hist_k(const Raw *in, uint32_t n, uint32_t shift, uint32_t mask,
                                                          uint32_t tiles, uint32_t *hist) {
  __shared__ uint32_t s_h[kDigits];
  const uint32_t tid = threadIdx.x, tile0 = blockIdx.x * kTile;
  s_h[tid] = 0;
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < kKpt; k++) {
    const uint32_t i = tile0 + k * kTpb + tid;
    if (i < n) atomicAdd(&s_h[(uint32_t)(in[i] >> shift) & mask], 1u);
  }
  __syncthreads();
  if (tid <= mask) hist[tid * tiles + blockIdx.x] = s_h[tid];
}

// v[0, m) becomes its exclusive prefix sum, v[m] the total.  One workgroup.
__global__ __launch_bounds__(kScanTpb) void dp_fibsort_scan_k(uint32_t *v, uint32_t m) {
  __shared__ uint32_t s_w[kScanTpb / 64];
  const uint32_t tid = threadIdx.x;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < m; base += kScanTpb * kScanPer) {
    const uint32_t i = base + tid * kScanPer;
    uint32_t x[kScanPer], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < kScanPer; k++) {
      x[k] = i + k < m ? v[i + k] : 0;
      sum += x[k];
    }
    uint32_t tot;
    uint32_t run = carry + block_excl_scan(sum, s_w, tot);
#pragma unroll
    for (uint32_t k = 0; k < kScanPer; k++) {
      if (i + k < m) v[i + k] = run;
      run += x[k];
    }
    carry += tot;
  }
  if (tid == 0) v[m] = carry;
}

__global__ __launch_bounds__(kTpb) void dp_fibsort_scatter_k(const Raw *in, Raw *out, uint32_t n, uint32_t shift,
                                                             uint32_t mask, uint32_t tiles, const uint32_t *hist) {
  __shared__ Raw s_rec[kTile];                     // the tile in digit order
  __shared__ uint32_t s_cnt[kTpb / 64][kDigits];   // per wave and digit: records so far, then the base
  __shared__ uint32_t s_start[kDigits];            // first position of a digit in s_rec
  __shared__ uint32_t s_goff[kDigits];             // first output position of (digit, this tile)
  __shared__ uint32_t s_w[kTpb / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t tile0 = blockIdx.x * kTile;
#pragma unroll
  for (uint32_t w = 0; w < kTpb / 64; w++) s_cnt[w][tid] = 0;
  s_goff[tid] = tid <= mask ? hist[tid * tiles + blockIdx.x] : 0;
  __syncthreads();

  Raw rec[kKpt];
  uint32_t rank[kKpt];
  const uint64_t lower = (1ull << lane) - 1;
#pragma unroll
  for (uint32_t r = 0; r < kKpt; r++) {
    const uint32_t i = tile0 + wave * kWaveKeys + r * 64 + lane;
    const bool valid = i < n;
    rec[r] = valid ? in[i] : 0;
    const uint32_t d = (uint32_t)(rec[r] >> shift) & mask;
    uint64_t match = __ballot(valid);  // the valid lanes that hold my digit
#pragma unroll
    for (uint32_t b = 0; b < 8; b++) {
      const bool bit = (d >> b) & 1u;
      const uint64_t bal = __ballot(bit);
      match &= bit ? bal : ~bal;
    }
    const uint32_t below = __popcll(match & lower);
    uint32_t old = 0;
    if (valid && below == 0) {  // the group's first lane
      old = s_cnt[wave][d];
      s_cnt[wave][d] = old + __popcll(match);
    }
    old = __shfl(old, valid ? __ffsll((unsigned long long)match) - 1 : (int)lane);
    rank[r] = old + below;
    __syncthreads();  // the wave's counters are read by another lane next round
  }

  // counters -> bases: digits in order, within a digit the waves in order
  uint32_t c[kTpb / 64], tot = 0, total;
#pragma unroll
  for (uint32_t w = 0; w < kTpb / 64; w++) {
    c[w] = s_cnt[w][tid];
    tot += c[w];
  }
  uint32_t start = block_excl_scan(tot, s_w, total);
  s_start[tid] = start;
#pragma unroll
  for (uint32_t w = 0; w < kTpb / 64; w++) {
    s_cnt[w][tid] = start;
    start += c[w];
  }
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < kKpt; r++) {
    const uint32_t i = tile0 + wave * kWaveKeys + r * 64 + lane;
    const uint32_t p = s_cnt[wave][(uint32_t)(rec[r] >> shift) & mask] + rank[r];
    if (i < n && p < kTile) s_rec[p] = rec[r];
  }
  __syncthreads();
  const uint32_t n_in = n - tile0 < kTile ? n - tile0 : kTile;
#pragma unroll
  for (uint32_t k = 0; k < kKpt; k++) {
    const uint32_t p = k * kTpb + tid;
    if (p < n_in) {
      const Raw x = s_rec[p];
      const uint32_t d = (uint32_t)(x >> shift) & mask;
      const uint32_t o = s_goff[d] + (p - s_start[d]);
      if (o < n) out[o] = x;  // (always: see "Bounds" above)
    }
  }
}

// the flags of a lane's 8 consecutive sorted records (0 past the end)
__device__ __forceinline__ void lane_flags(const Raw *r, uint32_t n, uint32_t i0, Raw *rec, uint32_t *f) {
  Raw prev = i0 && i0 <= n ? r[i0 - 1] : 0, cur = i0 < n ? r[i0] : 0;
#pragma unroll
  for (uint32_t k = 0; k < kKpt; k++) {
    const uint32_t i = i0 + k;
    const Raw next = i + 1 < n ? r[i + 1] : 0;
    rec[k] = cur;
    f[k] = i < n ? classify(prev, cur, next, i, n) : 0;
    prev = cur;
    cur = next;
  }
}

// cnt[tile], cnt[tiles + tile], cnt[2 * tiles + tile]: the tile's short survivors, long survivors, block heads
__global__ __launch_bounds__(kTpb) void dp_fibsort_count_k(const Raw *r, uint32_t n, uint32_t tiles, uint32_t *cnt) {
  __shared__ uint32_t s_w[kTpb / 64];
  Raw rec[kKpt];
  uint32_t f[kKpt], sl = 0, h = 0;
  lane_flags(r, n, blockIdx.x * kTile + threadIdx.x * kKpt, rec, f);
#pragma unroll
  for (uint32_t k = 0; k < kKpt; k++) {
    sl += (f[k] & kIsShort) | (f[k] & kIsLong) << 15;  // shorts in bits 0..15, longs in 16..31 (<= 2048 each)
    h += f[k] >> 2;
  }
  uint32_t tsl, th;
  block_excl_scan(sl, s_w, tsl);
  block_excl_scan(h, s_w, th);
  if (threadIdx.x == 0) {
    cnt[blockIdx.x] = tsl & 0xffffu;
    cnt[tiles + blockIdx.x] = tsl >> 16;
    cnt[2 * tiles + blockIdx.x] = th;
  }
}

// `pos`: cnt after the scan (3 * tiles + 1 words)
__global__ __launch_bounds__(kTpb) void dp_fibsort_emit_k(const SortJob j, const uint32_t *pos, uint32_t tiles) {
  __shared__ uint32_t s_w[kTpb / 64];
  const Raw *r = j.b;
  Raw rec[kKpt];
  uint32_t f[kKpt], sl = 0, h = 0;
  lane_flags(r, j.n, blockIdx.x * kTile + threadIdx.x * kKpt, rec, f);
#pragma unroll
  for (uint32_t k = 0; k < kKpt; k++) {
    sl += (f[k] & kIsShort) | (f[k] & kIsLong) << 15;
    h += f[k] >> 2;
  }
  uint32_t tsl, th;
  const uint32_t esl = block_excl_scan(sl, s_w, tsl);
  const uint32_t n_short = pos[tiles], n_long = pos[2 * tiles] - n_short;
  uint32_t ps = pos[blockIdx.x] + (esl & 0xffffu);
  uint32_t pl = pos[tiles + blockIdx.x] - n_short + (esl >> 16);
  uint32_t pb = pos[2 * tiles + blockIdx.x] - pos[2 * tiles] + block_excl_scan(h, s_w, th);
#pragma unroll
  for (uint32_t k = 0; k < kKpt; k++) {
    const uint32_t a = addr_of(rec[k]), len = len_of(rec[k]), nh = nh_of(rec[k]);
    if ((f[k] & kIsHead) && pb < j.cap_blocks) reinterpret_cast<uint4 *>(j.blocks)[pb] = make_uint4(a >> 8, pl, 0, 0);
    if ((f[k] & kIsShort) && ps < j.cap_short) reinterpret_cast<uint4 *>(j.shorts)[ps] = make_uint4(a >> 8, len, nh, ps);
    if ((f[k] & kIsLong) && pl < j.cap_long) j.longs[pl] = (a & 0xffu) | len << 8 | nh << 16;
    ps += f[k] & kIsShort;
    pl += (f[k] & kIsLong) >> 1;
    pb += f[k] >> 2;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    Counts c;
    c.n_short = n_short;
    c.n_long = n_long;
    c.n_blocks = pos[3 * tiles] - pos[2 * tiles];
    c.pad = 0;
    *j.counts = c;
  }
}

__device__ __forceinline__ uint64_t short_key(const Short *s, uint32_t i) {
  const uint2 v = *reinterpret_cast<const uint2 *>(s + i);  // {slot, len}
  return (uint64_t)v.x << 6 | v.y;
}

__global__ __launch_bounds__(kTpb) void dp_fibsort_parent_k(const SortJob j) {
  const uint32_t me = blockIdx.x * kTpb + threadIdx.x;
  const uint32_t n_short = j.counts->n_short < j.cap_short ? j.counts->n_short : j.cap_short;
  if (me >= n_short) return;
  const uint2 v = *reinterpret_cast<const uint2 *>(j.shorts + me);
  const uint32_t slot = v.x, len = v.y < 24 ? v.y : 24;
  uint32_t parent = me, hi = me;  // an enclosing route sorts before me
  for (uint32_t step = 0; step < 24 && step < len && hi; step++) {
    const uint32_t L = len - 1 - step;
    const uint64_t target = (uint64_t)(slot >> (24 - L) << (24 - L)) << 6 | L;
    uint32_t lo = 0, h = hi;
    for (uint32_t s = 0; s < 32 && lo < h; s++) {
      const uint32_t mid = lo + ((h - lo) >> 1);
      if (short_key(j.shorts, mid) < target) lo = mid + 1;
      else h = mid;
    }
    if (lo < hi && short_key(j.shorts, lo) == target) {
      parent = lo;
      break;
    }
    hi = lo;  // what sorts at or after lo is above every shorter target
  }
  j.shorts[me].parent = parent;
}

__global__ __launch_bounds__(kTpb) void dp_fibsort_blockcount_k(const SortJob j) {
  const uint32_t b = blockIdx.x * kTpb + threadIdx.x;
  const uint32_t n_blocks = j.counts->n_blocks < j.cap_blocks ? j.counts->n_blocks : j.cap_blocks;
  if (b >= n_blocks) return;
  const uint32_t end = b + 1 < n_blocks ? j.blocks[b + 1].first : j.counts->n_long;
  j.blocks[b].count = end - j.blocks[b].first;
}

}  // namespace

// One FIB's lists on `stream` from the records in job->a.  The caller owns the
// buffers `job` names, sized them by dp_fibsort.h, and reads job->counts after
// the stream has run.
extern "C" hipError_t dpk_fib_sort(const dps::SortJob *job, hipStream_t stream) {
  const SortJob &j = *job;
  if (!j.n || j.n > kMaxRoutes) return hipErrorInvalidValue;
  const uint32_t tiles = tiles_of(j.n);
  Raw *src = j.a, *dst = j.b;
  for (uint32_t p = 0; p < kPasses; p++) {
    hipLaunchKernelGGL(dp_fibsort_hist_k, dim3(tiles), dim3(kTpb), 0, stream, src, j.n, kShift[p], kMask[p], tiles, j.scratch);
    hipLaunchKernelGGL(dp_fibsort_scan_k, dim3(1), dim3(kScanTpb), 0, stream, j.scratch, (kMask[p] + 1) * tiles);
    hipLaunchKernelGGL(dp_fibsort_scatter_k, dim3(tiles), dim3(kTpb), 0, stream, src, dst, j.n, kShift[p], kMask[p], tiles,
                       j.scratch);
    Raw *t = src;
    src = dst;
    dst = t;
  }
  static_assert(kPasses % 2 == 1, "the sorted records end in b");
  hipLaunchKernelGGL(dp_fibsort_count_k, dim3(tiles), dim3(kTpb), 0, stream, j.b, j.n, tiles, j.scratch);
  hipLaunchKernelGGL(dp_fibsort_scan_k, dim3(1), dim3(kScanTpb), 0, stream, j.scratch, 3 * tiles);
  hipLaunchKernelGGL(dp_fibsort_emit_k, dim3(tiles), dim3(kTpb), 0, stream, j, j.scratch, tiles);
  if (j.cap_short) hipLaunchKernelGGL(dp_fibsort_parent_k, dim3((j.cap_short + kTpb - 1) / kTpb), dim3(kTpb), 0, stream, j);
  if (j.cap_blocks)
    hipLaunchKernelGGL(dp_fibsort_blockcount_k, dim3((j.cap_blocks + kTpb - 1) / kTpb), dim3(kTpb), 0, stream, j);
  return hipGetLastError();
}
