// SPDX-License-Identifier: Apache-2.0
//
// The TX plan on the device (include/dpgpu.h "TX plan"): a stable multisplit
// of a burst's packet indexes into at most 64 buckets -- one per TX port of
// the caller's list, one for Delivered packets without a port (the TX drop),
// one for everything the caller frees.  64 buckets so that a bucket is a wave
// lane wherever buckets are scanned.  Three launches, none of which waits on
// another workgroup:
//
//  1. dp_txplan_count_k: a workgroup of 256 takes a tile of 2048 packets in
//     eight rounds (packet tile*2048 + r*256 + tid in round r, so the 16-byte
//     record loads coalesce); a lane issues its eight loads, and while they
//     are in flight the workgroup builds the oif -> bucket table from the
//     port list (a kernel argument) in LDS: 128 slots, open addressing,
//     multiplicative hash, at most 62 keys.  A packet's bucket is then one or
//     two LDS probes.  Out: a bucket byte per packet, and the tile's 64 counts
//     and 64 byte sums.  Counts: six ballots over the bucket's bits give each
//     lane the mask of its peers (the lanes of its bucket); the lowest peer
//     adds the mask's population to the wave's row of an LDS histogram -- one
//     writer per cell and round, no atomics -- and the four rows are added at
//     the end.
//     Byte sums: LDS adds (no ballot form exists for a sum of lengths).
//  2. dp_txplan_scan_k: one workgroup of 16 waves, lane b of every wave owns
//     bucket b.  The waves split the tile range; a wave sums its tiles' rows
//     (one coalesced 256-byte read a row, twice: counts and byte sums), the
//     waves' sums meet in LDS, a wave scan of the 64 totals gives the bucket
//     bases, and a second walk over the wave's rows leaves every tile its 64
//     bases, both walks 16 rows a step with the step's loads issued together.
//     Wave 0 writes the dp_tx_port_t records.
//  3. dp_txplan_scatter_k: same tiling, over the bucket bytes.  A packet's
//     rank is its bucket's tile base + the bucket's packets in earlier (round,
//     wave) pairs of the tile (a 32 x 64 LDS histogram, filled by the peers
//     masks' leaders and scanned down its columns by one wave) + its peers in
//     lower lanes.  The tile's indexes are placed bucket-sorted in LDS first
//     and leave from there: consecutive lanes store consecutive words of a
//     bucket's run.
#include <hip/hip_runtime.h>

#include "dp_txplan.h"

namespace {

using namespace dpt;
using u64 = unsigned long long;

constexpr uint32_t kSlots = 128;  // of the oif -> bucket table
constexpr uint32_t kScanTpb = 1024, kScanWaves = kScanTpb / 64;
constexpr uint32_t kRowsAtOnce = 16;               // tile rows a scan wave has in flight
constexpr uint32_t kRows = kRounds * (kTpb / 64);  // (round, wave) pairs of a tile

__device__ __forceinline__ uint32_t slot_of(uint32_t oif) { return (oif * 0x9e3779b1u) >> 25; }

// The lanes of the wave that hold a packet of bucket b (bits 0..5), as every
// such lane sees them; meaningless in a lane with !valid.
__device__ __forceinline__ u64 peers_of(uint32_t b, bool valid) {
  u64 m = __ballot(valid);
#pragma unroll
  for (uint32_t i = 0; i < 6; i++) {
    const bool bit = (b >> i) & 1u;
    const u64 s = __ballot(bit);
    m &= bit ? s : ~s;
  }
  return m;
}

// Inclusive scan of v over the wave's 64 lanes.
__device__ __forceinline__ uint32_t wave_scan(uint32_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  return v;
}

__global__ __launch_bounds__(kTpb) void dp_txplan_count_k(const uint4 *__restrict__ recs, uint32_t n, const Ports pl,
                                                          uint8_t *__restrict__ bkt, uint32_t *__restrict__ tcount,
                                                          uint32_t *__restrict__ tbytes) {
  __shared__ uint32_t hkey[kSlots], hval[kSlots];
  __shared__ uint32_t wcnt[kTpb / 64][kBuckets];
  __shared__ uint32_t bsum[kBuckets];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u64 first = (u64)blockIdx.x * kTile;
  // every load of the lane before the first use
  uint4 rec[kRounds];
#pragma unroll
  for (uint32_t r = 0; r < kRounds; r++) {
    const u64 p = first + r * kTpb + tid;
    rec[r] = make_uint4(0, 0, 0, 0);
    if (p < n) rec[r] = recs[p];
  }
  if (tid < kSlots) hkey[tid] = 0;
  wcnt[wave][lane] = 0;
  if (tid < kBuckets) bsum[tid] = 0;
  __syncthreads();
  if (tid < pl.n) {
    // (0 is the empty slot: the runtime has refused a 0 in the list)
    const uint32_t key = pl.oif[tid];
    uint32_t h = slot_of(key);
    while (atomicCAS(&hkey[h], 0u, key) != 0u) h = (h + 1) & (kSlots - 1);
    hval[h] = tid;
  }
  __syncthreads();
  const u64 below = (1ull << lane) - 1;
#pragma unroll
  for (uint32_t r = 0; r < kRounds; r++) {
    const u64 p = first + r * kTpb + tid;
    const bool valid = p < n;
    // dp_pkt_out_t: x = off, y = len | done << 16 | acl << 24, z = oif
    const uint32_t len = rec[r].y & 0xffffu, done = (rec[r].y >> 16) & 0xffu, oif = rec[r].z;
    uint32_t b = pl.n + 1;  // the caller frees it
    if (done == DP_DONE_DELIVERED) {
      b = pl.n;  // Delivered without a port of the list
      if (oif) {
        // (at most 62 of 128 slots are taken: the probe ends)
        for (uint32_t h = slot_of(oif);; h = (h + 1) & (kSlots - 1)) {
          const uint32_t k = hkey[h];
          if (k == oif) b = hval[h];
          if (k == oif || k == 0) break;
        }
      }
    }
    if (valid) {
      bkt[p] = (uint8_t)b;
      atomicAdd(&bsum[b], len);
    }
    const u64 peers = peers_of(b, valid);
    // The lowest peer: one writer a cell in this round.  Another lane of the
    // wave may be the cell's writer in a later round; the wave's LDS accesses
    // complete in program order, so that read sees this write -- no atomic.
    if (valid && !(peers & below)) wcnt[wave][b] += (uint32_t)__popcll(peers);
  }
  __syncthreads();
  if (tid < kBuckets) {
    const size_t o = (size_t)blockIdx.x * kBuckets + tid;
    tcount[o] = wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
    tbytes[o] = bsum[tid];
  }
}

__global__ __launch_bounds__(kScanTpb) void dp_txplan_scan_k(const uint32_t *__restrict__ tcount,
                                                             const uint32_t *__restrict__ tbytes, uint32_t tiles,
                                                             const Ports pl, uint32_t *__restrict__ tbase,
                                                             dp_tx_port_t *__restrict__ ports) {
  __shared__ uint32_t wc[kScanWaves][kBuckets];
  __shared__ u64 wb[kScanWaves][kBuckets];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // the wave's tiles: a contiguous share of the range
  const uint32_t share = (tiles + kScanWaves - 1) / kScanWaves;
  const uint32_t t0 = wave * share < tiles ? wave * share : tiles, t1 = t0 + share < tiles ? t0 + share : tiles;
  uint32_t c = 0;
  u64 by = 0;
  // One workgroup: the walks are bound by load latency, not bytes, so rows
  // go kRowsAtOnce at a time with every load of a step issued before the
  // first use; a step's rows past the share's end load its last row again
  // (no branch between the loads) and count as 0.
  for (uint32_t tb = t0; tb < t1; tb += kRowsAtOnce) {
    uint32_t cv[kRowsAtOnce], bv[kRowsAtOnce];
#pragma unroll
    for (uint32_t i = 0; i < kRowsAtOnce; i++) {
      const size_t o = (size_t)(tb + i < t1 ? tb + i : t1 - 1) * kBuckets + lane;
      cv[i] = tcount[o];
      bv[i] = tbytes[o];
    }
#pragma unroll
    for (uint32_t i = 0; i < kRowsAtOnce; i++) {
      c += tb + i < t1 ? cv[i] : 0u;
      by += tb + i < t1 ? bv[i] : 0u;
    }
  }
  wc[wave][lane] = c;
  wb[wave][lane] = by;
  __syncthreads();
  uint32_t before = 0, count = 0;  // bucket `lane`: in the waves before this one, in all
  u64 bytes = 0;
#pragma unroll
  for (uint32_t w = 0; w < kScanWaves; w++) {
    const uint32_t v = wc[w][lane];
    if (w < wave) before += v;
    count += v;
    bytes += wb[w][lane];
  }
  const uint32_t bucket_first = wave_scan(count, lane) - count;
  uint32_t run = bucket_first + before;
  for (uint32_t tb = t0; tb < t1; tb += kRowsAtOnce) {
    uint32_t cv[kRowsAtOnce];
#pragma unroll
    for (uint32_t i = 0; i < kRowsAtOnce; i++)
      cv[i] = tcount[(size_t)(tb + i < t1 ? tb + i : t1 - 1) * kBuckets + lane];
#pragma unroll
    for (uint32_t i = 0; i < kRowsAtOnce; i++)
      if (tb + i < t1) {
        tbase[(size_t)(tb + i) * kBuckets + lane] = run;
        run += cv[i];
      }
  }
  if (wave == 0 && lane < pl.n + 2) {
    dp_tx_port_t o;
    o.oif = lane < pl.n ? pl.oif[lane] : 0u;
    o.first = bucket_first;
    o.count = count;
    o.pad = 0;
    o.bytes = bytes;
    ports[lane] = o;
  }
}

__global__ __launch_bounds__(kTpb) void dp_txplan_scatter_k(const uint8_t *__restrict__ bkt, uint32_t n,
                                                            const uint32_t *__restrict__ tbase,
                                                            uint32_t *__restrict__ order) {
  __shared__ uint32_t hist[kRows][kBuckets];  // a (round, wave) pair's packets a bucket, then those before it
  __shared__ uint32_t lfirst[kBuckets];       // the bucket's first place in `sorted`
  __shared__ uint32_t gfirst[kBuckets];       // ... and in `order`
  __shared__ uint32_t sorted[kTile];          // packet of the tile | bucket << 16, bucket after bucket
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u64 first = (u64)blockIdx.x * kTile;
  const uint32_t tile_n = (uint32_t)(n - first < kTile ? n - first : kTile);
  uint32_t b[kRounds], rank[kRounds];
#pragma unroll
  for (uint32_t r = 0; r < kRounds; r++) {
    const u64 p = first + r * kTpb + tid;
    b[r] = p < n ? bkt[p] & (kBuckets - 1) : kNoBucket;
  }
#pragma unroll
  for (uint32_t i = tid; i < kRows * kBuckets; i += kTpb) (&hist[0][0])[i] = 0;
  __syncthreads();
  const u64 below = (1ull << lane) - 1;
#pragma unroll
  for (uint32_t r = 0; r < kRounds; r++) {
    const bool valid = b[r] != kNoBucket;
    const u64 peers = peers_of(b[r], valid);
    rank[r] = (uint32_t)__popcll(peers & below);
    if (valid && !(peers & below)) hist[r * (kTpb / 64) + wave][b[r]] = (uint32_t)__popcll(peers);
  }
  __syncthreads();
  if (tid < kBuckets) {
    uint32_t run = 0;
#pragma unroll
    for (uint32_t row = 0; row < kRows; row++) {
      const uint32_t t = hist[row][tid];
      hist[row][tid] = run;
      run += t;
    }
    lfirst[tid] = wave_scan(run, lane) - run;
    gfirst[tid] = tbase[(size_t)blockIdx.x * kBuckets + tid];
  }
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < kRounds; r++)
    if (b[r] != kNoBucket)
      sorted[lfirst[b[r]] + hist[r * (kTpb / 64) + wave][b[r]] + rank[r]] = (r * kTpb + tid) | b[r] << 16;
  __syncthreads();
  for (uint32_t j = tid; j < tile_n; j += kTpb) {
    const uint32_t e = sorted[j], bb = e >> 16;
    order[gfirst[bb] + (j - lfirst[bb])] = (uint32_t)first + (e & 0xffffu);
  }
}

}  // namespace

// One plan over n records on `stream`: the three kernels.  `scratch` holds
// dpt::scratch_bytes(n); the caller has checked the port list and the
// alignment of the arrays.  Returns the launches' error.
extern "C" hipError_t dpk_tx_plan(const dp_pkt_out_t *out, uint32_t n, const dpt::Ports *pl, void *scratch,
                                  uint32_t *order, dp_tx_port_t *ports, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint32_t tiles = (uint32_t)tiles_of(n);
  uint8_t *bkt = static_cast<uint8_t *>(scratch);
  uint32_t *tcount = reinterpret_cast<uint32_t *>(bkt + bucket_bytes(n));
  uint32_t *tbytes = tcount + (size_t)tiles * kBuckets, *tbase = tbytes + (size_t)tiles * kBuckets;
  hipLaunchKernelGGL(dp_txplan_count_k, dim3(tiles), dim3(kTpb), 0, stream, reinterpret_cast<const uint4 *>(out), n,
                     *pl, bkt, tcount, tbytes);
  hipLaunchKernelGGL(dp_txplan_scan_k, dim3(1), dim3(kScanTpb), 0, stream, tcount, tbytes, tiles, *pl, tbase, ports);
  hipLaunchKernelGGL(dp_txplan_scatter_k, dim3(tiles), dim3(kTpb), 0, stream, bkt, n, tbase, order);
  return hipGetLastError();
}
