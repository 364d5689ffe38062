// SPDX-License-Identifier: Apache-2.0
//
// The DIR-24-8 tables of a v4 FIB built on the device (DP_OPT_DEVICE_FIB,
// include/dpgpu.h): the 2^24-entry direct table and the uint16_t[256] blocks,
// written in place in the image from the compact lists of dp_fibbuild.h.  The
// values are the host builder's (dp_tables.cpp build_lpm), entry for entry.
// Two launches on one stream; no atomics on HBM, no workgroup waits on another,
// every table byte leaves in one full-width vector store.
//
//  1. dp_fibbuild_direct_k: a workgroup of 256 paints a tile of 1024
//     consecutive slots (/24s), 4 adjacent slots a lane, one 16-byte store a
//     lane: the tile is one 4 KiB write.  A slot's entry is its longest short
//     route (length <= 24):
//      - two wave-uniform binary searches over the short list give the run
//        [a, b) of routes that START inside the tile; its first kStage records
//        are staged in LDS, a longer run's rest is read from HBM (L2) later;
//      - each route of the run that is the last one starting on its slot
//        (the next record starts elsewhere: one writer a slot, no LDS atomic)
//        marks the slot with its position; a prefix-max along the tile (4
//        slots in the lane, a wave scan, the 4 wave totals through LDS) turns
//        the marks into "the last route starting at or before me";
//      - from that route a slot climbs parent links to the first route that
//        holds it.  That is its longest match: the routes holding a slot nest,
//        the last route starting at or before the slot lies inside the longest
//        of them, and a climb visits enclosing routes longest first;
//      - a climb that leaves the run (parent < a) needs no further step.  The
//        tile is itself a prefix (an aligned /14), so a route that starts
//        before it and holds one of its slots holds all of it, and nested
//        prefixes make every such climb end on the same route: the longest
//        match of the tile's first slot among the routes before the run.  Lane
//        0 finds it once a tile (a climb from route a - 1, at most 25 steps)
//        while the others stage; a tile in which no route starts is that value
//        1024 times.
//  2. dp_fibbuild_blocks_k, behind it: one wave a block (a /24 holding routes
//     of length 25..32).  The painted entry of the block's slot is its
//     default; the block's long routes (at most 510) are staged in LDS and
//     every lane resolves 4 adjacent host addresses by scanning them in order,
//     the last holder winning (nested again: a later holder is a longer one).
//     The 4 values leave as one 8-byte store -- a block is one 512-byte write
//     -- and lane 0 then replaces direct[slot] with the block's index.
#include <hip/hip_runtime.h>

#include "dp_fibbuild.h"

namespace {

using namespace dpb;

// first index in [lo, hi) whose route starts at slot >= s (wave-uniform)
__device__ __forceinline__ uint32_t lower_slot(const Short *r, uint32_t lo, uint32_t hi, uint32_t s) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (r[mid].slot < s) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

__global__ __launch_bounds__(kTpb) void dp_fibbuild_direct_k(const Job j) {
  __shared__ uint4 s_route[kStage];    // the run's first records
  __shared__ uint32_t s_mark[kTile];   // per slot: 1 + run position of the last route starting there, 0 none
  __shared__ uint32_t s_wave[kTpb / 64];
  __shared__ uint32_t s_default;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t tile0 = blockIdx.x * kTile;
  const uint4 *recs = reinterpret_cast<const uint4 *>(j.shorts);

  const uint32_t a = lower_slot(j.shorts, 0, j.n_short, tile0);
  const uint32_t b = lower_slot(j.shorts, a, j.n_short, tile0 + kTile);
  reinterpret_cast<uint4 *>(s_mark)[tid] = make_uint4(0, 0, 0, 0);
  if (tid == 0) {
    // the longest route before the run that holds the tile (none before tile
    // 0's run: its slots all climb to the /0, route 0, inside the run)
    uint32_t nh = 0, i = a ? a - 1 : 0;
    for (uint32_t step = 0; step < 26 && a; step++) {
      const uint4 r = recs[i];  // {slot, len, nh, parent}
      nh = r.z;
      if (covers(r.x, r.y, tile0)) break;
      i = r.w;
    }
    s_default = nh;
  }
  __syncthreads();
  for (uint32_t i = a + tid; i < b; i += kTpb) {
    const uint4 r = recs[i];
    if (i - a < kStage) s_route[i - a] = r;
    const uint32_t next = i + 1 < b ? j.shorts[i + 1].slot : 0xffffffffu;
    if (next != r.x) s_mark[r.x - tile0] = i - a + 1;
  }
  __syncthreads();

  // prefix-max of the marks along the tile
  const uint4 mk = reinterpret_cast<const uint4 *>(s_mark)[tid];
  uint32_t m[kSpl] = {mk.x, mk.y, mk.z, mk.w};
#pragma unroll
  for (uint32_t k = 1; k < kSpl; k++) m[k] = umax(m[k], m[k - 1]);
  uint32_t incl = m[kSpl - 1];
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(incl, d);
    if (lane >= d) incl = umax(incl, t);
  }
  uint32_t before = __shfl_up(incl, 1);
  if (lane == 0) before = 0;
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  for (uint32_t w = 0; w < wave; w++) before = umax(before, s_wave[w]);

  // climb; the result of a climb that leaves the run is the tile's default
  const uint32_t dflt = s_default, s0 = tile0 + tid * kSpl;
  uint32_t nh[kSpl];
#pragma unroll
  for (uint32_t k = 0; k < kSpl; k++) {
    uint32_t pos = umax(m[k], before);
    nh[k] = dflt;
    for (uint32_t step = 0; step < 26 && pos; step++) {
      const uint4 r = pos - 1 < kStage ? s_route[pos - 1] : recs[a + pos - 1];
      if (covers(r.x, r.y, s0 + k)) {
        nh[k] = r.z;
        break;
      }
      pos = r.w >= a ? r.w - a + 1 : 0;
    }
  }
  *reinterpret_cast<uint4 *>(j.direct + s0) =
      make_uint4(0x80000000u | nh[0], 0x80000000u | nh[1], 0x80000000u | nh[2], 0x80000000u | nh[3]);
}

__global__ __launch_bounds__(kTpb) void dp_fibbuild_blocks_k(const Job j) {
  __shared__ uint32_t s_long[kTpb / kBlockLanes][kBlockStage];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t bi = blockIdx.x * (kTpb / kBlockLanes) + wave;
  const bool live = bi < j.n_blocks;
  uint32_t slot = 0, first = 0, cnt = 0, dflt = 0;
  if (live) {
    const uint4 d = reinterpret_cast<const uint4 *>(j.blocks)[bi];  // {slot, first, count, pad}
    slot = d.x;
    first = d.y;
    cnt = d.z < kBlockStage ? d.z : kBlockStage;
    dflt = j.direct[slot] & 0xffffu;  // the leaf the first kernel painted
    for (uint32_t i = lane; i < cnt; i += kBlockLanes) s_long[wave][i] = j.longs[first + i];
  }
  __syncthreads();
  if (!live) return;
  const uint32_t h0 = lane * 4;
  uint32_t v[4] = {dflt, dflt, dflt, dflt};
  for (uint32_t i = 0; i < cnt; i++) {
    const uint32_t w = s_long[wave][i];
    const uint32_t x = (w & 0xffu) ^ h0, sh = 32 - ((w >> 8) & 0xffu);  // length 25..32: shift 7..0
#pragma unroll
    for (uint32_t k = 0; k < 4; k++)
      if (((x ^ k) >> sh) == 0) v[k] = w >> 16;
  }
  // (the lanes' loads of direct[slot] have returned: v depends on them)
  *reinterpret_cast<uint2 *>(j.block16 + (size_t)bi * 256 + h0) = make_uint2(v[0] | v[1] << 16, v[2] | v[3] << 16);
  if (lane == 0) j.direct[slot] = bi;
}

}  // namespace

// One FIB's tables on `stream`: the direct table, then its blocks.  The
// caller owns the lists and the regions `job` names and checked their sizes.
extern "C" hipError_t dpk_fib_build(const dpb::Job *job, hipStream_t stream) {
  hipLaunchKernelGGL(dp_fibbuild_direct_k, dim3(kTiles), dim3(kTpb), 0, stream, *job);
  if (job->n_blocks)
    hipLaunchKernelGGL(dp_fibbuild_blocks_k, dim3((job->n_blocks + kTpb / kBlockLanes - 1) / (kTpb / kBlockLanes)),
                       dim3(kTpb), 0, stream, *job);
  return hipGetLastError();
}
