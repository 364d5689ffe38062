// SPDX-License-Identifier: Apache-2.0
//
// The Stats stage on the device (include/dpgpu.h "Per-VPC statistics"): a
// keyed reduction of a burst's records onto very few hot cells -- a burst of
// 2M packets between 4 VPCs lands on about a dozen counters.  Same-address
// global atomics serialise across the chip (about 12 ns each),
// so the burst is reduced in three levels and only (workgroups x live cells)
// updates reach the global table:
//
//  1. wave: every lane forms its packet's (at most two) cell updates; a
//     match-any loop takes the first pending lane's cell, ballots the lanes
//     that hold it, counts them with popcounts and sums their bytes with a
//     DPP wave reduction, and retires them.  The loop runs once per distinct
//     cell of the wave.
//  2. workgroup: the matched group's first lane adds the four sums to a small
//     LDS hash table (64-bit LDS atomics).  Workgroups are persistent (one
//     of 16 waves per compute unit, each taking chunk after chunk with the
//     next chunk's records already in flight), so the LDS table
//     absorbs a whole share of the burst.  A cell that finds no LDS slot
//     within its probe window goes straight to the global table.
//  3. device: at its end a workgroup flushes its LDS slots into the
//     context's global table (dp_vpcstats.h), one atomic per non-zero counter.
#include <hip/hip_runtime.h>

#include "dp_vpcstats.h"

namespace {

constexpr uint32_t kTpb = 1024;      // 16 waves; one packet per lane and chunk
constexpr uint32_t kLdsSlots = 256;  // 10 KiB of LDS
constexpr uint32_t kLdsProbe = 16;   // LDS slots tried before a cell goes global

__device__ __forceinline__ uint32_t cell_hash(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 29;
  return (uint32_t)k;
}

template <int kCtrl, int kRowMask>
__device__ __forceinline__ uint32_t dpp_add(uint32_t v) {
  // (the rows outside kRowMask keep v)
  return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, kRowMask, 0xf, false);
}

// Sum of v over the 64 lanes (all active), uniform.  VALU only: within the
// rows of 16 by quad permutes and row rotations, then across the rows by the
// two row broadcasts; lane 63 ends with the total.
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  v = dpp_add<0xb1, 0xf>(v);   // quad_perm:[1,0,3,2]
  v = dpp_add<0x4e, 0xf>(v);   // quad_perm:[2,3,0,1]
  v = dpp_add<0x124, 0xf>(v);  // row_ror:4
  v = dpp_add<0x128, 0xf>(v);  // row_ror:8
  v = dpp_add<0x142, 0xa>(v);  // row_bcast:15 into rows 1, 3
  v = dpp_add<0x143, 0xc>(v);  // row_bcast:31 into rows 2, 3
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// Level 3: c[] into the cell's slot of the global table (claimed if new).
__device__ void global_add(dpv::Table *t, unsigned long long key, const unsigned long long c[4]) {
  uint32_t h = cell_hash(key) & (DP_VPC_STATS_CELLS - 1);
  for (uint32_t p = 0; p < DP_VPC_STATS_CELLS; p++, h = (h + 1) & (DP_VPC_STATS_CELLS - 1)) {
    unsigned long long k = __hip_atomic_load(&t->key[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == 0) {
      k = atomicCAS(&t->key[h], 0ull, key);
      if (k == 0) {
        t->tick[h] = atomicAdd(&t->count, 1u) + 1;  // (read by the host only)
        k = key;
      }
    }
    if (k == key) {
      for (int j = 0; j < 4; j++)
        if (c[j]) atomicAdd(&t->ctr[h][j], c[j]);
      return;
    }
  }
  atomicAdd(&t->lost, c[dpv::kFwdPackets] + c[dpv::kDropPackets]);
}

// Level 2: one matched group's sums into the workgroup's LDS table.
__device__ void lds_add(unsigned long long *lkey, unsigned long long (*lctr)[4], dpv::Table *t,
                        unsigned long long key, const unsigned long long c[4]) {
  uint32_t h = cell_hash(key) & (kLdsSlots - 1);
  for (uint32_t p = 0; p < kLdsProbe; p++, h = (h + 1) & (kLdsSlots - 1)) {
    const unsigned long long k = atomicCAS(&lkey[h], 0ull, key);
    if (k == 0 || k == key) {
      for (int j = 0; j < 4; j++)
        if (c[j]) atomicAdd(&lctr[h][j], c[j]);
      return;
    }
  }
  global_add(t, key, c);  // more distinct cells than the LDS table takes: correct, slow
}

// What the stage reads of packet i (nothing of a packet past the burst).
struct Rec {
  uint32_t src, dst, len;
  bool drop;
};
__device__ __forceinline__ Rec load(const dp_pkt_out_t *out, const dp_pkt_meta_t *meta, uint32_t n, uint64_t i) {
  Rec r{0, 0, 0, false};
  if (i < n) {
    const dp_pkt_out_t o = out[i];  // 16 B
    r.dst = meta[i].dst_vni;        // the first 8 B of the 48
    r.src = meta[i].src_vni;
    r.len = o.len;
    r.drop = o.done != DP_DONE_DELIVERED;
  }
  return r;
}

__global__ __launch_bounds__(kTpb) void dp_vpc_stats_k(const dp_pkt_out_t *__restrict__ out,
                                                       const dp_pkt_meta_t *__restrict__ meta, uint32_t n,
                                                       dpv::Table *t) {
  __shared__ unsigned long long lkey[kLdsSlots];
  __shared__ unsigned long long lctr[kLdsSlots][4];
  for (uint32_t s = threadIdx.x; s < kLdsSlots; s += kTpb) {
    lkey[s] = 0;
    for (int j = 0; j < 4; j++) lctr[s][j] = 0;
  }
  __syncthreads();
  const int lane = (int)(threadIdx.x & 63);
  // every lane stays in both loops until its wave is done (the ballots, the
  // lane reads and the DPP sums need the whole wave)
  Rec next = load(out, meta, n, (uint64_t)blockIdx.x * kTpb + threadIdx.x);
  for (uint64_t base = (uint64_t)blockIdx.x * kTpb; base < n; base += (uint64_t)gridDim.x * kTpb) {
    const Rec r = next;
    // the next chunk's records are in flight while this one is reduced
    next = load(out, meta, n, base + (uint64_t)gridDim.x * kTpb + threadIdx.x);
    const uint32_t src = r.src, dst = r.dst, len = r.len;
    const bool drop = r.drop;
    // update a: a drop's total (src, 0) or a delivered packet's forward cell
    // (src, dst); update b: a drop's pair cell (src, dst)
    const uint32_t dst_a = drop ? 0u : dst;
    bool pend_a = src != 0 && (drop || dst != 0);
    bool pend_b = src != 0 && drop && dst != 0;
    unsigned long long pend = __ballot(pend_a);
    while (pend) {
      const int l = __ffsll(pend) - 1;  // the first lane with an update left
      const uint32_t cs = (uint32_t)__builtin_amdgcn_readlane((int)src, l);
      const uint32_t cd = (uint32_t)__builtin_amdgcn_readlane((int)(pend_a ? dst_a : dst), l);
      const bool ma = pend_a && src == cs && dst_a == cd, mb = pend_b && src == cs && dst == cd;
      const bool m = ma || mb;  // (never both: dst_a != dst where b is pending)
      const unsigned long long all = __ballot(m), dropped = __ballot(m && drop);
      unsigned long long c[4];
      c[dpv::kDropPackets] = __popcll(dropped);
      c[dpv::kFwdPackets] = __popcll(all) - c[dpv::kDropPackets];
      c[dpv::kFwdBytes] = c[dpv::kFwdPackets] ? wave_sum(m && !drop ? len : 0u) : 0u;  // <= 64 x 65535
      c[dpv::kDropBytes] = c[dpv::kDropPackets] ? wave_sum(m && drop ? len : 0u) : 0u;
      if (lane == l) lds_add(lkey, lctr, t, (unsigned long long)cs << 32 | cd, c);
      if (ma) pend_a = false;
      if (mb) pend_b = false;
      pend = __ballot(pend_a || pend_b);
    }
  }
  __syncthreads();
  for (uint32_t s = threadIdx.x; s < kLdsSlots; s += kTpb)
    if (lkey[s]) global_add(t, lkey[s], lctr[s]);
}

}  // namespace

// Accumulate n records into `table` (a dpv::Table) on `stream`, with at most
// `max_blocks` persistent workgroups.
extern "C" int dpk_vpc_stats(const dp_pkt_out_t *out, const dp_pkt_meta_t *meta, uint32_t n, void *table,
                             uint32_t max_blocks, hipStream_t stream) {
  if (n == 0) return 0;
  uint32_t blocks = (uint32_t)(((uint64_t)n + kTpb - 1) / kTpb);
  if (blocks > max_blocks) blocks = max_blocks;
  hipLaunchKernelGGL(dp_vpc_stats_k, dim3(blocks), dim3(kTpb), 0, stream, out, meta, n,
                     static_cast<dpv::Table *>(table));
  return hipGetLastError() == hipSuccess ? 0 : -5;
}
