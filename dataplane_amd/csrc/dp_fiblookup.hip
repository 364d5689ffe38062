// SPDX-License-Identifier: Apache-2.0
//
// The FIB lookup alone (include/dpgpu.h "The FIB lookup alone"): the longest
// prefix match behind IP-Forward as a batch kernel of its own.  The pipeline
// kernel walks one serial chain per packet (dp_kernel.hip lpm_walk); here the
// same walk over the same image (dp_device.h Lpm) is restated as rounds over
// a tile of keys, so that a lane has several table loads in flight:
//
//  1. load: a workgroup of 256 takes a tile of 1024 keys (4 a lane).  The
//     24-byte keys are copied into LDS as 8-byte words, lane after lane, and
//     parsed from there.  VRF -> FIB goes through the image's map once per
//     distinct VRF of a wave (a match-any loop over wave-uniform probes).
//     Each key is reduced to the image offset of the first table entry it
//     reads (the direct table's, or the window table's for a v6 key inside
//     the window) and what lies below it (blocks / Poptrie start bit).
//  2. walk: the first-table round issues the loads of all 4 keys before it
//     consumes any; then trips in which every unfinished key of the lane
//     advances one level (a DIR-24-8 block, a Poptrie node, a Poptrie leaf).
//     The last round reads the route's n_entries and forms the result.
//  3. store: a lane's key r sits at slot r * 256 + lane of the tile, so each
//     round's results leave as 8-byte stores, lane after lane, in input order.
//
// LDS: the 24 KiB of keys a workgroup, so 6 workgroups fit a compute unit's
// 160 KiB; registers allow 4 workgroups of 4 waves.
//
// A binned form -- the tile sorted in LDS on (first-table offset, slot) so that
// neighbouring lanes read the same or adjacent lines, runs of one entry loaded
// once -- was built and measured against this one; it lost on every stream
// (profiles/fib_lookup/ab_binned_timing.json) and was removed.
#include <hip/hip_runtime.h>

#include "../../include/dpgpu.h"
#include "dp_device.h"

namespace {

using namespace dpd;

constexpr uint32_t kTpb = 256;
constexpr uint32_t kKpl = 4;               // keys per lane
constexpr uint32_t kTile = kTpb * kKpl;    // 1024 keys
static_assert(sizeof(dp_fib_key_t) == 24 && sizeof(dp_fib_result_t) == 8, "record sizes");

constexpr uint32_t kNoTable = 0xffffffffu;  // first-table offset of a key that reads nothing
// what a key's walk does next
enum : uint32_t { kDone = 0, kNode = 1, kLeaf = 2, kBlock = 3 };
// forms of the first table (meta bits 8..9)
enum : uint32_t { kPoptrie = 0, kDir = 1, kDir16 = 2 };

typedef unsigned long long u64;

__device__ __forceinline__ u64 bswap64(u64 x) { return __builtin_bswap64(x); }

// bits [off, off + 6) of the 128-bit key (hi:lo), zero past bit 127
__device__ __forceinline__ uint32_t key6(u64 hi, u64 lo, int off) {
  const int o = off & 63;
  u64 x = off < 64 ? (hi << o) | ((lo >> 1) >> (63 - o)) : lo << o;
  if (off >= 128) x = 0;
  return (uint32_t)(x >> 58);
}

// VRF id -> FIB index through the image's map (kNoTable: none).  Called with
// a wave-uniform vrf, so the probe is one chain for the wave.
__device__ __forceinline__ uint32_t vrf_to_fib(const uint8_t *base, u64 slots, uint32_t mask, uint32_t count,
                                               uint32_t n_fibs, uint32_t vrf) {
  if (count == 0) return kNoTable;
  const HashSlot *s = reinterpret_cast<const HashSlot *>(base + slots);
  uint32_t i = hmix(vrf, 0, 0) & mask;
  for (uint32_t probe = 0; probe <= mask; probe++, i = (i + 1) & mask) {
    const uint32_t e2 = s[i].k2;
    if (!(e2 & 0x80000000u)) return kNoTable;
    if (s[i].k0 == vrf && s[i].k1 == 0 && e2 == 0x80000000u) return s[i].val < n_fibs ? s[i].val : kNoTable;
  }
  return kNoTable;
}

// One key between the rounds.
struct Key {
  u64 hi, lo;      // the address, bit 0 of the prefix space in bit 63 of hi
  uint32_t t0;     // image offset of the first table entry (kNoTable: none)
  uint32_t blk;    // DIR-24-8: image offset of the blocks
  uint32_t meta;   // Poptrie start bit | first-table form << 8 | result code << 16
};

__global__ __launch_bounds__(kTpb) void dp_fib_lookup_k(const uint8_t *__restrict__ base,
                                                        const Image *__restrict__ im,
                                                        const u64 *__restrict__ keys, u64 *__restrict__ out,
                                                        uint32_t n) {
  __shared__ u64 skey[kTile * 3];
  const uint32_t tid = threadIdx.x;
  const u64 first = (u64)blockIdx.x * kTile;
  const uint32_t cnt = n - first < kTile ? (uint32_t)(n - first) : kTile;

  // --- 1. load: the tile's words, nothing past keys[n]
#pragma unroll
  for (uint32_t k = 0; k < 3 * kKpl; k++) {
    const uint32_t w = tid + kTpb * k;
    skey[w] = w < cnt * 3 ? keys[first * 3 + w] : 0;
  }
  const u64 map_slots = im->vrf_fib.slots, fibs_off = im->fibs;
  const uint32_t map_mask = im->vrf_fib.mask, map_count = im->vrf_fib.count, n_fibs = im->n_fibs;
  __syncthreads();

  Key K[kKpl];
  uint32_t fib[kKpl], vrf[kKpl];
  bool pend[kKpl];
#pragma unroll
  for (uint32_t r = 0; r < kKpl; r++) {
    const uint32_t s = r * kTpb + tid;
    const u64 w0 = skey[3 * s];
    const uint32_t fam = (uint32_t)(w0 >> 32) & 0xffu;
    vrf[r] = (uint32_t)w0;
    K[r].hi = bswap64(skey[3 * s + 1]);
    K[r].lo = bswap64(skey[3 * s + 2]);
    if (fam == 4) {
      K[r].hi &= 0xffffffff00000000ull;
      K[r].lo = 0;
    }
    K[r].t0 = kNoTable;
    K[r].blk = 0;
    K[r].meta = (fam == 4 || fam == 6 ? (uint32_t)DP_FIB_NO_VRF : (uint32_t)DP_FIB_BAD_FAMILY) << 16 | fam << 24;
    fib[r] = kNoTable;
    pend[r] = s < cnt && (fam == 4 || fam == 6);
  }
  // each distinct VRF of the wave once
  for (;;) {
    uint32_t cand = 0;
    bool has = false;
#pragma unroll
    for (uint32_t r = 0; r < kKpl; r++)
      if (!has && pend[r]) {
        cand = vrf[r];
        has = true;
      }
    const u64 b = __ballot(has);
    if (!b) break;
    const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)cand, __ffsll((long long)b) - 1);
    const uint32_t f = vrf_to_fib(base, map_slots, map_mask, map_count, n_fibs, v);
#pragma unroll
    for (uint32_t r = 0; r < kKpl; r++)
      if (pend[r] && vrf[r] == v) {
        fib[r] = f;
        pend[r] = false;
      }
  }
  // the first table entry of each key
#pragma unroll
  for (uint32_t r = 0; r < kKpl; r++) {
    if (fib[r] == kNoTable) continue;
    const FibRec *F = reinterpret_cast<const FibRec *>(base + fibs_off) + fib[r];
    const bool v6 = (K[r].meta >> 24) == 6;
    const Lpm &L = v6 ? F->v6 : F->v4;
    const uint32_t dbits = L.dbits, b = dbits & 0xffu;
    const u64 blocks = L.blocks;
    uint32_t form = blocks ? ((dbits & DPD_LPM_D16) ? kDir16 : kDir) : kPoptrie, off = b;
    u64 t0 = L.direct + ((K[r].hi >> (64 - b)) << (form == kDir16 ? 1 : 2));
    if (v6) {
      const u64 wtab = L.wtab;
      const uint32_t wbits = L.wbits, wtb = L.wtb;
      if (wtab && (K[r].hi >> (64 - wbits)) == L.wpfx) {
        t0 = wtab + (((K[r].hi >> (64 - wbits - wtb)) & ((1ull << wtb) - 1)) << 2);
        off = wbits + wtb;
        form = kPoptrie;
      }
    }
    K[r].t0 = (uint32_t)t0;  // (image offsets are < 4 GiB: dp_tables.cpp refuses larger images)
    K[r].blk = (uint32_t)blocks;
    K[r].meta = off | form << 8 | (uint32_t)DP_FIB_ROUTE << 16;
  }

  // --- 2. walk.  First-table round: every load of the lane, then the entries
  uint32_t e[kKpl];
#pragma unroll
  for (uint32_t r = 0; r < kKpl; r++) {
    e[r] = 0;
    if (K[r].t0 != kNoTable)
      e[r] = ((K[r].meta >> 8) & 3u) == kDir16 ? *reinterpret_cast<const uint16_t *>(base + K[r].t0)
                                               : *reinterpret_cast<const uint32_t *>(base + K[r].t0);
  }
  uint32_t st[kKpl], ni[kKpl], nh[kKpl], off[kKpl];
#pragma unroll
  for (uint32_t r = 0; r < kKpl; r++) {
    const uint32_t form = (K[r].meta >> 8) & 3u;
    uint32_t x = e[r];
    if (form == kDir16) x = (x & 0x8000u) ? 0x80000000u | (x & 0x7fffu) : x;
    off[r] = K[r].meta & 0xffu;
    nh[r] = x & 0x7fffffffu;
    ni[r] = form == kPoptrie ? x : (x << 8) | ((uint32_t)(K[r].hi >> 32) & 0xffu);
    st[r] = K[r].t0 == kNoTable || (x & 0x80000000u) ? (uint32_t)kDone : form == kPoptrie ? (uint32_t)kNode
                                                                                           : (uint32_t)kBlock;
  }
  // The rounds below it: every unfinished key of the lane advances one level
  // a trip (a block entry, a Poptrie node, a Poptrie leaf), loads first.
  const PtNode *nodes = reinterpret_cast<const PtNode *>(base + im->pt_nodes);
  const uint32_t *leaves = reinterpret_cast<const uint32_t *>(base + im->pt_leaves);
  for (int trip = 0; trip < 28 && (st[0] | st[1] | st[2] | st[3]); trip++) {
    u64 vec[kKpl], lv[kKpl];
    uint32_t b1[kKpl], b0[kKpl], val[kKpl];
#pragma unroll
    for (uint32_t r = 0; r < kKpl; r++) {
      vec[r] = lv[r] = 0;
      b1[r] = b0[r] = val[r] = 0;
      if (st[r] == kNode) {
        const PtNode *nd = nodes + ni[r];
        vec[r] = nd->vec;
        lv[r] = nd->leafvec;
        b1[r] = nd->base1;
        b0[r] = nd->base0;
      } else if (st[r] == kLeaf) {
        val[r] = leaves[ni[r]];
      } else if (st[r] == kBlock) {
        val[r] = reinterpret_cast<const uint16_t *>(base + K[r].blk)[ni[r]];
      }
    }
#pragma unroll
    for (uint32_t r = 0; r < kKpl; r++) {
      if (st[r] == kNode) {
        const uint32_t v = key6(K[r].hi, K[r].lo, (int)off[r]);
        const u64 bit = 1ull << v;
        if (vec[r] & bit) {
          ni[r] = b1[r] + (uint32_t)__popcll(vec[r] & (bit - 1));
          off[r] += 6;
        } else {
          const u64 m = v == 63 ? ~0ull : (bit << 1) - 1;
          ni[r] = b0[r] + (uint32_t)__popcll(lv[r] & m) - 1;
          st[r] = kLeaf;
        }
      } else if (st[r] != kDone) {
        nh[r] = val[r];
        st[r] = kDone;
      }
    }
  }
  // Last round: the route's n_entries; the compiler's own drop route (the
  // last next hop of the image, Image.drop_nh) is the FIB's implicit default
  const uint32_t drop_nh = im->drop_nh;
  const RouteNh *rnh = reinterpret_cast<const RouteNh *>(base + im->route_nhs);
  uint32_t ne[kKpl];
#pragma unroll
  for (uint32_t r = 0; r < kKpl; r++) {
    const bool route = K[r].t0 != kNoTable && st[r] == kDone && nh[r] < drop_nh;
    ne[r] = route ? rnh[nh[r]].n_entries : 0;
    if (!route && K[r].t0 != kNoTable) K[r].meta = (K[r].meta & 0xff00ffffu) | (uint32_t)DP_FIB_DEFAULT << 16;
    if (!route) nh[r] = 0xffffffffu;
  }
  // --- 3. store: round r's results are 256 consecutive records
#pragma unroll
  for (uint32_t r = 0; r < kKpl; r++) {
    const uint32_t s = r * kTpb + tid;
    if (s < cnt)
      out[first + s] = (u64)nh[r] | (u64)(ne[r] & 0xffffu) << 32 | (u64)((K[r].meta >> 16) & 0xffu) << 48;
  }
}

}  // namespace

// Test and timing hook: the kernel form of later lookups in this process,
// 0 auto or 1 direct.  Auto is the direct form: the binned form, value 2, lost
// every measurement and went with its value, so the hook has
// nothing left to choose.  Not part of the product ABI (dpgpu.h).
extern "C" void dpd_debug_set_fib_lookup_form(int form) { (void)form; }

// n lookups over the image on `stream`; keys and results 8-byte aligned.
extern "C" int dpk_fib_lookup(const uint8_t *img_base, const void *image_dev, const dp_fib_key_t *keys,
                              dp_fib_result_t *out, uint32_t n, hipStream_t stream) {
  if (n == 0) return 0;
  const dim3 grid((uint32_t)(((uint64_t)n + kTile - 1) / kTile));
  const Image *im = static_cast<const Image *>(image_dev);
  const u64 *k = reinterpret_cast<const u64 *>(keys);
  u64 *o = reinterpret_cast<u64 *>(out);
  hipLaunchKernelGGL(dp_fib_lookup_k, grid, dim3(kTpb), 0, stream, img_base, im, k, o, n);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}
