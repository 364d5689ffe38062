// SPDX-License-Identifier: Apache-2.0
//
// Stand-alone host check of the device FIB build (DP_OPT_DEVICE_FIB), no GPU:
// the table compiler's device form (holes + build lists) with the holes filled
// by a host restatement of the two kernels of dp_fibbuild.hip (same tiles,
// marks, prefix-max, climb and tile default; same block scan) must give the
// host-built image byte for byte.  Tables: C2's from the workload generator
// (argv[1] v4 routes, default 1M); with a second argument also a dense tile,
// full /25../32 nests, blocks at slots 0 and 2^24 - 1 and in adjacent slots, a
// duplicate prefix and routes on tile borders.  Prints the host phase times of
// both forms.  Build and run from the repository root, e.g. under sanitizers:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined scripts/fib_build_check.cpp \
//       dataplane_amd/csrc/dp_tables.cpp -o /tmp/fib_build_check -lpthread
//   /tmp/fib_build_check 200000 extra
#include "../dataplane_amd/csrc/dp_workload.cpp"
#include "../dataplane_amd/csrc/dp_tables.h"
#include <chrono>

using namespace dpb;

static void emu_direct(const dpd::FibBuild &fb, uint32_t *direct) {
  const uint32_t n = (uint32_t)fb.shorts.size();
  auto lower = [&](uint32_t lo, uint32_t hi, uint32_t s) {
    while (lo < hi) { uint32_t m = lo + ((hi - lo) >> 1); if (fb.shorts[m].slot < s) lo = m + 1; else hi = m; }
    return lo;
  };
  std::vector<uint32_t> mark(kTile);
  for (uint32_t t = 0; t < kTiles; t++) {
    const uint32_t tile0 = t * kTile;
    const uint32_t a = lower(0, n, tile0), b = lower(a, n, tile0 + kTile);
    std::fill(mark.begin(), mark.end(), 0);
    uint32_t dnh = 0, i = a ? a - 1 : 0;
    for (uint32_t step = 0; step < 26 && a; step++) {
      const Short &r = fb.shorts[i];
      dnh = r.nh;
      if (covers(r.slot, r.len, tile0)) break;
      i = r.parent;
    }
    for (uint32_t k = a; k < b; k++) {
      const uint32_t next = k + 1 < b ? fb.shorts[k + 1].slot : 0xffffffffu;
      if (next != fb.shorts[k].slot) mark[fb.shorts[k].slot - tile0] = k - a + 1;
    }
    uint32_t run = 0;
    for (uint32_t s = 0; s < kTile; s++) {
      run = std::max(run, mark[s]);
      uint32_t pos = run, nh = dnh;
      for (uint32_t step = 0; step < 26 && pos; step++) {
        const Short &r = fb.shorts[a + pos - 1];
        if (covers(r.slot, r.len, tile0 + s)) { nh = r.nh; break; }
        pos = r.parent >= a ? r.parent - a + 1 : 0;
      }
      direct[tile0 + s] = 0x80000000u | nh;
    }
  }
}

static void emu_blocks(const dpd::FibBuild &fb, uint32_t *direct, uint16_t *b16) {
  for (uint32_t bi = 0; bi < fb.blocks.size(); bi++) {
    const Block &d = fb.blocks[bi];
    if (d.count > kBlockRoutes) { printf("block too long\n"); exit(1); }
    const uint32_t dflt = direct[d.slot] & 0xffffu;
    for (uint32_t h = 0; h < 256; h++) {
      uint32_t v = dflt;
      for (uint32_t i = 0; i < d.count; i++) {
        const uint32_t w = fb.longs[d.first + i];
        if ((((w & 0xff) ^ h) >> (32 - ((w >> 8) & 0xff))) == 0) v = w >> 16;
      }
      b16[(size_t)bi * 256 + h] = (uint16_t)v;
    }
    direct[d.slot] = bi;
  }
}

static void add(dpw_workload *w, uint32_t fib, uint32_t addr, int len, uint32_t nh) {
  dp_route_t r{};
  r.prefix.family = 4;
  r.prefix.len = (uint8_t)len;
  addr = len ? addr >> (32 - len) << (32 - len) : 0;
  put32(r.prefix.addr, addr);
  r.fib = fib;
  r.nh = nh % (uint32_t)w->nhs.size();
  w->routes.push_back(r);
}

static uint64_t us(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t).count();
}

int main(int argc, char **argv) {
  dpw_config_t c{};
  c.config = 2;
  c.n_packets = 64;
  c.seed = 11;
  c.n_routes_v4 = argc > 1 ? atoi(argv[1]) : 1000000;
  const bool extra = argc > 2;
  dpw_workload_t *w = nullptr;
  if (dpw_build(&c, &w)) return 2;
  if (extra) {
    uint32_t k = 1;
    const uint32_t base = 0x2c400000;  // a /14: the dense tile
    for (int len = 14; len <= 24; len++)
      for (uint32_t i = 0; i < (1u << (len - 14)); i++) add(w, 0, base + (i << (32 - len)), len, k++);
    for (uint32_t s : {0u, 0xffffffu, 0x123456u, 0x123457u})
      for (int len = 25; len <= 32; len++) add(w, 0, (s << 8) | 0x80 | (s & 1 ? 0x55 : 0), len, k++);
    add(w, 0, 0x12345600, 25, k++);
    add(w, 0, 0x12345600, 24, k++);
    add(w, 0, 0x12345600, 24, k++);  // duplicate: the last wins
    add(w, 0, 0, 0, k++);
    for (int len : {8, 12, 16, 20, 24}) add(w, 0, 0x0a0b0c00, len, k++);
    add(w, 0, 0x0a0c0000, 16, k++);
    add(w, 0, 0x4ffffc00 + 0x300, 24, k++);  // a tile's last slot
    add(w, 0, 0x50000000, 24, k++);          // a tile's first slot
    add(w, 0, 0x50000000, 14, k++);
    w->desc.routes = w->routes.data();
    w->desc.n_routes = w->routes.size();
  }
  const dp_tables_desc_t *d = &w->desc;
  for (int rep = 0; rep < 2; rep++) {
    dpd::BuiltImage host, dev;
    auto t = std::chrono::steady_clock::now();
    if (dpd::build_image(d, host)) return 3;
    const uint64_t th = us(t);
    t = std::chrono::steady_clock::now();
    if (dpd::build_image(d, dev, nullptr, true)) return 4;
    const uint64_t td = us(t);
    printf("host form: total %lu us sort %lu paint %lu rest %lu | device form: total %lu us sort+prep %lu paint %lu rest %lu\n",
           th, host.sort_us, host.paint_us, th - host.sort_us - host.paint_us, td, dev.sort_us, dev.paint_us,
           td - dev.sort_us - dev.paint_us);
    printf("image %lu bytes, device-form host bytes %zu, holes %zu, fibs %zu\n", (unsigned long)host.im.bytes,
           dev.bytes.size(), dev.holes.size(), dev.fib_builds.size());
    if (rep) continue;
    if (host.im.bytes != dev.im.bytes || memcmp(&host.im, &dev.im, sizeof host.im)) { printf("Image differs\n"); return 5; }
    std::vector<uint8_t> full(dev.im.bytes, 0xee);
    uint64_t off = 0, src = 0;
    for (auto &h : dev.holes) {
      memcpy(full.data() + off, dev.bytes.data() + src, h.off - off);
      src += h.off - off;
      off = h.off + h.bytes;
    }
    memcpy(full.data() + off, dev.bytes.data() + src, dev.im.bytes - off);
    if (src + dev.im.bytes - off != dev.bytes.size()) { printf("piece sizes\n"); return 6; }
    for (auto &fb : dev.fib_builds) {
      printf("fib: %zu short %zu long %zu blocks\n", fb.shorts.size(), fb.longs.size(), fb.blocks.size());
      emu_direct(fb, reinterpret_cast<uint32_t *>(full.data() + fb.direct));
      emu_blocks(fb, reinterpret_cast<uint32_t *>(full.data() + fb.direct), reinterpret_cast<uint16_t *>(full.data() + fb.block16));
    }
    size_t bad = 0;
    for (size_t i = 0; i < full.size(); i++)
      if (full[i] != host.bytes[i] && bad++ < 5) printf("differs at %zu: %02x vs %02x\n", i, full[i], host.bytes[i]);
    printf("%s (%zu bytes differ)\n", bad ? "MISMATCH" : "identical", bad);
    if (bad) return 7;
  }
  dpw_free(w);
  return 0;
}
