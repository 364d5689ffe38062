// SPDX-License-Identifier: Apache-2.0
//
// Stand-alone host check of the device FIB build (DP_OPT_DEVICE_FIB), no GPU:
// the table compiler's device form (holes + build lists) with the holes filled
// by a host restatement of the two kernels of dp_fibbuild.hip (same tiles,
// marks, prefix-max, climb and tile default; same block scan) must give the
// host-built image byte for byte.  Tables: C2's from the workload generator
// (argv[1] v4 routes, default 1M); with a second argument also a dense tile,
// full /25../32 nests, blocks at slots 0 and 2^24 - 1 and in adjacent slots, a
// duplicate prefix and routes on tile borders, and the order and duplicate
// shapes of tests/test_gpu_fib_device_sort.py.  The route-sort form
// (DP_OPT_DEVICE_FIB = 2) must reserve the same image from unsorted records,
// and a host restatement of the kernels of dp_fibsort.hip must turn them into
// the host's three lists element for element.  Prints the host phase times of
// the forms.  Build and run from the repository root, e.g. under sanitizers:
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

// The kernels of dp_fibsort.hip restated (DP_OPT_DEVICE_FIB = 2): the same
// tiles, digit-major histograms, scan, stable scatter (a record's in-tile rank
// is the count of its digit before it in tile order, which is what the ballots
// and wave counters compute), flags, list positions, parent search and block
// counts.  Returns the lists made from the raw records.
static dpd::FibBuild emu_sort(const dpd::FibBuild &in) {
  using namespace dps;
  constexpr uint32_t kSortTile = dps::kTile;
  const uint32_t n = (uint32_t)in.raw.size(), tiles = tiles_of(n);
  std::vector<Raw> a(in.raw), b(n);
  std::vector<uint32_t> sc(scratch_words(n));
  auto scan = [&](uint32_t m) {
    uint32_t run = 0;
    for (uint32_t i = 0; i < m; i++) { const uint32_t x = sc[i]; sc[i] = run; run += x; }
    sc[m] = run;
  };
  for (uint32_t p = 0; p < kPasses; p++) {
    const uint32_t nd = kMask[p] + 1;
    std::fill(sc.begin(), sc.end(), 0);
    for (uint32_t i = 0; i < n; i++) sc[((uint32_t)(a[i] >> kShift[p]) & kMask[p]) * tiles + i / kSortTile]++;
    scan(nd * tiles);
    for (uint32_t t = 0; t < tiles; t++) {
      uint32_t seen[kDigits] = {};
      for (uint32_t i = t * kSortTile; i < n && i < (t + 1) * kSortTile; i++) {
        const uint32_t d = (uint32_t)(a[i] >> kShift[p]) & kMask[p];
        b[sc[d * tiles + t] + seen[d]++] = a[i];
      }
    }
    a.swap(b);
  }
  auto flags = [&](uint32_t i) { return classify(i ? a[i - 1] : 0, a[i], i + 1 < n ? a[i + 1] : 0, i, n); };
  std::fill(sc.begin(), sc.end(), 0);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t f = flags(i), t = i / kSortTile;
    sc[t] += f & kIsShort, sc[tiles + t] += (f & kIsLong) >> 1, sc[2 * tiles + t] += f >> 2;
  }
  scan(3 * tiles);
  dpd::FibBuild out;
  const uint32_t n_short = sc[tiles], n_long = sc[2 * tiles] - n_short, n_blocks = sc[3 * tiles] - sc[2 * tiles];
  if (n_short > in.raw_short || n_long > in.raw_long || n_blocks != in.n_blocks) { printf("counts outside the host's bounds\n"); exit(1); }
  out.shorts.resize(n_short), out.longs.resize(n_long), out.blocks.resize(n_blocks);
  for (uint32_t t = 0; t < tiles; t++) {
    uint32_t ps = sc[t], pl = sc[tiles + t] - n_short, pb = sc[2 * tiles + t] - sc[2 * tiles];
    for (uint32_t i = t * kSortTile; i < n && i < (t + 1) * kSortTile; i++) {
      const uint32_t f = flags(i), ad = addr_of(a[i]), len = len_of(a[i]), nh = nh_of(a[i]);
      if (f & kIsHead) out.blocks.at(pb++) = Block{ad >> 8, pl, 0, 0};
      if (f & kIsShort) { out.shorts.at(ps) = Short{ad >> 8, len, nh, ps}; ps++; }
      if (f & kIsLong) out.longs.at(pl++) = (ad & 0xffu) | len << 8 | nh << 16;
    }
  }
  auto skey = [&](uint32_t i) { return (uint64_t)out.shorts.at(i).slot << 6 | out.shorts[i].len; };
  for (uint32_t me = 0; me < n_short; me++) {
    const uint32_t slot = out.shorts[me].slot, len = out.shorts[me].len;
    uint32_t parent = me, hi = me;
    for (uint32_t step = 0; step < 24 && step < len && hi; step++) {
      const uint32_t L = len - 1 - step;
      const uint64_t target = (uint64_t)(slot >> (24 - L) << (24 - L)) << 6 | L;
      uint32_t lo = 0, h = hi;
      for (uint32_t s = 0; s < 32 && lo < h; s++) { const uint32_t mid = lo + ((h - lo) >> 1); if (skey(mid) < target) lo = mid + 1; else h = mid; }
      if (lo < hi && skey(lo) == target) { parent = lo; break; }
      hi = lo;
    }
    out.shorts[me].parent = parent;
  }
  for (uint32_t k = 0; k < n_blocks; k++) out.blocks[k].count = (k + 1 < n_blocks ? out.blocks[k + 1].first : n_long) - out.blocks[k].first;
  out.direct = in.direct, out.block16 = in.block16;
  return out;
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
    const uint32_t F = w->routes[0].fib;  // the FIB that holds the generator's v4 routes: the DIR-24-8 one
    const uint32_t base = 0x2c400000;     // a /14: the dense tile
    for (int len = 14; len <= 24; len++)
      for (uint32_t i = 0; i < (1u << (len - 14)); i++) add(w, F, base + (i << (32 - len)), len, k++);
    for (uint32_t s : {0u, 0xffffffu, 0x123456u, 0x123457u})
      for (int len = 25; len <= 32; len++) add(w, F, (s << 8) | 0x80 | (s & 1 ? 0x55 : 0), len, k++);
    add(w, F, 0x12345600, 25, k++);
    add(w, F, 0x12345600, 24, k++);
    add(w, F, 0x12345600, 24, k++);  // duplicate: the last wins
    add(w, F, 0, 0, k++);
    for (int len : {8, 12, 16, 20, 24}) add(w, F, 0x0a0b0c00, len, k++);
    add(w, F, 0x0a0c0000, 16, k++);
    add(w, F, 0x4ffffc00 + 0x300, 24, k++);  // a tile's last slot
    add(w, F, 0x50000000, 24, k++);          // a tile's first slot
    add(w, F, 0x50000000, 14, k++);
    for (int i = 5000; i-- > 0;) add(w, F, 0x3c000000 + ((uint32_t)i << 8), 24, k++);   // descending
    for (int len = 8; len <= 32; len++) add(w, F, 0x0b000000, len, k++);                // one address, every length
    for (int len = 25; len <= 32; len++)                                                // a full /24 of 510 long routes
      for (uint32_t i = 0; i < (1u << (len - 24)); i++) add(w, F, 0x3d000000 + (i << (32 - len)), len, k++);
    add(w, F, 0x3d000100 + 77, 32, k++);                                                // next to a /24 holding one
    std::vector<dp_route_t> all;                                                        // one prefix 5,000 times,
    const size_t every = w->routes.size() / 5000;                                       // through the whole order
    for (size_t i = 0; i < w->routes.size(); i++) {
      all.push_back(w->routes[i]);
      if (i % every == 0) {
        dp_route_t r = w->routes.back();
        put32(r.prefix.addr, 0x3e000000 + (i % (3 * every) ? 0 : 0x80));  // (and a second one, long)
        r.prefix.len = i % (3 * every) ? 20 : 25;
        r.nh = (uint32_t)(i / every) % (uint32_t)w->nhs.size();
        all.push_back(r);
      }
    }
    w->routes.swap(all);
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
    // mode 2: the same layout from unsorted records, and the restated sort
    // kernels' lists against the host's, element for element
    dpd::BuiltImage raw;
    t = std::chrono::steady_clock::now();
    if (dpd::build_image(d, raw, nullptr, 2)) return 8;
    printf("raw form: total %lu us pack %lu paint %lu\n", us(t), raw.sort_us, raw.paint_us);
    if (raw.im.bytes != dev.im.bytes || memcmp(&raw.im, &dev.im, sizeof raw.im) || raw.bytes != dev.bytes ||
        raw.fib_builds.size() != dev.fib_builds.size()) { printf("raw form: image differs\n"); return 9; }
    for (size_t k = 0; k < raw.fib_builds.size(); k++) {
      const dpd::FibBuild &rb = raw.fib_builds[k], &hb = dev.fib_builds[k];
      if (rb.raw.empty() || !rb.shorts.empty() || rb.direct != hb.direct || rb.block16 != hb.block16) { printf("raw form: fib %zu\n", k); return 10; }
      const dpd::FibBuild made = emu_sort(rb);
      const bool same = made.shorts.size() == hb.shorts.size() && made.longs == hb.longs && made.blocks.size() == hb.blocks.size() &&
                        !memcmp(made.shorts.data(), hb.shorts.data(), sizeof(Short) * hb.shorts.size()) &&
                        !memcmp(made.blocks.data(), hb.blocks.data(), sizeof(Block) * hb.blocks.size());
      printf("fib %zu: %zu raw routes -> %zu short %zu long %zu blocks: lists %s\n", k, rb.raw.size(), made.shorts.size(),
             made.longs.size(), made.blocks.size(), same ? "identical" : "MISMATCH");
      if (!same) return 11;
    }
  }
  dpw_free(w);
  return 0;
}
