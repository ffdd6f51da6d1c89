// inflate_host — the inflate core of k_inflate (csrc/inflate_core.h) run on the CPU under
// ASan + UBSan against zlib: every vector of `python tools/rawdeflate.py --dump DIR` and 20 000
// fixed-seed single-byte mutations of them. Output and verdict must match zlib's gzip mode (the
// host route's gzip_decode loop), a decoded length other than the expected one must fail, and the
// loop iterations must stay within 8 * src_len + dlen + a constant. Also checks the lane-split
// CRC32 combine the kernel uses (crc pieces from zero, x^(8 j) multipliers) against zlib's crc32.
//
//   inflate_host DIR
#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "inflate_core.h"

using namespace pq::inf;

static uint32_t g_crc[256];

struct HostCtx {
  const uint8_t *src;
  uint32_t n;
  std::vector<uint8_t> out;
  size_t crc_from = 0;
  uint64_t steps = 0;
  uint32_t lane() const { return 0; }
  uint32_t nl() const { return 1; }
  void sync() {}
  uint32_t sa() const { return 0; }
  uint32_t word(uint32_t k) const {
    uint32_t w = 0;
    for (uint32_t i = 0; i < 4; i++) {
      const uint64_t at = 4ull * k + i;
      if (at < n) w |= (uint32_t)src[at] << (8 * i);
    }
    return w;
  }
  const uint32_t *crc_tab() const { return g_crc; }
  void lit(uint32_t b) { out.push_back((uint8_t)b); }
  void copy(uint32_t dist, uint32_t len) {
    for (uint32_t k = 0; k < len; k++) out.push_back(out[out.size() - dist]);
  }
  void stored(uint32_t off, uint32_t len) { out.insert(out.end(), src + off, src + off + len); }
  uint32_t member_crc() {
    uint32_t c = 0xffffffffu;
    for (size_t k = crc_from; k < out.size(); k++) c = crc_byte(g_crc, c, out[k]);
    crc_from = out.size();
    return ~c;
  }
  void step() { steps++; }
};

// format.cpp gzip_decode: members until the input is consumed
static bool zlib_decode(const uint8_t *src, size_t n, std::vector<uint8_t> *out) {
  out->clear();
  size_t cap = n * 4 + 1024, len = 0, pos = 0;
  out->resize(cap);
  int members = 0;
  while (pos < n || members == 0) {
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, 16 + MAX_WBITS) != Z_OK) abort();
    zs.next_in = (Bytef *)(src + pos);
    zs.avail_in = (uInt)(n - pos);
    int rc;
    do {
      if (len == cap) { cap *= 2; out->resize(cap); }
      zs.next_out = out->data() + len;
      zs.avail_out = (uInt)(cap - len);
      rc = inflate(&zs, Z_NO_FLUSH);
      len = cap - zs.avail_out;
      if (rc != Z_OK && rc != Z_STREAM_END && !(rc == Z_BUF_ERROR && zs.avail_out == 0)) {
        inflateEnd(&zs);
        return false;
      }
    } while (rc != Z_STREAM_END);
    pos = n - zs.avail_in;
    inflateEnd(&zs);
    members++;
  }
  out->resize(len);
  return true;
}

static int g_fail = 0;
static void fail(const std::string &what, const std::string &name) {
  fprintf(stderr, "FAIL %s: %s\n", name.c_str(), what.c_str());
  g_fail++;
}

static Tables g_tab;

static bool run_core(const std::vector<uint8_t> &in, uint32_t dlen, std::vector<uint8_t> *out, uint64_t *steps) {
  // an exact-size copy: ASan sees any read past the block
  uint8_t *copy = (uint8_t *)malloc(in.size() ? in.size() : 1);
  if (!in.empty()) memcpy(copy, in.data(), in.size());
  HostCtx c{copy, (uint32_t)in.size()};
  memcpy(g_tab.crc, g_crc, sizeof(g_crc));
  uint32_t members = 0;
  const bool ok = inflate_block(c, g_tab, (uint32_t)in.size(), dlen, &members);
  *steps = c.steps;
  out->swap(c.out);
  free(copy);
  return ok;
}

static void check(const std::vector<uint8_t> &in, uint32_t dlen_hint, const std::string &name) {
  std::vector<uint8_t> want, got;
  const bool zok = zlib_decode(in.data(), in.size(), &want);
  const uint32_t dlen = zok ? (uint32_t)want.size() : dlen_hint;
  uint64_t steps = 0;
  const bool ok = run_core(in, dlen, &got, &steps);
  if (ok != zok) return fail(std::string("verdict ") + (ok ? "ok" : "bad") + ", zlib " + (zok ? "ok" : "bad"), name);
  if (ok && got != want) return fail("output differs", name);
  if (got.size() > dlen) return fail("output passed dlen", name);
  if (steps > 8ull * in.size() + dlen + 64) return fail("steps " + std::to_string(steps), name);
  if (zok) {  // a page whose header gives another decoded size is corrupt
    if (run_core(in, dlen + 1, &got, &steps)) fail("accepted dlen + 1", name);
    if (dlen && run_core(in, dlen - 1, &got, &steps)) fail("accepted dlen - 1", name);
  }
}

// the kernel's checksum: 16-byte pieces from zero by 64 lanes, combined with x^(8 j)
static void check_crc_combine() {
  static constexpr X8Table x8 = make_x8();
  std::vector<uint8_t> d(5000);
  uint32_t s = 12345;
  for (auto &b : d) { s = s * 1664525u + 1013904223u; b = (uint8_t)(s >> 24); }
  for (uint32_t from : {0u, 5u, 16u, 33u}) {
    for (uint32_t to : {from, from + 1, from + 15, from + 16, from + 1000, from + 1024, from + 1025, from + 4000}) {
      uint32_t state = 0xffffffffu, pos = from;
      // two advances, as a flush followed by a member end
      for (uint32_t upto : {(from + (to - from) / 2) & ~15u, to}) {
        if (upto <= pos) continue;
        for (uint32_t x0 = pos & ~15u; x0 < upto; x0 += 1024) {
          const uint32_t end = std::min(upto, x0 + 1024);
          uint32_t red = 0;
          for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t x = x0 + 16 * lane, a = std::max(x, pos), b = std::min(x + 16, end);
            if (a >= b) continue;
            uint32_t r = 0;
            for (uint32_t k = a; k < b; k++) r = crc_byte(g_crc, r, d[k]);
            red ^= gf2_mulmod(r, x8.v[end - b]);
          }
          state = gf2_mulmod(state, x8.v[end - std::max(x0, pos)]) ^ red;
        }
        pos = upto;
      }
      const uint32_t want = (uint32_t)crc32(0L, d.data() + from, to - from);
      if (~state != want) fail("crc combine " + std::to_string(from) + ".." + std::to_string(to), "crc");
    }
  }
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: inflate_host DIR\n"); return 2; }
  for (uint32_t k = 0; k < 256; k++) g_crc[k] = crc_table_entry(k);
  check_crc_combine();
  std::vector<std::string> names;
  DIR *dp = opendir(argv[1]);
  if (!dp) { perror(argv[1]); return 2; }
  while (dirent *e = readdir(dp)) {
    std::string f = e->d_name;
    if (f.size() > 3 && f.substr(f.size() - 3) == ".gz") names.push_back(f);
  }
  closedir(dp);
  std::sort(names.begin(), names.end());
  if (names.empty()) { fprintf(stderr, "no vectors in %s\n", argv[1]); return 2; }
  std::vector<std::vector<uint8_t>> vec;
  std::vector<uint32_t> hint;
  for (const auto &f : names) {
    FILE *fp = fopen((std::string(argv[1]) + "/" + f).c_str(), "rb");
    if (!fp) { perror(f.c_str()); return 2; }
    std::vector<uint8_t> d;
    uint8_t buf[65536];
    size_t r;
    while ((r = fread(buf, 1, sizeof(buf), fp)) > 0) d.insert(d.end(), buf, buf + r);
    fclose(fp);
    vec.push_back(d);
    std::vector<uint8_t> o;
    hint.push_back(zlib_decode(d.data(), d.size(), &o) ? (uint32_t)o.size() : 4096u);
    check(d, hint.back(), f);
  }
  uint64_t rng = 0x9e3779b97f4a7c15ull;
  auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
  int mutated = 0;
  for (int k = 0; k < 20000; k++) {
    const size_t v = next() % vec.size();
    if (vec[v].empty()) continue;
    std::vector<uint8_t> d = vec[v];
    // mostly the head (headers, tables) of long vectors, where a byte decides the most
    const size_t span = (next() & 1) ? std::min<size_t>(d.size(), 96) : d.size();
    const size_t at = next() % span;
    d[at] ^= (uint8_t)(1 + next() % 255);
    check(d, hint[v], names[v] + "@" + std::to_string(at));
    mutated++;
  }
  printf("inflate_host: %zu vectors, %d mutations, %d failures\n", vec.size(), mutated, g_fail);
  return g_fail ? 1 : 0;
}
