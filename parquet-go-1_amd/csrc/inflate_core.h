// inflate_core.h — gzip members -> bytes (RFC 1952 / RFC 1951) with zlib's gzip-mode verdicts
// (inflate.c / inftrees.c): what the reference's GZIP codec accepts (compress.go:63-76) and what
// the host route (format.cpp gzip_decode) reports. One text for k_inflate (inflate.hip) and for
// the stand-alone host checker (tools/sanitize/inflate_host.cpp).
//
// The core is written against a context `C`:
//   lane(), nl()           this caller's index among nl() cooperating callers (host: 0 of 1)
//   sync()                 table memory written by one caller is visible to all (host: nothing)
//   sa()                   source bytes in front of the block inside its first aligned dword
//   word(k)                aligned dword k of the source; bytes outside the block read as zero
//   crc_tab()              the 256-entry CRC32 table
//   lit(b)                 emit one byte
//   copy(dist, len)        emit len bytes from dist bytes back (dist <= bytes of this member)
//   stored(off, len)       emit source bytes [off, off + len)
//   member_crc()           CRC32 of the bytes emitted since the last call (or the start)
//   step()                 one loop iteration (the host checker counts them)
// Every value the core computes is the same for all cooperating callers (wave-uniform on the
// device); only the table fills are split by lane().
//
// Termination: every loop iteration consumes at least one source bit or emits at least one byte,
// reads past the block return zero bits, and every loop stops once the bit position passes
// 8 * src_len.
#pragma once
#include <stdint.h>

#ifndef DEV
#define DEV inline
#endif

namespace pq {
namespace inf {

constexpr uint32_t kCrcPoly = 0xedb88320u;
constexpr uint32_t kLitRoot = 9, kDistRoot = 6, kClRoot = 7;
// first-level table plus every sub-table a complete code can need (zlib's ENOUGH_LENS / ENOUGH_DISTS:
// 286 symbols under root 9, 30 under root 6, 15-bit codes; the fixed code's 288 / 32 symbols fit too)
constexpr uint32_t kLitTab = 852, kDistTab = 592, kClTab = 128;
constexpr uint32_t kMaxSyms = 288 + 32;

// table entry: bits 0-3 code bits to drop, 4-6 op, 8-12 extra bits (link: sub-table index bits),
// 16-31 value (literal, base length / distance, code-length symbol, link: sub-table offset)
enum : uint32_t { OP_LIT = 0, OP_BASE = 1, OP_EOB = 2, OP_LINK = 3, OP_BAD = 4 };
DEV uint32_t mk_entry(uint32_t bits, uint32_t op, uint32_t extra, uint32_t val) {
  return bits | (op << 4) | (extra << 8) | (val << 16);
}
DEV uint32_t e_bits(uint32_t e) { return e & 15u; }
DEV uint32_t e_op(uint32_t e) { return (e >> 4) & 7u; }
DEV uint32_t e_extra(uint32_t e) { return (e >> 8) & 31u; }
DEV uint32_t e_val(uint32_t e) { return e >> 16; }

enum : uint32_t { K_CODES = 0, K_LENS = 1, K_DISTS = 2 };

struct Tables {
  uint32_t lit[kLitTab];
  uint32_t dist[kDistTab];
  uint32_t cl[kClTab];
  uint32_t crc[256];
  uint16_t sorted[288];  // symbols by (length, symbol)
  uint16_t code[288];    // canonical code of sorted[i], bit-reversed (LSB first)
  uint16_t sub[288];     // sorted[i] longer than the root: sub-table offset | index bits << 12
  uint8_t lens[kMaxSyms];
  uint16_t count[16], offs[16];  // build scratch of caller 0
  uint32_t status;       // build result of the serial pass
  uint32_t nsorted;
};

DEV uint32_t crc_table_entry(uint32_t k) {
  uint32_t c = k;
  for (int i = 0; i < 8; i++) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
  return c;
}
DEV uint32_t crc_byte(const uint32_t *T, uint32_t c, uint32_t b) { return T[(c ^ b) & 0xffu] ^ (c >> 8); }

// a(x) * b(x) mod P, reflected (x^0 = 0x80000000), zlib crc32.c multmodp
DEV uint32_t gf2_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t i = 0; i < 32; i++) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
  }
  return p;
}
// x^(8 j) mod P for j <= 1024: the CRC register after j more bytes is reg * x^(8 j) xor the
// register of those bytes from zero, so pieces checksummed from zero by different lanes combine.
struct X8Table {
  uint32_t v[1025];
};
constexpr X8Table make_x8() {
  X8Table t{};
  uint32_t b = 0x80000000u;
  for (int j = 0; j <= 1024; j++) {
    t.v[j] = b;
    for (int k = 0; k < 8; k++) b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return t;
}

DEV uint32_t rev16(uint32_t v, uint32_t len) {  // the low `len` bits of v reversed
  v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
  v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
  v = ((v & 0x0f0fu) << 4) | ((v >> 4) & 0x0f0fu);
  v = ((v & 0x00ffu) << 8) | ((v >> 8) & 0x00ffu);
  return v >> (16 - len);
}

DEV uint32_t sym_entry(uint32_t kind, uint32_t sym, uint32_t bits) {
  if (kind == K_CODES) return mk_entry(bits, OP_LIT, 0, sym);
  if (kind == K_LENS) {
    if (sym < 256) return mk_entry(bits, OP_LIT, 0, sym);
    if (sym == 256) return mk_entry(bits, OP_EOB, 0, 0);
    const uint32_t s = sym - 257;
    if (s >= 29) return mk_entry(bits, OP_BAD, 0, 0);  // fixed code 286 / 287
    if (s < 8) return mk_entry(bits, OP_BASE, 0, 3 + s);
    if (s == 28) return mk_entry(bits, OP_BASE, 0, 258);
    const uint32_t e = (s >> 2) - 1;
    return mk_entry(bits, OP_BASE, e, 3 + ((4 + (s & 3)) << e));
  }
  if (sym >= 30) return mk_entry(bits, OP_BAD, 0, 0);  // fixed distance code 30 / 31
  if (sym < 4) return mk_entry(bits, OP_BASE, 0, 1 + sym);
  const uint32_t e = (sym >> 1) - 1;
  return mk_entry(bits, OP_BASE, e, 1 + ((2 + (sym & 1)) << e));
}

// Decoding table of `n` code lengths (inftrees.c inflate_table's verdicts: an over-subscribed
// set is an error, an incomplete one too unless its longest code has 1 bit; no codes at all is
// accepted for distances and fails when one is used). Caller 0 counts, sorts, assigns the
// canonical codes and places the sub-tables; all callers fill the entries, a stride apart.
template <class C>
DEV bool build_table(C &c, Tables &t, uint32_t *tab, uint32_t cap, uint32_t root, const uint8_t *lens, uint32_t n,
                     uint32_t kind) {
  const uint32_t lane = c.lane(), nl = c.nl();
  for (uint32_t i = lane; i < cap; i += nl) tab[i] = mk_entry(1, OP_BAD, 0, 0);
  c.sync();  // lens written, table cleared
  if (lane == 0) {
    uint16_t *count = t.count, *offs = t.offs;
    for (uint32_t l = 0; l < 16; l++) count[l] = 0;
    for (uint32_t i = 0; i < n; i++) count[lens[i]]++;
    uint32_t max = 15;
    while (max > 0 && count[max] == 0) max--;
    int32_t left = 1;
    bool ok = true;
    for (uint32_t l = 1; l <= 15; l++) {
      left <<= 1;
      left -= (int32_t)count[l];
      if (left < 0) { ok = false; break; }
    }
    if (ok && max == 0) ok = kind == K_DISTS;
    else if (ok && left > 0 && (kind == K_CODES || max != 1)) ok = false;
    uint32_t ns = 0;
    if (ok && max > 0) {
      offs[1] = 0;
      for (uint32_t l = 1; l < 15; l++) offs[l + 1] = offs[l] + count[l];
      for (uint32_t i = 0; i < n; i++)
        if (lens[i]) t.sorted[offs[lens[i]]++] = (uint16_t)i;
      ns = offs[max];
      // canonical codes in sorted order; codes longer than the root share a sub-table per root
      // prefix, sized by the longest code under that prefix (the last one: lengths do not decrease)
      uint32_t code = 0, prev_len = lens[t.sorted[0]], used = 1u << root;
      uint32_t i = 0;
      while (i < ns) {
        const uint32_t len = lens[t.sorted[i]];
        code <<= (len - prev_len);
        prev_len = len;
        if (len <= root) {
          t.code[i] = (uint16_t)rev16(code, len);
          t.sub[i] = 0;
          code++;
          i++;
          continue;
        }
        const uint32_t prefix = code >> (len - root);
        uint32_t j = i, cj = code, pl = len, last_len = len;
        while (j < ns) {  // the symbols under this prefix
          const uint32_t lj = lens[t.sorted[j]];
          const uint32_t cc = cj << (lj - pl);
          if ((cc >> (lj - root)) != prefix) break;
          t.code[j] = (uint16_t)rev16(cc, lj);
          cj = cc + 1;
          pl = lj;
          last_len = lj;
          j++;
        }
        const uint32_t sb = last_len - root;
        if (used + (1u << sb) > cap) { ok = false; break; }
        for (uint32_t k = i; k < j; k++) t.sub[k] = (uint16_t)(used | (sb << 12));
        tab[rev16(prefix, root)] = mk_entry(root, OP_LINK, sb, used);
        used += 1u << sb;
        code = cj;
        prev_len = pl;
        i = j;
      }
    }
    t.nsorted = ns;
    t.status = ok ? 1u : 0u;
  }
  c.sync();
  if (!t.status) return false;
  const uint32_t ns = t.nsorted;
  for (uint32_t i = lane; i < ns; i += nl) {
    const uint32_t sym = t.sorted[i], len = lens[sym], rc = t.code[i];
    if (len <= root) {
      const uint32_t e = sym_entry(kind, sym, len);
      for (uint32_t k = rc; k < (1u << root); k += 1u << len) tab[k] = e;
    } else {
      const uint32_t so = t.sub[i] & 0xfffu, sb = t.sub[i] >> 12;
      const uint32_t e = sym_entry(kind, sym, len - root);
      for (uint32_t k = rc >> root; k < (1u << sb); k += 1u << (len - root)) tab[so + k] = e;
    }
  }
  c.sync();
  return true;
}

struct Bits {
  uint64_t hold;
  uint32_t cnt, nw;
};
template <class C>
DEV void fill(C &c, Bits &b) {  // afterwards at least 32 bits are held
  if (b.cnt <= 32) {
    b.hold |= (uint64_t)c.word(b.nw) << b.cnt;
    b.nw++;
    b.cnt += 32;
  }
}
DEV void drop(Bits &b, uint32_t k) { b.hold >>= k; b.cnt -= k; }
template <class C>
DEV uint32_t take(C &c, Bits &b, uint32_t k) {  // k <= 16
  fill(c, b);
  const uint32_t v = (uint32_t)b.hold & ((1u << k) - 1u);
  drop(b, k);
  return v;
}
template <class C>
DEV uint64_t bitpos(C &c, const Bits &b) { return 32ull * b.nw - b.cnt - 8ull * c.sa(); }
template <class C>
DEV void seek(C &c, Bits &b, uint32_t byte_off) {
  const uint32_t a = byte_off + c.sa();
  b.nw = a >> 2;
  b.hold = 0;
  b.cnt = 0;
  fill(c, b);
  drop(b, 8 * (a & 3));
}

template <class C>
DEV uint32_t lookup(C &c, Bits &b, const uint32_t *tab, uint32_t root) {  // the entry; its bits are dropped
  fill(c, b);
  uint32_t e = tab[(uint32_t)b.hold & ((1u << root) - 1u)];
  if (e_op(e) == OP_LINK) {
    drop(b, root);
    e = tab[e_val(e) + ((uint32_t)b.hold & ((1u << e_extra(e)) - 1u))];
  }
  if (e_op(e) != OP_BAD) drop(b, e_bits(e));
  return e;
}

// One page's block: every member in turn (gzip_decode's loop). `op` bytes in all must be exactly
// dlen. *members: members completed.
template <class C>
DEV bool inflate_block(C &c, Tables &t, uint32_t n, uint32_t dlen, uint32_t *members) {
  const uint64_t nbits = 8ull * n;
  const uint32_t lane = c.lane();
  const uint32_t *T = c.crc_tab();
  Bits b{0, 0, 0};
  seek(c, b, 0);
  uint32_t op = 0, nmem = 0;
  *members = 0;
  for (;;) {  // members
    c.step();
    // --- header (inflate.c HEAD .. HCRC) ---
    uint32_t hc = 0xffffffffu;
    auto byte = [&]() -> uint32_t {
      const uint32_t v = take(c, b, 8);
      hc = crc_byte(T, hc, v);
      return v;
    };
    const uint32_t id1 = byte(), id2 = byte(), cm = byte(), flg = byte();
    if (id1 != 0x1f || id2 != 0x8b || cm != 8 || (flg & 0xe0)) return false;
    for (int k = 0; k < 6; k++) byte();  // MTIME, XFL, OS
    if (bitpos(c, b) > nbits) return false;
    if (flg & 4) {  // FEXTRA
      uint32_t xlen = byte();
      xlen |= byte() << 8;
      for (; xlen && bitpos(c, b) <= nbits; xlen--) { c.step(); byte(); }
    }
    if (flg & 8)  // FNAME
      while (bitpos(c, b) <= nbits) { c.step(); if (!byte()) break; }
    if (flg & 16)  // FCOMMENT
      while (bitpos(c, b) <= nbits) { c.step(); if (!byte()) break; }
    if (flg & 2) {  // FHCRC
      const uint32_t want = ~hc & 0xffffu;
      uint32_t got = take(c, b, 8);
      got |= take(c, b, 8) << 8;
      if (got != want) return false;
    }
    if (bitpos(c, b) > nbits) return false;
    const uint32_t mstart = op;
    // --- blocks ---
    for (;;) {
      c.step();
      const uint32_t last = take(c, b, 1), type = take(c, b, 2);
      if (bitpos(c, b) > nbits) return false;
      if (type == 3) return false;
      if (type == 0) {
        drop(b, b.cnt & 7);
        const uint32_t len = take(c, b, 16), nlen = take(c, b, 16);
        if (len != (~nlen & 0xffffu)) return false;
        const uint64_t bp = bitpos(c, b);
        if (bp > nbits) return false;
        const uint32_t p = (uint32_t)(bp >> 3);
        if (len > n - p || len > dlen - op) return false;
        if (len) c.stored(p, len);
        op += len;
        seek(c, b, p + len);
      } else {
        if (type == 1) {
          for (uint32_t i = lane; i < 288; i += c.nl()) t.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
          for (uint32_t i = lane; i < 32; i += c.nl()) t.lens[288 + i] = 5;
          if (!build_table(c, t, t.lit, kLitTab, kLitRoot, t.lens, 288, K_LENS)) return false;
          if (!build_table(c, t, t.dist, kDistTab, kDistRoot, t.lens + 288, 32, K_DISTS)) return false;
        } else {
          const uint32_t hlit = take(c, b, 5) + 257, hdist = take(c, b, 5) + 1, hclen = take(c, b, 4) + 4;
          if (hlit > 286 || hdist > 30) return false;
          for (uint32_t i = 0; i < 19; i++) {
            const uint32_t v = i < hclen ? take(c, b, 3) : 0;
            // order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
            const uint32_t sym = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 7 - ((i - 5) >> 1) : ((i + 12) >> 1);
            if (lane == 0) t.lens[sym] = (uint8_t)v;
          }
          if (bitpos(c, b) > nbits) return false;
          if (!build_table(c, t, t.cl, kClTab, kClRoot, t.lens, 19, K_CODES)) return false;
          const uint32_t total = hlit + hdist;
          uint32_t have = 0, prev = 0;
          while (have < total) {
            c.step();
            if (bitpos(c, b) > nbits) return false;
            const uint32_t e = lookup(c, b, t.cl, kClRoot);
            if (e_op(e) == OP_BAD) return false;
            const uint32_t sym = e_val(e);
            if (sym < 16) {
              if (lane == 0) t.lens[have] = (uint8_t)sym;
              have++;
              prev = sym;
              continue;
            }
            uint32_t rep, val = 0;
            if (sym == 16) {
              if (have == 0) return false;
              val = prev;
              rep = 3 + take(c, b, 2);
            } else if (sym == 17) {
              rep = 3 + take(c, b, 3);
            } else {
              rep = 11 + take(c, b, 7);
            }
            if (have + rep > total) return false;
            if (lane == 0)
              for (uint32_t k = 0; k < rep; k++) t.lens[have + k] = (uint8_t)val;
            have += rep;
            prev = val;
          }
          if (bitpos(c, b) > nbits) return false;
          c.sync();
          if (t.lens[256] == 0) return false;  // missing end-of-block
          if (!build_table(c, t, t.lit, kLitTab, kLitRoot, t.lens, hlit, K_LENS)) return false;
          if (!build_table(c, t, t.dist, kDistTab, kDistRoot, t.lens + hlit, hdist, K_DISTS)) return false;
        }
        for (;;) {  // symbols
          c.step();
          if (bitpos(c, b) > nbits) return false;
          const uint32_t e = lookup(c, b, t.lit, kLitRoot);
          const uint32_t o = e_op(e);
          if (o == OP_LIT) {
            if (op >= dlen) return false;
            c.lit(e_val(e));
            op++;
            continue;
          }
          if (o == OP_EOB) break;
          if (o != OP_BASE) return false;
          const uint32_t xl = e_extra(e);
          const uint32_t len = e_val(e) + ((uint32_t)b.hold & ((1u << xl) - 1u));
          drop(b, xl);
          const uint32_t d = lookup(c, b, t.dist, kDistRoot);
          if (e_op(d) != OP_BASE) return false;
          const uint32_t xd = e_extra(d);
          const uint32_t dist = e_val(d) + ((uint32_t)b.hold & ((1u << xd) - 1u));
          drop(b, xd);
          if (bitpos(c, b) > nbits) return false;
          if (dist > op - mstart || len > dlen - op) return false;
          c.copy(dist, len);
          op += len;
        }
      }
      if (last) break;
    }
    // --- trailer ---
    drop(b, b.cnt & 7);
    uint32_t crc = take(c, b, 16);
    crc |= take(c, b, 16) << 16;
    uint32_t isize = take(c, b, 16);
    isize |= take(c, b, 16) << 16;
    const uint64_t bp = bitpos(c, b);
    if (bp > nbits) return false;
    if (c.member_crc() != crc || isize != op - mstart) return false;
    nmem++;
    *members = nmem;
    if ((bp >> 3) >= n) break;
  }
  return op == dlen;
}

}  // namespace inf
}  // namespace pq
