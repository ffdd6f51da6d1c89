// inflate.hip — k_inflate: a GZIP data page's block -> the page data, one wave per page
// (compress.go:63-76, :125-130: the reference's GZIP codec is compress/gzip's reader; verdicts are
// zlib's gzip mode, which the host route and the oracle use). The decode itself is
// inflate_core.h, shared with the host checker; this file gives it the device context:
//
//   source   the block is read 512 B ahead into two registers per lane (lane k: dwords k and
//            64 + k of the window) and handed out with readlane; the partial last dword is masked
//            by the block length (a resident block is followed by the next page's bytes).
//   tables   first-level + sub-tables in LDS, entries filled by the 64 lanes a stride apart.
//   symbols  decoded wave-uniformly. Literals collect in a register (lane k: the k-th pending
//            literal) and land in the window with one 64-lane store; a match is copied 64 bytes per
//            step by all lanes (distance < 64: lane i reads byte i mod distance of the period).
//   window   the most recent 32 KiB of the page in LDS: deflate's whole distance range, so no
//            copy reads flushed output back. It is flushed to HBM in aligned 16-B pieces when the
//            next write would overtake unflushed bytes.
//   CRC32    of each member over the pieces as they are flushed: every lane checksums its 16 bytes
//            from a zero register, the pieces combine by crc(A || B) = crc(A) x^(8|B|) xor crc(B)
//            (carry-less product mod P, as pagewalk.hip's k_page_crc), so the page is not read again.
//
// Output layout as k_snappy's: the V2 raw level prefix, the inflated bytes, zeros to the next
// 16-B boundary, then the 64-B zero pad. Any error: report(..., ST_DECOMP, PQ_ERR_DECOMPRESS).
#include "dev_util.h"
#include "inflate_core.h"

namespace pq {

constexpr uint32_t kInfRing = 32768, kInfMask = kInfRing - 1;
__device__ const inf::X8Table kInfX8 = inf::make_x8();

struct InfCtx {
  inf::Tables *t;
  uint8_t *ring;         // LDS, 16-B aligned
  uint8_t *dst;          // page data (global, 16-B aligned)
  const uint8_t *src;    // the block
  const uint32_t *srcw;  // its aligned floor
  uint32_t sa_, wlim;    // bytes in front of the block in its first dword; block end in aligned bytes
  uint32_t wb, W0, W1;   // window base (aligned bytes) and its two halves
  uint32_t flushed;      // page bytes [0, flushed) are in dst; a multiple of 16
  uint32_t P;            // page bytes [0, P) are in the window or flushed
  uint32_t crc_pos, crc_state;  // member checksum register over page bytes [member start, crc_pos)
  uint32_t nlit, litreg;        // pending literals (lane k: the k-th)
  uint32_t lane_;

  DEV uint32_t lane() const { return lane_; }
  DEV uint32_t nl() const { return 64; }
  DEV void sync() { wave_lds_sync(); }
  DEV uint32_t sa() const { return sa_; }
  DEV const uint32_t *crc_tab() const { return t->crc; }
  DEV void step() {}

  DEV uint32_t ldw(uint32_t at) const {  // the dword at aligned offset at + 4 * lane, zero past the block
    const uint32_t k = at + 4 * lane_;
    if (k >= wlim) return 0u;
    const uint32_t w = srcw[k >> 2];
    return k + 4 <= wlim ? w : w & ((1u << (8 * (wlim - k))) - 1u);
  }
  DEV uint32_t word(uint32_t k) {
    const uint32_t at = sgpr(4 * k);
    if (at - wb >= 512) {  // (also a position in front of the window)
      wb = at & ~255u;
      W0 = ldw(wb);
      W1 = ldw(wb + 256);
    } else if (at - wb >= 256) {
      W0 = W1;
      wb += 256;
      W1 = ldw(wb + 256);
    }
    return rdlane(W0, sgpr((at - wb) >> 2));
  }

  // member checksum over window bytes [crc_pos, upto)
  DEV void crc_advance(uint32_t upto) {
    const uint32_t *T = t->crc;
    for (uint32_t x0 = crc_pos & ~15u; x0 < upto; x0 += 1024) {
      const uint32_t end = min(upto, x0 + 1024);
      const uint32_t x = x0 + 16 * lane_, a = max(x, crc_pos), e = min(x + 16, end);
      uint32_t r = 0;
      if (a < e) {
        const uint4 v = *(const uint4 *)(ring + (x & kInfMask));
        const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t i = 0; i < 16; i++) {
          const uint32_t by = (vw[i >> 2] >> (8 * (i & 3))) & 0xffu;
          if (x + i >= a && x + i < e) r = inf::crc_byte(T, r, by);
        }
        r = inf::gf2_mulmod(r, kInfX8.v[end - e]);
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) r ^= __shfl_xor(r, d, 64);
      crc_state = sgpr(inf::gf2_mulmod(crc_state, kInfX8.v[end - max(x0, crc_pos)]) ^ r);
    }
    crc_pos = upto;
  }
  DEV void flush(uint32_t upto) {  // window [flushed, upto) -> dst, upto % 16 == 0
    if (upto > crc_pos) crc_advance(upto);
    for (uint32_t x = flushed + lane_ * 16; x < upto; x += 64 * 16)
      *(uint4 *)(dst + x) = *(const uint4 *)(ring + (x & kInfMask));
    flushed = upto;
  }
  // before page bytes [P, P + k) are written (k <= 256): the bytes they replace are flushed
  DEV void room(uint32_t k) {
    if (P + k - flushed > kInfRing) flush(P & ~15u);
  }
  DEV void flush_lits() {
    if (!nlit) return;
    room(nlit);
    if (lane_ < nlit) ring[(P + lane_) & kInfMask] = (uint8_t)litreg;
    P += nlit;
    nlit = 0;
    wave_lds_sync();
  }
  DEV void lit(uint32_t b) {
    if (lane_ == nlit) litreg = b;
    nlit++;
    if (nlit == 64) flush_lits();
  }
  DEV void copy(uint32_t dist, uint32_t len) {
    flush_lits();
    // distance < 64: the last `dist` bytes repeat; lane i takes byte i mod dist of that period
    uint32_t m = lane_;
    if (dist < 64) m = lane_ - dist * (uint32_t)(((float)lane_ + 0.5f) * __builtin_amdgcn_rcpf((float)dist));
    while (len) {
      const uint32_t k = min(len, 64u);
      room(k);
      uint32_t v = 0;
      if (lane_ < k) v = ring[(P - dist + m) & kInfMask];
      if (lane_ < k) ring[(P + lane_) & kInfMask] = (uint8_t)v;
      wave_lds_sync();
      P += k;
      len -= k;
    }
  }
  // global bytes S[0, len) -> the window
  DEV void put(const uint8_t *S, uint32_t len) {
    uint32_t o = 0;
    while (o < len) {
      const uint32_t k = min(len - o, 256u);
      room(k);
      uint32_t v[4];
#pragma unroll
      for (uint32_t u = 0; u < 4; u++) v[u] = 64 * u + lane_ < k ? S[o + 64 * u + lane_] : 0u;
#pragma unroll
      for (uint32_t u = 0; u < 4; u++)
        if (64 * u + lane_ < k) ring[(P + 64 * u + lane_) & kInfMask] = (uint8_t)v[u];
      P += k;
      o += k;
    }
    wave_lds_sync();
  }
  DEV void stored(uint32_t off, uint32_t len) {
    flush_lits();
    put(src + off, len);
  }
  DEV uint32_t member_crc() {
    flush_lits();
    if (P > crc_pos) crc_advance(P);
    const uint32_t c = ~crc_state;
    crc_state = 0xffffffffu;
    return c;
  }
};

__global__ void __launch_bounds__(64) k_inflate(BatchDev b_in, const InflateJob *jobs, unsigned long long *members) {
  const BatchDev b = global_view(b_in);
  __shared__ __attribute__((aligned(16))) uint8_t ring[kInfRing];
  __shared__ inf::Tables tab;
  const InflateJob &jb = gp(jobs)[blockIdx.x];
  const uint32_t lane = lane_id();
  const uint32_t n = sgpr(jb.src_len), raw = sgpr(jb.raw_len), dlen = sgpr(jb.dlen);
  for (uint32_t k = lane; k < 256; k += 64) tab.crc[k] = inf::crc_table_entry(k);
  InfCtx c;
  c.t = &tab;
  c.ring = ring;
  c.dst = gp_u64<uint8_t>(jb.dst);
  c.src = gp_u64<const uint8_t>(jb.src);
  c.sa_ = sgpr((uint32_t)((uintptr_t)c.src & 3));
  c.srcw = (const uint32_t *)(c.src - c.sa_);
  c.wlim = n + c.sa_;
  c.lane_ = lane;
  c.wb = 0;
  c.W0 = c.ldw(0);
  c.W1 = c.ldw(256);
  c.flushed = 0;
  c.P = 0;
  c.nlit = 0;
  c.litreg = 0;
  c.crc_state = 0xffffffffu;
  c.crc_pos = raw;  // the raw prefix belongs to no member
  wave_lds_sync();
  if (raw) c.put(gp_u64<const uint8_t>(jb.raw), raw);  // V2: the uncompressed level sections first
  uint32_t nmem = 0;
  const bool ok = inf::inflate_block(c, tab, n, dlen, &nmem);
  if (!ok) {
    if (lane == 0) report(b, jb.chunk, 0, jb.page_in_chunk, ST_DECOMP, 0, PQ_ERR_DECOMPRESS);
    return;
  }
  // last piece: zeros past the page end, then the 64 B zero pad every page section carries
  c.flush_lits();
  const uint32_t end = c.P, end16 = (end + 15) & ~15u;
  c.room(16);
  if (end + lane < end16) ring[(end + lane) & kInfMask] = 0;
  wave_lds_sync();
  c.flush(end16);
  if (lane < 4) *(uint4 *)(c.dst + end16 + lane * 16) = uint4{0, 0, 0, 0};
  if (lane == 0) atomicAdd(gp(members), (unsigned long long)nmem);
}

hipError_t launch_inflate(const BatchDev &b, const InflateJob *jobs, uint32_t njobs, unsigned long long *members,
                          hipStream_t s) {
  if (!njobs) return hipSuccess;
  hipLaunchKernelGGL(k_inflate, dim3(njobs), dim3(64), 0, s, b, jobs, members);
  return hipGetLastError();
}

}  // namespace pq
