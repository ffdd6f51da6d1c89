// arrow.hip — export of a decoded chunk in Arrow's physical layout (pqgpu_batch_export_arrow).
//
// The decoder's result keeps the reference's form (readValues: the non-null values packed, one
// offset per value, one byte per BOOLEAN); Arrow wants one slot per array slot. With
// valid(i) = bit i of the chunk's bitmap and rank(i) = the number of valid slots before i:
//
//   fixed width  dst[i] = valid(i) ? src[rank(i)] : 0          (bit copies)
//   BOOLEAN      bit i  = valid(i) ? src[rank(i)] & 1 : 0
//   BYTE_ARRAY   offsets[i] = src_offsets[rank(i)], i <= length (a null slot is empty)
//
//   k_arrow_rank     one workgroup per tile of kArT slots: popcount of the tile's 256 bitmap words
//   k_arrow_scan     one workgroup: exclusive 64-bit bases of the tile counts, kArS tiles per step
//   k_arrow_expand*  one workgroup per tile: the bitmap words and the block scan of their popcounts
//                    in LDS, then output-stationary emission: every lane owns aligned 16-B pieces
//                    of the output, takes each slot's rank from the word base and a masked
//                    popcount, reads the (monotone, near-contiguous) source and stores the piece
//                    whole, padding included
//   k_arrow_validity the bitmap itself (or all ones), masked by the length, zero past it
//
// The bitmap is read for ceil(length / 32) words and the last word is masked: words past that
// are arena memory the decoder does not define. Ranks are clamped to the value count, so a
// bitmap that disagreed with it could not send a read out of the source. Every kernel writes
// only [0, rounded size) of its destination. No atomics, no communication between workgroups.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace pq {

constexpr uint32_t kArT = kArrowTileHost, kArThreads = 256, kArS = kArrowScanHost;
static_assert(kArT == 32 * kArThreads, "one bitmap word per thread");
static_assert(kArS == 4 * kArThreads, "four tile counts per thread and scan step");

// bitmap word w of a `length`-slot array: no bitmap = all valid; bits at and past length are zero
__device__ __forceinline__ uint32_t ar_word(const uint32_t *bm, uint64_t w, uint64_t nwords, uint64_t length) {
  if (w >= nwords) return 0;
  uint32_t v = bm ? bm[w] : ~0u;
  const uint32_t r = (uint32_t)(length & 31);
  if (w == nwords - 1 && r) v &= (1u << r) - 1;
  return v;
}

// exclusive scan of v over the 256 threads (wsum: 4 LDS words, free again after the next barrier)
__device__ __forceinline__ uint32_t ar_block_excl(uint32_t v, uint32_t *wsum, uint32_t *total) {
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, 64);
    if ((int)lane >= d) x += y;
  }
  if (lane == 63) wsum[wv] = x;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) {
    const uint32_t s = wsum[k];
    if (k < wv) base += s;
    tot += s;
  }
  *total = tot;
  return base + x - v;
}

__global__ __launch_bounds__(256) void k_arrow_rank(const uint32_t *bm, uint64_t nwords, uint64_t length,
                                                    uint32_t *counts) {
  __shared__ uint32_t wsum[4];
  uint32_t c = __popc(ar_word(bm, (uint64_t)blockIdx.x * kArThreads + threadIdx.x, nwords, length));
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// bases[t] = sum of counts[0, t), bases[tiles] = the total
__global__ __launch_bounds__(256) void k_arrow_scan(const uint32_t *counts, uint32_t tiles, uint64_t *bases) {
  __shared__ uint32_t wsum[4];
  uint64_t carry = 0;
  for (uint32_t t0 = 0; t0 < tiles; t0 += kArS) {
    const uint32_t i0 = t0 + threadIdx.x * 4;
    uint32_t c[4], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
      c[k] = i0 + k < tiles ? counts[i0 + k] : 0;
      sum += c[k];
    }
    uint32_t tot;
    uint64_t b = carry + ar_block_excl(sum, wsum, &tot);  // a step sums at most kArS * kArT = 2^23
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
      if (i0 + k < tiles) bases[i0 + k] = b;
      b += c[k];
    }
    carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) bases[tiles] = carry;
}

// the tile's masked bitmap words and their exclusive popcount bases into LDS; returns the tile's
// rank base (no bases: every slot before the tile is valid)
__device__ __forceinline__ uint64_t ar_tile_setup(const uint32_t *bm, uint64_t nwords, uint64_t length,
                                                  const uint64_t *bases, uint32_t *words, uint32_t *wbase,
                                                  uint32_t *wsum) {
  const uint32_t v = ar_word(bm, (uint64_t)blockIdx.x * kArThreads + threadIdx.x, nwords, length);
  uint32_t tot;
  words[threadIdx.x] = v;
  wbase[threadIdx.x] = ar_block_excl(__popc(v), wsum, &tot);
  __syncthreads();
  return bases ? bases[blockIdx.x] : (uint64_t)blockIdx.x * kArT;
}

// 4- and 8-byte values (OFFS = false) and BYTE_ARRAY offsets (OFFS = true: entries [0, length] are
// src[rank], null slots included, the padding behind them zero). out_elems: the destination's
// rounded size in elements, a multiple of the elements per piece.
template <typename T, bool OFFS>
__global__ __launch_bounds__(256) void k_arrow_expand(const uint32_t *bm, uint64_t nwords, uint64_t length,
                                                      const uint64_t *bases, const T *src, uint64_t nv, T *dst,
                                                      uint64_t out_elems) {
  __shared__ uint32_t words[kArThreads], wbase[kArThreads], wsum[4];
  const uint64_t base = ar_tile_setup(bm, nwords, length, bases, words, wbase, wsum);
  constexpr uint32_t kPer = 16 / sizeof(T), kPieces = kArT / kPer;
  const uint64_t slot0 = (uint64_t)blockIdx.x * kArT;
  for (uint32_t p = threadIdx.x; p < kPieces; p += kArThreads) {
    const uint32_t ls = p * kPer, bit = ls & 31;
    const uint64_t gs = slot0 + ls;
    if (gs >= out_elems) break;
    const uint32_t wv = words[ls >> 5];
    uint64_t r = base + wbase[ls >> 5] + __popc(wv & ((1u << bit) - 1));
    union { T v[kPer]; uint4 q; } o;
#pragma unroll
    for (uint32_t k = 0; k < kPer; k++) {
      const uint32_t valid = (wv >> (bit + k)) & 1;
      if (OFFS) o.v[k] = gs + k <= length ? src[r < nv ? r : nv] : (T)0;
      else o.v[k] = (valid && r < nv) ? src[r] : (T)0;
      r += valid;
    }
    *(uint4 *)(dst + gs) = o.q;
  }
}

// BOOLEAN: one byte per value in, Arrow's bitmap out. Every thread packs the 32 slots of its
// bitmap word (a loop over the word's valid slots, whose source bytes are adjacent); the words go
// through LDS so that 64 lanes store the tile's 1 KiB in 16-B pieces. out_words: rounded size / 4.
__global__ __launch_bounds__(256) void k_arrow_expand_bool(const uint32_t *bm, uint64_t nwords, uint64_t length,
                                                           const uint64_t *bases, const uint8_t *src, uint64_t nv,
                                                           uint32_t *dst, uint64_t out_words) {
  __shared__ uint32_t words[kArThreads], wbase[kArThreads], wsum[4];
  __shared__ __attribute__((aligned(16))) uint32_t outw[kArThreads];
  const uint64_t base = ar_tile_setup(bm, nwords, length, bases, words, wbase, wsum);
  uint32_t m = words[threadIdx.x], out = 0;
  uint64_t r = base + wbase[threadIdx.x];
  while (m) {
    const uint32_t k = (uint32_t)__ffs((int)m) - 1;
    m &= m - 1;
    if (r < nv) out |= (uint32_t)(src[r] & 1) << k;
    r++;
  }
  outw[threadIdx.x] = out;
  __syncthreads();
  const uint64_t w0 = ((uint64_t)blockIdx.x * kArThreads) + threadIdx.x * 4;
  if (threadIdx.x < kArThreads / 4 && w0 < out_words) *(uint4 *)(dst + w0) = *(const uint4 *)(outw + threadIdx.x * 4);
}

// Any width (INT96, FIXED_LEN_BYTE_ARRAY): the general path, byte by byte into 16-B pieces.
// out_bytes: the destination's rounded size.
__global__ __launch_bounds__(256) void k_arrow_expand_bytes(const uint32_t *bm, uint64_t nwords, uint64_t length,
                                                            const uint64_t *bases, const uint8_t *src, uint64_t nv,
                                                            uint32_t width, uint8_t *dst, uint64_t out_bytes) {
  __shared__ uint32_t words[kArThreads], wbase[kArThreads], wsum[4];
  const uint64_t base = ar_tile_setup(bm, nwords, length, bases, words, wbase, wsum);
  const uint64_t byte0 = (uint64_t)blockIdx.x * kArT * width;
  const uint64_t pieces = (uint64_t)(kArT / 16) * width;
  for (uint64_t p = threadIdx.x; p < pieces; p += kArThreads) {
    const uint64_t gb = byte0 + p * 16;
    if (gb >= out_bytes) break;
    uint32_t ls = (uint32_t)(p * 16 / width), k = (uint32_t)(p * 16 - (uint64_t)ls * width);  // the piece's first byte: slot, byte of the slot
    uint32_t o[4] = {0, 0, 0, 0};
    bool valid = false;
    uint64_t r = 0;
    bool fresh = true;
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) {
      if (k == width) {
        k = 0;
        ls++;
        fresh = true;
      }
      if (fresh) {  // ls < kArT: the tile's bytes are a whole number of pieces
        const uint32_t wv = words[ls >> 5], bit = ls & 31;
        valid = (wv >> bit) & 1;
        r = base + wbase[ls >> 5] + __popc(wv & ((1u << bit) - 1));
        valid = valid && r < nv;
        fresh = false;
      }
      const uint32_t byte = valid ? src[r * width + k] : 0;
      o[i >> 2] |= byte << ((i & 3) * 8);
      k++;
    }
    *(uint4 *)(dst + gb) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// the validity destination: `pieces` 16-B pieces, bitmap words (or ones) below length, zero above
__global__ __launch_bounds__(256) void k_arrow_validity(const uint32_t *bm, uint64_t nwords, uint64_t length, uint4 *dst,
                                                        uint64_t pieces) {
  const uint64_t g = (uint64_t)blockIdx.x * kArThreads + threadIdx.x;
  if (g >= pieces) return;
  dst[g] = make_uint4(ar_word(bm, 4 * g, nwords, length), ar_word(bm, 4 * g + 1, nwords, length),
                      ar_word(bm, 4 * g + 2, nwords, length), ar_word(bm, 4 * g + 3, nwords, length));
}

hipError_t launch_arrow_rank(const uint32_t *bm, uint64_t length, uint32_t tiles, uint32_t *counts, uint64_t *bases,
                             hipStream_t s) {
  if (!tiles) return hipSuccess;
  hipLaunchKernelGGL(k_arrow_rank, dim3(tiles), dim3(kArThreads), 0, s, bm, (length + 31) / 32, length, counts);
  hipLaunchKernelGGL(k_arrow_scan, dim3(1), dim3(kArThreads), 0, s, (const uint32_t *)counts, tiles, bases);
  return hipGetLastError();
}

hipError_t launch_arrow_validity(const uint32_t *bm, uint64_t length, void *dst, uint64_t dst_bytes, hipStream_t s) {
  const uint64_t pieces = dst_bytes / 16;
  if (!pieces) return hipSuccess;
  hipLaunchKernelGGL(k_arrow_validity, dim3((uint32_t)((pieces + kArThreads - 1) / kArThreads)), dim3(kArThreads), 0, s,
                     bm, (length + 31) / 32, length, (uint4 *)dst, pieces);
  return hipGetLastError();
}

hipError_t launch_arrow_expand(ArrowKind kind, const uint32_t *bm, uint64_t length, const uint64_t *bases,
                               const void *src, uint64_t nv, uint32_t width, void *dst, uint64_t dst_bytes,
                               hipStream_t s) {
  if (!dst_bytes) return hipSuccess;
  const uint64_t nwords = (length + 31) / 32;
  // workgroups: the tiles that hold a byte of the rounded destination
  uint64_t per_tile = 0;
  switch (kind) {
    case ARROW_FIXED4: case ARROW_OFFSETS: per_tile = (uint64_t)kArT * 4; break;
    case ARROW_FIXED8: per_tile = (uint64_t)kArT * 8; break;
    case ARROW_BOOL: per_tile = kArT / 8; break;
    case ARROW_BYTES: per_tile = (uint64_t)kArT * width; break;
  }
  if (!per_tile) return hipErrorInvalidValue;
  const dim3 grid((uint32_t)((dst_bytes + per_tile - 1) / per_tile)), block(kArThreads);
  switch (kind) {
    case ARROW_FIXED4:
      hipLaunchKernelGGL((k_arrow_expand<uint32_t, false>), grid, block, 0, s, bm, nwords, length, bases,
                         (const uint32_t *)src, nv, (uint32_t *)dst, dst_bytes / 4);
      break;
    case ARROW_OFFSETS:
      hipLaunchKernelGGL((k_arrow_expand<uint32_t, true>), grid, block, 0, s, bm, nwords, length, bases,
                         (const uint32_t *)src, nv, (uint32_t *)dst, dst_bytes / 4);
      break;
    case ARROW_FIXED8:
      hipLaunchKernelGGL((k_arrow_expand<uint64_t, false>), grid, block, 0, s, bm, nwords, length, bases,
                         (const uint64_t *)src, nv, (uint64_t *)dst, dst_bytes / 8);
      break;
    case ARROW_BOOL:
      hipLaunchKernelGGL(k_arrow_expand_bool, grid, block, 0, s, bm, nwords, length, bases, (const uint8_t *)src, nv,
                         (uint32_t *)dst, dst_bytes / 4);
      break;
    case ARROW_BYTES:
      hipLaunchKernelGGL(k_arrow_expand_bytes, grid, block, 0, s, bm, nwords, length, bases, (const uint8_t *)src, nv,
                         width, (uint8_t *)dst, dst_bytes);
      break;
  }
  return hipGetLastError();
}

}  // namespace pq
