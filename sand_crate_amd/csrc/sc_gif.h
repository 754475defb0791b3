// GIF encoding of a palette frame on the device (sc_gif_encode_device / sc_render_gif): the image data of one frame,
// variable-width LZW over one index byte per pixel, restarted with a clear code every 1024 pixels.  The bitstream is
// specified in NumPy by tests/gif_spec.py; these kernels reproduce it byte for byte.  Included once by
// sandcrate_hip.hip.  Encoding only reads the frame: no counter, flag or particle array is written.
//
//   lzw     a wave per chunk of 1024 pixels.  The lanes stage the chunk's pixels in LDS and clear the dictionary, a
//           hash table in LDS keyed by (prefix code, byte); lane 0 then walks the chunk -- greedy longest match is one
//           chain of dependent look-ups, there is nothing for the other lanes to share -- and the lanes copy the codes
//           out.  Code widths follow from a code's position in its chunk, so only the codes and their count are kept
//   scan    one wave: each chunk's length in bits from its count and the width its clear code inherits from the chunk
//           before, an exclusive scan of those, the framed length of the whole stream
//   merge   a wave per chunk: a lane per code, ORed into the zeroed output at the chunk's bit offset (neighbouring
//           chunks share a byte, hence atomics).  Stream byte k lands at 2 + k + k / 255: behind the minimum code size
//           and one length byte per sub-block of 255, which this pass fills in as well
// The host reads the total length once, zeroes that much of the output, runs merge and copies the bytes.
#pragma once
#include "sc_device.h"
#include "sc_jpeg.h"  // wave_inclusive_sum

namespace sc {

constexpr int kGifChunk = 1024;             // pixels between two clear codes
constexpr int kGifSlots = 2 * kGifChunk;    // dictionary slots: a chunk adds at most 1023 strings, so at most half fill
constexpr unsigned kGifClear = 256u, kGifEnd = 257u, kGifFirst = 258u;

// The j-th code after a clear code (j = 1, 2, ..) is written with 9 bits up to j = 255, 10 up to 767, then 11: the
// dictionary's next free code is 257 + j when it goes out, and the width grows once that has reached a power of two.
__device__ __forceinline__ int gif_width_after(int n) { return n < 255 ? 9 : (n < 767 ? 10 : 11); }
// ... and the first n of them take this many bits together.
__device__ __forceinline__ int gif_code_bits(int n) {
  return 9 * min(n, 255) + 10 * min(max(n - 255, 0), 512) + 11 * max(n - 767, 0);
}

// One wave per chunk.  codes: kGifChunk per chunk; ncodes[c] of them are set (at least 1, at most the chunk's pixels).
__global__ void __launch_bounds__(64) k_gif_lzw(const unsigned char* __restrict__ index, long long pixels,
                                                unsigned short* __restrict__ codes, int* __restrict__ ncodes) {
  __shared__ unsigned table[kGifSlots];  // (prefix << 19 | byte << 11 | code), 0 = free (codes start at 258)
  __shared__ unsigned char pix[kGifChunk];
  __shared__ unsigned short out[kGifChunk];
  __shared__ int count;
  const int lane = (int)threadIdx.x;
  const long long first = (long long)blockIdx.x * kGifChunk;
  const int n = (int)min((long long)kGifChunk, pixels - first);
  for (int k = lane; k < n; k += 64) pix[k] = index[first + k];
  for (int k = lane; k < kGifSlots; k += 64) table[k] = 0u;
  __syncthreads();
  if (lane == 0) {
    unsigned prefix = pix[0], next = kGifFirst;
    int m = 0;
    for (int i = 1; i < n; ++i) {
      const unsigned key = (prefix << 8) | pix[i];  // 11 + 8 bits
      unsigned h = (key * 2654435761u) >> 21;       // 11 bits = kGifSlots
      unsigned e = table[h];
      while (e != 0u && (e >> 11) != key) {
        h = (h + 1u) & (kGifSlots - 1);
        e = table[h];
      }
      if (e != 0u) {
        prefix = e & 0x7FFu;
      } else {
        out[m++] = (unsigned short)prefix;
        table[h] = (key << 11) | next++;
        prefix = key & 0xFFu;
      }
    }
    out[m++] = (unsigned short)prefix;
    count = m;
  }
  __syncthreads();
  const int m = count;
  unsigned short* dst = codes + (size_t)blockIdx.x * kGifChunk;
  for (int k = lane; k < m; k += 64) dst[k] = out[k];
  if (lane == 0) ncodes[blockIdx.x] = m;
}

// One wave.  bit_off[c] = the bit at which chunk c's clear code starts, bit_off[chunks] = where the end code starts;
// totals[0] = the length of the image data (minimum code size, sub-blocks, terminator), totals[1] = that of the packed
// stream inside it.
__global__ void __launch_bounds__(64) k_gif_scan(int chunks, const int* __restrict__ ncodes,
                                                 long long* __restrict__ bit_off, long long* __restrict__ totals) {
  const int lane = (int)threadIdx.x;
  long long base = 0;
  for (int c0 = 0; c0 < chunks; c0 += 64) {
    const int c = c0 + lane;
    int v = 0;
    if (c < chunks) v = (c > 0 ? gif_width_after(ncodes[c - 1]) : 9) + gif_code_bits(ncodes[c]);
    const int incl = wave_inclusive_sum(v);
    if (c < chunks) bit_off[c] = base + incl - v;
    base += __shfl(incl, 63);
  }
  if (lane == 0) {
    bit_off[chunks] = base;
    const long long bytes = (base + gif_width_after(ncodes[chunks - 1]) + 7) >> 3;
    totals[0] = 2 + bytes + (bytes + 254) / 255;
    totals[1] = bytes;
  }
}

// ORs byte `b` of the packed stream's byte k into its framed place in `out` (zeroed, 4-byte aligned).
__device__ __forceinline__ void gif_or_byte(unsigned* __restrict__ out, long long k, unsigned b) {
  const long long at = 2 + k + k / 255;
  if (b) atomicOr(out + (at >> 2), b << (8 * (int)(at & 3)));
}

// The `width` low bits of `code` at bit `pos` of the LSB-first stream: at most 7 + 11 bits, three bytes.
__device__ __forceinline__ void gif_put(unsigned* __restrict__ out, long long pos, unsigned code, int width) {
  const unsigned v = code << (int)(pos & 7);
  const long long k = pos >> 3;
  const int last = (int)((pos + width - 1) >> 3) - (int)k;
  gif_or_byte(out, k, v & 0xFFu);
  if (last >= 1) gif_or_byte(out, k + 1, (v >> 8) & 0xFFu);
  if (last >= 2) gif_or_byte(out, k + 2, v >> 16);
}

// One wave per chunk; `out` holds totals[0] zeroed bytes (rounded up to whole words).
__global__ void __launch_bounds__(64) k_gif_merge(int chunks, const unsigned short* __restrict__ codes,
                                                  const int* __restrict__ ncodes, const long long* __restrict__ bit_off,
                                                  const long long* __restrict__ totals, unsigned* __restrict__ out) {
  const int c = (int)blockIdx.x, lane = (int)threadIdx.x;
  const int m = ncodes[c];
  const long long at = bit_off[c];
  const int clear_width = c > 0 ? gif_width_after(ncodes[c - 1]) : 9;
  const unsigned short* src = codes + (size_t)c * kGifChunk;
  if (lane == 0) gif_put(out, at, kGifClear, clear_width);
  for (int j = lane; j < m; j += 64)  // the (j + 1)-th code after the clear
    gif_put(out, at + clear_width + gif_code_bits(j), src[j], gif_width_after(j));
  if (c == chunks - 1 && lane == 0) gif_put(out, bit_off[chunks], kGifEnd, gif_width_after(m));
  // the framing: sub-block b's length byte stands at 1 + 256 b; the terminator stays zero
  const long long stream = totals[1], nblocks = (stream + 254) / 255;
  for (long long b = (long long)c * 64 + lane; b < nblocks; b += (long long)chunks * 64) {
    const long long p = 1 + 256 * b;
    atomicOr(out + (p >> 2), (unsigned)min(255LL, stream - 255 * b) << (8 * (int)(p & 3)));
  }
  if (c == 0 && lane == 0) atomicOr(out, 8u);  // the minimum code size
}

}  // namespace sc
