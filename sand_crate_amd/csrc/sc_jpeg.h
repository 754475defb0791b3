// JPEG encoding of an RGB frame on the device (sc_jpeg_encode_device / sc_render_jpeg): baseline sequential JPEG,
// 4:4:4, the Annex K tables, one restart interval per MCU row.  The bitstream is specified in NumPy by
// tests/jpeg_spec.py; these kernels reproduce it byte for byte.  Included once by sandcrate_hip.hip.  Encoding only
// reads the frame: no counter, flag or particle array is written.
//
//   dct     8 threads per 8x8 block (Y, Cb or Cr of one MCU): colour conversion with edge replication, the integer
//           DCT (a row of the block per thread, then a column through LDS), quantisation; writes the zig-zagged int16
//           coefficients, a mask of the nonzero AC positions and the block's AC code length in bits
//   rows    a wave per MCU row (restart interval): lanes take blocks, add the DC code, a wave prefix sum places them,
//           each lane ORs its codes into an LDS window that is flushed to the row's bit buffer as it fills; the row
//           is padded with 1-bits and its 0xFF bytes counted, which gives its stuffed length
//   scan    one wave: exclusive scan of the stuffed row lengths (an RST marker after all but the last row)
//   stuff   a wave per row: copies the row behind the others with a 0x00 after every 0xFF, then its RST marker
// The host builds the header (SOI .. SOS), reads the total length once, then copies the bytes and appends EOI.
#pragma once
#include "sc_device.h"

namespace sc {

// Annex K.1 quantisation tables (natural order) and K.3 Huffman tables (BITS, HUFFVAL)
constexpr unsigned char kJpegLumaQ[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                          14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                          18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                          49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr unsigned char kJpegChromaQ[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
                                            24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                            99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                            99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
constexpr unsigned char kJpegDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                              {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr unsigned char kJpegDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr unsigned char kJpegAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                              {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr unsigned char kJpegAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14,
     0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09,
     0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a,
     0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65,
     0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88,
     0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9,
     0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea,
     0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32,
     0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16,
     0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39,
     0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64,
     0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86,
     0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
     0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8,
     0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9,
     0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
// the zig-zag position of each natural (row-major) coefficient index
struct JpegZigzag {
  unsigned char of[64];
};
constexpr JpegZigzag kJpegZigzag = {{0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42,
                                     3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                     10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60,
                                     21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63}};
// A[u][x] = round(4096 / 2 c(u) cos((2x + 1) u pi / 16))
constexpr int kJpegDct[8][8] = {{1448, 1448, 1448, 1448, 1448, 1448, 1448, 1448},
                                {2009, 1703, 1138, 400, -400, -1138, -1703, -2009},
                                {1892, 784, -784, -1892, -1892, -784, 784, 1892},
                                {1703, -400, -2009, -1138, 1138, 2009, 400, -1703},
                                {1448, -1448, -1448, 1448, 1448, -1448, -1448, 1448},
                                {1138, -2009, 400, 1703, -1703, -400, 2009, -1138},
                                {784, -1892, 1892, -784, -784, 1892, -1892, 784},
                                {400, -1138, 1703, -2009, 2009, -1703, 1138, -400}};

// The longest a block's codes can be: a DC code of 11 bits plus 11 extra bits, and 63 AC codes of 16 bits plus 10
// (the quantised AC coefficients stay below 1024 in magnitude, so size 10 is the largest category: the sign patterns of
// the (0,4), (4,0) and (4,4) basis functions reach 1020 at quality 100 and nothing reaches more, which
// tests/test_jpeg_cases_cpu.py::test_quantised_ac_coefficients_stay_below_1024 pins).
constexpr int kJpegBlockBits = 22 + 63 * 26;
constexpr int kJpegWaveBits = 64 * kJpegBlockBits + 32;          // one round of the rows kernel, word offset included
constexpr int kJpegWindowWords = (kJpegWaveBits + 31) / 32 + 2;  // its LDS window (13.3 KB)

// Huffman codes as (length << 16) | code, Annex C.
struct JpegHuff {
  unsigned dc[2][12];
  unsigned ac[2][256];
};

constexpr JpegHuff make_jpeg_huff() {
  JpegHuff h{};
  for (int t = 0; t < 2; ++t) {
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < kJpegDcBits[t][len - 1]; ++i) h.dc[t][kJpegDcVals[k++]] = ((unsigned)len << 16) | code++;
      code <<= 1;
    }
    code = 0;
    k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < kJpegAcBits[t][len - 1]; ++i) h.ac[t][kJpegAcVals[t][k++]] = ((unsigned)len << 16) | code++;
      code <<= 1;
    }
  }
  return h;
}

__constant__ JpegHuff kJpegHuff = make_jpeg_huff();
__constant__ JpegZigzag kJpegZz = kJpegZigzag;

struct JpegDims {
  int width, height;
  int mcus;       // MCUs per row = ceil(W / 8), the restart interval
  int rows;       // MCU rows = ceil(H / 8)
  int quant[2][64];  // luminance, chrominance; natural order
};

__device__ __forceinline__ int jpeg_bits_of(int v) { return 32 - __clz(v < 0 ? -v : v); }  // magnitude category
__device__ __forceinline__ unsigned jpeg_extra(int v, int size) {  // v, or v - 1 if negative, in `size` bits
  return (unsigned)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
}

// 8 threads per block, blocks in coding order b = (row * mcus + mcu) * 3 + component.  Thread t of a block converts
// and transforms pixel row t, then finishes column t.
__global__ void __launch_bounds__(kBlock) k_jpeg_dct(JpegDims d, const unsigned char* __restrict__ rgb,
                                                     short* __restrict__ coef, unsigned long long* __restrict__ masks,
                                                     int* __restrict__ acbits) {
  __shared__ int t1s[kBlock / 8][8][9];
  const int nblocks = d.rows * d.mcus * 3;
  const int g = (int)(blockIdx.x * kBlock + threadIdx.x);
  const int b = g >> 3, t = g & 7, lb = (int)(threadIdx.x >> 3);
  const bool live = b < nblocks;  // the 8 threads of a block agree
  const int comp = live ? b % 3 : 0;
  if (live) {
    const int mcu = b / 3, r = mcu / d.mcus, m = mcu - r * d.mcus;
    const int y = min(r * 8 + t, d.height - 1);
    const unsigned char* row = rgb + (size_t)y * d.width * 3;
    int s[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      const unsigned char* p = row + 3 * min(m * 8 + x, d.width - 1);
      const int R = p[0], G = p[1], B = p[2];
      const int v = comp == 0 ? (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
                  : comp == 1 ? (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
                              : (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
      s[x] = v - 128;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      int T = 0;
#pragma unroll
      for (int x = 0; x < 8; ++x) T += kJpegDct[u][x] * s[x];
      t1s[lb][t][u] = (T + 256) >> 9;
    }
  }
  __syncthreads();
  unsigned long long mask = 0;
  int q[8];
  if (live) {
    int col[8];
#pragma unroll
    for (int yy = 0; yy < 8; ++yy) col[yy] = t1s[lb][yy][t];
    const int* Q = d.quant[comp == 0 ? 0 : 1];
    short* out = coef + (size_t)b * 64;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      int U = 0;
#pragma unroll
      for (int yy = 0; yy < 8; ++yy) U += kJpegDct[v][yy] * col[yy];
      const unsigned Qv = (unsigned)Q[v * 8 + t];
      const unsigned a = (unsigned)(U < 0 ? -U : U);
      const int m = (int)((a + (Qv << 14)) / (Qv << 15));
      q[v] = U < 0 ? -m : m;
      const int zz = kJpegZz.of[v * 8 + t];
      out[zz] = (short)q[v];
      if (q[v] != 0 && zz > 0) mask |= 1ull << zz;
    }
  }
  // the block's nonzero AC positions, then the length of its AC codes (each lane its own coefficients)
  mask |= __shfl_xor(mask, 1);
  mask |= __shfl_xor(mask, 2);
  mask |= __shfl_xor(mask, 4);
  int bits = 0;
  if (live) {
    const int tab = comp == 0 ? 0 : 1;
    const int zrl = (int)(kJpegHuff.ac[tab][0xF0] >> 16);
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const int zz = kJpegZz.of[v * 8 + t];
      if (q[v] != 0 && zz > 0) {
        const int prev = 63 - __clzll((long long)((mask | 1ull) & ((1ull << zz) - 1ull)));
        const int run = zz - prev - 1, size = jpeg_bits_of(q[v]);
        bits += (run >> 4) * zrl + (int)(kJpegHuff.ac[tab][((run & 15) << 4) | size] >> 16) + size;
      }
    }
    if (t == 0 && (mask >> 63) == 0) bits += (int)(kJpegHuff.ac[tab][0x00] >> 16);  // EOB
  }
  bits += __shfl_xor(bits, 1);
  bits += __shfl_xor(bits, 2);
  bits += __shfl_xor(bits, 4);
  if (live && t == 0) {
    masks[b] = mask;
    acbits[b] = bits;
  }
}

// ORs the `len` (<= 27) low bits of `val` into the MSB-first bit stream `w` at bit `pos`.
__device__ __forceinline__ void jpeg_put(unsigned* w, int pos, unsigned val, int len) {
  const int k = pos >> 5, s = pos & 31;
  if (s + len <= 32) {
    atomicOr(w + k, val << (32 - s - len));
  } else {
    atomicOr(w + k, val >> (s + len - 32));
    atomicOr(w + k + 1, val << (64 - s - len));
  }
}

__device__ __forceinline__ int jpeg_ff_bytes(unsigned x, int n) {  // 0xFF bytes among the n most significant of x
  int c = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) c += (i < n && ((x >> (24 - 8 * i)) & 0xFFu) == 0xFFu) ? 1 : 0;
  return c;
}

__device__ __forceinline__ int wave_inclusive_sum(int v) {
  const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  return v;
}

// One wave per MCU row.  rowbuf holds row r's bytes in stream order from word r * row_words; row_bytes[r] is its
// padded length, row_len[r] its length once stuffed, with the RST marker that follows all rows but the last.
__global__ void __launch_bounds__(64) k_jpeg_rows(JpegDims d, const short* __restrict__ coef,
                                                  const unsigned long long* __restrict__ masks,
                                                  const int* __restrict__ acbits, unsigned* __restrict__ rowbuf,
                                                  long long row_words, int* __restrict__ row_bytes,
                                                  int* __restrict__ row_len) {
  __shared__ unsigned win[kJpegWindowWords];
  const int r = (int)blockIdx.x, lane = (int)threadIdx.x;
  const int nb = 3 * d.mcus;
  const size_t b0 = (size_t)r * nb;
  unsigned* out = rowbuf + (size_t)r * row_words;
  for (int k = lane; k < kJpegWindowWords; k += 64) win[k] = 0u;
  __syncthreads();
  long long base = 0;  // bits of the row so far; win[0] is word base >> 5
  int ff = 0;
  for (int c0 = 0; c0 < nb; c0 += 64) {
    const int k = c0 + lane;
    const bool live = k < nb;
    const int tab = live && k % 3 != 0 ? 1 : 0;
    int diff = 0, cat = 0, bits = 0;
    unsigned long long mask = 0;
    unsigned dcc = 0;
    if (live) {
      const int dc = coef[(b0 + k) * 64];
      diff = dc - (k >= 3 ? (int)coef[(b0 + k - 3) * 64] : 0);
      cat = jpeg_bits_of(diff);
      dcc = kJpegHuff.dc[tab][cat];
      mask = masks[b0 + k];
      bits = (int)(dcc >> 16) + cat + acbits[b0 + k];
    }
    const int incl = wave_inclusive_sum(bits);
    const int total = __shfl(incl, 63);
    if (live) {
      int pos = (int)(base & 31) + incl - bits;
      const int dl = (int)(dcc >> 16);
      jpeg_put(win, pos, ((dcc & 0xFFFFu) << cat) | jpeg_extra(diff, cat), dl + cat);
      pos += dl + cat;
      const short* cf = coef + (b0 + k) * 64;
      const unsigned zrl = kJpegHuff.ac[tab][0xF0];
      int prev = 0;
      for (unsigned long long m = mask; m; m &= m - 1) {
        const int p = __builtin_ctzll(m);
        int run = p - prev - 1;
        for (; run >= 16; run -= 16) {
          jpeg_put(win, pos, zrl & 0xFFFFu, (int)(zrl >> 16));
          pos += (int)(zrl >> 16);
        }
        const int qv = cf[p], size = jpeg_bits_of(qv);
        const unsigned h = kJpegHuff.ac[tab][(run << 4) | size];
        const int len = (int)(h >> 16) + size;
        jpeg_put(win, pos, ((h & 0xFFFFu) << size) | jpeg_extra(qv, size), len);
        pos += len;
        prev = p;
      }
      if (prev < 63) {
        const unsigned eob = kJpegHuff.ac[tab][0x00];
        jpeg_put(win, pos, eob & 0xFFFFu, (int)(eob >> 16));
      }
    }
    __syncthreads();
    // flush the words this round completed; the partial last one moves to win[0]
    const long long end = base + total;
    const int full = (int)((end >> 5) - (base >> 5));
    for (int w = lane; w < full; w += 64) {
      const unsigned x = win[w];
      win[w] = 0u;
      ff += jpeg_ff_bytes(x, 4);
      out[(base >> 5) + w] = __builtin_bswap32(x);
    }
    __syncthreads();
    if (lane == 0 && full > 0) {
      win[0] = win[full];
      win[full] = 0u;
    }
    __syncthreads();
    base = end;
  }
  const int nbytes = (int)((base + 7) >> 3);
  if (lane == 0) {
    unsigned x = win[0];
    const int used = (int)(base & 31), pad = (int)(-base & 7);
    if (pad) x |= ((1u << pad) - 1u) << (32 - used - pad);  // 1-bits up to the byte boundary
    const int valid = nbytes - (int)((base >> 5) << 2);
    if (valid > 0) {
      out[base >> 5] = __builtin_bswap32(x);
      ff += jpeg_ff_bytes(x, valid);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ff += __shfl_xor(ff, o);
  if (lane == 0) {
    row_bytes[r] = nbytes;
    row_len[r] = nbytes + ff + (r + 1 < d.rows ? 2 : 0);
  }
}

// One wave: row_off[r] = sum of row_len[0 .. r), row_off[rows] = the total.
__global__ void __launch_bounds__(64) k_jpeg_scan(int rows, const int* __restrict__ row_len,
                                                  long long* __restrict__ row_off) {
  const int lane = (int)threadIdx.x;
  long long base = 0;
  for (int r0 = 0; r0 < rows; r0 += 64) {
    const int r = r0 + lane;
    const int v = r < rows ? row_len[r] : 0;
    const int incl = wave_inclusive_sum(v);
    if (r < rows) row_off[r] = base + incl - v;
    base += __shfl(incl, 63);
  }
  if (lane == 0) row_off[rows] = base;
}

// One wave per row: row r's bytes to out + row_off[r], a 0x00 after every 0xFF, then RST(r mod 8) unless last.
__global__ void __launch_bounds__(64) k_jpeg_stuff(int rows, const unsigned* __restrict__ rowbuf, long long row_words,
                                                   const int* __restrict__ row_bytes,
                                                   const long long* __restrict__ row_off,
                                                   unsigned char* __restrict__ out) {
  const int r = (int)blockIdx.x, lane = (int)threadIdx.x;
  const unsigned* src = rowbuf + (size_t)r * row_words;
  const int n = row_bytes[r];
  unsigned char* dst = out + row_off[r];
  long long at = 0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + 4 * lane;
    const int valid = max(0, min(4, n - i));
    const unsigned x = valid > 0 ? src[i >> 2] : 0u;  // bytes in stream order, little-endian in the word
    int cnt = valid;
#pragma unroll
    for (int j = 0; j < 4; ++j) cnt += (j < valid && ((x >> (8 * j)) & 0xFFu) == 0xFFu) ? 1 : 0;
    const int incl = wave_inclusive_sum(cnt);
    unsigned char* p = dst + at + (incl - cnt);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < valid) {
        const unsigned char c = (unsigned char)(x >> (8 * j));
        *p++ = c;
        if (c == 0xFF) *p++ = 0;
      }
    }
    at += __shfl(incl, 63);
  }
  if (lane == 0 && r + 1 < rows) {
    dst[at] = 0xFF;
    dst[at + 1] = (unsigned char)(0xD0 + (r & 7));
  }
}

}  // namespace sc
