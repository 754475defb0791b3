// A stable LSD radix sort of (32-bit key, 32-bit value) pairs, hand-written.  Included once by sandcrate_hip.hip; sc_host.h's
// radix_sort runs the passes over a RadixSpace.
//
// A pass orders by kRadixDigitBits bits of the key, from the lowest digit up, and moves the pairs from one set of arrays
// to the other:
//   k_radix_hist     a workgroup counts the digits of its kRadixTile keys in LDS (integer atomics) and writes its 256
//                    counts digit-major: hist[digit * tiles + tile].  The keys come from its type parameter: a functor
//                    that yields the key of element i -- the kernel then stores the pair (key, i), so the first pass of a
//                    sort makes the pairs without a launch or a pass over the keys of its own -- or RadixStored: the pairs
//                    are in the arrays already;
//   k_scan_local / k_scan_fix (sc_kernels.h)  the exclusive scan of those counts: in digit-major order it is, for every
//                    (digit, tile), the place of the tile's first key with that digit;
//   k_radix_scatter  a key goes to that place plus its rank among the tile's keys of the same digit: the lanes of a wave
//                    that hold the same digit find each other with eight ballots, the waves' counts meet in LDS.
// Keys of equal digit keep their order, so p passes order by the lowest 8 p bits of the key and leave equal keys in the
// order they came in.  No workgroup waits for another, no floating-point or order-dependent atomics: the result is a
// pure function of the pairs.  Cost: linear in the number of pairs, whatever the keys are.
#pragma once
#include <type_traits>

#include "sc_device.h"

namespace sc {

constexpr int kRadixTile = 256;  // keys (= threads) per workgroup of a sorting pass
constexpr int kRadixDigitBits = 8;
constexpr int kRadixBins = 1 << kRadixDigitBits;
static_assert(kRadixBins == kRadixTile, "thread t writes the tile's count of digit t");

struct RadixStored {};  // k_radix_hist's marker: the keys are in `keys`

template <class Key>
__global__ void __launch_bounds__(kRadixTile)
    k_radix_hist(Key key_of, unsigned* __restrict__ keys, int* __restrict__ vals, int m, int shift, int tiles,
                 int* __restrict__ hist) {
  __shared__ int s_h[kRadixBins];
  const int tid = (int)threadIdx.x;
  s_h[tid] = 0;
  __syncthreads();
  const int i = (int)blockIdx.x * kRadixTile + tid;
  if (i < m) {
    unsigned key;
    if constexpr (std::is_same_v<Key, RadixStored>) {
      key = keys[i];
    } else {
      key = key_of(i);
      keys[i] = key;
      vals[i] = i;
    }
    atomicAdd(&s_h[(key >> shift) & (kRadixBins - 1)], 1);
  }
  __syncthreads();
  hist[(size_t)tid * tiles + blockIdx.x] = s_h[tid];
}

__global__ void __launch_bounds__(kRadixTile)
    k_radix_scatter(const unsigned* __restrict__ keys_in, const int* __restrict__ vals_in, unsigned* __restrict__ keys_out,
                    int* __restrict__ vals_out, int m, int shift, int tiles, const int* __restrict__ offs) {
  __shared__ int s_cnt[kRadixTile / 64][kRadixBins];
  const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int w = 0; w < kRadixTile / 64; ++w) s_cnt[w][tid] = 0;
  __syncthreads();
  const int i = (int)blockIdx.x * kRadixTile + tid;
  const bool on = i < m;
  const unsigned key = on ? keys_in[i] : 0u;
  const int val = on ? vals_in[i] : 0;
  const int digit = (int)((key >> shift) & (kRadixBins - 1));
  // the lanes of this wave that hold a key with the same digit (every lane of the wave takes part in the ballots)
  unsigned long long peers = __ballot(on);
#pragma unroll
  for (int b = 0; b < kRadixDigitBits; ++b) {
    const bool bit = (digit >> b) & 1;
    const unsigned long long set = __ballot(on && bit);
    peers &= bit ? set : ~set;
  }
  const int rank = __popcll(peers & ((1ull << lane) - 1ull));
  if (on && rank == 0) s_cnt[wv][digit] = __popcll(peers);
  __syncthreads();
  if (on) {
    int before = 0;
    for (int w = 0; w < wv; ++w) before += s_cnt[w][digit];
    const int dest = offs[(size_t)digit * tiles + blockIdx.x] + before + rank;
    if ((unsigned)dest < (unsigned)m) {  // (always, when the counts are this launch's)
      keys_out[dest] = key;
      vals_out[dest] = val;
    }
  }
}

}  // namespace sc
