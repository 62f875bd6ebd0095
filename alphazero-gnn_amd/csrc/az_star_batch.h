// What the packed-star units share (az_star_batch.hip: inference; az_star_train.hip: the training
// forward and backward): the tile constants, a star's clamped row span and the shape rule.
#pragma once
#include "az_gemm.h"

namespace az {

constexpr int SB_TILE = 32;   // neighbour weights a block keeps in LDS at a time
constexpr int SB_CH = 8;      // neighbour rows whose loads are in flight before the first add
constexpr size_t SB_SPLIT_BYTES = size_t(40) << 20;   // split-K slabs of the layer GEMMs

struct StarSpan {
  int o, n;   // first row, rows
};

// offs[b] .. offs[b+1] clamped into the V rows (a bad value cannot index outside x), at least one
// row, wave-uniform
__device__ __forceinline__ StarSpan star_span(const int* __restrict__ offs, int b, int V) {
  int o = offs[b];
  const int e = offs[b + 1];
  o = o < 0 ? 0 : (o > V - 1 ? V - 1 : o);
  int n = e - o;
  n = n < 1 ? 1 : (n > V - o ? V - o : n);
  return {__builtin_amdgcn_readfirstlane(o), __builtin_amdgcn_readfirstlane(n)};
}

static inline size_t sb_pad(size_t bytes) { return (bytes + 255) / 256 * 256; }

static inline bool star_batch_shape(int B, int V, int F, int H, int L) {
  return B >= 0 && V >= B && F >= 16 && F % 16 == 0 && F <= (1 << 20) && H >= 4 && H % 4 == 0 &&
         H <= (1 << 16) && L >= 0 && L <= AZ_STAR_MAX_LAYERS && (size_t)V * F < (size_t(1) << 40);
}

}  // namespace az
