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

// az_star_batch.hip's two kernels for the exact layer stack (az_star_exact.hip), which runs them
// unchanged: TA[b] = [t | agg] of every star (t / Pt nullptr: the star's own row 0 and its P row),
// and x0[b] = the star's row 0 for every star (all != 0) or for the one-row stars only.
int star_batch_agg(const float* x, const int* offs, int B, int V, int F, int H, const float* P,
                   const float* t, const float* Pt, const float* b1, const float* w2,
                   const float* b2, float* TA, hipStream_t s);
int star_batch_row0(const float* x, const int* offs, int B, int V, int F, int all, float* x0,
                    hipStream_t s);
// the argument checks of az_gnn_star_batch_infer after the shape rule (pointers, alignment, the
// workspace size when L > 0, layer weights, a host offs that does not ascend from 0 to V); `who` names the entry point in the message
int star_batch_check(const char* who, const float* x, const int* offs, int B, int V, int L,
                     const az_gnn_layer_w* layers, const float* x0, const void* ws,
                     size_t ws_bytes, size_t ws_need);
int star_offs_check(const char* who, const int* offs, int B, int V);

}  // namespace az
