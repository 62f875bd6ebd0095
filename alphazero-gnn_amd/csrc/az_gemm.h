// Internal interface of the GEMM stack: the kernel argument block, the fused epilogue, and every
// az:: function that one translation unit calls in another (az_gemm.hip: the MFMA tiles, the
// M <= 8 GEMVs with the one-launch Connect4 leaf, their dispatch, and the kernels that split
// operands into fp16 planes; az_weights.hip: the registered-weights registry, its per-generation
// caches and the composed heads).  The build is
// -fno-gpu-rdc: a kernel is launched only from the unit that defines it, so a kernel two units
// need sits behind a host function of its owner.  Default arguments are written here, once.
#pragma once
#include "az_common.h"
#include "az_x3.h"

namespace az {


struct GemmArgs {
  int M, N, K;
  const float* A; int lda;
  const float* A2; int lda2; int K0;
  const int* a_rows;
  const float* B; int ldb;
  const int* b_rows;
  const float* bias; int act;
  const float* R; int ldr;
  const float* G; int ldg;
  float beta;
  float* C; int ldc;
  const int* c_rows;
  float* C2; int ldc2;
  // split-K: block (tile, s) covers k in [s*kc, min(K, (s+1)*kc)) and writes raw partial sums
  // to slab[s][M][N]; splitk_reduce_kernel sums the slabs in s order (deterministic) and runs
  // the epilogue.
  int splits, kc;
  float* slab;
  int vec_epi;  // host-checked: N, every leading dimension % 4 == 0 and 16-B aligned C/C2/R/G,
                // so whole float4 rows can leave through epilogue_store4
  int ablate;   // timing experiments only (AZ_GEMM_ABLATE, glds2): 1 = no DMA after the first
                // tile, 2 = no barrier in the k loop; results are then wrong
  // gemm_p3: A already split into its two fp16 planes (az_x3.h p2_chunk layout) at apl
  const unsigned short* apl;
  size_t apl_plane;   // elements per plane (M * K)
  // gemm_p3: W already split too, in the same layout at bpl
  const unsigned short* bpl;
  size_t bpl_plane;   // elements per plane (N * K)
  // gemm_x3 in its fp16 form (H3): per-row power-of-two scales of A ([2][M]: s, then 1/s) and of
  // W ([2][N]), row_scale_kernel
  const float* sa;
  const float* sw;
  // gemm_p3 HEADS: the heads' dot products per tile row instead of C / slabs (az_x3.h HeadsEpi)
  HeadsEpi he;
  int heads_done;   // host side: launch_x3 ran the HEADS form (no C, no slabs written)
};

__device__ __forceinline__ void epilogue_store(const GemmArgs& p, int row, int col, float acc) {
  if (row >= p.M || col >= p.N) return;
  float v = acc + (p.bias ? p.bias[col] : 0.f);
  if (p.act == AZ_ACT_DRELU) {
    v = p.G[(size_t)row * p.ldg + col] > 0.f ? v : 0.f;
  } else {
    v = apply_act(v, p.act);
  }
  if (p.C2) p.C2[(size_t)row * p.ldc2 + col] = v;
  const int cr = p.c_rows ? p.c_rows[row] : row;
  if (p.R) v = p.R[(size_t)cr * p.ldr + col] + (p.G ? p.G[(size_t)row * p.ldg + col] : 1.f) * v;
  float* dst = p.C + (size_t)cr * p.ldc + col;
  if (p.beta != 0.f) v += p.beta * *dst;
  *dst = v;
}

// epilogue_store for 4 consecutive columns (col % 4 == 0, col + 4 <= N, p.vec_epi): one float4
// load / store per operand instead of four scalar ones.
__device__ __forceinline__ void epilogue_store4(const GemmArgs& p, int row, int col, f32x4 v) {
  if (row >= p.M || col >= p.N) return;
  if (p.bias) {
    const f32x4 b = *reinterpret_cast<const f32x4*>(p.bias + col);
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] += b[c];
  }
  if (p.act == AZ_ACT_DRELU) {
    const f32x4 g = *reinterpret_cast<const f32x4*>(p.G + (size_t)row * p.ldg + col);
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = g[c] > 0.f ? v[c] : 0.f;
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = apply_act(v[c], p.act);
  }
  if (p.C2) *reinterpret_cast<f32x4*>(p.C2 + (size_t)row * p.ldc2 + col) = v;
  const int cr = p.c_rows ? p.c_rows[row] : row;
  if (p.R) {
    const f32x4 r = *reinterpret_cast<const f32x4*>(p.R + (size_t)cr * p.ldr + col);
    f32x4 g = {1.f, 1.f, 1.f, 1.f};
    if (p.G) g = *reinterpret_cast<const f32x4*>(p.G + (size_t)row * p.ldg + col);
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = r[c] + g[c] * v[c];
  }
  f32x4* dst = reinterpret_cast<f32x4*>(p.C + (size_t)cr * p.ldc + col);
  if (p.beta != 0.f) {
    const f32x4 o = *dst;
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] += p.beta * o[c];
  }
  *dst = v;
}

struct SideHeads;   // az_heads.h

// ---- az_gemm.hip
int gemm_f32(const az_gemm_desc* d, hipStream_t s);
int gemm_f32_partial(const az_gemm_desc* d, hipStream_t s, int* splits_out, const PreSplitA* pre,
                     const HeadsEpi* he = nullptr, bool* heads_done = nullptr);
int splitk_reduce(const az_gemm_desc* d, int splits, hipStream_t s);
bool gemm_p2_certain(const az_gemm_desc* d, hipStream_t s);
bool gemm_p2_weights(const float* w, int n, int k, int ld);
int gemv1_with_side_heads(const az_gemm_desc* d, const SideHeads* h, hipStream_t s);
int gemv_multi_fwd(const az_gemm_desc* d0, const az_gemm_desc* d1, const az_gemm_desc* d2,
                   hipStream_t s);
int c4_leaf_fwd(const az_c4_eval* e, const int8_t* boards, int B, float* pi, float* v, float* gpi,
                float* gv, hipStream_t s);
int splitk_reduce_split(const az_gemm_desc* d, int splits, unsigned short* planes, float* sc,
                        hipStream_t s, bool write_c = true);
// The kernels the weights cache launches, on stream s.  They sit in az_gemm.hip: launch_x3 runs
// the first two on A's rows per call, splitk_reduce_split_kernel writes the same planes, and a
// kernel in another code object than the GEMM it runs between cost the B = 512 step 0.3 us.
void launch_row_scale(const float* X, int rows, int cols, int ld, int T, float* out,
                      hipStream_t s);
void launch_h3_split_rows(const float* X, int rows, int cols, int ld, int T, unsigned short* out,
                          float* sc, hipStream_t s);
constexpr int W2P_UNITS = 4 * 18 * 64;                 // c4_w2_planes_kernel's output: 16-B units
constexpr int W2P_FLOATS = W2P_UNITS * 4 + 4 * 64;     // ... in floats, with the 1 / scale rows
void launch_c4_w2_planes(const float* w2, float* out, hipStream_t s);

// ---- az_weights.hip
bool weights_registered(const float* w, int n, int k, int ld);
const float* w_row_scales(const float* w, int n, int k, int ld, hipStream_t s);
const unsigned short* w_planes(const float* w, int n, int k, int ld, hipStream_t s,
                               const float** scales);
const float* conv2_planes(const float* w2, hipStream_t s);
size_t composed_heads_scratch_bytes(int F, int A);
const float* composed_heads(const float* w2, const float* b2, const float* wp, const float* bp,
                            const float* wv, const float* bv, int F, int A, float* scratch,
                            hipStream_t s);

}  // namespace az
