// The exact-fp32 GEMM of batch-invariant evaluation: the plan, the kernel and reduce
// templates with the epilogue as a template parameter, and what the units built on them share.
//   az_gemm_exact.hip      the plain epilogue (bias, ReLU): az_gemm_exact_f32, az_eval_exact_fwd
//   az_gemm_exact_ex.hip   sigmoid, the gated residual and the paired launch: az_gemm_exact_ex
//   az_star_exact.hip      the exact star layer stack and az_star_eval_exact_fwd (host code only)
// Each unit instantiates its own kernels, so a kernel's code does not depend on what the other
// epilogues need.
//
// The arithmetic of C[i][j] = epi(sum_k A[i][k] W[j][k] + bias[j]) is the contract:
//   - K is cut into S contiguous segments (exact_plan: a function of N and K only);
//   - each segment is ONE chain acc = fmaf(a[k], w[k], acc) in ascending k, from +0 -- the
//     f32-input MFMA (v_mfma_f32_32x32x2_f32) is that chain bit for bit, k0 before k1 inside an
//     instruction, one rounding per product;
//   - the segment sums are added in ascending order with plain fp32 adds, then the bias, then the
//     epilogue.
// Nothing here reads M except to size the launch (grid, waves per block) and to mask loads and
// stores, so row i of a call is the same bits whatever M is and wherever the row sits, and a CPU
// loop over the plan reproduces it (tests/exact_ref.py).  No atomics.  Rows past M / N and k past
// a segment's end are ZEROED in LDS (never loaded), so memory behind the operands may hold
// anything, NaN included: a padded step is fmaf(0, 0, acc) = acc.
#pragma once
#include <algorithm>

#include "az_common.h"

namespace az {

// Block tile: up to 4 waves x (32 rows x 64 columns).  A call of <= 32 / <= 64 rows launches
// blocks of 1 / 2 waves (a launch dimension, like the grid): every output is still the same chain,
// but a one-row call -- a pure weight stream -- does not spend three waves' MFMA time on empty
// rows (40 -> 22 us at N = K = 3136), and its smaller LDS tile lets five blocks share a CU.
constexpr int EX_BM = 128, EX_BN = 64, EX_BK = 32;
constexpr int EX_LDK = EX_BK + 4;
constexpr int EX_MAX_SEG = AZ_EXACT_MAX_SEGMENTS;
constexpr int EX_MIN_SEG = 128;       // shortest segment a plan cuts (but for the last one)
constexpr int EX_TARGET_BLOCKS = 512; // column tiles x segments a plan aims at: one row still
                                      // spreads over 256 CUs, two blocks each
constexpr int EX_DIRECT_BLOCKS = 128; // row tiles x column tiles from which a block walks all the
                                      // segments itself (grid.z = 1) and no slab is written

struct ExactPlan {
  int S;   // segments
  int L;   // length of every segment but the last (a multiple of EX_BK); the last: K - (S-1) L
};

// The K cut.  N and K only: there is no M to depend on.
static inline ExactPlan exact_plan(int N, int K) {
  const int nt = (N + EX_BN - 1) / EX_BN;
  int want = (EX_TARGET_BLOCKS + nt - 1) / nt;
  want = std::min(std::max(want, 1), EX_MAX_SEG);
  int L = (K + want - 1) / want;
  L = std::max(L, EX_MIN_SEG);
  L = (L + EX_BK - 1) / EX_BK * EX_BK;
  ExactPlan p;
  p.L = L;
  p.S = std::max(1, (K + L - 1) / L);
  return p;
}

struct ExactArgs {
  int M, N, K;
  const float* A; int lda;
  const float* W; int ldw;
  const float* bias; int act;
  float* C; int ldc;
  int S, L;
  float* slab;   // [S][M][N] raw segment sums when grid.z == S > 1
};

// What a block (or a reduce thread) works on: the plain form reads it straight from the
// arguments, the paired launch picks one of its two products by column tile.
struct ExactSel {
  int n0;              // first output column of the block's tile (unused by the reduce)
  const float* W;
  const float* bias;
  int act;
  float* C;
  float* slab;         // the product's [S][M][N] slabs
};

// The epilogue of az_gemm_exact_f32: bias, then AZ_ACT_NONE or AZ_ACT_RELU.
struct ExactEpiPlain {
  using Args = ExactArgs;
  static __device__ __forceinline__ ExactSel select(const Args& p, int tile) {
    return {tile * EX_BN, p.W, p.bias, p.act, p.C, p.slab};
  }
  // the reduce: element e of [products][M][N / 4] -> its product, e rebased into that product
  static __device__ __forceinline__ ExactSel reduce_select(const Args& p, size_t& e) {
    return {0, p.W, p.bias, p.act, p.C, p.slab};
  }
  static __device__ __forceinline__ int products(const Args& p) { return 1; }
  static __device__ __forceinline__ float apply(const Args& p, const ExactSel& s, float v, int row,
                                                int col) {
    if (s.act == AZ_ACT_RELU) v = v > 0.f ? v : 0.f;
    return v;
  }
};

// One 16-byte piece of a K-major operand tile into LDS, its 4 k values permuted so that a lane's
// ds_read_b128 at [g * 8 + 4 h] holds k = 8 g + 2 t + h, t = 0..3: MFMA t of the group then takes
// k = 8 g + 2 t (lanes 0-31) and 8 g + 2 t + 1 (lanes 32-63) -- ascending k.
__device__ __forceinline__ void exact_store_piece(float* tile, int row, int kq, f32x4 v) {
  float* d = tile + row * EX_LDK + (kq >> 1) * 8 + (kq & 1) * 2;
  d[0] = v[0];
  d[4] = v[1];
  d[1] = v[2];
  d[5] = v[3];
}

static inline int exact_waves(int M) { return M <= 32 ? 1 : M <= 64 ? 2 : EX_BM / 32; }

template <int NW, class EPI>   // waves per block, 32 rows each; the epilogue
__global__ __launch_bounds__(64 * NW) void gemm_exact_kernel(typename EPI::Args p) {
  // pieces of 16 bytes a thread: A's 32 rows per wave are 4 at every block size, W's 64 rows are
  // 8 / 4 / 2 at 1 / 2 / 4 waves
  constexpr int NT = 64 * NW, BM = 32 * NW, AP = 4, WP = EX_BN * EX_BK / 4 / NT;
  __shared__ __attribute__((aligned(16))) float As[2][BM * EX_LDK];
  __shared__ __attribute__((aligned(16))) float Ws[2][EX_BN * EX_LDK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const ExactSel sel = EPI::select(p, blockIdx.x);
  const int n0 = sel.n0, m0 = blockIdx.y * BM;
  // grid.z == S: this block owns segment blockIdx.z; grid.z == 1: it walks all of them in order
  const bool spread = gridDim.z > 1;
  const int s_lo = spread ? blockIdx.z : 0, s_hi = spread ? blockIdx.z + 1 : p.S;

  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 ra[AP], rw[WP];
  auto load = [&](int k0, int kend) {
#pragma unroll
    for (int i = 0; i < AP; ++i) {
      const int idx = tid + NT * i, row = m0 + (idx >> 3), k = k0 + (idx & 7) * 4;
      ra[i] = (row < p.M && k < kend)
                  ? *reinterpret_cast<const f32x4*>(p.A + (size_t)row * p.lda + k) : z4;
    }
#pragma unroll
    for (int i = 0; i < WP; ++i) {
      const int idx = tid + NT * i, row = n0 + (idx >> 3), k = k0 + (idx & 7) * 4;
      rw[i] = (row < p.N && k < kend)
                  ? *reinterpret_cast<const f32x4*>(sel.W + (size_t)row * p.ldw + k) : z4;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < AP; ++i) {
      const int idx = tid + NT * i;
      exact_store_piece(As[buf], idx >> 3, idx & 7, ra[i]);
    }
#pragma unroll
    for (int i = 0; i < WP; ++i) {
      const int idx = tid + NT * i;
      exact_store_piece(Ws[buf], idx >> 3, idx & 7, rw[i]);
    }
  };

  f32x16 total[2];
  for (int sg = s_lo; sg < s_hi; ++sg) {
    const int kbeg = sg * p.L, kend = min(p.K, kbeg + p.L);
    const int nk = (kend - kbeg + EX_BK - 1) / EX_BK;
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    __syncthreads();                 // the previous segment's last reads of buffer 0 are done
    load(kbeg, kend);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      if (kt + 1 < nk) load(kbeg + (kt + 1) * EX_BK, kend);
#pragma unroll
      for (int g = 0; g < EX_BK / 8; ++g) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(
            &As[cur][(wave * 32 + (lane & 31)) * EX_LDK + g * 8 + (lane >> 5) * 4]);
        f32x4 b[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
          b[j] = *reinterpret_cast<const f32x4*>(
              &Ws[cur][(j * 32 + (lane & 31)) * EX_LDK + g * 8 + (lane >> 5) * 4]);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[j][t], acc[j], 0, 0, 0);
      }
      if (kt + 1 < nk) store(cur ^ 1);
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) total[j][r] = sg == s_lo ? acc[j][r] : total[j][r] + acc[j][r];
  }

  // MFMA 32x32 C layout: register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column
  // l & 31
  float* slab = spread ? sel.slab + (size_t)blockIdx.z * p.M * p.N : nullptr;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = n0 + j * 32 + (lane & 31);
    if (col >= p.N) continue;
    const float bias = (!spread && sel.bias) ? sel.bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (row >= p.M) continue;
      if (spread) {
        slab[(size_t)row * p.N + col] = total[j][r];
      } else {
        float v = total[j][r];
        if (sel.bias) v = v + bias;
        sel.C[(size_t)row * p.ldc + col] = EPI::apply(p, sel, v, row, col);
      }
    }
  }
}

// The segment sums of the spread form added in ascending order, then bias and epilogue: four
// columns a thread.
template <class EPI>
__global__ __launch_bounds__(256) void gemm_exact_reduce_kernel(typename EPI::Args p) {
  const int n4 = p.N >> 2;
  const size_t total = (size_t)p.M * n4 * EPI::products(p), plane = (size_t)p.M * p.N;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    size_t e = i;
    const ExactSel sel = EPI::reduce_select(p, e);
    const int row = (int)(e / n4), col = (int)(e % n4) * 4;
    const float* src = sel.slab + (size_t)row * p.N + col;
    f32x4 v = *reinterpret_cast<const f32x4*>(src);
    for (int s = 1; s < p.S; ++s) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(src + s * plane);
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = v[c] + t[c];
    }
    if (sel.bias) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(sel.bias + col);
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = v[c] + b[c];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = EPI::apply(p, sel, v[c], row, col + c);
    *reinterpret_cast<f32x4*>(sel.C + (size_t)row * p.ldc + col) = v;
  }
}

// Does a call of M rows over `products` weight matrices of N rows each (2: the paired launch)
// spread its segments over grid.z (and need slabs)?  Grid size only: both forms add the same
// segment sums in the same order.
static inline bool exact_spread(int M, int N, const ExactPlan& pl, int products = 1) {
  const int bm = 32 * exact_waves(M);
  const long mt = (M + bm - 1) / bm, nt = (long)products * ((N + EX_BN - 1) / EX_BN);
  return pl.S > 1 && mt * nt < EX_DIRECT_BLOCKS;
}

static inline size_t exact_ws_bytes(int M, int N, int K, int products = 1) {
  const ExactPlan pl = exact_plan(N, K);
  return exact_spread(M, N, pl, products) ? (size_t)products * pl.S * M * N * 4 : 0;
}

// The most workspace any call of 1..max_M rows takes (the spread form ends at a row count).
static inline size_t exact_ws_bytes_upto(int max_M, int N, int K, int products = 1) {
  const int nt = products * ((N + EX_BN - 1) / EX_BN);
  const long mt = (EX_DIRECT_BLOCKS - 1) / nt;            // row tiles the spread form still serves
  const long m = std::min<long>(max_M, mt * EX_BM);
  return m < 1 ? 0 : exact_ws_bytes((int)m, N, K, products);
}

// The launch both forms share: grid.x column tiles of every product, grid.z the segments of the
// spread form, then its reduce.  `a` carries the plan (S, L) and the slab pointer.
template <class EPI>
static inline int exact_launch(const typename EPI::Args& a, int products, bool spread,
                               hipStream_t s) {
  const int waves = exact_waves(a.M), bm = 32 * waves;
  const dim3 g(products * ((a.N + EX_BN - 1) / EX_BN), (a.M + bm - 1) / bm, spread ? a.S : 1);
  if (waves == 1) hipLaunchKernelGGL((gemm_exact_kernel<1, EPI>), g, dim3(64), 0, s, a);
  else if (waves == 2) hipLaunchKernelGGL((gemm_exact_kernel<2, EPI>), g, dim3(128), 0, s, a);
  else hipLaunchKernelGGL((gemm_exact_kernel<4, EPI>), g, dim3(256), 0, s, a);
  if (spread) {
    const size_t work = (size_t)products * a.M * (a.N >> 2);
    const int blocks = (int)std::min<size_t>((work + 255) / 256, 4096);
    hipLaunchKernelGGL((gemm_exact_reduce_kernel<EPI>), dim3(blocks), dim3(256), 0, s, a);
  }
  return check_launch("gemm_exact_kernel");
}

// ---- what az_gemm_exact.hip gives the other exact units (host functions)
// az_gemm_exact_f32 without the argument checks
int gemm_exact(const float* A, int lda, const float* W, int ldw, const float* bias, int act,
               float* C, int ldc, int M, int N, int K, void* ws, size_t ws_bytes, hipStream_t s);
// The tail of az_eval_exact_fwd on B rows: the standard heads of rows xs (v != NULL), and
// output_transform.0 / .2 as two exact GEMMs plus the heads of rows xg (gv != NULL).  Scratch
// (h1, h2, hidden, y, logp, glogp) and weights from e; the GEMMs' slabs in ws.
int exact_eval_tail(const az_eval_exact* e, const float* xs, const float* xg, int B, float* pi,
                    float* v, float* gpi, float* gv, void* ws, size_t ws_bytes, hipStream_t s);
// az_eval_exact_fwd's descriptor checks (shape, weights, scratch, alignment), shared with
// az_star_eval_exact_fwd; `who` names the caller in the message
int exact_eval_check(const az_eval_exact* e, const char* who, bool std_heads, bool gnn_tail);
// the fused trunk of e's board on B rows into feat
int exact_eval_trunk(const az_eval_exact* e, const int8_t* boards, int B, float* feat,
                     void* stream);
size_t exact_eval_tail_ws_bytes(int max_B, int game, int nx, int ny);
bool exact_has_trunk(int game, int nx, int ny);
int exact_features(int game, int nx, int ny);

// ---- az_gemm_exact_ex.hip
struct ExactArgsEx : ExactArgs {
  const float* W2; const float* bias2; int act2; float* C2;   // the paired launch (W2 != nullptr)
  int nt;                                                      // column tiles of ONE product
  float* slab2;                                                // the second product's slabs
  const float* R; int ldr; const float* G; int ldg;            // C = fmaf(G, v, R) (G != nullptr)
};
// az_gemm_exact_ex without the argument checks: a.S, a.L, a.nt, a.slab and a.slab2 are set here
int gemm_exact_ex(ExactArgsEx a, void* ws, size_t ws_bytes, hipStream_t s);

}  // namespace az
