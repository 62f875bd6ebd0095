// Batch-invariant evaluation: an exact-fp32 GEMM whose every output is a fixed fmaf chain, and the
// one-call evaluator built on it (az_gemm_exact_f32, az_eval_exact_fwd).
//
// The arithmetic of C[i][j] = act(sum_k A[i][k] W[j][k] + bias[j]) is the contract:
//   - K is cut into S contiguous segments (exact_plan: a function of N and K only);
//   - each segment is ONE chain acc = fmaf(a[k], w[k], acc) in ascending k, from +0 -- the
//     f32-input MFMA (v_mfma_f32_32x32x2_f32) is that chain bit for bit, k0 before k1 inside an
//     instruction, one rounding per product;
//   - the segment sums are added in ascending order with plain fp32 adds, then the bias, then the
//     activation.
// Nothing here reads M except to size the launch (grid, waves per block) and to mask loads and
// stores, so row i of a call is the same bits whatever M is and wherever the row sits, and a CPU
// loop over the plan reproduces it (tests/exact_ref.py).  No atomics.  Rows past M / N and k past
// a segment's end are ZEROED in LDS (never loaded), so memory behind the operands may hold
// anything, NaN included: a padded step is fmaf(0, 0, acc) = acc.
#include <algorithm>

#include "az_common.h"
#include "az_heads.h"

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
static ExactPlan exact_plan(int N, int K) {
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

static int exact_waves(int M) { return M <= 32 ? 1 : M <= 64 ? 2 : EX_BM / 32; }

template <int NW>   // waves per block, 32 rows each
__global__ __launch_bounds__(64 * NW) void gemm_exact_kernel(ExactArgs p) {
  // pieces of 16 bytes a thread: A's 32 rows per wave are 4 at every block size, W's 64 rows are
  // 8 / 4 / 2 at 1 / 2 / 4 waves
  constexpr int NT = 64 * NW, BM = 32 * NW, AP = 4, WP = EX_BN * EX_BK / 4 / NT;
  __shared__ __attribute__((aligned(16))) float As[2][BM * EX_LDK];
  __shared__ __attribute__((aligned(16))) float Ws[2][EX_BN * EX_LDK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * EX_BN, m0 = blockIdx.y * BM;
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
                  ? *reinterpret_cast<const f32x4*>(p.W + (size_t)row * p.ldw + k) : z4;
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
  float* slab = spread ? p.slab + (size_t)blockIdx.z * p.M * p.N : nullptr;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = n0 + j * 32 + (lane & 31);
    if (col >= p.N) continue;
    const float bias = (!spread && p.bias) ? p.bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (row >= p.M) continue;
      if (spread) {
        slab[(size_t)row * p.N + col] = total[j][r];
      } else {
        float v = total[j][r];
        if (p.bias) v = v + bias;
        if (p.act == AZ_ACT_RELU) v = v > 0.f ? v : 0.f;
        p.C[(size_t)row * p.ldc + col] = v;
      }
    }
  }
}

// The segment sums of the spread form added in ascending order, then bias and activation: four
// columns a thread.
__global__ __launch_bounds__(256) void gemm_exact_reduce_kernel(ExactArgs p) {
  const int n4 = p.N >> 2;
  const size_t total = (size_t)p.M * n4, plane = (size_t)p.M * p.N;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int row = (int)(i / n4), col = (int)(i % n4) * 4;
    const float* src = p.slab + (size_t)row * p.N + col;
    f32x4 v = *reinterpret_cast<const f32x4*>(src);
    for (int s = 1; s < p.S; ++s) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(src + s * plane);
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = v[c] + t[c];
    }
    if (p.bias) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(p.bias + col);
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = v[c] + b[c];
    }
    if (p.act == AZ_ACT_RELU) {
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = v[c] > 0.f ? v[c] : 0.f;
    }
    *reinterpret_cast<f32x4*>(p.C + (size_t)row * p.ldc + col) = v;
  }
}

// Does a call of M rows spread its segments over grid.z (and need slabs)?  Grid size only: both
// forms add the same segment sums in the same order.
static bool exact_spread(int M, int N, const ExactPlan& pl) {
  const int bm = 32 * exact_waves(M);
  const long mt = (M + bm - 1) / bm, nt = (N + EX_BN - 1) / EX_BN;
  return pl.S > 1 && mt * nt < EX_DIRECT_BLOCKS;
}

static size_t exact_ws_bytes(int M, int N, int K) {
  const ExactPlan pl = exact_plan(N, K);
  return exact_spread(M, N, pl) ? (size_t)pl.S * M * N * 4 : 0;
}

// The most workspace any call of 1..max_M rows takes (the spread form ends at a row count).
static size_t exact_ws_bytes_upto(int max_M, int N, int K) {
  const int nt = (N + EX_BN - 1) / EX_BN;
  const long mt = (EX_DIRECT_BLOCKS - 1) / nt;            // row tiles the spread form still serves
  const long m = std::min<long>(max_M, mt * EX_BM);
  return m < 1 ? 0 : exact_ws_bytes((int)m, N, K);
}

static int gemm_exact(const float* A, int lda, const float* W, int ldw, const float* bias, int act,
                      float* C, int ldc, int M, int N, int K, void* ws, size_t ws_bytes,
                      hipStream_t s) {
  const ExactPlan pl = exact_plan(N, K);
  ExactArgs a;
  a.M = M; a.N = N; a.K = K;
  a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.bias = bias; a.act = act;
  a.C = C; a.ldc = ldc; a.S = pl.S; a.L = pl.L;
  a.slab = static_cast<float*>(ws);
  const bool spread = exact_spread(M, N, pl);
  AZ_REQUIRE(!spread || (ws && aligned16(ws) && ws_bytes >= exact_ws_bytes(M, N, K)), AZ_EINVAL,
             "az_gemm_exact_f32: workspace too small (az_gemm_exact_ws_bytes: %zu bytes, 16B "
             "aligned)", exact_ws_bytes(M, N, K));
  const int waves = exact_waves(M), bm = 32 * waves;
  const dim3 g((N + EX_BN - 1) / EX_BN, (M + bm - 1) / bm, spread ? pl.S : 1);
  AZ_REQUIRE(g.y <= 65535, AZ_EINVAL, "az_gemm_exact_f32: M=%d too large", M);
  if (waves == 1) hipLaunchKernelGGL(gemm_exact_kernel<1>, g, dim3(64), 0, s, a);
  else if (waves == 2) hipLaunchKernelGGL(gemm_exact_kernel<2>, g, dim3(128), 0, s, a);
  else hipLaunchKernelGGL(gemm_exact_kernel<4>, g, dim3(256), 0, s, a);
  if (spread) {
    const size_t work = (size_t)M * (N >> 2);
    const int blocks = (int)std::min<size_t>((work + 255) / 256, 4096);
    hipLaunchKernelGGL(gemm_exact_reduce_kernel, dim3(blocks), dim3(256), 0, s, a);
  }
  return check_launch("gemm_exact_kernel");
}

// The heads of one row per block, the same form at every B (heads_row_block: chunk partials by
// wave, summed in chunk order).
template <int AMAX>
__global__ __launch_bounds__(256) void exact_heads_kernel(
    const float* __restrict__ hp, int ldhp, const float* __restrict__ hv, int ldhv, int K,
    const float* __restrict__ wp, int A, const float* __restrict__ wv,
    const float* __restrict__ bp, const float* __restrict__ bv, float* __restrict__ logp,
    float* __restrict__ pi, float* __restrict__ v) {
  __shared__ float part[HEADS_ROWS_MAXC * (AMAX + 1)];
  __shared__ float sm[AMAX + 1];
  const int row = blockIdx.x;
  heads_row_block<AMAX, 4>(hp + (size_t)row * ldhp, hv + (size_t)row * ldhv, K, wp, A, wv, bp, bv,
                           row, logp, pi, v, part, sm);
}

static int exact_heads(const float* hp, const float* hv, int ld, int B, int K, const float* wp,
                       const float* bp, int A, const float* wv, const float* bv, float* logp,
                       float* pi, float* v, hipStream_t s) {
  const dim3 g(B), blk(256);
  if (A <= 8)
    hipLaunchKernelGGL(exact_heads_kernel<8>, g, blk, 0, s, hp, ld, hv, ld, K, wp, A, wv, bp, bv,
                       logp, pi, v);
  else if (A <= 16)
    hipLaunchKernelGGL(exact_heads_kernel<16>, g, blk, 0, s, hp, ld, hv, ld, K, wp, A, wv, bp, bv,
                       logp, pi, v);
  else
    hipLaunchKernelGGL(exact_heads_kernel<32>, g, blk, 0, s, hp, ld, hv, ld, K, wp, A, wv, bp, bv,
                       logp, pi, v);
  return check_launch("exact_heads_kernel");
}

enum ExactTrunk { EX_NONE, EX_C4_7, EX_C4N, EX_C4R, EX_TTT };

static ExactTrunk exact_trunk(int game, int nx, int ny) {
  if (game == AZ_EXACT_TTT) return nx == ny && nx >= 3 && nx <= 5 ? EX_TTT : EX_NONE;
  if (game != AZ_EXACT_C4) return EX_NONE;
  if (nx == 7 && ny == 7) return EX_C4_7;
  if (nx == ny && (nx == 4 || nx == 5 || nx == 6 || nx == 8)) return EX_C4N;
  if ((nx == 7 && ny == 6) || (nx == 6 && ny == 5) || (nx == 5 && ny == 4) || (nx == 8 && ny == 7))
    return EX_C4R;
  return EX_NONE;
}

static int exact_features(int game, int nx, int ny) {
  return game == AZ_EXACT_TTT ? 128 * (nx - 2) * (ny - 2) : 64 * nx * ny;
}

static size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

}  // namespace az

using namespace az;

extern "C" int az_gemm_exact_plan(int N, int K, int* segments, int* seg_len) {
  AZ_REQUIRE(N >= 4 && N % 4 == 0 && K >= 4 && K % 4 == 0, AZ_EINVAL,
             "az_gemm_exact_plan: bad shape N=%d K=%d (N %% 4 == 0, K %% 4 == 0)", N, K);
  AZ_REQUIRE(segments && seg_len, AZ_EINVAL, "az_gemm_exact_plan: null pointer");
  const ExactPlan pl = exact_plan(N, K);
  *segments = pl.S;
  for (int s = 0; s < pl.S; ++s) seg_len[s] = std::min(pl.L, K - s * pl.L);
  return AZ_OK;
}

extern "C" size_t az_gemm_exact_ws_bytes(int M, int N, int K) {
  if (M < 1 || N < 4 || N % 4 || K < 4 || K % 4) return 0;
  return exact_ws_bytes(M, N, K);
}

extern "C" int az_gemm_exact_f32(const float* A, int lda, const float* W, int ldw,
                                 const float* bias, int act, float* C, int ldc, int M, int N,
                                 int K, void* ws, size_t ws_bytes, void* stream) {
  AZ_REQUIRE(M >= 0 && N >= 4 && N % 4 == 0 && K >= 4 && K % 4 == 0, AZ_EINVAL,
             "az_gemm_exact_f32: bad shape M=%d N=%d K=%d (N %% 4 == 0, K %% 4 == 0)", M, N, K);
  AZ_REQUIRE(act == AZ_ACT_NONE || act == AZ_ACT_RELU, AZ_EINVAL,
             "az_gemm_exact_f32: act=%d (AZ_ACT_NONE or AZ_ACT_RELU)", act);
  if (M == 0) return AZ_OK;
  AZ_REQUIRE(A && W && C, AZ_EINVAL, "az_gemm_exact_f32: null pointer");
  AZ_REQUIRE(lda >= K && ldw >= K && ldc >= N && lda % 4 == 0 && ldw % 4 == 0 && ldc % 4 == 0,
             AZ_EINVAL, "az_gemm_exact_f32: leading dimensions lda=%d ldw=%d ldc=%d (>= K, K, N; "
             "%% 4 == 0)", lda, ldw, ldc);
  AZ_REQUIRE(aligned16(A) && aligned16(W) && aligned16(C) && aligned16(bias), AZ_EINVAL,
             "az_gemm_exact_f32: A, W, bias and C need 16B alignment");
  return gemm_exact(A, lda, W, ldw, bias, act, C, ldc, M, N, K, ws, ws_bytes, as_stream(stream));
}

extern "C" size_t az_eval_exact_ws_bytes(int max_B, int game, int nx, int ny, int A) {
  if (max_B < 1 || A < 1 || A > 32 || exact_trunk(game, nx, ny) == EX_NONE) return 0;
  const int F = exact_features(game, nx, ny);
  size_t b = exact_ws_bytes_upto(max_B, F, F);                        // output_transform.0 / .2
  if (game == AZ_EXACT_TTT) b = std::max(b, exact_ws_bytes_upto(max_B, 512, F));   // fc1 / fc2
  return align256(b) + 256;
}

extern "C" int az_eval_exact_fwd(const az_eval_exact* e, const int8_t* boards, int B, float* pi,
                                 float* v, float* gpi, float* gv, void* stream) {
  AZ_REQUIRE(e != nullptr, AZ_EINVAL, "az_eval_exact_fwd: null descriptor");
  AZ_REQUIRE(B >= 0 && B <= e->max_B, AZ_EINVAL, "az_eval_exact_fwd: B=%d max_B=%d", B, e->max_B);
  if (B == 0) return AZ_OK;
  const ExactTrunk tk = exact_trunk(e->game, e->nx, e->ny);
  AZ_REQUIRE(tk != EX_NONE, AZ_EINVAL,
             "az_eval_exact_fwd: no fused trunk for game=%d board %dx%d (Connect4: 7x7, 4x4, 5x5, "
             "6x6, 8x8, 7x6, 6x5, 5x4, 8x7; TicTacToe: 3x3, 4x4, 5x5)", e->game, e->nx, e->ny);
  const int F = exact_features(e->game, e->nx, e->ny);
  AZ_REQUIRE(e->A >= 1 && e->A <= 32 && e->F == F, AZ_EINVAL,
             "az_eval_exact_fwd: bad shape A=%d F=%d (A <= 32, F = %d)", e->A, e->F, F);
  AZ_REQUIRE(v || gv, AZ_EINVAL, "az_eval_exact_fwd: neither v nor gv requested");
  const bool ttt = tk == EX_TTT;
  AZ_REQUIRE(boards && e->conv1_w && e->conv1_b && e->conv2_w && e->conv2_b && e->fc_policy_w &&
                 e->fc_policy_b && e->fc_value_w && e->fc_value_b &&
                 (!ttt || (e->conv3_w && e->conv3_b && e->fc1_w && e->fc1_b && e->fc2_w &&
                           e->fc2_b)),
             AZ_EINVAL, "az_eval_exact_fwd: null boards / weight pointer");
  AZ_REQUIRE(e->feat && (!v || e->logp) && (!ttt || (e->h1 && e->h2)), AZ_EINVAL,
             "az_eval_exact_fwd: null scratch (feat / logp / h1 / h2)");
  AZ_REQUIRE(!gv || (e->ot0_w && e->ot0_b && e->ot2_w && e->ot2_b && e->hidden && e->y &&
                     e->glogp),
             AZ_EINVAL, "az_eval_exact_fwd: null GNN tail weights / scratch");
  const size_t need = az_eval_exact_ws_bytes(e->max_B, e->game, e->nx, e->ny, e->A);
  AZ_REQUIRE(e->ws && e->ws_bytes >= need, AZ_EINVAL,
             "az_eval_exact_fwd: workspace too small (az_eval_exact_ws_bytes: %zu bytes)", need);
  AZ_REQUIRE(aligned16(e->feat) && aligned16(e->ws) && aligned16(e->conv2_w) &&
                 aligned16(e->fc_policy_w) && aligned16(e->fc_value_w) &&
                 (!ttt || (aligned16(e->h1) && aligned16(e->h2) && aligned16(e->fc1_w) &&
                           aligned16(e->fc2_w) && aligned16(e->fc1_b) && aligned16(e->fc2_b))) &&
                 (!gv || (aligned16(e->hidden) && aligned16(e->y) && aligned16(e->ot0_w) &&
                          aligned16(e->ot2_w) && aligned16(e->ot0_b) && aligned16(e->ot2_b))),
             AZ_EINVAL, "az_eval_exact_fwd: weights and scratch need 16B alignment");
  hipStream_t s = as_stream(stream);
  int rc;
  switch (tk) {
    case EX_C4_7:
      rc = az_c4_trunk_fwd(boards, B, e->conv1_w, e->conv1_b, e->conv2_w, e->conv2_b, e->feat,
                           stream);
      break;
    case EX_C4N:
      rc = az_c4n_trunk_fwd(boards, B, e->nx, e->conv1_w, e->conv1_b, e->conv2_w, e->conv2_b,
                            e->feat, stream);
      break;
    case EX_C4R:
      rc = az_c4r_trunk_fwd(boards, B, e->nx, e->ny, e->conv1_w, e->conv1_b, e->conv2_w,
                            e->conv2_b, e->feat, stream);
      break;
    default:
      rc = az_ttt_trunk_fwd(boards, B, e->nx, e->conv1_w, e->conv1_b, e->conv2_w, e->conv2_b,
                            e->conv3_w, e->conv3_b, e->feat, stream);
  }
  if (rc) return rc;
  auto linear = [&](const float* x, int K, const float* w, const float* b, int act, float* out,
                    int N) {
    return gemm_exact(x, K, w, K, b, act, out, N, B, N, K, e->ws, e->ws_bytes, s);
  };
  // the policy / value heads of rows x: Connect4 reads x itself, TicTacToe relu(fc1 x), relu(fc2 x)
  auto heads = [&](const float* x, float* logp, float* p, float* val) {
    if (!ttt)
      return exact_heads(x, x, F, B, F, e->fc_policy_w, e->fc_policy_b, e->A, e->fc_value_w,
                         e->fc_value_b, logp, p, val, s);
    int r = linear(x, F, e->fc1_w, e->fc1_b, AZ_ACT_RELU, e->h1, 512);
    if (!r) r = linear(x, F, e->fc2_w, e->fc2_b, AZ_ACT_RELU, e->h2, 512);
    if (r) return r;
    return exact_heads(e->h1, e->h2, 512, B, 512, e->fc_policy_w, e->fc_policy_b, e->A,
                       e->fc_value_w, e->fc_value_b, logp, p, val, s);
  };
  if (v && (rc = heads(e->feat, e->logp, pi, v))) return rc;
  if (!gv) return AZ_OK;
  if ((rc = linear(e->feat, F, e->ot0_w, e->ot0_b, AZ_ACT_RELU, e->hidden, F))) return rc;
  if ((rc = linear(e->hidden, F, e->ot2_w, e->ot2_b, AZ_ACT_NONE, e->y, F))) return rc;
  return heads(e->y, e->glogp, gpi, gv);
}
