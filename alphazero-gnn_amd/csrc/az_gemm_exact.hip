// Batch-invariant evaluation: the exact-fp32 GEMM with its plain epilogue (bias, ReLU) and the
// one-call evaluator built on it (az_gemm_exact_f32, az_eval_exact_fwd).  The kernel
// templates, the plan and the arithmetic contract are in az_gemm_exact.h; this unit instantiates
// gemm_exact_kernel<1|2|4, ExactEpiPlain> and gemm_exact_reduce_kernel<ExactEpiPlain>.
#include "az_gemm_exact.h"
#include "az_heads.h"

namespace az {

int gemm_exact(const float* A, int lda, const float* W, int ldw, const float* bias, int act,
               float* C, int ldc, int M, int N, int K, void* ws, size_t ws_bytes, hipStream_t s) {
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
  AZ_REQUIRE((M + 32 * exact_waves(M) - 1) / (32 * exact_waves(M)) <= 65535, AZ_EINVAL,
             "az_gemm_exact_f32: M=%d too large", M);
  return exact_launch<ExactEpiPlain>(a, 1, spread, s);
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

bool exact_has_trunk(int game, int nx, int ny) { return exact_trunk(game, nx, ny) != EX_NONE; }

int exact_features(int game, int nx, int ny) {
  return game == AZ_EXACT_TTT ? 128 * (nx - 2) * (ny - 2) : 64 * nx * ny;
}


static size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

size_t exact_eval_tail_ws_bytes(int max_B, int game, int nx, int ny) {
  const int F = exact_features(game, nx, ny);
  size_t b = exact_ws_bytes_upto(max_B, F, F);                        // output_transform.0 / .2
  if (game == AZ_EXACT_TTT) b = std::max(b, exact_ws_bytes_upto(max_B, 512, F));   // fc1 / fc2
  return align256(b) + 256;
}

int exact_eval_check(const az_eval_exact* e, const char* who, bool std_heads, bool gnn_tail) {
  const ExactTrunk tk = exact_trunk(e->game, e->nx, e->ny);
  AZ_REQUIRE(tk != EX_NONE, AZ_EINVAL,
             "%s: no fused trunk for game=%d board %dx%d (Connect4: 7x7, 4x4, 5x5, "
             "6x6, 8x8, 7x6, 6x5, 5x4, 8x7; TicTacToe: 3x3, 4x4, 5x5)", who, e->game, e->nx, e->ny);
  const int F = exact_features(e->game, e->nx, e->ny);
  AZ_REQUIRE(e->A >= 1 && e->A <= 32 && e->F == F, AZ_EINVAL,
             "%s: bad shape A=%d F=%d (A <= 32, F = %d)", who, e->A, e->F, F);
  const bool ttt = tk == EX_TTT;
  AZ_REQUIRE(e->conv1_w && e->conv1_b && e->conv2_w && e->conv2_b && e->fc_policy_w &&
                 e->fc_policy_b && e->fc_value_w && e->fc_value_b &&
                 (!ttt || (e->conv3_w && e->conv3_b && e->fc1_w && e->fc1_b && e->fc2_w &&
                           e->fc2_b)),
             AZ_EINVAL, "%s: null boards / weight pointer", who);
  AZ_REQUIRE(e->feat && (!std_heads || e->logp) && (!ttt || (e->h1 && e->h2)), AZ_EINVAL,
             "%s: null scratch (feat / logp / h1 / h2)", who);
  AZ_REQUIRE(!gnn_tail || (e->ot0_w && e->ot0_b && e->ot2_w && e->ot2_b && e->hidden && e->y &&
                           e->glogp),
             AZ_EINVAL, "%s: null GNN tail weights / scratch", who);
  AZ_REQUIRE(aligned16(e->feat) && aligned16(e->conv2_w) &&
                 aligned16(e->fc_policy_w) && aligned16(e->fc_value_w) &&
                 (!ttt || (aligned16(e->h1) && aligned16(e->h2) && aligned16(e->fc1_w) &&
                           aligned16(e->fc2_w) && aligned16(e->fc1_b) && aligned16(e->fc2_b))) &&
                 (!gnn_tail || (aligned16(e->hidden) && aligned16(e->y) && aligned16(e->ot0_w) &&
                                aligned16(e->ot2_w) && aligned16(e->ot0_b) && aligned16(e->ot2_b))),
             AZ_EINVAL, "%s: weights and scratch need 16B alignment", who);
  return AZ_OK;
}

int exact_eval_trunk(const az_eval_exact* e, const int8_t* boards, int B, float* feat,
                     void* stream) {
  switch (exact_trunk(e->game, e->nx, e->ny)) {
    case EX_C4_7:
      return az_c4_trunk_fwd(boards, B, e->conv1_w, e->conv1_b, e->conv2_w, e->conv2_b, feat,
                             stream);
    case EX_C4N:
      return az_c4n_trunk_fwd(boards, B, e->nx, e->conv1_w, e->conv1_b, e->conv2_w, e->conv2_b,
                              feat, stream);
    case EX_C4R:
      return az_c4r_trunk_fwd(boards, B, e->nx, e->ny, e->conv1_w, e->conv1_b, e->conv2_w,
                              e->conv2_b, feat, stream);
    default:
      return az_ttt_trunk_fwd(boards, B, e->nx, e->conv1_w, e->conv1_b, e->conv2_w, e->conv2_b,
                              e->conv3_w, e->conv3_b, feat, stream);
  }
}

int exact_eval_tail(const az_eval_exact* e, const float* xs, const float* xg, int B, float* pi,
                    float* v, float* gpi, float* gv, void* ws, size_t ws_bytes, hipStream_t s) {
  const bool ttt = e->game == AZ_EXACT_TTT;
  const int F = e->F;
  int rc;
  auto linear = [&](const float* x, int K, const float* w, const float* b, int act, float* out,
                    int N) {
    return gemm_exact(x, K, w, K, b, act, out, N, B, N, K, ws, ws_bytes, s);
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
  if (v && (rc = heads(xs, e->logp, pi, v))) return rc;
  if (!gv) return AZ_OK;
  if ((rc = linear(xg, F, e->ot0_w, e->ot0_b, AZ_ACT_RELU, e->hidden, F))) return rc;
  if ((rc = linear(e->hidden, F, e->ot2_w, e->ot2_b, AZ_ACT_NONE, e->y, F))) return rc;
  return heads(e->y, e->glogp, gpi, gv);
}

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
  return exact_eval_tail_ws_bytes(max_B, game, nx, ny);
}

extern "C" int az_eval_exact_fwd(const az_eval_exact* e, const int8_t* boards, int B, float* pi,
                                 float* v, float* gpi, float* gv, void* stream) {
  AZ_REQUIRE(e != nullptr, AZ_EINVAL, "az_eval_exact_fwd: null descriptor");
  AZ_REQUIRE(B >= 0 && B <= e->max_B, AZ_EINVAL, "az_eval_exact_fwd: B=%d max_B=%d", B, e->max_B);
  if (B == 0) return AZ_OK;
  AZ_REQUIRE(v || gv, AZ_EINVAL, "az_eval_exact_fwd: neither v nor gv requested");
  AZ_REQUIRE(boards, AZ_EINVAL, "az_eval_exact_fwd: null boards / weight pointer");
  int rc = exact_eval_check(e, "az_eval_exact_fwd", v != nullptr, gv != nullptr);
  if (rc) return rc;
  const size_t need = az_eval_exact_ws_bytes(e->max_B, e->game, e->nx, e->ny, e->A);
  AZ_REQUIRE(e->ws && aligned16(e->ws) && e->ws_bytes >= need, AZ_EINVAL,
             "az_eval_exact_fwd: workspace too small (az_eval_exact_ws_bytes: %zu bytes)", need);
  if ((rc = exact_eval_trunk(e, boards, B, e->feat, stream))) return rc;
  return exact_eval_tail(e, e->feat, e->feat, B, pi, v, gpi, gv, e->ws, e->ws_bytes,
                         as_stream(stream));
}
