// TicTacToeNet evaluation (tictactoe/TicTacToeNet.py:28-48, TicTacToeGNN.py:25-45): the three
// conv layers fused into one launch, and az_ttt_eval_fwd, the one-call evaluator on top of it
// (the paired head-input GEMVs are gemv_multi in az_gemm.hip).
#include <algorithm>

#include "az_common.h"
#include "az_conv_chain.h"
#include "az_gemm.h"

namespace az {

constexpr int TTT_THREADS = 1024;

// conv1 (1 -> 32, pad 1) -> conv2 (32 -> 64, pad 1) -> conv3 (64 -> 128, no pad), ReLU after each,
// for ONE board per workgroup: the board and both intermediate planes stay in LDS
// ((1 + 36 + 68) N^2 floats: 3.8 / 6.7 / 10.5 KB at N = 3 / 4 / 5).  One thread per output; the
// chain of an output is serial (864 dependent fmaf through conv2 and conv3), so the 16 waves are
// there to cover whole layers in one or two rounds (conv2 has 576 / 1,024 / 1,600 outputs, conv3
// 128 / 512 / 1,152) and to hide each other's LDS latency.  feat [B][128 (N-2)^2] is the NCHW
// flatten.
template <int N, bool VEC>
__global__ __launch_bounds__(TTT_THREADS) void ttt_trunk_kernel(
    const int8_t* __restrict__ boards, const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ w3,
    const float* __restrict__ b3, float* __restrict__ feat) {
  constexpr int HW = N * N, M = N - 2, HW3 = M * M;
  __shared__ float bd[HW];
  __shared__ __attribute__((aligned(16))) float p1[HW * 36];
  __shared__ __attribute__((aligned(16))) float p2[HW * 68];
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  if (tid < HW) bd[tid] = (float)boards[b * HW + tid];
  __syncthreads();
  for (int idx = tid; idx < 32 * HW; idx += TTT_THREADS) {
    const int co = idx / HW, pos = idx % HW;
    const float s = conv_chain<1, N, N, 1, false>(w1 + co * 9, bd, pos / N, pos % N) + b1[co];
    p1[pos * 36 + co] = s > 0.f ? s : 0.f;
  }
  __syncthreads();
  for (int idx = tid; idx < 64 * HW; idx += TTT_THREADS) {
    const int co = idx / HW, pos = idx % HW;
    const float s = conv_chain<32, N, N, 1, VEC>(w2 + co * 32 * 9, p1, pos / N, pos % N) + b2[co];
    p2[pos * 68 + co] = s > 0.f ? s : 0.f;
  }
  __syncthreads();
  for (int idx = tid; idx < 128 * HW3; idx += TTT_THREADS) {
    const int co = idx / HW3, pos = idx % HW3;
    const float s = conv_chain<64, N, N, 0, VEC>(w3 + co * 64 * 9, p2, pos / M, pos % M) + b3[co];
    feat[b * (128 * HW3) + idx] = s > 0.f ? s : 0.f;
  }
}

template <int N>
static void launch_ttt_trunk(const int8_t* boards, int B, const float* w1, const float* b1,
                             const float* w2, const float* b2, const float* w3, const float* b3,
                             float* feat, hipStream_t s) {
  if (aligned16(w2) && aligned16(w3))
    hipLaunchKernelGGL((ttt_trunk_kernel<N, true>), dim3(B), dim3(TTT_THREADS), 0, s, boards, w1,
                       b1, w2, b2, w3, b3, feat);
  else
    hipLaunchKernelGGL((ttt_trunk_kernel<N, false>), dim3(B), dim3(TTT_THREADS), 0, s, boards, w1,
                       b1, w2, b2, w3, b3, feat);
}

static size_t align256(size_t b) { return (b + 255) & ~size_t(255); }
}  // namespace az

using namespace az;

extern "C" int az_ttt_trunk_fwd(const int8_t* boards, int B, int n, const float* conv1_w,
                                const float* conv1_b, const float* conv2_w, const float* conv2_b,
                                const float* conv3_w, const float* conv3_b, float* feat,
                                void* stream) {
  AZ_REQUIRE(B >= 0 && n >= 3 && n <= 5, AZ_EINVAL, "az_ttt_trunk_fwd: bad shape B=%d n=%d", B, n);
  if (B == 0) return AZ_OK;
  AZ_REQUIRE(boards && conv1_w && conv1_b && conv2_w && conv2_b && conv3_w && conv3_b && feat,
             AZ_EINVAL, "az_ttt_trunk_fwd: null pointer");
  hipStream_t s = as_stream(stream);
  if (n == 3)
    launch_ttt_trunk<3>(boards, B, conv1_w, conv1_b, conv2_w, conv2_b, conv3_w, conv3_b, feat, s);
  else if (n == 4)
    launch_ttt_trunk<4>(boards, B, conv1_w, conv1_b, conv2_w, conv2_b, conv3_w, conv3_b, feat, s);
  else
    launch_ttt_trunk<5>(boards, B, conv1_w, conv1_b, conv2_w, conv2_b, conv3_w, conv3_b, feat, s);
  return check_launch("ttt_trunk_kernel");
}

extern "C" size_t az_ttt_eval_ws_bytes(int max_B, int n, int A) {
  if (max_B < 1 || n < 3 || n > 5 || A < 1 || A > 32) return 0;
  const size_t heads = align256(az_heads_ws_bytes(max_B, 512, A)) + 256;
  if (max_B <= 8) return heads;   // the GEMVs take no workspace
  // above 8 rows every linear layer is az_gemm_f32 with the rest of the workspace: room for the
  // most split-K slabs any of its plans asks for (16) of the widest output, A's fp16 planes and
  // the row scales of the fp16 form, so each plan is the one a large workspace gets
  const size_t F = (size_t)128 * (n - 2) * (n - 2), W = std::max<size_t>(F, 512);
  return heads + (size_t)16 * max_B * W * 4 + align256((size_t)4 * max_B * W) +
         align256((size_t)8 * (max_B + W)) + (2u << 20);
}

extern "C" int az_ttt_eval_fwd(const az_ttt_eval* e, const int8_t* boards, int B, float* pi,
                               float* v, float* gpi, float* gv, void* stream) {
  AZ_REQUIRE(e != nullptr, AZ_EINVAL, "az_ttt_eval_fwd: null descriptor");
  AZ_REQUIRE(B >= 1 && B <= e->max_B, AZ_EINVAL, "az_ttt_eval_fwd: B=%d max_B=%d", B, e->max_B);
  AZ_REQUIRE(e->n >= 3 && e->n <= 5 && e->A >= 1 && e->A <= 32 &&
                 e->F == 128 * (e->n - 2) * (e->n - 2),
             AZ_EINVAL, "az_ttt_eval_fwd: bad shape n=%d A=%d F=%d (n in 3..5, A <= 32, "
             "F = 128 (n-2)^2)", e->n, e->A, e->F);
  AZ_REQUIRE(v || gv, AZ_EINVAL, "az_ttt_eval_fwd: neither v nor gv requested");
  AZ_REQUIRE(boards && e->conv1_w && e->conv1_b && e->conv2_w && e->conv2_b && e->conv3_w &&
                 e->conv3_b && e->fc1_w && e->fc1_b && e->fc2_w && e->fc2_b && e->fc_policy_w &&
                 e->fc_policy_b && e->fc_value_w && e->fc_value_b,
             AZ_EINVAL, "az_ttt_eval_fwd: null boards / weight pointer");
  AZ_REQUIRE(e->feat && e->h1 && e->h2 && e->ws && (!v || e->logp), AZ_EINVAL,
             "az_ttt_eval_fwd: null scratch (feat / h1 / h2 / logp / ws)");
  AZ_REQUIRE(!gv || (e->ot0_w && e->ot0_b && e->ot2_w && e->ot2_b && e->hidden && e->y &&
                     e->glogp),
             AZ_EINVAL, "az_ttt_eval_fwd: GNN tail requested without its weights / scratch");
  AZ_REQUIRE(aligned16(e->feat) && aligned16(e->h1) && aligned16(e->h2) && aligned16(e->ws) &&
                 aligned16(e->fc1_w) && aligned16(e->fc2_w) && aligned16(e->fc_policy_w) &&
                 aligned16(e->fc_value_w) &&
                 (!gv || (aligned16(e->hidden) && aligned16(e->y) && aligned16(e->ot0_w) &&
                          aligned16(e->ot2_w))),
             AZ_EINVAL, "az_ttt_eval_fwd: weights and scratch need 16B alignment");
  AZ_REQUIRE(e->ws_bytes >= az_ttt_eval_ws_bytes(e->max_B, e->n, e->A), AZ_EINVAL,
             "az_ttt_eval_fwd: workspace too small (az_ttt_eval_ws_bytes)");
  const int F = e->F, H = 512;
  hipStream_t s = as_stream(stream);
  int rc = az_ttt_trunk_fwd(boards, B, e->n, e->conv1_w, e->conv1_b, e->conv2_w, e->conv2_b,
                            e->conv3_w, e->conv3_b, e->feat, stream);
  if (rc) return rc;
  const size_t heads_bytes = align256(az_heads_ws_bytes(e->max_B, H, e->A)) + 256;
  char* const gws = static_cast<char*>(e->ws) + heads_bytes;
  const size_t gws_bytes = e->ws_bytes - heads_bytes;
  auto linear = [&](const float* x, const float* w, const float* b, int act, float* out, int N) {
    az_gemm_desc d = {};
    d.M = B; d.N = N; d.K = F;
    d.A = x; d.lda = F; d.a_kmajor = 1;
    d.B = w; d.ldb = F; d.b_kmajor = 1; d.bias = b; d.act = act;
    d.C = out; d.ldc = N;
    if (gws_bytes >= 256) { d.ws = gws; d.ws_bytes = gws_bytes; }
    return d;
  };
  // fc1 / fc2 of rows x (and output_transform.0 when `ot` is set): one launch at <= 8 rows
  auto hidden_layers = [&](const float* x, bool ot) {
    const az_gemm_desc d1 = linear(x, e->fc1_w, e->fc1_b, AZ_ACT_RELU, e->h1, H);
    const az_gemm_desc d2 = linear(x, e->fc2_w, e->fc2_b, AZ_ACT_RELU, e->h2, H);
    const az_gemm_desc d0 = linear(x, e->ot0_w, e->ot0_b, AZ_ACT_RELU, e->hidden, F);
    if (B <= 8) {
      const int r = gemv_multi_fwd(&d1, &d2, ot ? &d0 : nullptr, s);
      if (r) return r < 0 ? r : AZ_OK;
    }
    int r = gemm_f32(&d1, s);
    if (!r) r = gemm_f32(&d2, s);
    if (!r && ot) r = gemm_f32(&d0, s);
    return r;
  };
  auto heads = [&](float* logp, float* p, float* val) {
    return az_heads_fwd(e->h1, H, e->h2, H, B, H, e->fc_policy_w, e->fc_policy_b, e->A,
                        e->fc_value_w, e->fc_value_b, logp, p, val, e->ws, heads_bytes, stream);
  };
  if (v) {
    if ((rc = hidden_layers(e->feat, gv != nullptr))) return rc;
    if ((rc = heads(e->logp, pi, v))) return rc;
  }
  if (!gv) return AZ_OK;
  if (!v) {
    const az_gemm_desc d0 = linear(e->feat, e->ot0_w, e->ot0_b, AZ_ACT_RELU, e->hidden, F);
    if ((rc = gemm_f32(&d0, s))) return rc;
  }
  const az_gemm_desc dy = linear(e->hidden, e->ot2_w, e->ot2_b, AZ_ACT_NONE, e->y, F);
  if ((rc = gemm_f32(&dy, s))) return rc;
  // the GNN heads' fc1 / fc2 reuse h1 / h2: the stream orders them after the standard heads
  if ((rc = hidden_layers(e->y, false))) return rc;
  return heads(e->glogp, gpi, gv);
}
