// Connect4Net evaluation on boards other than 7x7 (connect4/Connect4Net.py:42-60,
// Connect4GNN.py:31-57 with --board_size 4, 5, 6 or 8): conv1 and conv2 fused into one launch
// that can also form the policy/value heads from its LDS feature tile, and az_c4n_eval_fwd, the
// one-call evaluator on top of it.  The 7x7 board keeps its MFMA trunk (az_trunk.hip).
#include "az_common.h"
#include "az_conv_chain.h"
#include "az_heads.h"

namespace az {

constexpr int C4N_THREADS = 1024;

// conv1 (1 -> 32, pad 1) -> conv2 (32 -> 64, pad 1), ReLU after each, for ONE board per
// workgroup: the board, conv1's plane (position-major [N^2][36], what conv_chain<32> reads) and
// conv2's output (NCHW [64][N^2], the feature row) stay in LDS: (1 + 36 + 64) N^2 floats, 6.3 /
// 9.9 / 14.2 / 25.3 KB at N = 4 / 5 / 6 / 8, plus the heads' chunk partials.  One thread per
// output, each the fmaf chain of conv3x3_relu_kernel (conv_chain), so feat has the bits of two
// az_conv3x3_relu_fwd calls.  The row leaves as float4 stores when feat != NULL.
// AMAX > 0: the same block then runs the heads on the LDS row -- wave w forms the partials of
// chunks w, w + 16, ... (heads_chunk_part: heads_row_block's per-chunk arithmetic) and
// heads_finalize_row sums them in chunk order: az_heads_fwd's bits.  F = 64 N^2 is 4 / 6.25 / 9 /
// 16 chunks of 256 columns (N = 5: the last one partial).
template <int N, int AMAX>
__global__ __launch_bounds__(C4N_THREADS) void c4n_trunk_heads_kernel(
    const int8_t* __restrict__ boards, const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ feat,
    const float* __restrict__ wp, const float* __restrict__ bp, int A,
    const float* __restrict__ wv, const float* __restrict__ bv, float* __restrict__ logp,
    float* __restrict__ pi, float* __restrict__ v) {
  constexpr int HW = N * N, F = 64 * HW;
  constexpr int NCH = (F + HEADS_KC - 1) / HEADS_KC;
  __shared__ float bd[HW];
  __shared__ __attribute__((aligned(16))) float p1[HW * 36];
  __shared__ __attribute__((aligned(16))) float tile[F];
  __shared__ float part[AMAX > 0 ? NCH * (AMAX + 1) : 1];
  __shared__ float sm[AMAX + 1];
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  if (tid < HW) bd[tid] = (float)boards[b * HW + tid];
  __syncthreads();
  for (int idx = tid; idx < 32 * HW; idx += C4N_THREADS) {
    const int co = idx / HW, pos = idx % HW;
    const float s = conv_chain<1, N, N, 1, false>(w1 + co * 9, bd, pos / N, pos % N) + b1[co];
    p1[pos * 36 + co] = s > 0.f ? s : 0.f;
  }
  __syncthreads();
  for (int idx = tid; idx < F; idx += C4N_THREADS) {
    const int co = idx / HW, pos = idx % HW;
    const float s = conv_chain<32, N, N, 1, true>(w2 + co * 32 * 9, p1, pos / N, pos % N) + b2[co];
    tile[idx] = s > 0.f ? s : 0.f;
  }
  __syncthreads();
  if (feat) {
    f32x4* dst = reinterpret_cast<f32x4*>(feat + b * F);
    for (int i = tid; i < F / 4; i += C4N_THREADS)
      dst[i] = *reinterpret_cast<const f32x4*>(tile + i * 4);
  }
  if constexpr (AMAX > 0) {
    for (int c = tid >> 6; c < NCH; c += C4N_THREADS / 64)
      heads_chunk_part<AMAX>(tile, tile, F, wp, A, wv, c, part + c * (AMAX + 1));
    __syncthreads();
    heads_finalize_row<AMAX>(part, NCH, A, bp, bv, (int)b, logp, pi, v, sm);
  }
}

struct C4nHeads {
  const float* wp; const float* bp; int A; const float* wv; const float* bv;
  float* logp; float* pi; float* v;
};

template <int N>
static void launch_c4n(const int8_t* boards, int B, const float* w1, const float* b1,
                       const float* w2, const float* b2, float* feat, const C4nHeads* h,
                       hipStream_t s) {
  const dim3 g(B), blk(C4N_THREADS);
  if (!h)
    hipLaunchKernelGGL((c4n_trunk_heads_kernel<N, 0>), g, blk, 0, s, boards, w1, b1, w2, b2, feat,
                       nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
  else if (h->A <= 8)     // AMAX by A, as az_heads_fwd picks it
    hipLaunchKernelGGL((c4n_trunk_heads_kernel<N, 8>), g, blk, 0, s, boards, w1, b1, w2, b2, feat,
                       h->wp, h->bp, h->A, h->wv, h->bv, h->logp, h->pi, h->v);
  else if (h->A <= 16)
    hipLaunchKernelGGL((c4n_trunk_heads_kernel<N, 16>), g, blk, 0, s, boards, w1, b1, w2, b2, feat,
                       h->wp, h->bp, h->A, h->wv, h->bv, h->logp, h->pi, h->v);
  else
    hipLaunchKernelGGL((c4n_trunk_heads_kernel<N, 32>), g, blk, 0, s, boards, w1, b1, w2, b2, feat,
                       h->wp, h->bp, h->A, h->wv, h->bv, h->logp, h->pi, h->v);
}

static bool c4n_side(int n) { return n == 4 || n == 5 || n == 6 || n == 8; }

// The checked launch behind the three entry points (h == NULL: the trunk alone).
static int c4n_launch(const int8_t* boards, int B, int n, const float* w1, const float* b1,
                      const float* w2, const float* b2, float* feat, const C4nHeads* h,
                      hipStream_t s) {
  switch (n) {
    case 4: launch_c4n<4>(boards, B, w1, b1, w2, b2, feat, h, s); break;
    case 5: launch_c4n<5>(boards, B, w1, b1, w2, b2, feat, h, s); break;
    case 6: launch_c4n<6>(boards, B, w1, b1, w2, b2, feat, h, s); break;
    default: launch_c4n<8>(boards, B, w1, b1, w2, b2, feat, h, s); break;
  }
  return check_launch("c4n_trunk_heads_kernel");
}

}  // namespace az

using namespace az;

extern "C" int az_c4n_trunk_fwd(const int8_t* boards, int B, int n, const float* conv1_w,
                                const float* conv1_b, const float* conv2_w, const float* conv2_b,
                                float* feat, void* stream) {
  AZ_REQUIRE(B >= 0 && c4n_side(n), AZ_EINVAL,
             "az_c4n_trunk_fwd: bad shape B=%d n=%d (n in {4, 5, 6, 8}; 7 is az_c4_trunk_fwd)", B,
             n);
  if (B == 0) return AZ_OK;
  AZ_REQUIRE(boards && conv1_w && conv1_b && conv2_w && conv2_b && feat, AZ_EINVAL,
             "az_c4n_trunk_fwd: null pointer");
  AZ_REQUIRE(aligned16(conv2_w) && aligned16(feat), AZ_EINVAL,
             "az_c4n_trunk_fwd: conv2_w and feat need 16B alignment");
  return c4n_launch(boards, B, n, conv1_w, conv1_b, conv2_w, conv2_b, feat, nullptr,
                    as_stream(stream));
}

extern "C" int az_c4n_trunk_heads_fwd(const int8_t* boards, int B, int n, const float* conv1_w,
                                      const float* conv1_b, const float* conv2_w,
                                      const float* conv2_b, const float* wp, const float* bp,
                                      int A, const float* wv, const float* bv, float* feat,
                                      float* logp, float* pi, float* v, void* stream) {
  AZ_REQUIRE(B >= 0 && c4n_side(n) && A >= 1 && A <= 32, AZ_EINVAL,
             "az_c4n_trunk_heads_fwd: bad shape B=%d n=%d A=%d (n in {4, 5, 6, 8}, A <= 32)", B,
             n, A);
  if (B == 0) return AZ_OK;
  AZ_REQUIRE(boards && conv1_w && conv1_b && conv2_w && conv2_b && wp && bp && wv && bv && logp &&
                 v,
             AZ_EINVAL, "az_c4n_trunk_heads_fwd: null pointer");
  AZ_REQUIRE(aligned16(conv2_w) && aligned16(feat) && aligned16(wp) && aligned16(wv), AZ_EINVAL,
             "az_c4n_trunk_heads_fwd: conv2_w, feat, wp and wv need 16B alignment");
  const C4nHeads h{wp, bp, A, wv, bv, logp, pi, v};
  return c4n_launch(boards, B, n, conv1_w, conv1_b, conv2_w, conv2_b, feat, &h,
                    as_stream(stream));
}

extern "C" size_t az_c4n_eval_ws_bytes(int max_B, int n, int A) {
  if (max_B < 1 || !c4n_side(n) || A < 1 || A > 32) return 0;
  return az_transform_heads_ws_bytes(max_B, 64 * n * n, A);
}

extern "C" int az_c4n_eval_fwd(const az_c4n_eval* e, const int8_t* boards, int B, float* pi,
                               float* v, float* gpi, float* gv, void* stream) {
  AZ_REQUIRE(e != nullptr, AZ_EINVAL, "az_c4n_eval_fwd: null descriptor");
  AZ_REQUIRE(B >= 1 && B <= e->max_B, AZ_EINVAL, "az_c4n_eval_fwd: B=%d max_B=%d", B, e->max_B);
  AZ_REQUIRE(e->n != 7, AZ_EINVAL,
             "az_c4n_eval_fwd: n=7 is az_c4_eval_fwd's board (this evaluator: n in {4, 5, 6, 8})");
  AZ_REQUIRE(c4n_side(e->n) && e->A >= 1 && e->A <= 32 && e->F == 64 * e->n * e->n, AZ_EINVAL,
             "az_c4n_eval_fwd: bad shape n=%d A=%d F=%d (n in {4, 5, 6, 8}, A <= 32, F = 64 n^2)",
             e->n, e->A, e->F);
  AZ_REQUIRE(v || gv, AZ_EINVAL, "az_c4n_eval_fwd: neither v nor gv requested");
  AZ_REQUIRE(boards && e->conv1_w && e->conv1_b && e->conv2_w && e->conv2_b && e->fc_policy_w &&
                 e->fc_policy_b && e->fc_value_w && e->fc_value_b,
             AZ_EINVAL, "az_c4n_eval_fwd: null boards / weight pointer");
  AZ_REQUIRE(e->feat && (!v || e->logp), AZ_EINVAL, "az_c4n_eval_fwd: null scratch (feat / logp)");
  AZ_REQUIRE(!gv || (e->ot0_w && e->ot0_b && e->ot2_w && e->ot2_b && e->hidden && e->glogp &&
                     e->ws),
             AZ_EINVAL, "az_c4n_eval_fwd: GNN tail requested without its weights / scratch");
  AZ_REQUIRE(aligned16(e->conv2_w) && aligned16(e->feat) && aligned16(e->fc_policy_w) &&
                 aligned16(e->fc_value_w) &&
                 (!gv || (aligned16(e->hidden) && aligned16(e->ws) && aligned16(e->ot0_w) &&
                          aligned16(e->ot2_w))),
             AZ_EINVAL, "az_c4n_eval_fwd: weights and scratch need 16B alignment");
  AZ_REQUIRE(!gv || e->ws_bytes >= az_c4n_eval_ws_bytes(e->max_B, e->n, e->A), AZ_EINVAL,
             "az_c4n_eval_fwd: workspace too small (az_c4n_eval_ws_bytes)");
  // the fused launch: the feature rows leave for the GNN tail only, the standard heads come
  // from the LDS tile
  const C4nHeads h{e->fc_policy_w, e->fc_policy_b, e->A, e->fc_value_w, e->fc_value_b, e->logp,
                   pi, v};
  int rc = c4n_launch(boards, B, e->n, e->conv1_w, e->conv1_b, e->conv2_w, e->conv2_b,
                      gv ? e->feat : nullptr, v ? &h : nullptr, as_stream(stream));
  if (rc || !gv) return rc;
  // output_transform + heads on feat: up to 8 rows both layers are whole-K / chunked GEMVs whose
  // lane-strided chain does not depend on the number of rows, and the heads run one block per
  // row, so a row has the bits of the same board evaluated alone
  return az_transform_heads_fwd(e->feat, B, e->F, e->ot0_w, e->ot0_b, e->ot2_w, e->ot2_b,
                                e->fc_policy_w, e->fc_policy_b, e->A, e->fc_value_w,
                                e->fc_value_b, e->hidden, nullptr, e->glogp, gpi, gv, e->ws,
                                e->ws_bytes, stream);
}
