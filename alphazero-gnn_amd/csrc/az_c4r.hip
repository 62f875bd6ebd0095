// Connect4Net evaluation on rectangular boards (connect4/Connect4Net.py:42-60, Connect4GNN.py:31-57
// with a (cols, rows) board from Connect4Game(board_size, rows)): the standard 7 x 6 game and its
// nearest relatives 6 x 5, 5 x 4 and 8 x 7.  conv1 and conv2 fused into one launch that can also
// form the policy/value heads from its LDS feature tile, and az_c4r_eval_fwd, the one-call
// evaluator on top of it.  Square boards keep az_c4_* (7 x 7) and az_c4n_* (4, 5, 6, 8).
#include "az_common.h"
#include "az_conv_chain.h"
#include "az_heads.h"

namespace az {

constexpr int C4R_THREADS = 1024;

// c4n_trunk_heads_kernel for an NX-column, NY-row board.  The board is int8 [NX][NY] (board[x][y],
// y fastest) and the network reads it as a [1][NX][NY] image, so the conv's H is NX and its W is NY
// (Connect4Net.py:43 view(-1, 1, board_x, board_y)); position pos = x * NY + y, feature index
// c * NX*NY + pos (the NCHW flatten of Connect4Net.py:49).
// One board per workgroup: the board, conv1's plane (position-major [NX*NY][36], what
// conv_chain<32> reads) and conv2's output (NCHW [64][NX*NY], the feature row) stay in LDS:
// (1 + 36 + 64) NX NY floats, 17.0 / 12.1 / 8.1 / 22.6 KB at 7x6 / 6x5 / 5x4 / 8x7, plus the heads'
// chunk partials.  One thread per output, each the fmaf chain of conv3x3_relu_kernel (conv_chain),
// so feat has the bits of two az_conv3x3_relu_fwd(H = NX, W = NY) calls.  The row leaves as float4
// stores when feat != NULL (F = 64 NX NY is a multiple of 128 for all four).
// AMAX > 0: the same block then runs the heads on the LDS row -- wave w forms the partials of
// chunks w, w + 16, ... (heads_chunk_part: heads_row_block's per-chunk arithmetic) and
// heads_finalize_row sums them in chunk order: az_heads_fwd's bits.  F is 10.5 / 7.5 / 5 / 14
// chunks of 256 columns (7x6 and 6x5: the last one partial).
template <int NX, int NY, int AMAX>
__global__ __launch_bounds__(C4R_THREADS) void c4r_trunk_heads_kernel(
    const int8_t* __restrict__ boards, const float* __restrict__ w1, const float* __restrict__ b1,
    const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ feat,
    const float* __restrict__ wp, const float* __restrict__ bp, int A,
    const float* __restrict__ wv, const float* __restrict__ bv, float* __restrict__ logp,
    float* __restrict__ pi, float* __restrict__ v) {
  constexpr int HW = NX * NY, F = 64 * HW;
  constexpr int NCH = (F + HEADS_KC - 1) / HEADS_KC;
  static_assert(F % 4 == 0, "float4 row stores");
  __shared__ float bd[HW];
  __shared__ __attribute__((aligned(16))) float p1[HW * 36];
  __shared__ __attribute__((aligned(16))) float tile[F];
  __shared__ float part[AMAX > 0 ? NCH * (AMAX + 1) : 1];
  __shared__ float sm[AMAX + 1];
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  if (tid < HW) bd[tid] = (float)boards[b * HW + tid];
  __syncthreads();
  for (int idx = tid; idx < 32 * HW; idx += C4R_THREADS) {
    const int co = idx / HW, pos = idx % HW;
    const float s = conv_chain<1, NX, NY, 1, false>(w1 + co * 9, bd, pos / NY, pos % NY) + b1[co];
    p1[pos * 36 + co] = s > 0.f ? s : 0.f;
  }
  __syncthreads();
  for (int idx = tid; idx < F; idx += C4R_THREADS) {
    const int co = idx / HW, pos = idx % HW;
    const float s =
        conv_chain<32, NX, NY, 1, true>(w2 + co * 32 * 9, p1, pos / NY, pos % NY) + b2[co];
    tile[idx] = s > 0.f ? s : 0.f;
  }
  __syncthreads();
  if (feat) {
    f32x4* dst = reinterpret_cast<f32x4*>(feat + b * F);
    for (int i = tid; i < F / 4; i += C4R_THREADS)
      dst[i] = *reinterpret_cast<const f32x4*>(tile + i * 4);
  }
  if constexpr (AMAX > 0) {
    for (int c = tid >> 6; c < NCH; c += C4R_THREADS / 64)
      heads_chunk_part<AMAX>(tile, tile, F, wp, A, wv, c, part + c * (AMAX + 1));
    __syncthreads();
    heads_finalize_row<AMAX>(part, NCH, A, bp, bv, (int)b, logp, pi, v, sm);
  }
}

struct C4rHeads {
  const float* wp; const float* bp; int A; const float* wv; const float* bv;
  float* logp; float* pi; float* v;
};

template <int NX, int NY>
static void launch_c4r(const int8_t* boards, int B, const float* w1, const float* b1,
                       const float* w2, const float* b2, float* feat, const C4rHeads* h,
                       hipStream_t s) {
  const dim3 g(B), blk(C4R_THREADS);
  if (!h)
    hipLaunchKernelGGL((c4r_trunk_heads_kernel<NX, NY, 0>), g, blk, 0, s, boards, w1, b1, w2, b2,
                       feat, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
  // AMAX by A, as az_heads_fwd picks it.  The boards' own A = NX + 1 is 6 .. 9: AMAX 8 or 16, no
  // scratch.  AMAX = 32 (a caller's A of 17 .. 32) holds 33 float4 weight chunks per lane and
  // spills ~110 B/lane at 1,024 threads, as c4n_trunk_heads_kernel<N, 32> does.
  else if (h->A <= 8)
    hipLaunchKernelGGL((c4r_trunk_heads_kernel<NX, NY, 8>), g, blk, 0, s, boards, w1, b1, w2, b2,
                       feat, h->wp, h->bp, h->A, h->wv, h->bv, h->logp, h->pi, h->v);
  else if (h->A <= 16)
    hipLaunchKernelGGL((c4r_trunk_heads_kernel<NX, NY, 16>), g, blk, 0, s, boards, w1, b1, w2, b2,
                       feat, h->wp, h->bp, h->A, h->wv, h->bv, h->logp, h->pi, h->v);
  else
    hipLaunchKernelGGL((c4r_trunk_heads_kernel<NX, NY, 32>), g, blk, 0, s, boards, w1, b1, w2, b2,
                       feat, h->wp, h->bp, h->A, h->wv, h->bv, h->logp, h->pi, h->v);
}

// the fused shapes: (cols, rows) = (7, 6), (6, 5), (5, 4), (8, 7)
static bool c4r_shape(int nx, int ny) {
  return (nx == 7 && ny == 6) || (nx == 6 && ny == 5) || (nx == 5 && ny == 4) ||
         (nx == 8 && ny == 7);
}

#define C4R_SHAPES "(nx, ny) in {(7, 6), (6, 5), (5, 4), (8, 7)}"

// The evaluator a square board belongs to (NULL: none, the eager path).
static const char* c4r_square_owner(int nx, int ny) {
  if (nx != ny) return nullptr;
  if (nx == 7) return "az_c4_eval_fwd";
  if (nx == 4 || nx == 5 || nx == 6 || nx == 8) return "az_c4n_eval_fwd";
  return nullptr;
}

// The checked launch behind the three entry points (h == NULL: the trunk alone).
static int c4r_launch(const int8_t* boards, int B, int nx, int ny, const float* w1,
                      const float* b1, const float* w2, const float* b2, float* feat,
                      const C4rHeads* h, hipStream_t s) {
  switch (nx) {
    case 7: launch_c4r<7, 6>(boards, B, w1, b1, w2, b2, feat, h, s); break;
    case 6: launch_c4r<6, 5>(boards, B, w1, b1, w2, b2, feat, h, s); break;
    case 5: launch_c4r<5, 4>(boards, B, w1, b1, w2, b2, feat, h, s); break;
    default: launch_c4r<8, 7>(boards, B, w1, b1, w2, b2, feat, h, s); break;
  }
  return check_launch("c4r_trunk_heads_kernel");
}

}  // namespace az

using namespace az;

extern "C" int az_c4r_trunk_fwd(const int8_t* boards, int B, int nx, int ny,
                                const float* conv1_w, const float* conv1_b,
                                const float* conv2_w, const float* conv2_b, float* feat,
                                void* stream) {
  AZ_REQUIRE(B >= 0 && c4r_shape(nx, ny), AZ_EINVAL,
             "az_c4r_trunk_fwd: bad shape B=%d nx=%d ny=%d (" C4R_SHAPES
             "; square boards are az_c4_trunk_fwd / az_c4n_trunk_fwd)",
             B, nx, ny);
  if (B == 0) return AZ_OK;
  AZ_REQUIRE(boards && conv1_w && conv1_b && conv2_w && conv2_b && feat, AZ_EINVAL,
             "az_c4r_trunk_fwd: null pointer");
  AZ_REQUIRE(aligned16(conv2_w) && aligned16(feat), AZ_EINVAL,
             "az_c4r_trunk_fwd: conv2_w and feat need 16B alignment");
  return c4r_launch(boards, B, nx, ny, conv1_w, conv1_b, conv2_w, conv2_b, feat, nullptr,
                    as_stream(stream));
}

extern "C" int az_c4r_trunk_heads_fwd(const int8_t* boards, int B, int nx, int ny,
                                      const float* conv1_w, const float* conv1_b,
                                      const float* conv2_w, const float* conv2_b,
                                      const float* wp, const float* bp, int A, const float* wv,
                                      const float* bv, float* feat, float* logp, float* pi,
                                      float* v, void* stream) {
  AZ_REQUIRE(B >= 0 && c4r_shape(nx, ny) && A >= 1 && A <= 32, AZ_EINVAL,
             "az_c4r_trunk_heads_fwd: bad shape B=%d nx=%d ny=%d A=%d (" C4R_SHAPES ", A <= 32)",
             B, nx, ny, A);
  if (B == 0) return AZ_OK;
  AZ_REQUIRE(boards && conv1_w && conv1_b && conv2_w && conv2_b && wp && bp && wv && bv && logp &&
                 v,
             AZ_EINVAL, "az_c4r_trunk_heads_fwd: null pointer");
  AZ_REQUIRE(aligned16(conv2_w) && aligned16(feat) && aligned16(wp) && aligned16(wv), AZ_EINVAL,
             "az_c4r_trunk_heads_fwd: conv2_w, feat, wp and wv need 16B alignment");
  const C4rHeads h{wp, bp, A, wv, bv, logp, pi, v};
  return c4r_launch(boards, B, nx, ny, conv1_w, conv1_b, conv2_w, conv2_b, feat, &h,
                    as_stream(stream));
}

extern "C" size_t az_c4r_eval_ws_bytes(int max_B, int nx, int ny, int A) {
  if (max_B < 1 || !c4r_shape(nx, ny) || A < 1 || A > 32) return 0;
  return az_transform_heads_ws_bytes(max_B, 64 * nx * ny, A);
}

extern "C" int az_c4r_eval_fwd(const az_c4r_eval* e, const int8_t* boards, int B, float* pi,
                               float* v, float* gpi, float* gv, void* stream) {
  AZ_REQUIRE(e != nullptr, AZ_EINVAL, "az_c4r_eval_fwd: null descriptor");
  AZ_REQUIRE(B >= 1 && B <= e->max_B, AZ_EINVAL, "az_c4r_eval_fwd: B=%d max_B=%d", B, e->max_B);
  const char* owner = c4r_square_owner(e->nx, e->ny);
  AZ_REQUIRE(owner == nullptr, AZ_EINVAL,
             "az_c4r_eval_fwd: nx=%d ny=%d is %s's board (this evaluator: " C4R_SHAPES ")", e->nx,
             e->ny, owner ? owner : "");
  AZ_REQUIRE(c4r_shape(e->nx, e->ny) && e->A >= 1 && e->A <= 32 && e->F == 64 * e->nx * e->ny,
             AZ_EINVAL,
             "az_c4r_eval_fwd: bad shape nx=%d ny=%d A=%d F=%d (" C4R_SHAPES
             ", A <= 32, F = 64 nx ny)",
             e->nx, e->ny, e->A, e->F);
  AZ_REQUIRE(v || gv, AZ_EINVAL, "az_c4r_eval_fwd: neither v nor gv requested");
  AZ_REQUIRE(boards && e->conv1_w && e->conv1_b && e->conv2_w && e->conv2_b && e->fc_policy_w &&
                 e->fc_policy_b && e->fc_value_w && e->fc_value_b,
             AZ_EINVAL, "az_c4r_eval_fwd: null boards / weight pointer");
  AZ_REQUIRE(e->feat && (!v || e->logp), AZ_EINVAL, "az_c4r_eval_fwd: null scratch (feat / logp)");
  AZ_REQUIRE(!gv || (e->ot0_w && e->ot0_b && e->ot2_w && e->ot2_b && e->hidden && e->glogp &&
                     e->ws),
             AZ_EINVAL, "az_c4r_eval_fwd: GNN tail requested without its weights / scratch");
  AZ_REQUIRE(aligned16(e->conv2_w) && aligned16(e->feat) && aligned16(e->fc_policy_w) &&
                 aligned16(e->fc_value_w) &&
                 (!gv || (aligned16(e->hidden) && aligned16(e->ws) && aligned16(e->ot0_w) &&
                          aligned16(e->ot2_w))),
             AZ_EINVAL, "az_c4r_eval_fwd: weights and scratch need 16B alignment");
  AZ_REQUIRE(!gv || e->ws_bytes >= az_c4r_eval_ws_bytes(e->max_B, e->nx, e->ny, e->A), AZ_EINVAL,
             "az_c4r_eval_fwd: workspace too small (az_c4r_eval_ws_bytes)");
  // the fused launch: the feature rows leave for the GNN tail only, the standard heads come
  // from the LDS tile
  const C4rHeads h{e->fc_policy_w, e->fc_policy_b, e->A, e->fc_value_w, e->fc_value_b, e->logp,
                   pi, v};
  int rc = c4r_launch(boards, B, e->nx, e->ny, e->conv1_w, e->conv1_b, e->conv2_w, e->conv2_b,
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
