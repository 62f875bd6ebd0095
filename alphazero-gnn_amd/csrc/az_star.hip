// GNN leaf evaluation over the leaf's children: the layer stack of gnn_utils.py:34-74 on a few
// small stars (row 0 = the leaf, rows 1.. = its children), and az_c4_star_eval_fwd, the one-call
// Connect4 evaluator on top of it (trunk -> star layers -> output_transform -> heads of row 0).
//
// Only row 0 of a star changes in a layer (gnn_utils.py:71-74), so a layer is, per star,
//   P_t = W1[:, :F] t,  P_s(i) = W1[:, F:] x_i                 attention.0, factored per node
//   a_i = sigmoid(w2 . relu(P_t + P_s(i) + b1) + b2)           gnn_utils.py:30-32
//   a'  = a / sum(a) when sum(a) > 0;  agg = sum_i a'_i x_i    gnn_utils.py:57-65
//   t'  = t + sigmoid(Wg [t; agg] + bg) * (Wu2 relu(Wu1 [t; agg] + bu1) + bu2)
// and the B <= 8 stars of a call share one pass over every weight matrix: their row 0s are the rows
// of one GEMV.  Four launches per layer:
//   star_attn_proj_kernel   blocks own (16 hidden units) x (256 columns of F) of one star: the
//                           3.2 MB of attention.0 come from HBM once, not once per node, and
//                           each block leaves its k-slice partial of P per node;
//   star_agg_kernel         per star: sums the partials in slice order, relu, w2, sigmoid, the
//                           normalisation, and agg from the <= 8 source rows;
//   star_gemv_kernel<PAIR>  gate.0 and update_net.0 on [t; agg] in one grid;
//   star_gemv_kernel<UPD2>  update_net.2 with the gated residual t + g * u.
// Every output is a fixed-order fp32 fmaf chain (lane-strided over K, then a wave butterfly); no
// atomics, nothing shared between stars, and no chain depends on B or on a star's position in the
// call, so star b's row has the same bits alone and in any batch.
#include "az_common.h"

namespace az {

constexpr int STAR_NODES = AZ_STAR_MAX_NODES;   // row slots per star
constexpr int STAR_KS = 256;                    // columns of F per attention block (64 lanes x 4)
constexpr int STAR_HQ = 16;                     // hidden units per attention block
constexpr int STAR_KC = 1024;                   // GEMV: columns of K staged per step
constexpr int STAR_R = 2;                       // GEMV: output columns per wave
constexpr int STAR_MAX_H = 1024;                // star_agg_kernel keeps P of one star in LDS

// counts[b] clamped into [1, 9] (a bad value cannot index outside a star), wave-uniform
__device__ __forceinline__ int star_count(const int* __restrict__ counts, int b) {
  int n = counts[b];
  n = n < 1 ? 1 : (n > STAR_NODES ? STAR_NODES : n);
  return __builtin_amdgcn_readfirstlane(n);
}

__device__ __forceinline__ float dot4(f32x4 a, f32x4 w, float acc) {
  return fmaf(a[0], w[0], fmaf(a[1], w[1], fmaf(a[2], w[2], fmaf(a[3], w[3], acc))));
}

// part[ks][b * 9 + i][q]: slice ks (columns ks*256 ..) of W1[q, :F] . t_b for i == 0 and of
// W1[q, F:] . x_{b,i} for a source row i.  Slots at or beyond counts[b] (and every slot of a
// one-row star) are neither read nor written.  grid (ceil(F / 256), ceil(H / 16), B), 256
// threads: a wave keeps its 16 x 2 weight float4s in registers and takes rows wave, wave + 4,
// wave + 8 of star blockIdx.z (the stars after the first find attention.0 in L2).
__global__ __launch_bounds__(256) void star_attn_proj_kernel(
    const float* __restrict__ x, int ldstar, const float* __restrict__ t, int ldt,
    const int* __restrict__ counts, int F, int H, const float* __restrict__ w1,
    float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int k = blockIdx.x * STAR_KS + lane * 4;
  const bool kin = k < F;                       // F % 4 == 0: a float4 is whole or absent
  const int kc = kin ? k : 0;
  const int q0 = blockIdx.y * STAR_HQ;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  f32x4 wt[STAR_HQ], ws[STAR_HQ];
#pragma unroll
  for (int q = 0; q < STAR_HQ; ++q) {
    const int row = q0 + q < H ? q0 + q : 0;    // past H: row 0, never stored
    const float* r = w1 + (size_t)row * 2 * F + kc;
    const f32x4 a = *reinterpret_cast<const f32x4*>(r);
    const f32x4 c = *reinterpret_cast<const f32x4*>(r + F);
    wt[q] = kin ? a : z;
    ws[q] = kin ? c : z;
  }
  // star blockIdx.z: the wave's rows first (row wave + 4 j), every load in flight before the
  // first product
  const int b = blockIdx.z;
  const int n = star_count(counts, b);
  if (n < 2) return;
  const int slots = gridDim.z * STAR_NODES;
  constexpr int NJ = (STAR_NODES + 3) / 4;
  f32x4 rows[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int i = wave + 4 * j;
    const float* row = i == 0 ? t + (size_t)b * ldt : x + (size_t)b * ldstar + (size_t)i * F;
    rows[j] = z;
    if (i < n) rows[j] = *reinterpret_cast<const f32x4*>(row + kc);   // meets zeros in w past F
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int i = wave + 4 * j;
    if (i >= n) break;
    const f32x4 a = rows[j];
    float v[STAR_HQ];
    if (i == 0) {
#pragma unroll
      for (int q = 0; q < STAR_HQ; ++q) v[q] = dot4(a, wt[q], 0.f);
    } else {
#pragma unroll
      for (int q = 0; q < STAR_HQ; ++q) v[q] = dot4(a, ws[q], 0.f);
    }
    const float s = wave_multi_sum<STAR_HQ>(v);  // lanes 4j .. 4j+3 hold hidden unit q0 + j
    const int q = q0 + (lane >> 2);
    if ((lane & 3) == 0 && q < H)
      part[((size_t)blockIdx.x * slots + b * STAR_NODES + i) * H + q] = s;
  }
}

// agg[b][:] for star b (zeros for a one-row star, whose agg feeds nothing that is kept).
// grid (ceil(F / 4096), B), 1,024 threads, 9 H floats of dynamic LDS; every block of a star forms
// the star's P rows and its <= 8 weights itself: wave w the edge 1 + w.
__global__ __launch_bounds__(1024) void star_agg_kernel(
    const float* __restrict__ x, int ldstar, const int* __restrict__ counts, int B, int F, int H,
    int KS, const float* __restrict__ part, const float* __restrict__ b1,
    const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ agg) {
  __shared__ float al[STAR_NODES];
  extern __shared__ float P[];                   // [n][H]: P_t, then P_s(i)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.y;
  const int n = star_count(counts, b);
  const int k = (blockIdx.x * 1024 + threadIdx.x) * 4;
  if (n < 2) {
    if (k < F) *reinterpret_cast<f32x4*>(agg + (size_t)b * F + k) = f32x4{0.f, 0.f, 0.f, 0.f};
    return;
  }
  // P of the star's n rows: one (row, hidden unit) per thread and step, its slices summed in
  // slice order, sixteen loads in flight at a time (a slice past KS adds 0)
  const size_t slice = (size_t)B * STAR_NODES * H;
  const float* mine = part + (size_t)b * STAR_NODES * H;
  for (int idx = threadIdx.x; idx < n * H; idx += 1024) {
    float s = 0.f;
    for (int ks = 0; ks < KS; ks += 16) {
      float v[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = ks + j < KS ? mine[(ks + j) * slice + idx] : 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) s += v[j];
    }
    P[idx] = s;
  }
  __syncthreads();
  for (int i = 1 + wave; i < n; i += 16) {
    float acc = 0.f;
    for (int q = lane; q < H; q += 64) {
      const float h = P[q] + P[i * H + q] + b1[q];
      acc = fmaf(w2[q], h > 0.f ? h : 0.f, acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) al[i] = sigmoidf_ref(acc + b2[0]);
  }
  __syncthreads();
  float s = 0.f;
  for (int i = 1; i < n; ++i) s += al[i];
  if (k >= F) return;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const float* xs = x + (size_t)b * ldstar + k;
  for (int i = 1; i < n; ++i) {                  // the caller's row order
    const float a = s > 0.f ? al[i] / s : al[i];
    const f32x4 v = *reinterpret_cast<const f32x4*>(xs + (size_t)i * F);
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = fmaf(a, v[c], acc[c]);
  }
  *reinterpret_cast<f32x4*>(agg + (size_t)b * F + k) = acc;
}

// The two weight-streaming GEMVs of the node update over the M <= 8 row 0s.
struct StarGemv {
  int M, N, K;                                   // rows (stars), output columns, dot length
  const float* a0; int lda0;                     // A[m][k] = a0[m * lda0 + k]        for k <  K0
  const float* a1; int lda1; int K0;             //         = a1[m * lda1 + k - K0]   for k >= K0
  const float* w0; const float* bias0; int N0;   // column j < N0: weight row w0 + j * K
  const float* w1; const float* bias1;           // column j >= N0: w1 + (j - N0) * K
  float* c0; float* c1; int ldc;                 // PAIR: sigmoid -> c0[m][j], relu -> c1[m][j - N0]
  const float* t; int ldt; const float* g;       // UPD2: c0[m][j] = t[m][j] + g[m][j] * (. + bias0)
  const int* counts;                             //       (a one-row star: t[m][j] itself)
};

// Each wave owns STAR_R output columns and streams their weight rows (float4 per lane, all loads
// of a K step in flight before the first FMA); A goes through LDS in 1,024-column steps shared by
// the block's 4 waves.  Loads past the step's end re-read its start and meet zeros in the staged
// A; columns past N are clamped to column 0 and never stored.  acc[m][r] is the same chain at
// every MR, so a row's result does not depend on the number of rows.
template <int MR, bool UPD2, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void star_gemv_kernel(StarGemv p) {
  __shared__ __attribute__((aligned(16))) float As[MR * STAR_KC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n_base = (blockIdx.x * WAVES + wave) * STAR_R;
  const float* wrow[STAR_R];
#pragma unroll
  for (int r = 0; r < STAR_R; ++r) {
    const int j = n_base + r < p.N ? n_base + r : 0;
    wrow[r] = j < p.N0 ? p.w0 + (size_t)j * p.K : p.w1 + (size_t)(j - p.N0) * p.K;
  }
  float acc[MR][STAR_R];
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int r = 0; r < STAR_R; ++r) acc[m][r] = 0.f;
  for (int kc = 0; kc < p.K; kc += STAR_KC) {
    const int klen = min(STAR_KC, p.K - kc);
    f32x4 w[STAR_R][STAR_KC / 256];
#pragma unroll
    for (int r = 0; r < STAR_R; ++r)
#pragma unroll
      for (int s = 0; s < STAR_KC / 256; ++s) {
        const int k4 = (lane + 64 * s) * 4;
        w[r][s] = *reinterpret_cast<const f32x4*>(wrow[r] + kc + (k4 < klen ? k4 : 0));
      }
    __syncthreads();                             // the previous step's A has been read
    for (int idx = threadIdx.x; idx < MR * (STAR_KC / 4); idx += WAVES * 64) {
      const int m = idx / (STAR_KC / 4), k4 = (idx % (STAR_KC / 4)) * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      const int k = kc + k4;
      if (m < p.M && k4 < klen)
        v = *reinterpret_cast<const f32x4*>(k < p.K0 ? p.a0 + (size_t)m * p.lda0 + k
                                                     : p.a1 + (size_t)m * p.lda1 + (k - p.K0));
      *reinterpret_cast<f32x4*>(&As[m * STAR_KC + k4]) = v;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < STAR_KC / 256; ++s) {
      const int k4 = (lane + 64 * s) * 4;
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(&As[m * STAR_KC + k4]);
#pragma unroll
        for (int r = 0; r < STAR_R; ++r) acc[m][r] = dot4(a, w[r][s], acc[m][r]);
      }
    }
  }
  float mine = 0.f;   // lane m * STAR_R + r keeps the sum of output (m, n_base + r)
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int r = 0; r < STAR_R; ++r) {
      const float s = wave_sum(acc[m][r]);
      if (lane == m * STAR_R + r) mine = s;
    }
  if (lane >= MR * STAR_R) return;
  const int m = lane / STAR_R, j = n_base + lane % STAR_R;
  if (m >= p.M || j >= p.N) return;
  if constexpr (UPD2) {
    int n = p.counts[m];
    n = n < 1 ? 1 : n;
    const float tv = p.t[(size_t)m * p.ldt + j];
    const float u = mine + p.bias0[j];
    p.c0[(size_t)m * p.ldc + j] = n > 1 ? fmaf(p.g[(size_t)m * p.ldc + j], u, tv) : tv;
  } else if (j < p.N0) {
    p.c0[(size_t)m * p.ldc + j] = sigmoidf_ref(mine + p.bias0[j]);
  } else {
    const float u = mine + p.bias1[j - p.N0];
    p.c1[(size_t)m * p.ldc + (j - p.N0)] = u > 0.f ? u : 0.f;
  }
}

// x0[b][:] = x[b][0][:] (L == 0).  grid (ceil(F / 1024), B)
__global__ __launch_bounds__(256) void star_row0_kernel(const float* __restrict__ x, int ldstar,
                                                        int F, float* __restrict__ x0) {
  const int k = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (k < F)
    *reinterpret_cast<f32x4*>(x0 + (size_t)blockIdx.y * F + k) =
        *reinterpret_cast<const f32x4*>(x + (size_t)blockIdx.y * ldstar + k);
}

template <bool UPD2>
static void launch_star_gemv(const StarGemv& p, hipStream_t s) {
  // 4 waves per block up to 2 rows; above, 8 waves share the staged rows (half the L2 reads of
  // A, which at 8 rows are as many bytes per block as its weights)
  const int W = p.M <= 2 ? 4 : 8;
  const dim3 g((p.N + W * STAR_R - 1) / (W * STAR_R)), blk(W * 64);
  if (p.M <= 1) hipLaunchKernelGGL((star_gemv_kernel<1, UPD2, 4>), g, blk, 0, s, p);
  else if (p.M <= 2) hipLaunchKernelGGL((star_gemv_kernel<2, UPD2, 4>), g, blk, 0, s, p);
  else if (p.M <= 4) hipLaunchKernelGGL((star_gemv_kernel<4, UPD2, 8>), g, blk, 0, s, p);
  else hipLaunchKernelGGL((star_gemv_kernel<8, UPD2, 8>), g, blk, 0, s, p);
}

static size_t pad64(size_t floats) { return (floats + 63) / 64 * 64; }

struct StarWs {
  size_t part, agg, gate, u1, tbuf, total;       // float offsets (tbuf: two [B][F] rows)
};

static StarWs star_ws(int B, int F, int H) {
  StarWs w;
  const size_t KS = (F + STAR_KS - 1) / STAR_KS, rows = pad64((size_t)B * F);
  w.part = 0;
  w.agg = w.part + pad64(KS * B * STAR_NODES * H);
  w.gate = w.agg + rows;
  w.u1 = w.gate + rows;
  w.tbuf = w.u1 + rows;
  w.total = w.tbuf + 2 * rows;
  return w;
}

static bool star_shape(int B, int F, int H, int L) {
  return B >= 0 && B <= AZ_STAR_MAX_STARS && F >= 4 && F % 4 == 0 && F <= (1 << 20) && H >= 2 &&
         H % 2 == 0 && H <= STAR_MAX_H && L >= 0 && L <= AZ_STAR_MAX_LAYERS;
}

}  // namespace az

using namespace az;

extern "C" size_t az_gnn_star_infer_ws_bytes(int B, int F, int H, int L) {
  if (!star_shape(B, F, H, L) || B < 1) return 0;
  return star_ws(B, F, H).total * sizeof(float);
}

extern "C" int az_gnn_star_infer(const float* x, int ldstar, const int* counts, int B, int F,
                                 int H, int L, const az_gnn_layer_w* layers, float* x0, void* ws,
                                 size_t ws_bytes, void* stream) {
  AZ_REQUIRE(star_shape(B, F, H, L), AZ_EINVAL,
             "az_gnn_star_infer: bad shape B=%d F=%d H=%d L=%d (B <= %d, F %% 4 == 0, H %% 2 == 0, "
             "0 <= L <= %d)",
             B, F, H, L, AZ_STAR_MAX_STARS, AZ_STAR_MAX_LAYERS);
  if (B == 0) return AZ_OK;
  AZ_REQUIRE(ldstar >= F && ldstar % 4 == 0, AZ_EINVAL,
             "az_gnn_star_infer: ldstar=%d (>= F=%d, %% 4 == 0)", ldstar, F);
  AZ_REQUIRE(x && counts && x0 && (L == 0 || (layers && ws)), AZ_EINVAL,
             "az_gnn_star_infer: null pointer");
  AZ_REQUIRE(aligned16(x) && aligned16(x0) && aligned16(ws), AZ_EINVAL,
             "az_gnn_star_infer: x, x0 and ws need 16B alignment");
  AZ_REQUIRE(L == 0 || ws_bytes >= az_gnn_star_infer_ws_bytes(B, F, H, L), AZ_EINVAL,
             "az_gnn_star_infer: workspace of %zu bytes too small (az_gnn_star_infer_ws_bytes)",
             ws_bytes);
  for (int l = 0; l < L; ++l) {
    const az_gnn_layer_w& w = layers[l];
    AZ_REQUIRE(w.att_w1 && w.att_b1 && w.att_w2 && w.att_b2 && w.upd_w1 && w.upd_b1 && w.upd_w2 &&
                   w.upd_b2 && w.gate_w && w.gate_b,
               AZ_EINVAL, "az_gnn_star_infer: null weight pointer in layer %d", l);
    AZ_REQUIRE(aligned16(w.att_w1) && aligned16(w.upd_w1) && aligned16(w.upd_w2) &&
                   aligned16(w.gate_w),
               AZ_EINVAL, "az_gnn_star_infer: layer %d weights need 16B alignment", l);
  }
  hipStream_t s = as_stream(stream);
  const dim3 blk(256), rows_grid((F + 1023) / 1024, B), agg_grid((F + 4095) / 4096, B);
  if (L == 0) {
    hipLaunchKernelGGL(star_row0_kernel, rows_grid, blk, 0, s, x, ldstar, F, x0);
    return check_launch("star_row0_kernel");
  }
  const StarWs o = star_ws(B, F, H);
  float* base = static_cast<float*>(ws);
  float* part = base + o.part;
  float* agg = base + o.agg;
  float* gate = base + o.gate;
  float* u1 = base + o.u1;
  const size_t rows = pad64((size_t)B * F);
  const int KS = (F + STAR_KS - 1) / STAR_KS;
  const float* t = x;
  int ldt = ldstar;
  for (int l = 0; l < L; ++l) {
    const az_gnn_layer_w& w = layers[l];
    float* t_out = l == L - 1 ? x0 : base + o.tbuf + (l & 1) * rows;
    hipLaunchKernelGGL(star_attn_proj_kernel, dim3(KS, (H + STAR_HQ - 1) / STAR_HQ, B), blk, 0, s,
                       x, ldstar, t, ldt, counts, F, H, w.att_w1, part);
    hipLaunchKernelGGL(star_agg_kernel, agg_grid, dim3(1024), STAR_NODES * H * sizeof(float), s, x,
                       ldstar, counts, B, F, H, KS,
                       part, w.att_b1, w.att_w2, w.att_b2, agg);
    StarGemv p{};
    p.M = B; p.N = 2 * F; p.K = 2 * F;
    p.a0 = t; p.lda0 = ldt; p.a1 = agg; p.lda1 = F; p.K0 = F;
    p.w0 = w.gate_w; p.bias0 = w.gate_b; p.N0 = F; p.w1 = w.upd_w1; p.bias1 = w.upd_b1;
    p.c0 = gate; p.c1 = u1; p.ldc = F;
    launch_star_gemv<false>(p, s);
    StarGemv q{};
    q.M = B; q.N = F; q.K = F;
    q.a0 = u1; q.lda0 = F; q.a1 = u1; q.lda1 = F; q.K0 = F;
    q.w0 = w.upd_w2; q.bias0 = w.upd_b2; q.N0 = F; q.w1 = w.upd_w2; q.bias1 = w.upd_b2;
    q.c0 = t_out; q.c1 = nullptr; q.ldc = F;
    q.t = t; q.ldt = ldt; q.g = gate; q.counts = counts;
    launch_star_gemv<true>(q, s);
    const int rc = check_launch("az_gnn_star_infer layer");
    if (rc) return rc;
    t = t_out;
    ldt = F;
  }
  return AZ_OK;
}

// ------------------------------------------------------------------------ the one-call evaluator
// 0: no fused trunk; 1: az_c4_trunk_fwd (7x7); 2: az_c4n_trunk_fwd; 3: az_c4r_trunk_fwd
static int star_trunk(int nx, int ny) {
  if (nx == ny) return nx == 7 ? 1 : (nx == 4 || nx == 5 || nx == 6 || nx == 8) ? 2 : 0;
  return ((nx == 7 && ny == 6) || (nx == 6 && ny == 5) || (nx == 5 && ny == 4) ||
          (nx == 8 && ny == 7)) ? 3 : 0;
}

static size_t pad256(size_t b) { return (b + 255) / 256 * 256; }

extern "C" size_t az_c4_star_eval_ws_bytes(int max_B, int nx, int ny, int A, int L) {
  if (max_B < 1 || max_B > AZ_STAR_MAX_STARS || !star_trunk(nx, ny) || A < 1 || A > 32 || L < 0 ||
      L > AZ_STAR_MAX_LAYERS)
    return 0;
  const int F = 64 * nx * ny;
  return pad256(az_gnn_star_infer_ws_bytes(max_B, F, AZ_STAR_HIDDEN, L)) +
         az_transform_heads_ws_bytes(max_B, F, A);
}

extern "C" int az_c4_star_eval_fwd(const az_c4_star_eval* e, const int8_t* boards,
                                   const int* counts, int B, float* gpi, float* gv, void* stream) {
  AZ_REQUIRE(e != nullptr, AZ_EINVAL, "az_c4_star_eval_fwd: null descriptor");
  AZ_REQUIRE(B >= 0 && B <= AZ_STAR_MAX_STARS && B <= e->max_B, AZ_EINVAL,
             "az_c4_star_eval_fwd: B=%d max_B=%d (at most %d stars)", B, e->max_B,
             AZ_STAR_MAX_STARS);
  const int kind = star_trunk(e->nx, e->ny);
  AZ_REQUIRE(kind != 0, AZ_EINVAL,
             "az_c4_star_eval_fwd: nx=%d ny=%d has no fused trunk (7x7, 4x4, 5x5, 6x6, 8x8, 7x6, "
             "6x5, 5x4, 8x7)",
             e->nx, e->ny);
  AZ_REQUIRE(e->L >= 0 && e->L <= AZ_STAR_MAX_LAYERS, AZ_EINVAL,
             "az_c4_star_eval_fwd: L=%d (0 <= L <= %d)", e->L, AZ_STAR_MAX_LAYERS);
  AZ_REQUIRE(e->F == 64 * e->nx * e->ny, AZ_EINVAL,
             "az_c4_star_eval_fwd: F=%d is not 64 nx ny = %d", e->F, 64 * e->nx * e->ny);
  AZ_REQUIRE(e->A >= 1 && e->A <= 32, AZ_EINVAL, "az_c4_star_eval_fwd: A=%d (1 <= A <= 32)", e->A);
  if (B == 0) return AZ_OK;
  AZ_REQUIRE(boards && counts && gv, AZ_EINVAL,
             "az_c4_star_eval_fwd: null pointer (boards / counts / gv)");
  AZ_REQUIRE(e->conv1_w && e->conv1_b && e->conv2_w && e->conv2_b && e->fc_policy_w &&
                 e->fc_policy_b && e->fc_value_w && e->fc_value_b && e->ot0_w && e->ot0_b &&
                 e->ot2_w && e->ot2_b,
             AZ_EINVAL, "az_c4_star_eval_fwd: null pointer (weights)");
  AZ_REQUIRE(e->feat && e->x0 && e->hidden && e->glogp && e->ws, AZ_EINVAL,
             "az_c4_star_eval_fwd: null pointer (scratch: feat / x0 / hidden / glogp / ws)");
  AZ_REQUIRE(aligned16(e->feat) && aligned16(e->x0) && aligned16(e->hidden) && aligned16(e->ws),
             AZ_EINVAL, "az_c4_star_eval_fwd: scratch needs 16B alignment");
  AZ_REQUIRE(e->ws_bytes >= az_c4_star_eval_ws_bytes(e->max_B, e->nx, e->ny, e->A, e->L),
             AZ_EINVAL, "az_c4_star_eval_fwd: workspace of %zu bytes too small "
             "(az_c4_star_eval_ws_bytes)", e->ws_bytes);
  const int F = e->F, HW = e->nx * e->ny, NB = B * STAR_NODES;
  (void)HW;
  // the trunk on all 9 slots of every star, one workgroup per board: a slot past counts[b] holds
  // whatever the caller left there, and its feature row is never read
  int rc;
  if (kind == 1)
    rc = az_c4_trunk_fwd(boards, NB, e->conv1_w, e->conv1_b, e->conv2_w, e->conv2_b, e->feat,
                         stream);
  else if (kind == 2)
    rc = az_c4n_trunk_fwd(boards, NB, e->nx, e->conv1_w, e->conv1_b, e->conv2_w, e->conv2_b,
                          e->feat, stream);
  else
    rc = az_c4r_trunk_fwd(boards, NB, e->nx, e->ny, e->conv1_w, e->conv1_b, e->conv2_w,
                          e->conv2_b, e->feat, stream);
  if (rc) return rc;
  const size_t star_bytes = pad256(az_gnn_star_infer_ws_bytes(e->max_B, F, AZ_STAR_HIDDEN, e->L));
  rc = az_gnn_star_infer(e->feat, STAR_NODES * F, counts, B, F, AZ_STAR_HIDDEN, e->L, e->layers,
                         e->x0, e->ws, star_bytes, stream);
  if (rc) return rc;
  return az_transform_heads_fwd(e->x0, B, F, e->ot0_w, e->ot0_b, e->ot2_w, e->ot2_b,
                                e->fc_policy_w, e->fc_policy_b, e->A, e->fc_value_w,
                                e->fc_value_b, e->hidden, nullptr, e->glogp, gpi, gv,
                                static_cast<char*>(e->ws) + star_bytes, e->ws_bytes - star_bytes,
                                stream);
}
