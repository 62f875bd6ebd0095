// GNN leaf evaluation over the leaf's children for TicTacToe: the layer stack of
// gnn_utils.py:34-74 on a few PACKED stars of up to 26 rows (row 0 = the leaf, rows 1.. = its
// children; a 5x5 opening has 25), and az_ttt_star_eval_fwd, the one-call evaluator on top of it
// (az_ttt_trunk_fwd -> star layers -> output_transform -> fc1 / fc2 -> heads of row 0).
//
// The arithmetic is az_star.hip's, on the packed layout of az_gnn_star_batch_infer.  Only row 0 of
// a star changes in a layer (gnn_utils.py:71-74), so a layer is, per star,
//   P_t = W1[:, :F] t,  P_s(i) = W1[:, F:] x_i                 attention.0, factored per node
//   a_i = sigmoid(w2 . relu(P_t + P_s(i) + b1) + b2)           gnn_utils.py:30-32
//   a'  = a / sum(a) when sum(a) > 0;  agg = sum_i a'_i x_i    gnn_utils.py:57-65
//   t'  = t + sigmoid(Wg [t; agg] + bg) * (Wu2 relu(Wu1 [t; agg] + bu1) + bu2)
// and the B <= 8 stars of a call share one pass over every weight matrix: their row 0s are the rows
// of one GEMV.  Four launches per layer:
//   tstar_attn_proj_kernel   blocks own (16 hidden units) x (256 columns of F) of one star; a wave
//                            keeps its 16 x 2 weight float4s in registers and takes rows wave,
//                            wave + 4, .. wave + 24 of the star (up to 7 row float4s in flight);
//                            F = 128 is half a slice (lanes 32.. add zeros), F = 1,152 is 4.5;
//   tstar_agg_kernel         per star: sums the slice partials in slice order, relu, w2, sigmoid,
//                            the normalisation, and agg from the <= 25 source rows (wave w takes
//                            edges 1 + w and 17 + w); P of a star is 26 H floats of LDS;
//   tstar_gemv_kernel<PAIR>  gate.0 and update_net.0 on [t; agg] in one grid;
//   tstar_gemv_kernel<UPD2>  update_net.2 with the gated residual t + g * u.
// Every output is a fixed-order fp32 fmaf chain (lane-strided over K, then a wave butterfly); no
// atomics, nothing shared between stars, and no chain depends on B, on a star's position in the
// pack or on the other stars' sizes, so star b's row has the same bits alone and in any pack.
#include "az_common.h"
#include "az_gemm.h"

namespace az {

constexpr int TS_NODES = AZ_TTT_STAR_MAX_NODES;  // most rows of a star
constexpr int TS_KS = 256;                       // columns of F per attention block (64 lanes x 4)
constexpr int TS_HQ = 16;                        // hidden units per attention block
constexpr int TS_KC = 1024;                      // GEMV: columns of K staged per step
constexpr int TS_R = 2;                          // GEMV: output columns per wave
constexpr int TS_H = AZ_STAR_HIDDEN;             // tstar_agg_kernel keeps 26 x H floats in LDS
constexpr int TS_AGG_WAVES = 16;

struct TSpan {
  int o, n;   // first row, rows
};

// offs[b] .. offs[b+1] clamped into the V rows and to 1 .. 26 rows (a bad value cannot index
// outside x or a star's slots); b may differ between the lanes of a wave
__device__ __forceinline__ TSpan tstar_span_lane(const int* __restrict__ offs, int b, int V) {
  int o = offs[b];
  const int e = offs[b + 1];
  o = o < 0 ? 0 : (o > V - 1 ? V - 1 : o);
  int n = e - o;
  n = n > V - o ? V - o : n;
  n = n < 1 ? 1 : (n > TS_NODES ? TS_NODES : n);
  return {o, n};
}

// the same for a wave-uniform b, in scalar registers
__device__ __forceinline__ TSpan tstar_span(const int* __restrict__ offs, int b, int V) {
  const TSpan s = tstar_span_lane(offs, b, V);
  return {__builtin_amdgcn_readfirstlane(s.o), __builtin_amdgcn_readfirstlane(s.n)};
}

__device__ __forceinline__ float tdot4(f32x4 a, f32x4 w, float acc) {
  return fmaf(a[0], w[0], fmaf(a[1], w[1], fmaf(a[2], w[2], fmaf(a[3], w[3], acc))));
}

// part[ks][b * 26 + i][q]: slice ks (columns ks*256 ..) of W1[q, :F] . t_b for i == 0 and of
// W1[q, F:] . x_{b,i} for a source row i.  Slots at or beyond the star's rows (and every slot of a
// one-row star) are neither read nor written.  t == nullptr: the star's own row 0 in x (layer 0).
// grid (ceil(F / 256), H / 16, B), 256 threads.
__global__ __launch_bounds__(256) void tstar_attn_proj_kernel(
    const float* __restrict__ x, const float* __restrict__ t, const int* __restrict__ offs, int V,
    int F, int H, const float* __restrict__ w1, float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int k = blockIdx.x * TS_KS + lane * 4;
  const bool kin = k < F;                       // F % 4 == 0: a float4 is whole or absent
  const int kc = kin ? k : 0;
  const int q0 = blockIdx.y * TS_HQ;
  const int b = blockIdx.z;
  const TSpan sp = tstar_span(offs, b, V);
  const int n = sp.n;
  if (n < 2) return;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  f32x4 wt[TS_HQ], ws[TS_HQ];
#pragma unroll
  for (int q = 0; q < TS_HQ; ++q) {
    const int row = q0 + q < H ? q0 + q : 0;    // past H: row 0, never stored
    const float* r = w1 + (size_t)row * 2 * F + kc;
    const f32x4 a = *reinterpret_cast<const f32x4*>(r);
    const f32x4 c = *reinterpret_cast<const f32x4*>(r + F);
    wt[q] = kin ? a : z;
    ws[q] = kin ? c : z;
  }
  // the wave's rows (row wave + 4 j), every load in flight before the first product
  constexpr int NJ = (TS_NODES + 3) / 4;
  const float* xs = x + (size_t)sp.o * F;
  f32x4 rows[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int i = wave + 4 * j;
    const float* row = (i == 0 && t) ? t + (size_t)b * F : xs + (size_t)i * F;
    rows[j] = z;
    if (i < n) rows[j] = *reinterpret_cast<const f32x4*>(row + kc);   // meets zeros in w past F
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int i = wave + 4 * j;
    if (i >= n) break;
    const f32x4 a = rows[j];
    float v[TS_HQ];
    if (i == 0) {
#pragma unroll
      for (int q = 0; q < TS_HQ; ++q) v[q] = tdot4(a, wt[q], 0.f);
    } else {
#pragma unroll
      for (int q = 0; q < TS_HQ; ++q) v[q] = tdot4(a, ws[q], 0.f);
    }
    const float s = wave_multi_sum<TS_HQ>(v);    // lanes 4j .. 4j+3 hold hidden unit q0 + j
    const int q = q0 + (lane >> 2);
    if ((lane & 3) == 0 && q < H)
      part[((size_t)blockIdx.x * gridDim.z * TS_NODES + b * TS_NODES + i) * H + q] = s;
  }
}

// agg[b][:] for star b (zeros for a one-row star, whose agg feeds nothing that is kept).
// grid (ceil(F / 4096), B), 1,024 threads; every block of a star forms the star's P rows and its
// <= 25 weights itself: wave w the edges 1 + w and 17 + w.
__global__ __launch_bounds__(1024) void tstar_agg_kernel(
    const float* __restrict__ x, const int* __restrict__ offs, int B, int V, int F, int KS,
    const float* __restrict__ part, const float* __restrict__ b1, const float* __restrict__ w2,
    const float* __restrict__ b2, float* __restrict__ agg) {
  constexpr int H = TS_H;
  __shared__ float al[TS_NODES];
  __shared__ float P[TS_NODES * H];              // [n][H]: P_t, then P_s(i)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.y;
  const TSpan sp = tstar_span(offs, b, V);
  const int n = sp.n;
  const int k = (blockIdx.x * 1024 + threadIdx.x) * 4;
  if (n < 2) {
    if (k < F) *reinterpret_cast<f32x4*>(agg + (size_t)b * F + k) = f32x4{0.f, 0.f, 0.f, 0.f};
    return;
  }
  // P of the star's n rows: one (row, hidden unit) per thread and step, its slices summed in
  // slice order, eight loads in flight at a time (a slice past KS adds 0)
  const size_t slice = (size_t)B * TS_NODES * H;
  const float* mine = part + (size_t)b * TS_NODES * H;
  for (int idx = threadIdx.x; idx < n * H; idx += 1024) {
    float s = 0.f;
    for (int ks = 0; ks < KS; ks += 8) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = ks + j < KS ? mine[(ks + j) * slice + idx] : 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[j];
    }
    P[idx] = s;
  }
  __syncthreads();
  for (int i = 1 + wave; i < n; i += TS_AGG_WAVES) {
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
  const float* xs = x + (size_t)sp.o * F + k;
  for (int i = 1; i < n; ++i) {                  // the caller's row order
    const float a = s > 0.f ? al[i] / s : al[i];
    const f32x4 v = *reinterpret_cast<const f32x4*>(xs + (size_t)i * F);
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = fmaf(a, v[c], acc[c]);
  }
  *reinterpret_cast<f32x4*>(agg + (size_t)b * F + k) = acc;
}

// The two weight-streaming GEMVs of the node update over the M <= 8 row 0s.
struct TStarGemv {
  int M, N, K;                                   // rows (stars), output columns, dot length
  const float* a0; int lda0;                     // A[m][k] = a0[ra(m) * lda0 + k]    for k <  K0
  const float* a1; int lda1; int K0;             //         = a1[m * lda1 + k - K0]   for k >= K0
  const float* w0; const float* bias0; int N0;   // column j < N0: weight row w0 + j * K
  const float* w1; const float* bias1;           // column j >= N0: w1 + (j - N0) * K
  float* c0; float* c1; int ldc;                 // PAIR: sigmoid -> c0[m][j], relu -> c1[m][j - N0]
  const float* t; int ldt; const float* g;       // UPD2: c0[m][j] = t[rt(m)][j] + g[m][j] * (. + bias0)
  const int* offs; int V;                        //       (a one-row star: t[rt(m)][j] itself)
  int a_packed, t_packed;                        // ra(m) / rt(m) = star m's first packed row when
};                                               // a0 / t is x itself (layer 0), else m

// Each wave owns TS_R output columns and streams their weight rows (float4 per lane, all loads of
// a K step in flight before the first FMA); A goes through LDS in 1,024-column steps shared by the
// block's waves.  Loads past the step's end re-read its start and meet zeros in the staged A;
// columns past N are clamped to column 0 and never stored.  acc[m][r] is the same chain at every
// MR, so a row's result does not depend on the number of rows.
template <int MR, bool UPD2, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void tstar_gemv_kernel(TStarGemv p) {
  __shared__ __attribute__((aligned(16))) float As[MR * TS_KC];
  __shared__ int r0[MR];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n_base = (blockIdx.x * WAVES + wave) * TS_R;
  if (threadIdx.x < MR)
    r0[threadIdx.x] = threadIdx.x < p.M && p.a_packed
                          ? tstar_span_lane(p.offs, threadIdx.x, p.V).o : threadIdx.x;
  const float* wrow[TS_R];
#pragma unroll
  for (int r = 0; r < TS_R; ++r) {
    const int j = n_base + r < p.N ? n_base + r : 0;
    wrow[r] = j < p.N0 ? p.w0 + (size_t)j * p.K : p.w1 + (size_t)(j - p.N0) * p.K;
  }
  float acc[MR][TS_R];
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int r = 0; r < TS_R; ++r) acc[m][r] = 0.f;
  for (int kc = 0; kc < p.K; kc += TS_KC) {
    const int klen = min(TS_KC, p.K - kc);
    f32x4 w[TS_R][TS_KC / 256];
#pragma unroll
    for (int r = 0; r < TS_R; ++r)
#pragma unroll
      for (int s = 0; s < TS_KC / 256; ++s) {
        const int k4 = (lane + 64 * s) * 4;
        w[r][s] = *reinterpret_cast<const f32x4*>(wrow[r] + kc + (k4 < klen ? k4 : 0));
      }
    __syncthreads();                             // r0 is set; the previous step's A has been read
    for (int idx = threadIdx.x; idx < MR * (TS_KC / 4); idx += WAVES * 64) {
      const int m = idx / (TS_KC / 4), k4 = (idx % (TS_KC / 4)) * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      const int k = kc + k4;
      if (m < p.M && k4 < klen)
        v = *reinterpret_cast<const f32x4*>(k < p.K0 ? p.a0 + (size_t)r0[m] * p.lda0 + k
                                                     : p.a1 + (size_t)m * p.lda1 + (k - p.K0));
      *reinterpret_cast<f32x4*>(&As[m * TS_KC + k4]) = v;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < TS_KC / 256; ++s) {
      const int k4 = (lane + 64 * s) * 4;
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(&As[m * TS_KC + k4]);
#pragma unroll
        for (int r = 0; r < TS_R; ++r) acc[m][r] = tdot4(a, w[r][s], acc[m][r]);
      }
    }
  }
  float mine = 0.f;   // lane m * TS_R + r keeps the sum of output (m, n_base + r)
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int r = 0; r < TS_R; ++r) {
      const float s = wave_sum(acc[m][r]);
      if (lane == m * TS_R + r) mine = s;
    }
  if (lane >= MR * TS_R) return;
  const int m = lane / TS_R, j = n_base + lane % TS_R;
  if (m >= p.M || j >= p.N) return;
  if constexpr (UPD2) {
    const TSpan sp = tstar_span_lane(p.offs, m, p.V);
    const int n = sp.n;
    const float tv = p.t[(size_t)(p.t_packed ? sp.o : m) * p.ldt + j];
    const float u = mine + p.bias0[j];
    p.c0[(size_t)m * p.ldc + j] = n > 1 ? fmaf(p.g[(size_t)m * p.ldc + j], u, tv) : tv;
  } else if (j < p.N0) {
    p.c0[(size_t)m * p.ldc + j] = sigmoidf_ref(mine + p.bias0[j]);
  } else {
    const float u = mine + p.bias1[j - p.N0];
    p.c1[(size_t)m * p.ldc + (j - p.N0)] = u > 0.f ? u : 0.f;
  }
}

// x0[b][:] = the first row of star b (L == 0).  grid (ceil(F / 1024), B)
__global__ __launch_bounds__(256) void tstar_row0_kernel(const float* __restrict__ x,
                                                         const int* __restrict__ offs, int V,
                                                         int F, float* __restrict__ x0) {
  const int k = (blockIdx.x * 256 + threadIdx.x) * 4;
  const int o = tstar_span(offs, blockIdx.y, V).o;
  if (k < F)
    *reinterpret_cast<f32x4*>(x0 + (size_t)blockIdx.y * F + k) =
        *reinterpret_cast<const f32x4*>(x + (size_t)o * F + k);
}

template <bool UPD2>
static void launch_tstar_gemv(const TStarGemv& p, hipStream_t s) {
  // 4 waves per block up to 2 rows; above, 8 waves share the staged rows
  const int W = p.M <= 2 ? 4 : 8;
  const dim3 g((p.N + W * TS_R - 1) / (W * TS_R)), blk(W * 64);
  if (p.M <= 1) hipLaunchKernelGGL((tstar_gemv_kernel<1, UPD2, 4>), g, blk, 0, s, p);
  else if (p.M <= 2) hipLaunchKernelGGL((tstar_gemv_kernel<2, UPD2, 4>), g, blk, 0, s, p);
  else if (p.M <= 4) hipLaunchKernelGGL((tstar_gemv_kernel<4, UPD2, 8>), g, blk, 0, s, p);
  else hipLaunchKernelGGL((tstar_gemv_kernel<8, UPD2, 8>), g, blk, 0, s, p);
}

static size_t tpad64(size_t floats) { return (floats + 63) / 64 * 64; }
static size_t tpad256(size_t b) { return (b + 255) / 256 * 256; }

struct TStarWs {
  size_t part, agg, gate, u1, tbuf, total;       // float offsets (tbuf: two [B][F] rows)
};

static TStarWs tstar_ws(int B, int F, int H) {
  TStarWs w;
  const size_t KS = (F + TS_KS - 1) / TS_KS, rows = tpad64((size_t)B * F);
  w.part = 0;
  w.agg = w.part + tpad64(KS * B * TS_NODES * H);
  w.gate = w.agg + rows;
  w.u1 = w.gate + rows;
  w.tbuf = w.u1 + rows;
  w.total = w.tbuf + 2 * rows;
  return w;
}

static bool tstar_shape(int B, int F, int H, int L) {
  return B >= 0 && B <= AZ_STAR_MAX_STARS && F >= 4 && F % 4 == 0 && F <= (1 << 20) &&
         H == AZ_STAR_HIDDEN && L >= 0 && L <= AZ_STAR_MAX_LAYERS;
}

// offs in host memory the device maps (az_host_alloc, pinned) is checked here; offs in HBM is
// clamped by the kernels (tstar_span)
static int tstar_offs_check(const char* who, const int* offs, int B, int V) {
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, offs) != hipSuccess) {
    (void)hipGetLastError();
  } else if (attr.type == hipMemoryTypeHost) {
    AZ_REQUIRE(offs[0] == 0 && offs[B] == V, AZ_EINVAL,
               "%s: offs[0]=%d offs[B]=%d (need 0 and V=%d)", who, offs[0], offs[B], V);
    for (int b = 0; b < B; ++b) {
      const int n = offs[b + 1] - offs[b];
      AZ_REQUIRE(n >= 1, AZ_EINVAL, "%s: offs not ascending at star %d (%d, %d)", who, b, offs[b],
                 offs[b + 1]);
      AZ_REQUIRE(n <= TS_NODES, AZ_EINVAL, "%s: star %d has %d rows (at most %d)", who, b, n,
                 TS_NODES);
    }
  }
  return AZ_OK;
}

static int tstar_layers_check(const char* who, const az_gnn_layer_w* layers, int L) {
  for (int l = 0; l < L; ++l) {
    const az_gnn_layer_w& w = layers[l];
    AZ_REQUIRE(w.att_w1 && w.att_b1 && w.att_w2 && w.att_b2 && w.upd_w1 && w.upd_b1 && w.upd_w2 &&
                   w.upd_b2 && w.gate_w && w.gate_b,
               AZ_EINVAL, "%s: null weight pointer in layer %d", who, l);
    AZ_REQUIRE(aligned16(w.att_w1) && aligned16(w.upd_w1) && aligned16(w.upd_w2) &&
                   aligned16(w.gate_w),
               AZ_EINVAL, "%s: layer %d weights need 16B alignment", who, l);
  }
  return AZ_OK;
}

}  // namespace az

using namespace az;

extern "C" size_t az_gnn_star_packed_infer_ws_bytes(int B, int F, int H, int L) {
  if (!tstar_shape(B, F, H, L) || B < 1) return 0;
  return tstar_ws(B, F, H).total * sizeof(float);
}

extern "C" int az_gnn_star_packed_infer(const float* x, const int* offs, int B, int V, int F,
                                        int H, int L, const az_gnn_layer_w* layers, float* x0,
                                        void* ws, size_t ws_bytes, void* stream) {
  const char* who = "az_gnn_star_packed_infer";
  AZ_REQUIRE(tstar_shape(B, F, H, L), AZ_EINVAL,
             "%s: bad shape B=%d F=%d H=%d L=%d (B <= %d, F %% 4 == 0, H == %d, 0 <= L <= %d)", who,
             B, F, H, L, AZ_STAR_MAX_STARS, AZ_STAR_HIDDEN, AZ_STAR_MAX_LAYERS);
  if (B == 0) return AZ_OK;
  AZ_REQUIRE(V >= B && V <= B * TS_NODES, AZ_EINVAL,
             "%s: V=%d rows for B=%d stars (1 .. %d rows per star)", who, V, B, TS_NODES);
  AZ_REQUIRE(x && offs && x0 && (L == 0 || (layers && ws)), AZ_EINVAL, "%s: null pointer", who);
  AZ_REQUIRE(aligned16(x) && aligned16(x0) && aligned16(ws) && ((uintptr_t)offs & 3u) == 0,
             AZ_EINVAL, "%s: x, x0 and ws need 16B alignment, offs 4B alignment", who);
  AZ_REQUIRE(x != x0, AZ_EINVAL, "%s: x0 may not alias x", who);
  AZ_REQUIRE(L == 0 || ws_bytes >= az_gnn_star_packed_infer_ws_bytes(B, F, H, L), AZ_EINVAL,
             "%s: workspace of %zu bytes too small (az_gnn_star_packed_infer_ws_bytes)", who,
             ws_bytes);
  int rc = tstar_layers_check(who, layers, L);
  if (rc) return rc;
  if ((rc = tstar_offs_check(who, offs, B, V))) return rc;
  hipStream_t s = as_stream(stream);
  const dim3 blk(256), rows_grid((F + 1023) / 1024, B), agg_grid((F + 4095) / 4096, B);
  if (L == 0) {
    hipLaunchKernelGGL(tstar_row0_kernel, rows_grid, blk, 0, s, x, offs, V, F, x0);
    return check_launch("tstar_row0_kernel");
  }
  const TStarWs o = tstar_ws(B, F, H);
  float* base = static_cast<float*>(ws);
  float* part = base + o.part;
  float* agg = base + o.agg;
  float* gate = base + o.gate;
  float* u1 = base + o.u1;
  const size_t rows = tpad64((size_t)B * F);
  const int KS = (F + TS_KS - 1) / TS_KS;
  const float* t = nullptr;                      // layer 0: the stars' own first rows
  for (int l = 0; l < L; ++l) {
    const az_gnn_layer_w& w = layers[l];
    float* t_out = l == L - 1 ? x0 : base + o.tbuf + (l & 1) * rows;
    hipLaunchKernelGGL(tstar_attn_proj_kernel, dim3(KS, (H + TS_HQ - 1) / TS_HQ, B), blk, 0, s, x,
                       t, offs, V, F, H, w.att_w1, part);
    hipLaunchKernelGGL(tstar_agg_kernel, agg_grid, dim3(TS_AGG_WAVES * 64), 0, s, x, offs, B, V, F,
                       KS, part, w.att_b1, w.att_w2, w.att_b2, agg);
    TStarGemv p{};
    p.M = B; p.N = 2 * F; p.K = 2 * F;
    p.a0 = t ? t : x; p.lda0 = F; p.a1 = agg; p.lda1 = F; p.K0 = F;
    p.w0 = w.gate_w; p.bias0 = w.gate_b; p.N0 = F; p.w1 = w.upd_w1; p.bias1 = w.upd_b1;
    p.c0 = gate; p.c1 = u1; p.ldc = F;
    p.offs = offs; p.V = V; p.a_packed = t == nullptr;
    launch_tstar_gemv<false>(p, s);
    TStarGemv q{};
    q.M = B; q.N = F; q.K = F;
    q.a0 = u1; q.lda0 = F; q.a1 = u1; q.lda1 = F; q.K0 = F;
    q.w0 = w.upd_w2; q.bias0 = w.upd_b2; q.N0 = F; q.w1 = w.upd_w2; q.bias1 = w.upd_b2;
    q.c0 = t_out; q.c1 = nullptr; q.ldc = F;
    q.t = t ? t : x; q.ldt = F; q.g = gate;
    q.offs = offs; q.V = V; q.t_packed = t == nullptr;
    launch_tstar_gemv<true>(q, s);
    rc = check_launch("az_gnn_star_packed_infer layer");
    if (rc) return rc;
    t = t_out;
  }
  return AZ_OK;
}

// ------------------------------------------------------------------------ the one-call evaluator
static size_t ttt_star_heads_bytes(int max_B, int A) {
  return tpad256(az_heads_ws_bytes(max_B, 512, A)) + 256;
}

extern "C" size_t az_ttt_star_eval_ws_bytes(int max_B, int n, int A, int L) {
  if (max_B < 1 || max_B > AZ_STAR_MAX_STARS || n < 3 || n > 5 || A < 1 || A > 32 || L < 0 ||
      L > AZ_STAR_MAX_LAYERS)
    return 0;
  const int F = 128 * (n - 2) * (n - 2);
  return tpad256(az_gnn_star_packed_infer_ws_bytes(max_B, F, AZ_STAR_HIDDEN, L)) +
         ttt_star_heads_bytes(max_B, A);
}

extern "C" int az_ttt_star_eval_fwd(const az_ttt_star_eval* e, const int8_t* rows, const int* offs,
                                    int B, int V, float* gpi, float* gv, void* stream) {
  const char* who = "az_ttt_star_eval_fwd";
  AZ_REQUIRE(e != nullptr, AZ_EINVAL, "%s: null descriptor", who);
  AZ_REQUIRE(B >= 0 && B <= AZ_STAR_MAX_STARS && B <= e->max_B, AZ_EINVAL,
             "%s: B=%d max_B=%d (at most %d stars)", who, B, e->max_B, AZ_STAR_MAX_STARS);
  AZ_REQUIRE(e->n >= 3 && e->n <= 5 && e->A >= 1 && e->A <= 32 &&
                 e->F == 128 * (e->n - 2) * (e->n - 2),
             AZ_EINVAL, "%s: bad shape n=%d A=%d F=%d (n in 3..5, A <= 32, F = 128 (n-2)^2)", who,
             e->n, e->A, e->F);
  AZ_REQUIRE(e->L >= 0 && e->L <= AZ_STAR_MAX_LAYERS, AZ_EINVAL, "%s: L=%d (0 <= L <= %d)", who,
             e->L, AZ_STAR_MAX_LAYERS);
  if (B == 0) return AZ_OK;
  AZ_REQUIRE(V >= B && V <= B * TS_NODES, AZ_EINVAL,
             "%s: V=%d rows for B=%d stars (1 .. %d boards per star)", who, V, B, TS_NODES);
  AZ_REQUIRE(rows && offs && gv, AZ_EINVAL, "%s: null pointer (rows / offs / gv)", who);
  AZ_REQUIRE(((uintptr_t)offs & 3u) == 0, AZ_EINVAL, "%s: offs needs 4B alignment", who);
  AZ_REQUIRE(e->conv1_w && e->conv1_b && e->conv2_w && e->conv2_b && e->conv3_w && e->conv3_b &&
                 e->fc1_w && e->fc1_b && e->fc2_w && e->fc2_b && e->fc_policy_w &&
                 e->fc_policy_b && e->fc_value_w && e->fc_value_b && e->ot0_w && e->ot0_b &&
                 e->ot2_w && e->ot2_b,
             AZ_EINVAL, "%s: null pointer (weights)", who);
  AZ_REQUIRE(e->feat && e->x0 && e->hidden && e->y && e->h1 && e->h2 && e->glogp && e->ws,
             AZ_EINVAL,
             "%s: null pointer (scratch: feat / x0 / hidden / y / h1 / h2 / glogp / ws)", who);
  AZ_REQUIRE(aligned16(e->feat) && aligned16(e->x0) && aligned16(e->hidden) && aligned16(e->y) &&
                 aligned16(e->h1) && aligned16(e->h2) && aligned16(e->ws),
             AZ_EINVAL, "%s: scratch needs 16B alignment", who);
  AZ_REQUIRE(aligned16(e->fc1_w) && aligned16(e->fc2_w) && aligned16(e->fc_policy_w) &&
                 aligned16(e->fc_value_w) && aligned16(e->ot0_w) && aligned16(e->ot2_w),
             AZ_EINVAL, "%s: weights need 16B alignment", who);
  AZ_REQUIRE(e->ws_bytes >= az_ttt_star_eval_ws_bytes(e->max_B, e->n, e->A, e->L), AZ_EINVAL,
             "%s: workspace of %zu bytes too small (az_ttt_star_eval_ws_bytes)", who, e->ws_bytes);
  int rc = tstar_layers_check(who, e->layers, e->L);
  if (rc) return rc;
  if ((rc = tstar_offs_check(who, offs, B, V))) return rc;
  const int F = e->F, H = 512;
  hipStream_t s = as_stream(stream);
  // the trunk on the V packed boards, one workgroup per board
  rc = az_ttt_trunk_fwd(rows, V, e->n, e->conv1_w, e->conv1_b, e->conv2_w, e->conv2_b, e->conv3_w,
                        e->conv3_b, e->feat, stream);
  if (rc) return rc;
  const size_t star_bytes =
      tpad256(az_gnn_star_packed_infer_ws_bytes(e->max_B, F, AZ_STAR_HIDDEN, e->L));
  rc = az_gnn_star_packed_infer(e->feat, offs, B, V, F, AZ_STAR_HIDDEN, e->L, e->layers, e->x0,
                                e->ws, star_bytes, stream);
  if (rc) return rc;
  // the GNN tail of az_ttt_eval_fwd on the B row 0s: output_transform.0 / .2, fc1 and fc2 as one
  // launch, the heads
  auto linear = [&](const float* x, int K, const float* w, const float* b, int act, float* out,
                    int N) {
    az_gemm_desc d = {};
    d.M = B; d.N = N; d.K = K;
    d.A = x; d.lda = K; d.a_kmajor = 1;
    d.B = w; d.ldb = K; d.b_kmajor = 1; d.bias = b; d.act = act;
    d.C = out; d.ldc = N;
    return d;
  };
  const az_gemm_desc d0 = linear(e->x0, F, e->ot0_w, e->ot0_b, AZ_ACT_RELU, e->hidden, F);
  if ((rc = gemm_f32(&d0, s))) return rc;
  const az_gemm_desc dy = linear(e->hidden, F, e->ot2_w, e->ot2_b, AZ_ACT_NONE, e->y, F);
  if ((rc = gemm_f32(&dy, s))) return rc;
  const az_gemm_desc d1 = linear(e->y, F, e->fc1_w, e->fc1_b, AZ_ACT_RELU, e->h1, H);
  const az_gemm_desc d2 = linear(e->y, F, e->fc2_w, e->fc2_b, AZ_ACT_RELU, e->h2, H);
  rc = gemv_multi_fwd(&d1, &d2, nullptr, s);
  if (rc < 0) return rc;
  if (rc == 0) {
    if ((rc = gemm_f32(&d1, s))) return rc;
    if ((rc = gemm_f32(&d2, s))) return rc;
  }
  return az_heads_fwd(e->h1, H, e->h2, H, B, H, e->fc_policy_w, e->fc_policy_b, e->A,
                      e->fc_value_w, e->fc_value_b, e->glogp, gpi, gv,
                      static_cast<char*>(e->ws) + star_bytes, ttt_star_heads_bytes(e->max_B, e->A),
                      stream);
}
