// FrozenLakeNet (frozenlake/FrozenLakeNet.py:253-335): the one-launch leaf evaluator
// az_fl_eval_fwd, the gradients of train()'s loss az_fl_grads, and az_clip_grad_norm.
//
// A leaf is n = 1..5 node boards.  Under the all-ones normalised adjacency every GNN layer gives
// every node the same row, so the network collapses to (az_hip.h has the formulas)
//   h_j = relu(fe2 relu(fe0 x_j));  r_0 = sum_j h_j;  r_1 = relu(c (W_1 r_0 + n b_1));
//   r_l = relu(c n (W_l r_{l-1} + b_l));  pi = softmax(P r_L);  v = tanh(V r_L)
// which is the same function of the parameters, so its derivative is the reference's gradient.
// The working set of a leaf (5 nodes x 128 floats at most) lives in LDS; one workgroup of 128
// threads per leaf, one thread per output of a layer, each output a fixed-order fmaf chain.
#include <algorithm>

#include "az_common.h"

namespace az {

constexpr int FL_THREADS = 128;
constexpr int FL_NODES = AZ_FL_MAX_NODES;
constexpr int FL_H = AZ_FL_HIDDEN;
constexpr int FL_MAXS = 64;
constexpr int FL_MAXE = 128;
constexpr int FL_A = 4;
constexpr float FL_PI_MIN = 1e-8f;     // out_pi.clamp(min=1e-8), FrozenLakeNet.py:158

// fp32(n^-1/2), n = 0..5 (torch.pow(rowsum, -0.5) of FrozenLakeNet.create_adjacency)
__device__ const float FL_DINV[FL_NODES + 1] = {1.f, 1.f, 0.70710677f, 0.57735026f, 0.5f,
                                                0.4472136f};

struct FlLds {
  float x[FL_NODES][FL_MAXS];                    // the node boards
  float h1[FL_NODES][FL_H];                      // relu(fe0 x_j)
  float h2[FL_NODES][FL_MAXE];                   // relu(fe2 h1_j)
  float r[AZ_FL_MAX_LAYERS + 1][FL_MAXE];        // r[0] = sum_j h2_j, r[l] = GNN layer l's row
  float z[8];                                    // logits 0..3, value pre-activation at 4
  float out[8];                                  // pi 0..3, v at 4
};

__device__ __forceinline__ int fl_count(const int* counts, int b) {
  return min(max(counts[b], 1), FL_NODES);
}

// w . x for a 16-byte aligned weight row and an LDS vector, K % 4 == 0: four chains over k mod 4,
// combined (p0 + p1) + (p2 + p3)
__device__ __forceinline__ float fl_dot(const float* __restrict__ w, const float* x, int K) {
  float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
  for (int k = 0; k < K; k += 4) {
    const f32x4 wv = *reinterpret_cast<const f32x4*>(w + k);
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + k);
    p0 = fmaf(wv[0], xv[0], p0);
    p1 = fmaf(wv[1], xv[1], p1);
    p2 = fmaf(wv[2], xv[2], p2);
    p3 = fmaf(wv[3], xv[3], p3);
  }
  return (p0 + p1) + (p2 + p3);
}

// sum_o W[o][t] d[o] (a column of W against an LDS vector), O % 4 == 0, chains over o mod 4
__device__ __forceinline__ float fl_dot_col(const float* __restrict__ w, int ld, int t,
                                            const float* d, int O) {
  float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
  for (int o = 0; o < O; o += 4) {
    p0 = fmaf(w[(size_t)(o + 0) * ld + t], d[o + 0], p0);
    p1 = fmaf(w[(size_t)(o + 1) * ld + t], d[o + 1], p1);
    p2 = fmaf(w[(size_t)(o + 2) * ld + t], d[o + 2], p2);
    p3 = fmaf(w[(size_t)(o + 3) * ld + t], d[o + 3], p3);
  }
  return (p0 + p1) + (p2 + p3);
}

// The forward pass of one leaf into LDS.  nodes: this leaf's [5][S] rows, of which the first n
// are read.  Ends with a barrier: s.out holds pi and v for every thread.
__device__ void fl_forward(const az_fl_eval& e, const float* __restrict__ nodes, int n, FlLds& s) {
  const int t = threadIdx.x, S = e.S, E = e.E, L = e.L;
  const az_fl_params& w = e.w;
  for (int i = t; i < n * S; i += FL_THREADS) s.x[i / S][i % S] = nodes[i];
  __syncthreads();
  {   // feature_extractor.0: thread t owns hidden unit t of every node
    float acc[FL_NODES] = {0.f, 0.f, 0.f, 0.f, 0.f};
    const float* wr = w.fe0_w + (size_t)t * S;
    for (int k = 0; k < S; ++k) {
      const float wk = wr[k];
#pragma unroll
      for (int j = 0; j < FL_NODES; ++j)
        if (j < n) acc[j] = fmaf(wk, s.x[j][k], acc[j]);
    }
    const float b = w.fe0_b[t];
#pragma unroll
    for (int j = 0; j < FL_NODES; ++j)
      if (j < n) s.h1[j][t] = fmaxf(acc[j] + b, 0.f);
  }
  __syncthreads();
  if (t < E) {   // feature_extractor.2, then the node sum
    const float* wr = w.fe2_w + (size_t)t * FL_H;
    const float b = w.fe2_b[t];
    float sum = 0.f;
    for (int j = 0; j < n; ++j) {
      const float h = fmaxf(fl_dot(wr, s.h1[j], FL_H) + b, 0.f);
      s.h2[j][t] = h;
      sum += h;
    }
    s.r[0][t] = sum;
  }
  __syncthreads();
  const float d = FL_DINV[n], c = d * d, cn = c * (float)n;
  for (int l = 1; l <= L; ++l) {
    if (t < E) {
      const float dot = fl_dot(w.gnn_w[l - 1] + (size_t)t * E, s.r[l - 1], E);
      const float b = w.gnn_b[l - 1][t];
      const float a = l == 1 ? c * fmaf((float)n, b, dot) : cn * (dot + b);
      s.r[l][t] = fmaxf(a, 0.f);
    }
    __syncthreads();
  }
  if (t < FL_A) s.z[t] = fl_dot(w.policy_w + (size_t)t * E, s.r[L], E) + w.policy_b[t];
  if (t == FL_A) s.z[FL_A] = fl_dot(w.value_w, s.r[L], E) + w.value_b[0];
  __syncthreads();
  if (t == 0) {
    const float m = fmaxf(fmaxf(s.z[0], s.z[1]), fmaxf(s.z[2], s.z[3]));
    float ex[FL_A], sum = 0.f;
#pragma unroll
    for (int a = 0; a < FL_A; ++a) {
      ex[a] = expf(s.z[a] - m);
      sum += ex[a];
    }
#pragma unroll
    for (int a = 0; a < FL_A; ++a) s.out[a] = ex[a] / sum;
    s.out[FL_A] = tanhf(s.z[FL_A]);
  }
  __syncthreads();
}

__global__ __launch_bounds__(FL_THREADS) void fl_eval_kernel(az_fl_eval e,
                                                             const float* __restrict__ nodes,
                                                             const int* __restrict__ counts,
                                                             float* __restrict__ pi,
                                                             float* __restrict__ v) {
  __shared__ __attribute__((aligned(16))) FlLds s;
  const size_t b = blockIdx.x;
  fl_forward(e, nodes + b * FL_NODES * e.S, fl_count(counts, b), s);
  if (threadIdx.x < FL_A) pi[b * FL_A + threadIdx.x] = s.out[threadIdx.x];
  if (threadIdx.x == FL_A) v[b] = s.out[FL_A];
}

// Where az_fl_grads keeps a batch's saved activations and layer deltas (floats, B leaves)
struct FlWs {
  float* rin;     // [L + 1][B][E]: the input row of GNN layer l + 1; [L] is the heads' input
  float* ds;      // [L][B][E]: dloss / d(W_l r + b_l)
  float* dhead;   // [B][8]: dloss / dlogits 0..3, dloss / d(value pre-activation) at 4
  float* h1;      // [B][5][128]
  float* dz1;     // [B][5][128]: dloss / d(fe0 x_j + b)
  float* dz2;     // [B][5][E]:   dloss / d(fe2 h1_j + b)
  float* lossb;   // [B][2]: -sum_a tpi log(max(pi, 1e-8)),  (v - tv)^2
};

static size_t fl_ws_floats(int B, int E, int L) {
  return (size_t)B * ((size_t)(2 * L + 1) * E + 8 + 2 * FL_NODES * FL_H + FL_NODES * E + 2);
}

static FlWs fl_ws_layout(float* p, int B, int E, int L) {
  FlWs w;
  w.rin = p;    p += (size_t)(L + 1) * B * E;
  w.ds = p;     p += (size_t)L * B * E;
  w.dhead = p;  p += (size_t)B * 8;
  w.h1 = p;     p += (size_t)B * FL_NODES * FL_H;
  w.dz1 = p;    p += (size_t)B * FL_NODES * FL_H;
  w.dz2 = p;    p += (size_t)B * FL_NODES * E;
  w.lossb = p;
  return w;
}

// Forward, then backward down to the pre-activation delta of every linear layer, for ONE leaf per
// workgroup.  The softmax-clamp-log and MSE backward, the tanh backward and the backward of the
// node aggregation (every node receives the gradient of the sum) happen here; the weight
// gradients are fl_wgrad_kernel's.
__global__ __launch_bounds__(FL_THREADS) void fl_bwd_kernel(az_fl_eval e,
                                                            const float* __restrict__ nodes,
                                                            const int* __restrict__ counts, int B,
                                                            const float* __restrict__ tpi,
                                                            const float* __restrict__ tv, FlWs ws,
                                                            float* __restrict__ dlogits) {
  __shared__ __attribute__((aligned(16))) FlLds s;
  __shared__ float dr[2][FL_MAXE];                // gradient of the current row, ping-pong
  __shared__ float dsv[FL_MAXE];
  __shared__ float dz2[FL_NODES][FL_MAXE];
  __shared__ float dh[8];
  const int t = threadIdx.x, E = e.E, L = e.L;
  const size_t b = blockIdx.x;
  const int n = fl_count(counts, b);
  const az_fl_params& w = e.w;
  fl_forward(e, nodes + b * FL_NODES * e.S, n, s);
  if (t == 0) {
    const float invB = 1.f / (float)B;
    float g[FL_A], lp = 0.f, gp = 0.f;
#pragma unroll
    for (int a = 0; a < FL_A; ++a) {
      const float p = s.out[a], q = tpi[b * FL_A + a];
      lp = fmaf(q, logf(fmaxf(p, FL_PI_MIN)), lp);
      g[a] = p >= FL_PI_MIN ? -(q / p) * invB : 0.f;     // the clamp passes nothing below min
      gp = fmaf(g[a], p, gp);
    }
#pragma unroll
    for (int a = 0; a < FL_A; ++a) dh[a] = s.out[a] * (g[a] - gp);   // softmax backward
    // MSE, then tanh backward, from the pre-activation u: with ex = exp(-2|u|),
    // tanh u = sgn (1 - 2 ex / (1 + ex)) and 1 - tanh^2 u = 4 ex / (1 + ex)^2, which keep their
    // relative precision where tanh saturates (1 - v * v and v - 1 cancel there)
    const float u = s.z[FL_A], sgn = u >= 0.f ? 1.f : -1.f, ex = expf(-2.f * fabsf(u));
    const float dv = (sgn - tv[b]) - sgn * (2.f * ex / (1.f + ex));
    dh[FL_A] = 2.f * dv * invB * (4.f * ex / ((1.f + ex) * (1.f + ex)));
    ws.lossb[b * 2] = -lp;
    ws.lossb[b * 2 + 1] = dv * dv;
  }
  __syncthreads();
  if (t < 8) ws.dhead[b * 8 + t] = t <= FL_A ? dh[t] : 0.f;
  if (dlogits && t < FL_A) dlogits[b * FL_A + t] = dh[t];
  int cur = 0;
  if (t < E) {
    float a = w.value_w[t] * dh[FL_A];
#pragma unroll
    for (int k = 0; k < FL_A; ++k) a = fmaf(w.policy_w[(size_t)k * E + t], dh[k], a);
    dr[0][t] = a;
    ws.rin[((size_t)L * B + b) * E + t] = s.r[L][t];
  }
  __syncthreads();
  const float d = FL_DINV[n], c = d * d, cn = c * (float)n;
  for (int l = L; l >= 1; --l) {
    if (t < E) {
      const float da = s.r[l][t] > 0.f ? dr[cur][t] : 0.f;
      const float x = (l == 1 ? c : cn) * da;
      dsv[t] = x;
      ws.ds[((size_t)(l - 1) * B + b) * E + t] = x;
      ws.rin[((size_t)(l - 1) * B + b) * E + t] = s.r[l - 1][t];
    }
    __syncthreads();
    if (t < E) dr[cur ^ 1][t] = fl_dot_col(w.gnn_w[l - 1], E, t, dsv, E);
    __syncthreads();
    cur ^= 1;
  }
  // dr[cur] is the gradient of the node sum: every node's h2 row receives it
  for (int j = 0; j < n; ++j) {
    if (t < E) {
      const float x = s.h2[j][t] > 0.f ? dr[cur][t] : 0.f;
      dz2[j][t] = x;
      ws.dz2[(b * FL_NODES + j) * E + t] = x;
    }
    ws.h1[(b * FL_NODES + j) * FL_H + t] = s.h1[j][t];
  }
  __syncthreads();
  for (int j = 0; j < n; ++j) {
    const float x = fl_dot_col(w.fe2_w, FL_H, t, dz2[j], E);
    ws.dz1[(b * FL_NODES + j) * FL_H + t] = s.h1[j][t] > 0.f ? x : 0.f;
  }
}

// One weight tensor's gradient: gw[o][k] = sum over leaves b (in order) and their rows j of
// dz[b][j][o] in[b][j][k];  gb[o] = sum dz[b][j][o] (times n_b for GNN layer 1, whose bias
// enters once per node)
struct FlWJob {
  const float* dz; const float* in; float* gw; float* gb;
  int O, K;
  int ldz;         // floats between rows of dz (O, or 8 for the heads' shared [B][8] rows)
  int R;           // rows per leaf in dz / in: 5 (per-node layers, counts[b] of them valid) or 1
  int bias_by_n;
};
constexpr int FL_MAX_JOBS = AZ_FL_MAX_LAYERS + 4;
struct FlWJobs { FlWJob job[FL_MAX_JOBS]; int n; };

__global__ __launch_bounds__(256) void fl_wgrad_kernel(FlWJobs jobs, const int* __restrict__ counts,
                                                       int B, const float* __restrict__ lossb,
                                                       float* __restrict__ loss) {
  if ((int)blockIdx.y == jobs.n) {   // the loss: the mean over leaves of each term, in leaf order
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      float lp = 0.f, lv = 0.f;
      for (int b = 0; b < B; ++b) {
        lp += lossb[b * 2];
        lv += lossb[b * 2 + 1];
      }
      *loss = lp / (float)B + lv / (float)B;
    }
    return;
  }
  const FlWJob& J = jobs.job[blockIdx.y];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= J.O * J.K) return;
  const int o = idx / J.K, k = idx % J.K;
  float acc = 0.f;
  for (int b = 0; b < B; ++b) {
    const int rows = J.R == 1 ? 1 : fl_count(counts, b);
    for (int j = 0; j < rows; ++j) {
      const size_t row = (size_t)b * J.R + j;
      acc = fmaf(J.dz[row * J.ldz + o], J.in[row * J.K + k], acc);
    }
  }
  J.gw[idx] = acc;
  if (idx < J.O) {   // the first O threads also own a bias element each
    float ab = 0.f;
    for (int b = 0; b < B; ++b) {
      const int nb = fl_count(counts, b);
      const int rows = J.R == 1 ? 1 : nb;
      const float scale = J.bias_by_n ? (float)nb : 1.f;
      for (int j = 0; j < rows; ++j) ab = fmaf(J.dz[((size_t)b * J.R + j) * J.ldz + idx], scale, ab);
    }
    J.gb[idx] = ab;
  }
}

constexpr int CLIP_MAX_BUFS = 16;
constexpr int CLIP_THREADS = 1024;
struct ClipBufs { float* p[CLIP_MAX_BUFS]; long n[CLIP_MAX_BUFS]; int count; };

// sqrt of the sum of squares of every buffer: thread t takes elements t, t + 1024, ... of each
// buffer in buffer order, fp64 throughout, then a fixed tree over the 1,024 partial sums
__global__ __launch_bounds__(CLIP_THREADS) void clip_norm_kernel(ClipBufs bufs,
                                                                 float* __restrict__ total_norm) {
  __shared__ double part[CLIP_THREADS];
  const int t = threadIdx.x;
  double acc = 0.0;
  for (int i = 0; i < bufs.count; ++i)
    for (long k = t; k < bufs.n[i]; k += CLIP_THREADS) {
      const double x = (double)bufs.p[i][k];
      acc = fma(x, x, acc);
    }
  part[t] = acc;
  __syncthreads();
  for (int h = CLIP_THREADS / 2; h > 0; h >>= 1) {
    if (t < h) part[t] += part[t + h];
    __syncthreads();
  }
  if (t == 0) *total_norm = (float)sqrt(part[0]);
}

__global__ __launch_bounds__(256) void clip_scale_kernel(ClipBufs bufs, float max_norm,
                                                         const float* __restrict__ total_norm) {
  const float coef = fminf(max_norm / (*total_norm + 1e-6f), 1.f);
  float* p = bufs.p[blockIdx.y];
  const long n = bufs.n[blockIdx.y];
  for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < n; k += (long)gridDim.x * 256)
    p[k] *= coef;
}

static bool fl_params_ok(const az_fl_params& p, int L) {
  bool ok = p.fe0_w && p.fe0_b && p.fe2_w && p.fe2_b && p.policy_w && p.policy_b && p.value_w &&
            p.value_b;
  for (int l = 0; l < L; ++l) ok = ok && p.gnn_w[l] && p.gnn_b[l];
  return ok;
}

static bool fl_shape_ok(int S, int E, int L) {
  return S >= 4 && S <= FL_MAXS && (E == 64 || E == 128) && L >= 1 && L <= AZ_FL_MAX_LAYERS;
}
}  // namespace az

using namespace az;

// The checks az_fl_eval_fwd and az_fl_grads share; `fn` names the caller in the message.
static int fl_check(const char* fn, const az_fl_eval* e, const float* nodes, const int* counts,
                    int B) {
  AZ_REQUIRE(e != nullptr, AZ_EINVAL, "%s: null descriptor", fn);
  AZ_REQUIRE(B >= 1 && B <= e->max_B, AZ_EINVAL, "%s: B=%d max_B=%d", fn, B, e->max_B);
  AZ_REQUIRE(fl_shape_ok(e->S, e->E, e->L) && e->A == FL_A && e->H == FL_H, AZ_EINVAL,
             "%s: bad shape S=%d E=%d L=%d A=%d H=%d (S in 4..64, E 64 or 128, L in 1..4, A = 4, "
             "H = 128)", fn, e->S, e->E, e->L, e->A, e->H);
  AZ_REQUIRE(counts != nullptr, AZ_EINVAL, "%s: null counts", fn);
  AZ_REQUIRE(nodes && fl_params_ok(e->w, e->L), AZ_EINVAL, "%s: null nodes / weight pointer", fn);
  bool al = aligned16(e->w.fe2_w) && aligned16(e->w.policy_w) && aligned16(e->w.value_w);
  for (int l = 0; l < e->L; ++l) al = al && aligned16(e->w.gnn_w[l]);
  AZ_REQUIRE(al, AZ_EINVAL, "%s: fe2 / gnn / head weights need 16B alignment", fn);
  return AZ_OK;
}

extern "C" size_t az_fl_eval_ws_bytes(int max_B, int S, int E, int L) {
  if (max_B < 1 || !fl_shape_ok(S, E, L)) return 0;
  return fl_ws_floats(max_B, E, L) * sizeof(float);
}

extern "C" int az_fl_eval_fwd(const az_fl_eval* e, const float* nodes, const int* counts, int B,
                              float* pi, float* v, void* ws, void* stream) {
  (void)ws;
  if (int rc = fl_check("az_fl_eval_fwd", e, nodes, counts, B)) return rc;
  AZ_REQUIRE(pi && v, AZ_EINVAL, "az_fl_eval_fwd: null pi / v");
  hipLaunchKernelGGL(fl_eval_kernel, dim3(B), dim3(FL_THREADS), 0, as_stream(stream), *e, nodes,
                     counts, pi, v);
  return check_launch("fl_eval_kernel");
}

extern "C" int az_fl_grads(const az_fl_eval* e, const float* nodes, const int* counts, int B,
                           const float* target_pi, const float* target_v, const az_fl_params* g,
                           float* loss, float* dlogits, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = fl_check("az_fl_grads", e, nodes, counts, B)) return rc;
  AZ_REQUIRE(target_pi && target_v && loss, AZ_EINVAL, "az_fl_grads: null targets / loss");
  AZ_REQUIRE(g && fl_params_ok(*g, e->L), AZ_EINVAL, "az_fl_grads: null gradient pointer");
  AZ_REQUIRE(ws && ws_bytes >= az_fl_eval_ws_bytes(e->max_B, e->S, e->E, e->L), AZ_EINVAL,
             "az_fl_grads: workspace null or too small (az_fl_eval_ws_bytes)");
  const int S = e->S, E = e->E, L = e->L;
  hipStream_t s = as_stream(stream);
  const FlWs w = fl_ws_layout(static_cast<float*>(ws), B, E, L);
  hipLaunchKernelGGL(fl_bwd_kernel, dim3(B), dim3(FL_THREADS), 0, s, *e, nodes, counts, B,
                     target_pi, target_v, w, dlogits);
  if (int rc = check_launch("fl_bwd_kernel")) return rc;
  FlWJobs jobs = {};
  int nj = 0, most = 0;
  auto add = [&](const float* dz, int ldz, const float* in, float* gw, float* gb, int O, int K,
                 int R, int bias_by_n) {
    jobs.job[nj++] = FlWJob{dz, in, gw, gb, O, K, ldz, R, bias_by_n};
    most = std::max(most, O * K);
  };
  add(w.dz1, FL_H, nodes, g->fe0_w, g->fe0_b, FL_H, S, FL_NODES, 0);
  add(w.dz2, E, w.h1, g->fe2_w, g->fe2_b, E, FL_H, FL_NODES, 0);
  for (int l = 0; l < L; ++l)
    add(w.ds + (size_t)l * B * E, E, w.rin + (size_t)l * B * E, g->gnn_w[l], g->gnn_b[l], E, E, 1,
        l == 0);
  const float* rL = w.rin + (size_t)L * B * E;
  add(w.dhead, 8, rL, g->policy_w, g->policy_b, FL_A, E, 1, 0);
  add(w.dhead + FL_A, 8, rL, g->value_w, g->value_b, 1, E, 1, 0);
  jobs.n = nj;
  // row nj of the grid is the loss
  hipLaunchKernelGGL(fl_wgrad_kernel, dim3((most + 255) / 256, nj + 1), dim3(256), 0, s, jobs,
                     counts, B, w.lossb, loss);
  return check_launch("fl_wgrad_kernel");
}

extern "C" int az_clip_grad_norm(float* const* bufs, const int64_t* sizes, int n, float max_norm,
                                 float* total_norm, void* stream) {
  AZ_REQUIRE(n >= 1 && n <= CLIP_MAX_BUFS, AZ_EINVAL, "az_clip_grad_norm: n=%d buffers (1..%d)", n,
             CLIP_MAX_BUFS);
  AZ_REQUIRE(bufs && sizes && total_norm, AZ_EINVAL, "az_clip_grad_norm: null pointer");
  AZ_REQUIRE(max_norm > 0.f, AZ_EINVAL, "az_clip_grad_norm: max_norm=%g", (double)max_norm);
  ClipBufs cb = {};
  long most = 1;
  for (int i = 0; i < n; ++i) {
    AZ_REQUIRE(sizes[i] >= 0 && (bufs[i] || sizes[i] == 0), AZ_EINVAL,
               "az_clip_grad_norm: buffer %d is null or has a negative size", i);
    cb.p[i] = bufs[i];
    cb.n[i] = (long)sizes[i];
    most = std::max(most, cb.n[i]);
  }
  cb.count = n;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(clip_norm_kernel, dim3(1), dim3(CLIP_THREADS), 0, s, cb, total_norm);
  if (int rc = check_launch("clip_norm_kernel")) return rc;
  const long blocks = std::min<long>((most + 255) / 256, 1024);
  hipLaunchKernelGGL(clip_scale_kernel, dim3(blocks, n), dim3(256), 0, s, cb, max_norm, total_norm);
  return check_launch("clip_scale_kernel");
}
