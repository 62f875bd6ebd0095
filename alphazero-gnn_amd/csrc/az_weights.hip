// Registered parameter storage and what is cached per weight generation for weights inside it:
// the fp16 form's row scales and pre-split planes of a GEMM's W, conv2's MFMA fragment planes for
// the Connect4 trunk, and the heads composed with the Linear in front of them.  The kernels that
// fill the first three are az_gemm.hip's (launch_row_scale, launch_h3_split_rows,
// launch_c4_w2_planes); the compose kernels are here.
#include <atomic>
#include <mutex>
#include <utility>
#include <vector>

#include "az_gemm.h"

namespace az {

// W row-scale cache: weights change only between calls that say so (az_weights_changed, which
// az_adam_f32 also calls; the Python parameter store calls it on every load / copy), so a
// weight matrix's scales are computed once per weight update.  Each entry has two buffers: a
// recompute writes the other one and synchronises its stream before publishing it, so a GEMM
// launched earlier on another stream keeps reading consistent scales, and one launched later on
// any stream sees finished ones.
static std::atomic<long> g_wgen{1};
struct WScaleEntry {
  const float* w;
  int n, k, ld;
  long gen;                    // generation buf[cur] (the in-tile GEMM's row scales) is from
  float* buf[2];
  int cur;
  unsigned short* planes[2];   // the P2 GEMM's W planes [2][n][k] (nullptr until first asked)
  float* pbuf[2];              // their row scales: a double buffer of its own, so a recompute
  int pcur;                    // of one kind never overwrites the other kind's live buffer
  long pgen;                   // generation planes[pcur] / pbuf[pcur] were split at
  float* frags[2];             // conv2's fp16 fragment planes for the trunk (conv2_planes)
  int fcur;
  long fgen;
};

static std::mutex g_wmu;
static std::vector<WScaleEntry> g_wcache;

// Composed heads cache (composed_heads below): one entry per (W2, b2, fc_policy.weight / .bias,
// fc_value.weight / .bias, F, A) whose six tensors all lie in registered parameter storage, kept
// per weight generation like the planes above (double buffer, the recompute synchronises its
// stream before publishing; az_weights_unregister frees it).
struct ComposedEntry {
  const float* in[6];
  int F, A;
  float* buf[2];               // Wc [A + 1][F], then bc [A + 1]
  double* part;                // the compose kernels' fp64 partials (same allocation as buf)
  int cur;
  long gen;
};
static std::vector<ComposedEntry> g_ccache;   // under g_wmu

// the entry of (w, n, k, ld), created on first use (caller holds g_wmu); nullptr when out of memory
static WScaleEntry* wcache_entry(const float* w, int n, int k, int ld) {
  for (auto& x : g_wcache)
    if (x.w == w && x.n == n && x.k == k && x.ld == ld) return &x;
  WScaleEntry x{w, n, k, ld, 0, {nullptr, nullptr}, 1, {nullptr, nullptr}, {nullptr, nullptr},
                1, 0, {nullptr, nullptr}, 1, 0};
  if (hipMalloc(&x.buf[0], (size_t)8 * n * sizeof(float)) != hipSuccess) return nullptr;
  x.buf[1] = x.buf[0] + 2 * n;
  x.pbuf[0] = x.buf[0] + 4 * n;
  x.pbuf[1] = x.buf[0] + 6 * n;
  g_wcache.push_back(x);
  return &g_wcache.back();
}

// Parameter storage the caller registered (az_weights_register): only weights inside it are
// cached -- anywhere else a pointer says nothing about the values behind it (a freed tensor's
// memory can hold the next one), so their scales are computed per call and the pre-split planes
// are not used.
static std::mutex g_regmu;
static std::vector<std::pair<uintptr_t, uintptr_t>> g_regs;

bool weights_registered(const float* w, int n, int k, int ld) {
  const uintptr_t b = reinterpret_cast<uintptr_t>(w);
  const uintptr_t e = b + ((size_t)(n - 1) * ld + k) * sizeof(float);
  std::lock_guard<std::mutex> lk(g_regmu);
  for (const auto& r : g_regs)
    if (b >= r.first && e <= r.second) return true;
  return false;
}

}  // namespace az
extern "C" int az_weights_changed(void) {
  az::g_wgen.fetch_add(1);
  return AZ_OK;
}
extern "C" int az_weights_register(const void* base, size_t bytes) {
  AZ_REQUIRE(base && bytes > 0, AZ_EINVAL, "az_weights_register: null / empty range");
  {
    std::lock_guard<std::mutex> lk(az::g_regmu);
    const uintptr_t b = reinterpret_cast<uintptr_t>(base);
    az::g_regs.emplace_back(b, b + bytes);
  }
  return az_weights_changed();           // a reused range must not meet old cache entries
}
extern "C" int az_weights_unregister(const void* base) {
  std::vector<std::pair<uintptr_t, uintptr_t>> gone;
  {
    std::lock_guard<std::mutex> lk(az::g_regmu);
    const uintptr_t b = reinterpret_cast<uintptr_t>(base);
    for (size_t i = 0; i < az::g_regs.size();)
      if (az::g_regs[i].first == b) {
        gone.push_back(az::g_regs[i]);
        az::g_regs.erase(az::g_regs.begin() + i);
      } else {
        ++i;
      }
  }
  // free the cache entries (row scales + fp16 planes: 8 N K bytes per weight, 79 MB for a
  // 3136 x 3136 one) of weights inside the range, once no launched GEMM can still read them
  if (!gone.empty()) {
    std::lock_guard<std::mutex> lk(az::g_wmu);
    bool synced = false;
    for (size_t i = 0; i < az::g_ccache.size();) {   // composed heads with any input in the range
      bool inside = false;
      for (const float* p : az::g_ccache[i].in) {
        const uintptr_t w = reinterpret_cast<uintptr_t>(p);
        for (const auto& r : gone) inside |= w >= r.first && w < r.second;
      }
      if (!inside) {
        ++i;
        continue;
      }
      if (!synced) {
        AZ_REQUIRE(hipDeviceSynchronize() == hipSuccess, AZ_EDEVICE,
                   "az_weights_unregister: hipDeviceSynchronize failed");
        synced = true;
      }
      (void)hipFree(az::g_ccache[i].buf[0]);
      az::g_ccache.erase(az::g_ccache.begin() + i);
    }
    for (size_t i = 0; i < az::g_wcache.size();) {
      const uintptr_t w = reinterpret_cast<uintptr_t>(az::g_wcache[i].w);
      bool inside = false;
      for (const auto& r : gone) inside |= w >= r.first && w < r.second;
      if (!inside) {
        ++i;
        continue;
      }
      if (!synced) {
        AZ_REQUIRE(hipDeviceSynchronize() == hipSuccess, AZ_EDEVICE,
                   "az_weights_unregister: hipDeviceSynchronize failed");
        synced = true;
      }
      (void)hipFree(az::g_wcache[i].buf[0]);
      if (az::g_wcache[i].planes[0]) (void)hipFree(az::g_wcache[i].planes[0]);
      if (az::g_wcache[i].frags[0]) (void)hipFree(az::g_wcache[i].frags[0]);
      az::g_wcache.erase(az::g_wcache.begin() + i);
    }
  }
  return az_weights_changed();
}
namespace az {

const float* w_row_scales(const float* w, int n, int k, int ld, hipStream_t s) {
  if (!weights_registered(w, n, k, ld)) return nullptr;   // the caller computes them per call
  const long gen = g_wgen.load();
  std::lock_guard<std::mutex> lk(g_wmu);
  WScaleEntry* e = wcache_entry(w, n, k, ld);
  if (!e) return nullptr;
  if (e->gen == gen) return e->buf[e->cur];
  const int nxt = e->cur ^ 1;
  launch_row_scale(w, n, k, ld, H3_TW, e->buf[nxt], s);
  if (hipStreamSynchronize(s) != hipSuccess) return nullptr;
  e->cur = nxt;
  e->gen = gen;
  return e->buf[nxt];
}

// W's fp16 planes and scales for the P2 GEMM, cached like the scales above (two buffers, the
// recompute synchronises its stream before publishing); nullptr when memory is short.
const unsigned short* w_planes(const float* w, int n, int k, int ld, hipStream_t s,
                               const float** scales) {
  if (!weights_registered(w, n, k, ld)) return nullptr;
  const long gen = g_wgen.load();
  std::lock_guard<std::mutex> lk(g_wmu);
  WScaleEntry* e = wcache_entry(w, n, k, ld);
  if (!e) return nullptr;
  if (!e->planes[0]) {
    const size_t one = (size_t)2 * n * k;
    if (hipMalloc(&e->planes[0], 2 * one * sizeof(unsigned short)) != hipSuccess) {
      e->planes[0] = nullptr;
      return nullptr;
    }
    e->planes[1] = e->planes[0] + one;
    e->pgen = 0;
  }
  if (e->pgen == gen) {
    *scales = e->pbuf[e->pcur];
    return e->planes[e->pcur];
  }
  const int nxt = e->pcur ^ 1;
  launch_h3_split_rows(w, n, k, ld, H3_TW, e->planes[nxt], e->pbuf[nxt], s);
  if (hipStreamSynchronize(s) != hipSuccess) return nullptr;
  e->pcur = nxt;
  e->pgen = gen;
  *scales = e->pbuf[nxt];
  return e->planes[nxt];
}

// conv2_planes: the fragment planes of registered conv2 weights, cached per weight generation
// like w_planes (double buffer, the recompute synchronises its stream before publishing);
// nullptr for unregistered weights or when memory is short (the trunk then stages the weights
// through LDS and splits them itself: the same planes, the same bits).
const float* conv2_planes(const float* w2, hipStream_t s) {
  if (!weights_registered(w2, 64, 288, 288)) return nullptr;
  const long gen = g_wgen.load();
  std::lock_guard<std::mutex> lk(g_wmu);
  WScaleEntry* e = wcache_entry(w2, 64, 288, 288);
  if (!e) return nullptr;
  if (!e->frags[0]) {
    if (hipMalloc(&e->frags[0], (size_t)2 * W2P_FLOATS * sizeof(float)) != hipSuccess) {
      e->frags[0] = nullptr;
      return nullptr;
    }
    e->frags[1] = e->frags[0] + W2P_FLOATS;
    e->fgen = 0;
  }
  if (e->fgen == gen) return e->frags[e->fcur];
  const int nxt = e->fcur ^ 1;
  launch_c4_w2_planes(w2, e->frags[nxt], s);
  if (hipStreamSynchronize(s) != hipSuccess) return nullptr;
  e->fcur = nxt;
  e->fgen = gen;
  return e->frags[nxt];
}

// The heads composed with the Linear in front of them (output_transform.2 -> fc_policy /
// fc_value, no nonlinearity between: Connect4GNN.py:106-114, gnn_utils.py:115):
//   out[a][k] = sum_j Wh[a][j] W2[j][k]   (rows 0..A-1: fc_policy, row A: fc_value)
//   out[(A + 1) F + a] = sum_j Wh[a][j] b2[j] + bh[a]
// accumulated in fp64 from the fp32 inputs (each product is exact) and rounded once to fp32.
// W2 (39 MB at F = 3136) is read once, row-major, by the whole chip: block (x, y) owns columns
// 64 x .. 64 x + 63 (lane = column, coalesced rows of W2) and the y-th of COMPOSE_JB row ranges;
// wave g of its 16 sums the range's 4-row groups g, g + 16, ... in row order (the groups' head
// weights are wave-uniform 16-byte loads), the 16 wave sums are added in wave order through LDS
// and leave as fp64 partials part[y][9][F] (slot 8: the value row); compose_heads_sum_kernel adds
// the COMPOSE_JB partials in order and rounds.  A fixed summation order, no atomics.  Block
// (ceil(F / 64), 0) forms the composed biases the same way over 256 strided partial sums.
constexpr int COMPOSE_JB = 4;
__global__ __launch_bounds__(1024) void compose_heads_kernel(
    const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ wp,
    const float* __restrict__ bp, const float* __restrict__ wv, const float* __restrict__ bv,
    int F, int A, double* __restrict__ part, float* __restrict__ out) {
  __shared__ double sh[3][16][64];
  const int lane = threadIdx.x & 63;
  const int g = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if ((int)blockIdx.x == (F + 63) / 64) {       // the biases: bc = Wh b2 + bh
    if (blockIdx.y != 0) return;
    double* ps = &sh[0][0][0];                  // [9][256] partial sums, then [9][16]
    double* ps2 = ps + 9 * 256;
    const int t = threadIdx.x;
    if (t < 256) {
      double acc[9];
#pragma unroll
      for (int a = 0; a < 9; ++a) acc[a] = 0.0;
      for (int j = t; j < F; j += 256) {
        const double b = (double)b2[j];
#pragma unroll
        for (int a = 0; a < 8; ++a)
          if (a < A) acc[a] += (double)wp[(size_t)a * F + j] * b;
        acc[8] += (double)wv[j] * b;
      }
#pragma unroll
      for (int a = 0; a < 9; ++a) ps[a * 256 + t] = acc[a];
    }
    __syncthreads();
    if (t < 9 * 16) {
      const int a = t >> 4, q = t & 15;
      double s = 0.0;
      for (int i = 0; i < 16; ++i) s += ps[a * 256 + q * 16 + i];
      ps2[a * 16 + q] = s;
    }
    __syncthreads();
    if (t < 9 && (t < A || t == 8)) {
      double s = 0.0;
      for (int q = 0; q < 16; ++q) s += ps2[t * 16 + q];
      const int row = t == 8 ? A : t;
      out[(size_t)(A + 1) * F + row] = (float)(s + (double)(t == 8 ? bv[0] : bp[t]));
    }
    return;
  }
  const int k = blockIdx.x * 64 + lane;
  const bool kin = k < F;
  const int kc = kin ? k : F - 1;
  double acc[9];
#pragma unroll
  for (int a = 0; a < 9; ++a) acc[a] = 0.0;
  // the range's rows (a multiple of 4, as F is): two 4-row groups per pass, 8 rows in flight
  const int JR = ((F + COMPOSE_JB - 1) / COMPOSE_JB + 3) & ~3;
  const int j0 = blockIdx.y * JR, j1 = min(F, j0 + JR);
  auto add4 = [&](int j, const float (&x)[4]) {
    f32x4 wh[9];
#pragma unroll
    for (int a = 0; a < 8; ++a)
      wh[a] = *reinterpret_cast<const f32x4*>(wp + (size_t)min(a, A - 1) * F + j);
    wh[8] = *reinterpret_cast<const f32x4*>(wv + j);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double xd = (double)x[u];
#pragma unroll
      for (int a = 0; a < 8; ++a)
        if (a < A) acc[a] += (double)wh[a][u] * xd;
      acc[8] += (double)wh[8][u] * xd;
    }
  };
  for (int j = j0 + 4 * g; j < j1; j += 128) {
    const bool two = j + 64 < j1;
    const int jb = two ? j + 64 : j;
    float xa[4], xb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) xa[u] = w2[(size_t)(j + u) * F + kc];
#pragma unroll
    for (int u = 0; u < 4; ++u) xb[u] = w2[(size_t)(jb + u) * F + kc];
    add4(j, xa);
    if (two) add4(jb, xb);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 3; ++i) sh[i][g][lane] = acc[3 * r + i];
    __syncthreads();
    if (threadIdx.x < 192) {
      const int i = threadIdx.x >> 6, a = 3 * r + i;
      double s = 0.0;
      for (int q = 0; q < 16; ++q) s += sh[i][q][lane];
      if (kin && (a < A || a == 8)) part[((size_t)blockIdx.y * 9 + a) * F + k] = s;
    }
  }
}

// Wc = the COMPOSE_JB partials of compose_heads_kernel added in range order, rounded to fp32
__global__ __launch_bounds__(256) void compose_heads_sum_kernel(const double* __restrict__ part,
                                                                int F, int A,
                                                                float* __restrict__ out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= 9 * F) return;
  const int a = idx / F, k = idx - a * F;
  if (a >= A && a != 8) return;
  double s = 0.0;
#pragma unroll
  for (int y = 0; y < COMPOSE_JB; ++y) s += part[((size_t)y * 9 + a) * F + k];
  out[(size_t)(a == 8 ? A : a) * F + k] = (float)s;
}

// Floats of Wc [A + 1][F] + bc [A + 1], and the bytes composing them needs: that, then the fp64
// partials [COMPOSE_JB][9][F]
size_t composed_heads_floats(int F, int A) { return (size_t)(A + 1) * F + (size_t)(A + 1); }
static size_t composed_out_bytes(int F, int A) {
  return (composed_heads_floats(F, A) * sizeof(float) + 255) / 256 * 256;
}
size_t composed_heads_scratch_bytes(int F, int A) {
  return composed_out_bytes(F, A) + (size_t)COMPOSE_JB * 9 * F * sizeof(double);
}

static int launch_compose(const float* w2, const float* b2, const float* wp, const float* bp,
                          const float* wv, const float* bv, int F, int A, float* out,
                          double* part, hipStream_t s) {
  hipLaunchKernelGGL(compose_heads_kernel, dim3((F + 63) / 64 + 1, COMPOSE_JB), dim3(1024), 0, s,
                     w2, b2, wp, bp, wv, bv, F, A, part, out);
  hipLaunchKernelGGL(compose_heads_sum_kernel, dim3((9 * F + 255) / 256), dim3(256), 0, s, part, F,
                     A, out);
  return check_launch("compose_heads_kernel");
}

// Wc [A + 1][F] followed by bc [A + 1] for heads (wp, bp, wv, bv) behind y = x W2^T + b2
// (A <= 8, F % 4 == 0, wp / wv 16-byte aligned): the cached copy when every input is registered,
// else composed into `scratch` (composed_heads_scratch_bytes(F, A) bytes of the caller's
// workspace, 256-byte aligned) on the caller's stream -- the same kernels either way, so the
// same bits.  nullptr: a launch failed.

const float* composed_heads(const float* w2, const float* b2, const float* wp, const float* bp,
                            const float* wv, const float* bv, int F, int A, float* scratch,
                            hipStream_t s) {
  const bool reg = weights_registered(w2, F, F, F) && weights_registered(b2, 1, F, F) &&
                   weights_registered(wp, A, F, F) && weights_registered(bp, 1, A, A) &&
                   weights_registered(wv, 1, F, F) && weights_registered(bv, 1, 1, 1);
  if (reg) {
    const long gen = g_wgen.load();
    std::lock_guard<std::mutex> lk(g_wmu);
    ComposedEntry* e = nullptr;
    for (auto& x : g_ccache)
      if (x.in[0] == w2 && x.in[1] == b2 && x.in[2] == wp && x.in[3] == bp && x.in[4] == wv &&
          x.in[5] == bv && x.F == F && x.A == A)
        e = &x;
    if (!e) {
      // one allocation: the two Wc / bc buffers, then the partials (used only while a recompute
      // runs, which ends before g_wmu is released)
      ComposedEntry x{{w2, b2, wp, bp, wv, bv}, F, A, {nullptr, nullptr}, nullptr, 1, 0};
      const size_t one = composed_out_bytes(F, A);
      char* base = nullptr;
      if (hipMalloc(&base, one + composed_heads_scratch_bytes(F, A)) == hipSuccess) {
        x.buf[0] = reinterpret_cast<float*>(base);
        x.buf[1] = reinterpret_cast<float*>(base + one);
        x.part = reinterpret_cast<double*>(base + 2 * one);
        g_ccache.push_back(x);
        e = &g_ccache.back();
      }
    }
    if (e) {
      if (e->gen == gen) return e->buf[e->cur];
      const int nxt = e->cur ^ 1;
      if (launch_compose(w2, b2, wp, bp, wv, bv, F, A, e->buf[nxt], e->part, s) ||
          hipStreamSynchronize(s) != hipSuccess)
        return nullptr;
      e->cur = nxt;
      e->gen = gen;
      return e->buf[nxt];
    }
  }
  double* part = reinterpret_cast<double*>(reinterpret_cast<char*>(scratch) +
                                           composed_out_bytes(F, A));
  return launch_compose(w2, b2, wp, bp, wv, bv, F, A, scratch, part, s) ? nullptr : scratch;
}

}  // namespace az
