// Loss metrics of a batch of network outputs against their targets (az_policy_value_metrics):
// policy cross-entropy, value squared error, top-1 agreement, policy entropy, target entropy and
// the row count, summed over the rows into six doubles on the device.
//
// A row is at most 32 floats, so a half-wave owns a row: lane a of the half holds element a, the
// row's four fp32 terms and its two argmaxes are reduced over the 32 lanes with xor exchanges
// (16, 8, 4, 2, 1: never across the halves), and lane 0 of the half adds them to its fp64 sums.
// No atomics anywhere: a block's 8 half-waves take rows in a fixed order, the block's sums go to
// its slot of the workspace, and a second one-block launch adds the slots in block order (thread
// t takes slots t, t + 256, ..., then a fixed tree), the pattern of az_clip_grad_norm.
#include <float.h>
#include <math.h>

#include "az_common.h"

namespace az {

constexpr int MET_THREADS = 256;             // 8 half-waves
constexpr int MET_HALVES = MET_THREADS / 32;
constexpr int MET_ROWS = 64;                 // rows per block: 8 passes of 8 rows
constexpr int MET_N = AZ_METRICS_N;

// a + (a of lane ^ m) within the half-wave, every lane active
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
  for (int m = 16; m > 0; m >>= 1) v += __shfl_xor(v, m, 32);
  return v;
}

// index of the largest value over the half-wave; ties go to the lowest index
__device__ __forceinline__ int half_argmax(float v, int idx) {
#pragma unroll
  for (int m = 16; m > 0; m >>= 1) {
    const float ov = __shfl_xor(v, m, 32);
    const int oi = __shfl_xor(idx, m, 32);
    if (ov > v || (ov == v && oi < idx)) {
      v = ov;
      idx = oi;
    }
  }
  return idx;
}

__global__ __launch_bounds__(MET_THREADS) void metrics_rows_kernel(
    const float* __restrict__ p, int ldp, int is_log, const float* __restrict__ v,
    const float* __restrict__ tpi, const float* __restrict__ tv, int B, int A,
    double* __restrict__ part) {
  __shared__ double sums[MET_HALVES][MET_N];
  const int a = threadIdx.x & 31, h = threadIdx.x >> 5;
  const float log_min = logf(FLT_MIN);
  double ce = 0.0, se = 0.0, top = 0.0, ent = 0.0, tent = 0.0, cnt = 0.0;
  const long row0 = (long)blockIdx.x * MET_ROWS;
  for (int i = 0; i < MET_ROWS / MET_HALVES; ++i) {
    const long row = row0 + i * MET_HALVES + h;      // uniform over the half-wave
    const bool on = row < B && a < A;
    const float x = on ? p[row * ldp + a] : 0.f;
    const float t = on ? tpi[row * A + a] : 0.f;
    // log p, never below log(FLT_MIN): p == 0 under a positive target is a finite term
    const float lp = fmaxf(is_log ? x : logf(fmaxf(x, FLT_MIN)), log_min);
    const float pr = is_log ? expf(x) : x;
    const float f_ce = (on && t != 0.f) ? -t * lp : 0.f;          // t == 0: exactly 0
    const float f_ent = (on && pr > 0.f) ? -pr * lp : 0.f;
    const float f_tent = (on && t > 0.f) ? -t * logf(t) : 0.f;
    const float r_ce = half_sum(f_ce), r_ent = half_sum(f_ent), r_tent = half_sum(f_tent);
    const float ninf = -INFINITY;
    const int am_p = half_argmax(on ? x : ninf, a);
    const int am_t = half_argmax(on ? t : ninf, a);
    if (a == 0 && row < B) {
      const float d = tv[row] - v[row];
      ce += (double)r_ce;
      se += (double)(d * d);
      top += am_p == am_t ? 1.0 : 0.0;
      ent += (double)r_ent;
      tent += (double)r_tent;
      cnt += 1.0;
    }
  }
  if (a == 0) {
    sums[h][AZ_METRICS_CE] = ce;
    sums[h][AZ_METRICS_SE] = se;
    sums[h][AZ_METRICS_TOP1] = top;
    sums[h][AZ_METRICS_ENT] = ent;
    sums[h][AZ_METRICS_TENT] = tent;
    sums[h][AZ_METRICS_ROWS] = cnt;
  }
  __syncthreads();
  if (threadIdx.x < MET_N) {
    double s = 0.0;
    for (int k = 0; k < MET_HALVES; ++k) s += sums[k][threadIdx.x];
    part[(size_t)blockIdx.x * MET_N + threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(MET_THREADS) void metrics_finish_kernel(
    const double* __restrict__ part, int blocks, double* __restrict__ acc, int accumulate) {
  __shared__ double tree[MET_THREADS];
  const int t = threadIdx.x;
  for (int q = 0; q < MET_N; ++q) {
    double s = 0.0;
    for (int b = t; b < blocks; b += MET_THREADS) s += part[(size_t)b * MET_N + q];
    tree[t] = s;
    __syncthreads();
    for (int half = MET_THREADS / 2; half > 0; half >>= 1) {
      if (t < half) tree[t] += tree[t + half];
      __syncthreads();
    }
    if (t == 0) acc[q] = accumulate ? acc[q] + tree[0] : tree[0];
    __syncthreads();
  }
}

static long metrics_blocks(int B) { return ((long)B + MET_ROWS - 1) / MET_ROWS; }

}  // namespace az

using namespace az;

extern "C" size_t az_policy_value_metrics_ws_bytes(int B, int A) {
  if (B < 0 || A < 1 || A > 32) return 0;
  return (size_t)metrics_blocks(B) * MET_N * sizeof(double);
}

extern "C" int az_policy_value_metrics(const float* p, int ldp, int is_log, const float* v,
                                       const float* target_pi, const float* target_v, int B, int A,
                                       double* acc, int accumulate, void* ws, void* stream) {
  AZ_REQUIRE(B >= 0 && A >= 1 && A <= 32, AZ_EINVAL,
             "az_policy_value_metrics: bad shape B=%d A=%d (B >= 0, A in 1..32)", B, A);
  AZ_REQUIRE(ldp >= A, AZ_EINVAL, "az_policy_value_metrics: ldp=%d < A=%d", ldp, A);
  AZ_REQUIRE(is_log == 0 || is_log == 1, AZ_EINVAL, "az_policy_value_metrics: is_log=%d", is_log);
  AZ_REQUIRE(acc && ((uintptr_t)acc & 7u) == 0, AZ_EINVAL,
             "az_policy_value_metrics: acc is null or not 8-byte aligned");
  AZ_REQUIRE(B == 0 || (p && v && target_pi && target_v), AZ_EINVAL,
             "az_policy_value_metrics: null input");
  AZ_REQUIRE(B == 0 || (ws && ((uintptr_t)ws & 7u) == 0), AZ_EINVAL,
             "az_policy_value_metrics: ws is null or not 8-byte aligned "
             "(az_policy_value_metrics_ws_bytes)");
  if (B == 0 && accumulate) return AZ_OK;
  hipStream_t s = as_stream(stream);
  const int blocks = (int)metrics_blocks(B);
  double* part = static_cast<double*>(ws);
  if (B > 0) {
    hipLaunchKernelGGL(metrics_rows_kernel, dim3(blocks), dim3(MET_THREADS), 0, s, p, ldp, is_log,
                       v, target_pi, target_v, B, A, part);
    if (int rc = check_launch("metrics_rows_kernel")) return rc;
  }
  hipLaunchKernelGGL(metrics_finish_kernel, dim3(1), dim3(MET_THREADS), 0, s, part, blocks, acc,
                     accumulate ? 1 : 0);
  return check_launch("metrics_finish_kernel");
}
