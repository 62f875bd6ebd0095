// The exact GEMM's epilogues for the GNN node update (az_gemm_exact_ex), each applied
// after "segment sums in ascending order, then bias" of az_gemm_exact.h's contract:
//   AZ_ACT_SIGMOID     sigmoidf_ref(v), the function the other star kernels use
//   gated residual     C = fmaf(G, v, R), one rounding, no activation
//   the paired launch  two weight matrices [N][K], two biases, two activations and two outputs on
//                      ONE A operand: grid.x covers the 2 ceil(N / 64) column tiles and a block
//                      picks its product by tile index.  The plan is exact_plan(N, K) of one
//                      product, so each output has the bits of two separate calls; in the spread
//                      form each product has its own slabs and one reduce launch serves both.
// This unit instantiates gemm_exact_kernel<1|2|4, ExactEpiEx> and
// gemm_exact_reduce_kernel<ExactEpiEx>; the plain forms stay in az_gemm_exact.hip.
#include "az_gemm_exact.h"

namespace az {

struct ExactEpiEx {
  using Args = ExactArgsEx;
  static __device__ __forceinline__ ExactSel pick(const Args& p, bool second, int n0) {
    if (second) return {n0, p.W2, p.bias2, p.act2, p.C2, p.slab2};
    return {n0, p.W, p.bias, p.act, p.C, p.slab};
  }
  static __device__ __forceinline__ ExactSel select(const Args& p, int tile) {
    const bool second = tile >= p.nt;             // block-uniform
    return pick(p, second, (second ? tile - p.nt : tile) * EX_BN);
  }
  static __device__ __forceinline__ int products(const Args& p) { return p.W2 ? 2 : 1; }
  static __device__ __forceinline__ ExactSel reduce_select(const Args& p, size_t& e) {
    const size_t one = (size_t)p.M * (p.N >> 2);
    const bool second = e >= one;
    if (second) e -= one;
    return pick(p, second, 0);
  }
  static __device__ __forceinline__ float apply(const Args& p, const ExactSel& s, float v, int row,
                                                int col) {
    if (p.G)   // an explicit fmaf: G * v is not rounded before R is added
      return fmaf(p.G[(size_t)row * p.ldg + col], v, p.R[(size_t)row * p.ldr + col]);
    if (s.act == AZ_ACT_RELU) return v > 0.f ? v : 0.f;
    if (s.act == AZ_ACT_SIGMOID) return sigmoidf_ref(v);
    return v;
  }
};

int gemm_exact_ex(ExactArgsEx a, void* ws, size_t ws_bytes, hipStream_t s) {
  const ExactPlan pl = exact_plan(a.N, a.K);
  const int products = a.W2 ? 2 : 1;
  a.S = pl.S; a.L = pl.L;
  a.nt = (a.N + EX_BN - 1) / EX_BN;
  a.slab = static_cast<float*>(ws);
  a.slab2 = a.slab + (size_t)pl.S * a.M * a.N;
  const bool spread = exact_spread(a.M, a.N, pl, products);
  const size_t need = exact_ws_bytes(a.M, a.N, a.K, products);
  AZ_REQUIRE(!spread || (ws && aligned16(ws) && ws_bytes >= need), AZ_EINVAL,
             "az_gemm_exact_ex: workspace too small (az_gemm_exact_ex_ws_bytes: %zu bytes, 16B "
             "aligned)", need);
  AZ_REQUIRE((a.M + 32 * exact_waves(a.M) - 1) / (32 * exact_waves(a.M)) <= 65535, AZ_EINVAL,
             "az_gemm_exact_ex: M=%d too large", a.M);
  return exact_launch<ExactEpiEx>(a, products, spread, s);
}

}  // namespace az

using namespace az;

extern "C" size_t az_gemm_exact_ex_ws_bytes(int M, int N, int K, int paired) {
  if (M < 1 || N < 4 || N % 4 || K < 4 || K % 4) return 0;
  return exact_ws_bytes(M, N, K, paired ? 2 : 1);
}

extern "C" int az_gemm_exact_ex(const az_gemm_exact_desc* d, void* stream) {
  AZ_REQUIRE(d != nullptr, AZ_EINVAL, "az_gemm_exact_ex: null descriptor");
  const int M = d->M, N = d->N, K = d->K;
  AZ_REQUIRE(M >= 0 && N >= 4 && N % 4 == 0 && K >= 4 && K % 4 == 0, AZ_EINVAL,
             "az_gemm_exact_ex: bad shape M=%d N=%d K=%d (N %% 4 == 0, K %% 4 == 0)", M, N, K);
  auto act_ok = [](int a) { return a == AZ_ACT_NONE || a == AZ_ACT_RELU || a == AZ_ACT_SIGMOID; };
  AZ_REQUIRE(act_ok(d->act) && (!d->W2 || act_ok(d->act2)), AZ_EINVAL,
             "az_gemm_exact_ex: act=%d act2=%d (AZ_ACT_NONE, AZ_ACT_RELU or AZ_ACT_SIGMOID)",
             d->act, d->act2);
  AZ_REQUIRE((d->R != nullptr) == (d->G != nullptr), AZ_EINVAL,
             "az_gemm_exact_ex: the gated residual needs both R and G");
  AZ_REQUIRE(!d->G || (d->act == AZ_ACT_NONE && !d->W2), AZ_EINVAL,
             "az_gemm_exact_ex: the gated residual takes no activation (act=%d) and no paired "
             "product", d->act);
  AZ_REQUIRE(d->W2 || (!d->C2 && !d->bias2), AZ_EINVAL,
             "az_gemm_exact_ex: C2 / bias2 without W2 (the paired launch needs the second weight)");
  if (M == 0) return AZ_OK;
  AZ_REQUIRE(d->A && d->W && d->C && (!d->W2 || d->C2), AZ_EINVAL,
             "az_gemm_exact_ex: null pointer");
  AZ_REQUIRE(d->lda >= K && d->ldw >= K && d->ldc >= N && d->lda % 4 == 0 && d->ldw % 4 == 0 &&
                 d->ldc % 4 == 0,
             AZ_EINVAL, "az_gemm_exact_ex: leading dimensions lda=%d ldw=%d ldc=%d (>= K, K, N; "
             "%% 4 == 0)", d->lda, d->ldw, d->ldc);
  AZ_REQUIRE(!d->G || (d->ldr >= N && d->ldg >= N && d->ldr % 4 == 0 && d->ldg % 4 == 0),
             AZ_EINVAL, "az_gemm_exact_ex: leading dimensions ldr=%d ldg=%d (>= N; %% 4 == 0)",
             d->ldr, d->ldg);
  AZ_REQUIRE(aligned16(d->A) && aligned16(d->W) && aligned16(d->C) && aligned16(d->bias) &&
                 aligned16(d->W2) && aligned16(d->C2) && aligned16(d->bias2) && aligned16(d->R) &&
                 aligned16(d->G),
             AZ_EINVAL, "az_gemm_exact_ex: A, W, bias, C, W2, bias2, C2, R and G need 16B "
             "alignment");
  AZ_REQUIRE(d->C != d->C2, AZ_EINVAL, "az_gemm_exact_ex: C2 may not alias C");
  ExactArgsEx a = {};
  a.M = M; a.N = N; a.K = K;
  a.A = d->A; a.lda = d->lda; a.W = d->W; a.ldw = d->ldw; a.bias = d->bias; a.act = d->act;
  a.C = d->C; a.ldc = d->ldc;
  a.W2 = d->W2; a.bias2 = d->bias2; a.act2 = d->act2; a.C2 = d->C2;
  a.R = d->R; a.ldr = d->ldr; a.G = d->G; a.ldg = d->ldg;
  return gemm_exact_ex(a, d->ws, d->ws_bytes, as_stream(stream));
}
