// The 3x3 conv fmaf chain on an LDS-resident input, shared by the one-workgroup-per-board trunks
// (az_ttt.hip, az_c4n.hip, az_c4r.hip).
#pragma once

#include "az_common.h"

namespace az {

// One output of a 3x3 conv whose input sits in LDS: the fmaf chain of conv3x3_relu_kernel,
// (ci, kh, kw) order with out-of-range taps skipped (a select, no branch).  w is the output
// channel's [CIN][3][3] weight row.
// The input is H x W (row index yo < H, column index xo < W; a square board has H == W).
// CIN == 1: `in` is the H x W plane.  Otherwise `in` is position-major, [H*W][CIN + 4] (the pad
// keeps positions on different banks and rows 16-byte aligned): one ds_read_b128 brings a tap's
// four consecutive input channels, so a step of four channels is 9 LDS reads for 36 fmaf.
// VEC: a 16-byte aligned weight row, its 36 weights per step arrive as nine float4 loads.
template <int CIN, int H, int W, int PAD, bool VEC>
__device__ __forceinline__ float conv_chain(const float* __restrict__ w, const float* in, int yo,
                                            int xo) {
  constexpr int LD = CIN == 1 ? 1 : CIN + 4;
  int off[9];
  bool ok[9];
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int yi = yo + kh - PAD, xi = xo + kw - PAD;
      const bool in_range = PAD == 0 || (yi >= 0 && yi < H && xi >= 0 && xi < W);
      ok[kh * 3 + kw] = in_range;
      off[kh * 3 + kw] = in_range ? (yi * W + xi) * LD : 0;
    }
  float s = 0.f;
  if constexpr (CIN == 1) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const float x = fmaf(w[t], in[off[t]], s);
      s = ok[t] ? x : s;
    }
  } else {
    static_assert(CIN % 4 == 0, "four input channels per step");
#pragma unroll 2
    for (int c4 = 0; c4 < CIN; c4 += 4) {
      float wf[36];
      if constexpr (VEC) {
#pragma unroll
        for (int j = 0; j < 9; ++j) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(w + c4 * 9 + j * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) wf[j * 4 + e] = v[e];
        }
      } else {
#pragma unroll
        for (int q = 0; q < 36; ++q) wf[q] = w[c4 * 9 + q];
      }
      f32x4 iv[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) iv[t] = *reinterpret_cast<const f32x4*>(in + off[t] + c4);
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const float x = fmaf(wf[c * 9 + t], iv[t][c], s);
          s = ok[t] ? x : s;
        }
    }
  }
  return s;
}

}  // namespace az
