// Training on child stars: the packed-star layer stack of az_star_batch.hip keeping what the
// backward needs, and that backward (include/az_hip.h, az_gnn_star_batch_fwd_train / _bwd).
// Only row 0 of a star changes in a layer and x is an input (the trunk is frozen in the GNN step),
// so the forward never copies x and the backward forms no gradient with respect to it: between
// layers only dt [B][F] flows.  Per layer the forward is az_gnn_star_batch_infer's launch list
// with every intermediate written into `save`:
//   P = x W1'^T (and Pt = t W1'^T from layer 1 on), star_train_agg_kernel (TA = [t | agg], the raw
//   weights a [V] and their sums s [B]), gate.0, update_net.0, update_net.2 (u kept through C2)
// and the backward, last layer first:
//   star_gate_bwd_kernel          du = dt g, dg = dt u g (1 - g); zero rows for a one-row star
//   du1 = (du Wu2) [u1 > 0]       d update_net.2 = du^T u1, bias az_colsum(du)
//   d update_net.0 = du1^T TA, d gate.0 = dg^T TA (K = B), biases az_colsum
//   dagg = du1 Wu1[:, F:] + dg Wg[:, F:];  from layer 1 on dt += du1 Wu1[:, :F] + dg Wg[:, :F]
//   star_batch_agg_bwd_kernel     one star per block: the dots dagg . x_j, the normalisation and
//                                 sigmoid backward, dP / dPt and the per-star partials
//   az_colsum x 3                 d attention.2.weight, d attention.0.bias, d attention.2.bias
//   d attention.0.weight = dP^T x (K = V), + dPt^T t (K = B) from layer 1 on
//   dt += dPt W1'                 from layer 1 on (layer 0's dt has no reader)
// Every product is an az::gemm_f32 descriptor; no atomics, fixed summation orders.
#include "az_star_batch.h"

namespace az {

constexpr int ST_QPT = 4;   // hidden units a thread of the backward kernel owns: H <= 256 * 4

// star_batch_agg_kernel (az_star_batch.hip) that also keeps the raw weights and their sum: block
// column 0 of a star writes a[o + i] for its neighbours i = 1 .. n-1 (0 at the star's first row)
// and s[b] (0 for a one-row star).  grid (ceil(F / 1024), B), 256 threads.  A kernel of its own:
// the build is -fno-gpu-rdc (a kernel is launched from the unit that defines it), and the
// inference kernel keeps its argument list and code as they are.
__global__ __launch_bounds__(256) void star_train_agg_kernel(
    const float* __restrict__ x, const int* __restrict__ offs, int V, int F, int H,
    const float* __restrict__ P, const float* __restrict__ t, const float* __restrict__ Pt,
    const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
    float* __restrict__ TA, float* __restrict__ a_out, float* __restrict__ s_out) {
  __shared__ float al[SB_TILE];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.y;
  const StarSpan sp = star_span(offs, b, V);
  const int o = sp.o, n = sp.n;
  const bool keep = blockIdx.x == 0;
  const int k = (blockIdx.x * 256 + threadIdx.x) * 4;
  const bool kin = k < F;                        // F % 4 == 0: a float4 is whole or absent
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  const float* trow = (t && n > 1) ? t + (size_t)b * F : x + (size_t)o * F;
  const f32x4 tv = kin ? *reinterpret_cast<const f32x4*>(trow + k) : z;
  float* out = TA + (size_t)b * 2 * F;
  if (keep && threadIdx.x == 0) a_out[o] = 0.f;
  if (n < 2) {
    if (kin) {
      *reinterpret_cast<f32x4*>(out + k) = tv;
      *reinterpret_cast<f32x4*>(out + F + k) = z;
    }
    if (keep && threadIdx.x == 0) s_out[b] = 0.f;
    return;
  }
  const float* pt = Pt ? Pt + (size_t)b * 2 * H : P + (size_t)o * 2 * H;
  const float bias2 = b2[0];
  auto scores = [&](int i0) {                    // al[j] = weight of neighbour row i0 + j
    for (int j = wave; j < SB_TILE && i0 + j < n; j += 4) {
      const float* ps = P + (size_t)(o + i0 + j) * 2 * H;
      float acc = 0.f;
      for (int q = lane; q < H; q += 64) {
        const float h = pt[2 * q] + ps[2 * q + 1] + b1[q];
        acc = fmaf(w2[q], h > 0.f ? h : 0.f, acc);
      }
      acc = wave_sum(acc);
      if (lane == 0) {
        const float w = sigmoidf_ref(acc + bias2);
        al[j] = w;
        if (keep) a_out[o + i0 + j] = w;
      }
    }
  };
  float s = 0.f;
  for (int i0 = 1; i0 < n; i0 += SB_TILE) {
    if (i0 > 1) __syncthreads();                 // the previous tile's weights have been read
    scores(i0);
    __syncthreads();
    const int m = min(SB_TILE, n - i0);
    for (int j = 0; j < m; ++j) s += al[j];      // neighbour order
  }
  if (keep && threadIdx.x == 0) s_out[b] = s;
  const bool one_tile = n - 1 <= SB_TILE;        // al still holds every weight
  f32x4 acc = z;
  for (int i0 = 1; i0 < n; i0 += SB_TILE) {
    if (!one_tile) {
      __syncthreads();
      scores(i0);
      __syncthreads();
    }
    const int m = min(SB_TILE, n - i0);
    const float* xs = x + (size_t)(o + i0) * F + k;
    for (int j0 = 0; j0 < m; j0 += SB_CH) {
      f32x4 v[SB_CH];
#pragma unroll
      for (int c = 0; c < SB_CH; ++c)
        v[c] = (kin && j0 + c < m) ? *reinterpret_cast<const f32x4*>(xs + (size_t)(j0 + c) * F) : z;
#pragma unroll
      for (int c = 0; c < SB_CH; ++c) {
        if (j0 + c < m) {
          const float a = s > 0.f ? al[j0 + c] / s : al[j0 + c];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = fmaf(a, v[c][e], acc[e]);
        }
      }
    }
  }
  if (kin) {
    *reinterpret_cast<f32x4*>(out + k) = tv;
    *reinterpret_cast<f32x4*>(out + F + k) = acc;
  }
}

// x0[b] = the star's own row 0 for every star (all != 0: L == 0) or for the one-row stars only.
// grid (ceil(F / 1024), B)
__global__ __launch_bounds__(256) void star_train_row0_kernel(const float* __restrict__ x,
                                                              const int* __restrict__ offs, int V,
                                                              int F, int all,
                                                              float* __restrict__ x0) {
  const StarSpan sp = star_span(offs, blockIdx.y, V);
  const int k = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (k < F && (all || sp.n < 2))
    *reinterpret_cast<f32x4*>(x0 + (size_t)blockIdx.y * F + k) =
        *reinterpret_cast<const f32x4*>(x + (size_t)sp.o * F + k);
}

// Gated-residual backward of t' = t + g u on the B row 0s: du = dt g, dg = dt u g (1 - g) (the
// gradient at gate.0's pre-activation).  A one-row star took no update: both rows are zero, and
// its dt passes to the layer below untouched.  grid (ceil(F / 1024), B)
__global__ __launch_bounds__(256) void star_gate_bwd_kernel(
    const int* __restrict__ offs, int V, int F, const float* __restrict__ dt,
    const float* __restrict__ gate, const float* __restrict__ u, float* __restrict__ du,
    float* __restrict__ dg) {
  const StarSpan sp = star_span(offs, blockIdx.y, V);
  const int k = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (k >= F) return;
  const size_t i = (size_t)blockIdx.y * F + k;
  f32x4 a = {0.f, 0.f, 0.f, 0.f}, c = a;
  if (sp.n > 1) {
    const f32x4 d = *reinterpret_cast<const f32x4*>(dt + i);
    const f32x4 g = *reinterpret_cast<const f32x4*>(gate + i);
    const f32x4 uu = *reinterpret_cast<const f32x4*>(u + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a[e] = d[e] * g[e];
      c[e] = d[e] * uu[e] * (g[e] * (1.f - g[e]));
    }
  }
  *reinterpret_cast<f32x4*>(du + i) = a;
  *reinterpret_cast<f32x4*>(dg + i) = c;
}

// Aggregation and attention backward of star blockIdx.y (one block per star, 256 threads):
//   da'_j   = dagg_b . x_j                         wave w the neighbours w, w + 4, ... of a
//             32-neighbour tile, 8 rows' float4s loaded before the first fmaf
//   da_j    = s > 0 ? (da'_j - sum_i a'_i da'_i) / s : da'_j,   a'_i = s > 0 ? a_i / s : a_i
//   dsc_j   = da_j a_j (1 - a_j)
//   dh_jq   = dsc_j w2[q] [h_jq > 0],  h_jq = pt[2q] + P[j][2q+1] + b1[q] as the forward formed it
//   dP[j]   = {0, dh_jq} (source half);  dP[leaf] = {sum_j dh_jq, 0} at layer 0, zeros from layer 1
//             on, where the target half goes to dPt[b]; sums in neighbour order
//   part[b] = [sum_j dsc_j relu(h_jq) | sum_j dh_jq | sum_j dsc_j | pad], [2H + 4] floats
// Thread i owns the hidden units i, i + 256, ... (H <= 1024).  A star of more than 33 rows forms
// its dots twice: once for sum_i a'_i da'_i, once tile by tile for the rest.  A one-row star
// writes zeros.  With one neighbour a' = a / a = 1, so da = da' - da' = 0 exactly.
__global__ __launch_bounds__(256) void star_batch_agg_bwd_kernel(
    const float* __restrict__ x, const int* __restrict__ offs, int V, int F, int H,
    const float* __restrict__ P, const float* __restrict__ Pt, const float* __restrict__ a,
    const float* __restrict__ ssum, const float* __restrict__ dagg, const float* __restrict__ b1,
    const float* __restrict__ w2, float* __restrict__ dP, float* __restrict__ dPt,
    float* __restrict__ part) {
  __shared__ float dal[SB_TILE];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.y;
  const StarSpan sp = star_span(offs, b, V);
  const int o = sp.o, n = sp.n;
  const int PW = 2 * H + 4;
  float* dpl = dP + (size_t)o * 2 * H;           // the leaf's row
  float* dptb = dPt ? dPt + (size_t)b * 2 * H : nullptr;
  float* pb = part + (size_t)b * PW;
  if (n < 2) {
    for (int i = tid; i < 2 * H; i += 256) {
      dpl[i] = 0.f;
      if (dptb) dptb[i] = 0.f;
    }
    for (int i = tid; i < PW; i += 256) pb[i] = 0.f;
    return;
  }
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  const float* dag = dagg + (size_t)b * F;
  const float s = ssum[b];
  const float* pt = Pt ? Pt + (size_t)b * 2 * H : P + (size_t)o * 2 * H;
  auto dots = [&](int i0) {                      // dal[j] = dagg . x[o + i0 + j]
    const float* xs = x + (size_t)(o + i0 + wave) * F;
    float acc[SB_CH];
#pragma unroll
    for (int c = 0; c < SB_CH; ++c) acc[c] = 0.f;
    for (int k0 = 0; k0 < F; k0 += 256) {
      const int k = k0 + lane * 4;
      const bool kin = k < F;
      const f32x4 d = kin ? *reinterpret_cast<const f32x4*>(dag + k) : z;
      f32x4 v[SB_CH];
#pragma unroll
      for (int c = 0; c < SB_CH; ++c)
        v[c] = (kin && i0 + wave + 4 * c < n)
                   ? *reinterpret_cast<const f32x4*>(xs + (size_t)(4 * c) * F + k) : z;
#pragma unroll
      for (int c = 0; c < SB_CH; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[c] = fmaf(d[e], v[c][e], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < SB_CH; ++c) {
      const float r = wave_sum(acc[c]);
      if (lane == 0 && i0 + wave + 4 * c < n) dal[wave + 4 * c] = r;
    }
  };
  float dot = 0.f;                               // sum_i a'_i da'_i, neighbour order
  for (int i0 = 1; i0 < n; i0 += SB_TILE) {
    if (i0 > 1) __syncthreads();                 // the previous tile's dots have been read
    dots(i0);
    __syncthreads();
    const int m = min(SB_TILE, n - i0);
    for (int j = 0; j < m; ++j) {
      const float aj = a[o + i0 + j];
      dot = fmaf(s > 0.f ? aj / s : aj, dal[j], dot);
    }
  }
  const bool one_tile = n - 1 <= SB_TILE;        // dal still holds every dot
  float tsum[ST_QPT], wsum[ST_QPT], ptq[ST_QPT], w2q[ST_QPT];
#pragma unroll
  for (int c = 0; c < ST_QPT; ++c) {
    const int q = tid + 256 * c;
    tsum[c] = wsum[c] = 0.f;
    ptq[c] = q < H ? pt[2 * q] : 0.f;
    w2q[c] = q < H ? w2[q] : 0.f;
  }
  float bsum = 0.f;
  for (int i0 = 1; i0 < n; i0 += SB_TILE) {
    __syncthreads();                             // every thread has read the tile before
    if (!one_tile) {
      dots(i0);
      __syncthreads();
    }
    const int m = min(SB_TILE, n - i0);
    if (tid < m) {                               // da' -> d score, in place
      const float aj = a[o + i0 + tid];
      const float dap = dal[tid];
      const float da = s > 0.f ? (dap - dot) / s : dap;
      dal[tid] = da * (aj * (1.f - aj));
    }
    __syncthreads();
    for (int j = 0; j < m; ++j) bsum += dal[j];
#pragma unroll
    for (int c = 0; c < ST_QPT; ++c) {
      const int q = tid + 256 * c;
      if (q < H) {
        const float bq = b1[q];
        for (int j = 0; j < m; ++j) {
          const size_t r = (size_t)(o + i0 + j) * 2 * H + 2 * q;
          const float h = ptq[c] + P[r + 1] + bq;
          const float dsc = dal[j];
          const float dh = h > 0.f ? dsc * w2q[c] : 0.f;
          dP[r] = 0.f;
          dP[r + 1] = dh;
          tsum[c] += dh;
          wsum[c] = fmaf(dsc, h > 0.f ? h : 0.f, wsum[c]);
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < ST_QPT; ++c) {
    const int q = tid + 256 * c;
    if (q < H) {
      dpl[2 * q] = dptb ? 0.f : tsum[c];
      dpl[2 * q + 1] = 0.f;
      if (dptb) {
        dptb[2 * q] = tsum[c];
        dptb[2 * q + 1] = 0.f;
      }
      pb[q] = wsum[c];
      pb[H + q] = tsum[c];
    }
  }
  if (tid < 4) pb[2 * H + tid] = tid == 0 ? bsum : 0.f;
}

struct StarSave {     // byte offsets inside one layer's block, and the block's size
  size_t P, Pt, TA, gate, u1, u, a, s, layer;
};

static StarSave star_save(int B, int V, int F, int H) {
  StarSave w;
  const size_t row = sb_pad((size_t)B * F * 4);
  w.P = 0;
  w.Pt = w.P + sb_pad((size_t)V * 2 * H * 4);
  w.TA = w.Pt + sb_pad((size_t)B * 2 * H * 4);
  w.gate = w.TA + sb_pad((size_t)B * 2 * F * 4);
  w.u1 = w.gate + row;
  w.u = w.u1 + row;
  w.a = w.u + row;
  w.s = w.a + sb_pad((size_t)V * 4);
  w.layer = w.s + sb_pad((size_t)B * 4);
  return w;
}

struct StarTrainWs {  // byte offsets; t is the forward's row 0s between layers, the backward's dt
  size_t t, du, dg, du1, dagg, dP, dPt, part, cs, cs_bytes, split, split_bytes, total;
};

static StarTrainWs star_train_ws(int B, int V, int F, int H) {
  StarTrainWs w;
  const size_t row = sb_pad((size_t)B * F * 4);
  w.t = 0;
  w.du = w.t + row;
  w.dg = w.du + row;
  w.du1 = w.dg + row;
  w.dagg = w.du1 + row;
  w.dP = w.dagg + row;
  w.dPt = w.dP + sb_pad((size_t)V * 2 * H * 4);
  w.part = w.dPt + sb_pad((size_t)B * 2 * H * 4);
  w.cs = w.part + sb_pad((size_t)B * (2 * H + 4) * 4);
  w.cs_bytes = sb_pad(az_colsum_ws_bytes(B, std::max(F, H)));
  w.split = w.cs + w.cs_bytes;
  // the slabs, and room for the fp16 planes of the largest A with its row scales, as
  // az_gnn_star_batch_infer keeps
  const size_t planes = 4 * std::max((size_t)V * F, (size_t)B * 2 * F);
  w.split_bytes = SB_SPLIT_BYTES + sb_pad(planes) + sb_pad(8 * ((size_t)V + B + 2 * F + 2 * H)) +
                  (size_t(1) << 20);
  w.total = w.split + w.split_bytes;
  return w;
}

static bool star_train_shape(int B, int V, int F, int H, int L) {
  return star_batch_shape(B, V, F, H, L) && H <= 256 * ST_QPT;
}

// The checks both calls share; `who` names the entry point in the message.
static int star_train_check(const char* who, const float* x, const int* offs, int B, int V, int F,
                            int H, int L, const az_gnn_layer_w* layers, const void* save,
                            size_t save_bytes, const void* ws, size_t ws_bytes) {
  AZ_REQUIRE(x && offs && (L == 0 || (layers && save && ws)), AZ_EINVAL, "%s: null pointer", who);
  AZ_REQUIRE(aligned16(x) && aligned16(save) && aligned16(ws) && ((uintptr_t)offs & 3u) == 0,
             AZ_EINVAL, "%s: x, save and ws need 16B alignment, offs 4B alignment", who);
  AZ_REQUIRE(L == 0 || save_bytes >= az_gnn_star_batch_save_bytes(B, V, F, H, L), AZ_EINVAL,
             "%s: save of %zu bytes too small (az_gnn_star_batch_save_bytes)", who, save_bytes);
  AZ_REQUIRE(L == 0 || ws_bytes >= az_gnn_star_batch_train_ws_bytes(B, V, F, H, L), AZ_EINVAL,
             "%s: workspace of %zu bytes too small (az_gnn_star_batch_train_ws_bytes)", who,
             ws_bytes);
  for (int l = 0; l < L; ++l) {
    const az_gnn_layer_w& w = layers[l];
    AZ_REQUIRE(w.att_w1 && w.att_b1 && w.att_w2 && w.att_b2 && w.upd_w1 && w.upd_b1 && w.upd_w2 &&
                   w.upd_b2 && w.gate_w && w.gate_b,
               AZ_EINVAL, "%s: null weight pointer in layer %d", who, l);
    AZ_REQUIRE(aligned16(w.att_w1) && aligned16(w.upd_w1) && aligned16(w.upd_w2) &&
                   aligned16(w.gate_w) && aligned16(w.upd_b1) && aligned16(w.upd_b2) &&
                   aligned16(w.gate_b),
               AZ_EINVAL, "%s: layer %d weights need 16B alignment", who, l);
  }
  // offs in host memory the device maps (az_host_alloc, pinned) is checked here; offs in HBM is
  // clamped by the kernels (star_span)
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, offs) != hipSuccess) {
    (void)hipGetLastError();
  } else if (attr.type == hipMemoryTypeHost) {
    AZ_REQUIRE(offs[0] == 0 && offs[B] == V, AZ_EINVAL, "%s: offs[0]=%d offs[B]=%d (need 0 and V=%d)",
               who, offs[0], offs[B], V);
    for (int b = 0; b < B; ++b)
      AZ_REQUIRE(offs[b + 1] > offs[b], AZ_EINVAL, "%s: offs not ascending at star %d (%d, %d)",
                 who, b, offs[b], offs[b + 1]);
  }
  return AZ_OK;
}

}  // namespace az

using namespace az;

extern "C" size_t az_gnn_star_batch_save_bytes(int B, int V, int F, int H, int L) {
  if (!star_train_shape(B, V, F, H, L) || B < 1) return 0;
  return star_save(B, V, F, H).layer * (size_t)L;
}

extern "C" size_t az_gnn_star_batch_train_ws_bytes(int B, int V, int F, int H, int L) {
  if (!star_train_shape(B, V, F, H, L) || B < 1) return 0;
  return star_train_ws(B, V, F, H).total;
}

extern "C" int az_gnn_star_batch_fwd_train(const float* x, const int* offs, int B, int V, int F,
                                           int H, int L, const az_gnn_layer_w* layers, float* x0,
                                           void* save, size_t save_bytes, void* ws,
                                           size_t ws_bytes, void* stream) {
  static const char* who = "az_gnn_star_batch_fwd_train";
  AZ_REQUIRE(star_train_shape(B, V, F, H, L), AZ_EINVAL,
             "%s: bad shape B=%d V=%d F=%d H=%d L=%d (V >= B, F %% 16 == 0, H %% 4 == 0, "
             "H <= %d, 0 <= L <= %d)", who, B, V, F, H, L, 256 * ST_QPT, AZ_STAR_MAX_LAYERS);
  if (B == 0) return AZ_OK;
  AZ_REQUIRE(x0 && aligned16(x0), AZ_EINVAL, "%s: x0 null or not 16B aligned", who);
  AZ_REQUIRE(x != x0, AZ_EINVAL, "%s: x0 may not alias x", who);
  int rc;
  if ((rc = star_train_check(who, x, offs, B, V, F, H, L, layers, save, save_bytes, ws, ws_bytes)))
    return rc;
  hipStream_t s = as_stream(stream);
  const dim3 blk(256), grid((F + 1023) / 1024, B);
  if (L == 0) {
    hipLaunchKernelGGL(star_train_row0_kernel, grid, blk, 0, s, x, offs, V, F, 1, x0);
    return check_launch("star_train_row0_kernel");
  }
  const StarSave so = star_save(B, V, F, H);
  const StarTrainWs o = star_train_ws(B, V, F, H);
  char* base = static_cast<char*>(ws);
  float* tbuf = reinterpret_cast<float*>(base + o.t);
  void* split = base + o.split;
  for (int l = 0; l < L; ++l) {
    const az_gnn_layer_w& w = layers[l];
    char* sv = static_cast<char*>(save) + so.layer * (size_t)l;
    float* P = reinterpret_cast<float*>(sv + so.P);
    float* Pt = reinterpret_cast<float*>(sv + so.Pt);
    float* TA = reinterpret_cast<float*>(sv + so.TA);
    float* gate = reinterpret_cast<float*>(sv + so.gate);
    float* u1 = reinterpret_cast<float*>(sv + so.u1);
    float* uu = reinterpret_cast<float*>(sv + so.u);
    float* t_out = l == L - 1 ? x0 : tbuf;
    // 1. P = x W1'^T over the V rows; from layer 1 on also Pt over the updated row 0s
    az_gemm_desc d = {};
    d.M = V; d.N = 2 * H; d.K = F;
    d.A = x; d.lda = F; d.a_kmajor = 1;
    d.B = w.att_w1; d.ldb = F; d.b_kmajor = 1;
    d.C = P; d.ldc = 2 * H;
    d.ws = split; d.ws_bytes = o.split_bytes;
    if ((rc = gemm_f32(&d, s))) return rc;
    if (l > 0) {
      d.M = B; d.A = tbuf; d.C = Pt;
      if ((rc = gemm_f32(&d, s))) return rc;
    }
    // 2. weights (kept raw, with their sums), aggregate and the operand rows [t | agg]
    hipLaunchKernelGGL(star_train_agg_kernel, grid, blk, 0, s, x, offs, V, F, H, P,
                       l > 0 ? tbuf : nullptr, l > 0 ? Pt : nullptr, w.att_b1, w.att_w2, w.att_b2,
                       TA, reinterpret_cast<float*>(sv + so.a), reinterpret_cast<float*>(sv + so.s));
    if ((rc = check_launch("star_train_agg_kernel"))) return rc;
    // 3. gate.0 and update_net.0 on TA, update_net.2 (u kept) with the gated residual
    az_gemm_desc c = {};
    c.M = B; c.N = F; c.K = 2 * F;
    c.A = TA; c.lda = 2 * F; c.a_kmajor = 1;
    c.b_kmajor = 1; c.ldb = 2 * F; c.ldc = F;
    c.ws = split; c.ws_bytes = o.split_bytes;
    c.B = w.gate_w; c.bias = w.gate_b; c.act = AZ_ACT_SIGMOID; c.C = gate;
    if ((rc = gemm_f32(&c, s))) return rc;
    c.B = w.upd_w1; c.bias = w.upd_b1; c.act = AZ_ACT_RELU; c.C = u1;
    if ((rc = gemm_f32(&c, s))) return rc;
    az_gemm_desc u = {};
    u.M = B; u.N = F; u.K = F;
    u.A = u1; u.lda = F; u.a_kmajor = 1;
    u.B = w.upd_w2; u.ldb = F; u.b_kmajor = 1; u.bias = w.upd_b2;
    u.C2 = uu; u.ldc2 = F;
    u.R = TA; u.ldr = 2 * F; u.G = gate; u.ldg = F;
    u.C = t_out; u.ldc = F;
    u.ws = split; u.ws_bytes = o.split_bytes;
    if ((rc = gemm_f32(&u, s))) return rc;
  }
  // 4. one-row stars: their own row, bit for bit
  hipLaunchKernelGGL(star_train_row0_kernel, grid, blk, 0, s, x, offs, V, F, 0, x0);
  return check_launch("star_train_row0_kernel");
}

extern "C" int az_gnn_star_batch_bwd(const float* x, const int* offs, int B, int V, int F, int H,
                                     int L, const az_gnn_layer_w* layers, const void* save,
                                     size_t save_bytes, const float* dx0,
                                     const az_gnn_layer_grads* grads, void* ws, size_t ws_bytes,
                                     void* stream) {
  static const char* who = "az_gnn_star_batch_bwd";
  AZ_REQUIRE(star_train_shape(B, V, F, H, L), AZ_EINVAL,
             "%s: bad shape B=%d V=%d F=%d H=%d L=%d (V >= B, F %% 16 == 0, H %% 4 == 0, "
             "H <= %d, 0 <= L <= %d)", who, B, V, F, H, L, 256 * ST_QPT, AZ_STAR_MAX_LAYERS);
  if (B == 0 || L == 0) return AZ_OK;
  AZ_REQUIRE(dx0 && aligned16(dx0) && grads, AZ_EINVAL, "%s: dx0 / grads null or dx0 not 16B aligned",
             who);
  int rc;
  if ((rc = star_train_check(who, x, offs, B, V, F, H, L, layers, save, save_bytes, ws, ws_bytes)))
    return rc;
  for (int l = 0; l < L; ++l) {
    const az_gnn_layer_grads& g = grads[l];
    AZ_REQUIRE(g.att_w1 && g.att_b1 && g.att_w2 && g.att_b2 && g.upd_w1 && g.upd_b1 && g.upd_w2 &&
                   g.upd_b2 && g.gate_w && g.gate_b,
               AZ_EINVAL, "%s: null gradient pointer in layer %d", who, l);
    AZ_REQUIRE(aligned16(g.att_w1) && aligned16(g.upd_w1) && aligned16(g.upd_w2) &&
                   aligned16(g.gate_w),
               AZ_EINVAL, "%s: layer %d gradient matrices need 16B alignment", who, l);
  }
  hipStream_t s = as_stream(stream);
  const dim3 blk(256), grid((F + 1023) / 1024, B);
  const StarSave so = star_save(B, V, F, H);
  const StarTrainWs o = star_train_ws(B, V, F, H);
  char* base = static_cast<char*>(ws);
  float* dt = reinterpret_cast<float*>(base + o.t);
  float* du = reinterpret_cast<float*>(base + o.du);
  float* dg = reinterpret_cast<float*>(base + o.dg);
  float* du1 = reinterpret_cast<float*>(base + o.du1);
  float* dagg = reinterpret_cast<float*>(base + o.dagg);
  float* dP = reinterpret_cast<float*>(base + o.dP);
  float* dPt = reinterpret_cast<float*>(base + o.dPt);
  float* part = reinterpret_cast<float*>(base + o.part);
  void* cs = base + o.cs;
  void* split = base + o.split;
  const int PW = 2 * H + 4;
  if (hipMemcpyAsync(dt, dx0, (size_t)B * F * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return check_launch("hipMemcpyAsync");
  for (int l = L - 1; l >= 0; --l) {
    const az_gnn_layer_w& w = layers[l];
    const az_gnn_layer_grads& g = grads[l];
    const char* sv = static_cast<const char*>(save) + so.layer * (size_t)l;
    const float* P = reinterpret_cast<const float*>(sv + so.P);
    const float* Pt = l > 0 ? reinterpret_cast<const float*>(sv + so.Pt) : nullptr;
    const float* TA = reinterpret_cast<const float*>(sv + so.TA);
    const float* gate = reinterpret_cast<const float*>(sv + so.gate);
    const float* u1 = reinterpret_cast<const float*>(sv + so.u1);
    const float* uu = reinterpret_cast<const float*>(sv + so.u);
    // 1. gated residual
    hipLaunchKernelGGL(star_gate_bwd_kernel, grid, blk, 0, s, offs, V, F, dt, gate, uu, du, dg);
    if ((rc = check_launch("star_gate_bwd_kernel"))) return rc;
    // 2. update_net.2: du1 = (du Wu2) [u1 > 0]; dWu2 = du^T u1; dbu2 = colsum(du)
    az_gemm_desc d = {};
    d.M = B; d.N = F; d.K = F;
    d.A = du; d.lda = F; d.a_kmajor = 1;
    d.B = w.upd_w2; d.ldb = F; d.b_kmajor = 0;
    d.act = AZ_ACT_DRELU; d.G = u1; d.ldg = F;
    d.C = du1; d.ldc = F; d.ws = split; d.ws_bytes = o.split_bytes;
    if ((rc = gemm_f32(&d, s))) return rc;
    d = {};
    d.M = F; d.N = F; d.K = B;
    d.A = du; d.lda = F; d.a_kmajor = 0;
    d.B = u1; d.ldb = F; d.b_kmajor = 0;
    d.C = g.upd_w2; d.ldc = F; d.ws = split; d.ws_bytes = o.split_bytes;
    if ((rc = gemm_f32(&d, s))) return rc;
    if ((rc = az_colsum(du, B, F, F, g.upd_b2, 0.f, cs, o.cs_bytes, s))) return rc;
    // 3. update_net.0 and gate.0: dW = dpre^T [t | agg] (K = B), biases
    const float* pre[2] = {du1, dg};
    float* wout[2] = {g.upd_w1, g.gate_w};
    float* bout[2] = {g.upd_b1, g.gate_b};
    const float* wmat[2] = {w.upd_w1, w.gate_w};
    for (int i = 0; i < 2; ++i) {
      d = {};
      d.M = F; d.N = 2 * F; d.K = B;
      d.A = pre[i]; d.lda = F; d.a_kmajor = 0;
      d.B = TA; d.ldb = 2 * F; d.b_kmajor = 0;
      d.C = wout[i]; d.ldc = 2 * F; d.ws = split; d.ws_bytes = o.split_bytes;
      if ((rc = gemm_f32(&d, s))) return rc;
      if ((rc = az_colsum(pre[i], B, F, F, bout[i], 0.f, cs, o.cs_bytes, s))) return rc;
    }
    // 4. d[t | agg] = du1 Wu1 + dg Wg: the agg half into dagg, the t half into dt (layer 0's dt
    //    has no reader)
    for (int i = 0; i < 2; ++i) {
      d = {};
      d.M = B; d.N = F; d.K = F;
      d.A = pre[i]; d.lda = F; d.a_kmajor = 1;
      d.B = wmat[i] + F; d.ldb = 2 * F; d.b_kmajor = 0;
      d.beta = i == 0 ? 0.f : 1.f;
      d.C = dagg; d.ldc = F; d.ws = split; d.ws_bytes = o.split_bytes;
      if ((rc = gemm_f32(&d, s))) return rc;
      if (l > 0) {
        d.B = wmat[i]; d.beta = 1.f; d.C = dt;
        if ((rc = gemm_f32(&d, s))) return rc;
      }
    }
    // 5. aggregation and attention backward, one star per block
    hipLaunchKernelGGL(star_batch_agg_bwd_kernel, dim3(1, B), blk, 0, s, x, offs, V, F, H, P, Pt,
                       reinterpret_cast<const float*>(sv + so.a),
                       reinterpret_cast<const float*>(sv + so.s), dagg, w.att_b1, w.att_w2, dP,
                       l > 0 ? dPt : nullptr, part);
    if ((rc = check_launch("star_batch_agg_bwd_kernel"))) return rc;
    if ((rc = az_colsum(part, B, H, PW, g.att_w2, 0.f, cs, o.cs_bytes, s))) return rc;
    if ((rc = az_colsum(part + H, B, H, PW, g.att_b1, 0.f, cs, o.cs_bytes, s))) return rc;
    if ((rc = az_colsum(part + 2 * H, B, 1, PW, g.att_b2, 0.f, cs, o.cs_bytes, s))) return rc;
    // 6. d attention.0.weight read as [2H][F]: dP^T x over the V rows; from layer 1 on the target
    //    rows come from dPt^T t over the B updated row 0s (dP's target half is zero there)
    d = {};
    d.M = 2 * H; d.N = F; d.K = V;
    d.A = dP; d.lda = 2 * H; d.a_kmajor = 0;
    d.B = x; d.ldb = F; d.b_kmajor = 0;
    d.C = g.att_w1; d.ldc = F; d.ws = split; d.ws_bytes = o.split_bytes;
    if ((rc = gemm_f32(&d, s))) return rc;
    if (l > 0) {
      d.K = B; d.A = dPt; d.B = TA; d.ldb = 2 * F; d.beta = 1.f;
      if ((rc = gemm_f32(&d, s))) return rc;
      // 7. dt += dPt W1' (the source columns of dPt are zero)
      d = {};
      d.M = B; d.N = F; d.K = 2 * H;
      d.A = dPt; d.lda = 2 * H; d.a_kmajor = 1;
      d.B = w.att_w1; d.ldb = F; d.b_kmajor = 0;
      d.beta = 1.f; d.C = dt; d.ldc = F; d.ws = split; d.ws_bytes = o.split_bytes;
      if ((rc = gemm_f32(&d, s))) return rc;
    }
  }
  return AZ_OK;
}
