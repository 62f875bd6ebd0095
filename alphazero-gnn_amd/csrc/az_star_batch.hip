// Batched star evaluation: the layer stack of gnn_utils.py:34-74 on ANY number of stars of any
// size in one packed [V][F] row buffer (star b = rows offs[b] .. offs[b+1]-1, row 0 the leaf).
// az_gnn_star_infer (az_star.hip) streams every weight matrix once per call for at most 8 row 0s;
// a lock-step self-play round has hundreds of leaves, and at that size the node update is three
// dense products over the B row 0s.  Only row 0 of a star changes in a layer, so x is never
// copied or written: per layer
//   P  = x W1'^T              attention.0 factored per node, W1 [H][2F] read as [2H][F]: one
//                             K-major GEMM over the V rows (P[v][2q] target half, [2q+1] source
//                             half); from layer 1 on the target half of the UPDATED row 0s comes
//                             from a second, B-row product (Pt)
//   star_batch_agg_kernel     scores, their sum in neighbour order, the normalisation, the
//                             aggregate, and the operand row TA[b] = [t | agg] ([B][2F])
//   gate.0, update_net.0      two plain K-major GEMMs on TA (K = 2F), sigmoid / ReLU epilogues
//   update_net.2              K = F, gated-residual epilogue R = TA's t half, G = gate
// and one last pass puts the untouched row back for one-row stars (t + g u is not t).
// Every GEMM goes through az::gemm_f32, so which tile serves which B is the dispatch's business:
// rows are within 1e-5 of az_gnn_star_infer's but not bit-identical to them, and may differ
// between values of B; two identical calls give equal bits (no atomics, fixed summation orders).
#include "az_star_batch.h"

namespace az {

// TA[b] = [t_b | agg_b] for star blockIdx.y, columns blockIdx.x * 1024 ...; grid
// (ceil(F / 1024), B), 256 threads.  t_b is t[b] (the row 0 the previous layer wrote) or, at
// layer 0 and for a one-row star at every layer, the star's own row 0 in x; its projection is
// Pt[b] or P[offs[b]].  Every block of a star forms the star's weights itself (wave w the
// neighbours w, w + 4, ... of a 32-neighbour tile; (n - 1) KB of P against (n - 1) * 4 KB of
// rows).  A star of more than 33 rows forms its weights twice: once for their sum, once tile by
// tile for the aggregate.  The aggregate loads 8 rows' float4s before the first fmaf and adds
// them in neighbour order.
__global__ __launch_bounds__(256) void star_batch_agg_kernel(
    const float* __restrict__ x, const int* __restrict__ offs, int V, int F, int H,
    const float* __restrict__ P, const float* __restrict__ t, const float* __restrict__ Pt,
    const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
    float* __restrict__ TA) {
  __shared__ float al[SB_TILE];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.y;
  const StarSpan sp = star_span(offs, b, V);
  const int o = sp.o, n = sp.n;
  const int k = (blockIdx.x * 256 + threadIdx.x) * 4;
  const bool kin = k < F;                        // F % 4 == 0: a float4 is whole or absent
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  const float* trow = (t && n > 1) ? t + (size_t)b * F : x + (size_t)o * F;
  const f32x4 tv = kin ? *reinterpret_cast<const f32x4*>(trow + k) : z;
  float* out = TA + (size_t)b * 2 * F;
  if (n < 2) {
    if (kin) {
      *reinterpret_cast<f32x4*>(out + k) = tv;
      *reinterpret_cast<f32x4*>(out + F + k) = z;
    }
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
      if (lane == 0) al[j] = sigmoidf_ref(acc + bias2);
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

// x0[b] = the star's own row 0 for every star (all != 0: L == 0) or for the one-row stars only
// (a 1-row input passes the layers unchanged, gnn_utils.py:35-36).  grid (ceil(F / 1024), B)
__global__ __launch_bounds__(256) void star_batch_row0_kernel(const float* __restrict__ x,
                                                              const int* __restrict__ offs, int V,
                                                              int F, int all,
                                                              float* __restrict__ x0) {
  const StarSpan sp = star_span(offs, blockIdx.y, V);
  const int k = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (k < F && (all || sp.n < 2))
    *reinterpret_cast<f32x4*>(x0 + (size_t)blockIdx.y * F + k) =
        *reinterpret_cast<const f32x4*>(x + (size_t)sp.o * F + k);
}

struct StarBatchWs {
  size_t P, Pt, TA, gate, u1, tbuf, split, split_bytes, total;   // byte offsets
};

static StarBatchWs star_batch_ws(int B, int V, int F, int H) {
  StarBatchWs w;
  const size_t row = sb_pad((size_t)B * F * 4);
  w.P = 0;
  w.Pt = w.P + sb_pad((size_t)V * 2 * H * 4);
  w.TA = w.Pt + sb_pad((size_t)B * 2 * H * 4);
  w.gate = w.TA + sb_pad((size_t)B * 2 * F * 4);
  w.u1 = w.gate + row;
  w.tbuf = w.u1 + row;
  w.split = w.tbuf + row;
  // the slabs, and room for the fp16 planes of the largest A (launch_x3: 4 M K bytes) with its
  // row scales
  const size_t planes = 4 * std::max((size_t)V * F, (size_t)B * 2 * F);
  w.split_bytes = SB_SPLIT_BYTES + sb_pad(planes) + sb_pad(8 * ((size_t)V + B + 2 * F + 2 * H)) +
                  (size_t(1) << 20);
  w.total = w.split + w.split_bytes;
  return w;
}

int star_batch_agg(const float* x, const int* offs, int B, int V, int F, int H, const float* P,
                   const float* t, const float* Pt, const float* b1, const float* w2,
                   const float* b2, float* TA, hipStream_t s) {
  hipLaunchKernelGGL(star_batch_agg_kernel, dim3((F + 1023) / 1024, B), dim3(256), 0, s, x, offs,
                     V, F, H, P, t, Pt, b1, w2, b2, TA);
  return check_launch("star_batch_agg_kernel");
}

int star_batch_row0(const float* x, const int* offs, int B, int V, int F, int all, float* x0,
                    hipStream_t s) {
  hipLaunchKernelGGL(star_batch_row0_kernel, dim3((F + 1023) / 1024, B), dim3(256), 0, s, x, offs,
                     V, F, all, x0);
  return check_launch("star_batch_row0_kernel");
}

int star_offs_check(const char* who, const int* offs, int B, int V) {
  // offs in host memory the device maps (az_host_alloc, pinned) is checked here; offs in HBM is
  // clamped by the kernels (star_span)
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, offs) != hipSuccess) {
    (void)hipGetLastError();
  } else if (attr.type == hipMemoryTypeHost) {
    AZ_REQUIRE(offs[0] == 0 && offs[B] == V, AZ_EINVAL, "%s: offs[0]=%d offs[B]=%d (need 0 and "
               "V=%d)", who, offs[0], offs[B], V);
    for (int b = 0; b < B; ++b)
      AZ_REQUIRE(offs[b + 1] > offs[b], AZ_EINVAL, "%s: offs not ascending at star %d (%d, %d)",
                 who, b, offs[b], offs[b + 1]);
  }
  return AZ_OK;
}

int star_batch_check(const char* who, const float* x, const int* offs, int B, int V, int L,
                     const az_gnn_layer_w* layers, const float* x0, const void* ws,
                     size_t ws_bytes, size_t ws_need) {
  AZ_REQUIRE(x && offs && x0 && (L == 0 || (layers && ws)), AZ_EINVAL, "%s: null pointer", who);
  AZ_REQUIRE(aligned16(x) && aligned16(x0) && aligned16(ws) && ((uintptr_t)offs & 3u) == 0,
             AZ_EINVAL, "%s: x, x0 and ws need 16B alignment, offs 4B alignment", who);
  AZ_REQUIRE(x != x0, AZ_EINVAL, "%s: x0 may not alias x", who);
  AZ_REQUIRE(L == 0 || ws_bytes >= ws_need, AZ_EINVAL,
             "%s: workspace of %zu bytes too small (%zu needed)", who, ws_bytes, ws_need);
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
  return star_offs_check(who, offs, B, V);
}

}  // namespace az

using namespace az;

extern "C" size_t az_gnn_star_batch_ws_bytes(int B, int V, int F, int H, int L) {
  if (!star_batch_shape(B, V, F, H, L) || B < 1) return 0;
  return star_batch_ws(B, V, F, H).total;
}

extern "C" int az_gnn_star_batch_infer(const float* x, const int* offs, int B, int V, int F, int H,
                                       int L, const az_gnn_layer_w* layers, float* x0, void* ws,
                                       size_t ws_bytes, void* stream) {
  AZ_REQUIRE(star_batch_shape(B, V, F, H, L), AZ_EINVAL,
             "az_gnn_star_batch_infer: bad shape B=%d V=%d F=%d H=%d L=%d (V >= B, F %% 16 == 0, "
             "H %% 4 == 0, 0 <= L <= %d)",
             B, V, F, H, L, AZ_STAR_MAX_LAYERS);
  if (B == 0) return AZ_OK;
  int rc = star_batch_check("az_gnn_star_batch_infer", x, offs, B, V, L, layers, x0, ws, ws_bytes,
                            az_gnn_star_batch_ws_bytes(B, V, F, H, L));
  if (rc) return rc;
  hipStream_t s = as_stream(stream);
  const dim3 blk(256), grid((F + 1023) / 1024, B);
  if (L == 0) {
    hipLaunchKernelGGL(star_batch_row0_kernel, grid, blk, 0, s, x, offs, V, F, 1, x0);
    return check_launch("star_batch_row0_kernel");
  }
  const StarBatchWs o = star_batch_ws(B, V, F, H);
  char* base = static_cast<char*>(ws);
  float* P = reinterpret_cast<float*>(base + o.P);
  float* Pt = reinterpret_cast<float*>(base + o.Pt);
  float* TA = reinterpret_cast<float*>(base + o.TA);
  float* gate = reinterpret_cast<float*>(base + o.gate);
  float* u1 = reinterpret_cast<float*>(base + o.u1);
  float* tbuf = reinterpret_cast<float*>(base + o.tbuf);
  void* split = base + o.split;
  for (int l = 0; l < L; ++l) {
    const az_gnn_layer_w& w = layers[l];
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
    // 2. weights, aggregate and the operand rows [t | agg]
    hipLaunchKernelGGL(star_batch_agg_kernel, grid, blk, 0, s, x, offs, V, F, H, P,
                       l > 0 ? tbuf : nullptr, l > 0 ? Pt : nullptr, w.att_b1, w.att_w2, w.att_b2,
                       TA);
    if ((rc = check_launch("star_batch_agg_kernel"))) return rc;
    // 3. gate.0 and update_net.0 on TA, update_net.2 with the gated residual
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
    u.R = TA; u.ldr = 2 * F; u.G = gate; u.ldg = F;
    u.C = t_out; u.ldc = F;
    u.ws = split; u.ws_bytes = o.split_bytes;
    if ((rc = gemm_f32(&u, s))) return rc;
  }
  // 4. one-row stars: their own row, bit for bit
  hipLaunchKernelGGL(star_batch_row0_kernel, grid, blk, 0, s, x, offs, V, F, 0, x0);
  return check_launch("star_batch_row0_kernel");
}
