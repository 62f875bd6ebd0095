// Batch-invariant star evaluation: az_gnn_star_batch_infer's layer stack with every
// product an exact GEMM (az_gnn_star_batch_exact_infer), and the one-call evaluator on top of it
// (az_star_eval_exact_fwd).  Host code only: the kernels are az_star_batch.hip's
// star_batch_agg_kernel / star_batch_row0_kernel (a star's weights and aggregate from that star's
// rows only, in neighbour order, no atomics), az_gemm_exact.hip's plain exact GEMM and heads, and
// az_gemm_exact_ex.hip's epilogues.  No call into az::gemm_f32: nothing here picks a tile, a
// split-K count or a stream-K plan from a row count, so x0[b] is a function of star b's rows and
// the weights only.
#include "az_gemm_exact.h"
#include "az_star_batch.h"

namespace az {

struct StarExactWs {
  size_t P, Pt, TA, gate, u1, tbuf, slab, slab_bytes, total;   // byte offsets
};

// Sized by capacity: every term grows with B and V (exact_ws_bytes_upto is the most any smaller
// call takes), and the offsets of a call are computed from ITS B and V, so they lie inside.
static StarExactWs star_exact_ws(int B, int V, int F, int H) {
  StarExactWs w;
  const size_t row = sb_pad((size_t)B * F * 4);
  w.P = 0;
  w.Pt = w.P + sb_pad((size_t)V * 2 * H * 4);
  w.TA = w.Pt + sb_pad((size_t)B * 2 * H * 4);
  w.gate = w.TA + sb_pad((size_t)B * 2 * F * 4);
  w.u1 = w.gate + row;
  w.tbuf = w.u1 + row;
  w.slab = w.tbuf + row;
  size_t s = exact_ws_bytes_upto(V, 2 * H, F);                   // P
  s = std::max(s, exact_ws_bytes_upto(B, 2 * H, F));             // Pt
  s = std::max(s, exact_ws_bytes_upto(B, F, 2 * F, 2));          // gate.0 + update_net.0, paired
  s = std::max(s, exact_ws_bytes_upto(B, F, F));                 // update_net.2
  w.slab_bytes = sb_pad(s) + 256;
  w.total = w.slab + w.slab_bytes;
  return w;
}

static int star_exact_layers(const float* x, const int* offs, int B, int V, int F, int H, int L,
                             const az_gnn_layer_w* layers, float* x0, void* ws, hipStream_t s) {
  int rc;
  if (L == 0) return star_batch_row0(x, offs, B, V, F, 1, x0, s);
  const StarExactWs o = star_exact_ws(B, V, F, H);
  char* base = static_cast<char*>(ws);
  float* P = reinterpret_cast<float*>(base + o.P);
  float* Pt = reinterpret_cast<float*>(base + o.Pt);
  float* TA = reinterpret_cast<float*>(base + o.TA);
  float* gate = reinterpret_cast<float*>(base + o.gate);
  float* u1 = reinterpret_cast<float*>(base + o.u1);
  float* tbuf = reinterpret_cast<float*>(base + o.tbuf);
  void* slab = base + o.slab;
  for (int l = 0; l < L; ++l) {
    const az_gnn_layer_w& w = layers[l];
    float* t_out = l == L - 1 ? x0 : tbuf;
    // 1. P = x W1'^T over the V rows (att_w1 [H][2F] read as [2H][F]); from layer 1 on also Pt
    //    over the updated row 0s
    if ((rc = gemm_exact(x, F, w.att_w1, F, nullptr, AZ_ACT_NONE, P, 2 * H, V, 2 * H, F, slab,
                         o.slab_bytes, s)))
      return rc;
    if (l > 0 && (rc = gemm_exact(tbuf, F, w.att_w1, F, nullptr, AZ_ACT_NONE, Pt, 2 * H, B, 2 * H,
                                  F, slab, o.slab_bytes, s)))
      return rc;
    // 2. weights, aggregate and the operand rows [t | agg]
    if ((rc = star_batch_agg(x, offs, B, V, F, H, P, l > 0 ? tbuf : nullptr,
                             l > 0 ? Pt : nullptr, w.att_b1, w.att_w2, w.att_b2, TA, s)))
      return rc;
    // 3. gate.0 and update_net.0 on TA in one paired launch
    ExactArgsEx g = {};
    g.M = B; g.N = F; g.K = 2 * F;
    g.A = TA; g.lda = 2 * F; g.ldw = 2 * F; g.ldc = F;
    g.W = w.gate_w; g.bias = w.gate_b; g.act = AZ_ACT_SIGMOID; g.C = gate;
    g.W2 = w.upd_w1; g.bias2 = w.upd_b1; g.act2 = AZ_ACT_RELU; g.C2 = u1;
    if ((rc = gemm_exact_ex(g, slab, o.slab_bytes, s))) return rc;
    // 4. update_net.2 with the gated residual t + g * u
    ExactArgsEx u = {};
    u.M = B; u.N = F; u.K = F;
    u.A = u1; u.lda = F; u.W = w.upd_w2; u.ldw = F; u.bias = w.upd_b2; u.act = AZ_ACT_NONE;
    u.C = t_out; u.ldc = F;
    u.R = TA; u.ldr = 2 * F; u.G = gate; u.ldg = F;
    if ((rc = gemm_exact_ex(u, slab, o.slab_bytes, s))) return rc;
  }
  // 5. one-row stars: their own row, bit for bit
  return star_batch_row0(x, offs, B, V, F, 0, x0, s);
}

static size_t star_exact_layers_bytes(int B, int V, int F, int H) {
  return star_exact_ws(B, V, F, H).total;
}

}  // namespace az

using namespace az;

extern "C" size_t az_gnn_star_batch_exact_ws_bytes(int B, int V, int F, int H, int L) {
  if (!star_batch_shape(B, V, F, H, L) || B < 1) return 0;
  return star_exact_layers_bytes(B, V, F, H);
}

extern "C" int az_gnn_star_batch_exact_infer(const float* x, const int* offs, int B, int V, int F,
                                             int H, int L, const az_gnn_layer_w* layers,
                                             float* x0, void* ws, size_t ws_bytes, void* stream) {
  AZ_REQUIRE(star_batch_shape(B, V, F, H, L), AZ_EINVAL,
             "az_gnn_star_batch_exact_infer: bad shape B=%d V=%d F=%d H=%d L=%d (V >= B, F %% 16 "
             "== 0, H %% 4 == 0, 0 <= L <= %d)",
             B, V, F, H, L, AZ_STAR_MAX_LAYERS);
  if (B == 0) return AZ_OK;
  const int rc = star_batch_check("az_gnn_star_batch_exact_infer", x, offs, B, V, L, layers, x0,
                                  ws, ws_bytes, az_gnn_star_batch_exact_ws_bytes(B, V, F, H, L));
  if (rc) return rc;
  return star_exact_layers(x, offs, B, V, F, H, L, layers, x0, ws, as_stream(stream));
}

extern "C" size_t az_star_eval_exact_ws_bytes(int max_B, int max_V, int game, int nx, int ny,
                                              int A, int L, int H) {
  if (max_B < 1 || A < 1 || A > 32 || !exact_has_trunk(game, nx, ny)) return 0;
  const int F = exact_features(game, nx, ny);
  if (!star_batch_shape(max_B, max_V, F, H, L)) return 0;
  return sb_pad(star_exact_layers_bytes(max_B, max_V, F, H)) +
         exact_eval_tail_ws_bytes(max_B, game, nx, ny);
}

extern "C" int az_star_eval_exact_fwd(const az_star_eval_exact* d, const int8_t* rows,
                                      const int* offs, int B, int V, float* pi, float* v,
                                      float* gpi, float* gv, void* stream) {
  AZ_REQUIRE(d != nullptr, AZ_EINVAL, "az_star_eval_exact_fwd: null descriptor");
  const az_eval_exact* e = &d->e;
  AZ_REQUIRE(B >= 0 && B <= e->max_B && (B == 0 || (V >= B && V <= d->max_V)), AZ_EINVAL,
             "az_star_eval_exact_fwd: B=%d V=%d max_B=%d max_V=%d (B <= V)", B, V, e->max_B,
             d->max_V);
  if (B == 0) return AZ_OK;
  int rc = exact_eval_check(e, "az_star_eval_exact_fwd", true, true);
  if (rc) return rc;
  const int F = e->F;
  AZ_REQUIRE(star_batch_shape(B, V, F, d->H, d->L) &&
                 star_batch_shape(e->max_B, d->max_V, F, d->H, d->L),
             AZ_EINVAL, "az_star_eval_exact_fwd: bad shape F=%d H=%d L=%d (H %% 4 == 0, 0 <= L <= "
             "%d, max_V >= max_B)", F, d->H, d->L, AZ_STAR_MAX_LAYERS);
  AZ_REQUIRE(rows && offs && v && gv && d->leaf && d->x0, AZ_EINVAL,
             "az_star_eval_exact_fwd: null pointer (rows / offs / v / gv / leaf / x0)");
  AZ_REQUIRE(aligned16(d->leaf) && aligned16(d->x0) && aligned16(e->ws) &&
                 ((uintptr_t)offs & 3u) == 0,
             AZ_EINVAL, "az_star_eval_exact_fwd: leaf, x0 and ws need 16B alignment, offs 4B "
             "alignment");
  const size_t layer_bytes = sb_pad(star_exact_layers_bytes(e->max_B, d->max_V, F, d->H));
  const size_t need = az_star_eval_exact_ws_bytes(e->max_B, d->max_V, e->game, e->nx, e->ny, e->A,
                                                  d->L, d->H);
  AZ_REQUIRE(e->ws && e->ws_bytes >= need, AZ_EINVAL,
             "az_star_eval_exact_fwd: workspace too small (az_star_eval_exact_ws_bytes: %zu "
             "bytes)", need);
  if ((rc = star_batch_check("az_star_eval_exact_fwd", e->feat, offs, B, V, d->L, d->layers,
                             d->x0, e->ws, e->ws_bytes, 0)))
    return rc;
  hipStream_t s = as_stream(stream);
  // 1. the trunk on the V rows; 2. the row-0 gather
  if ((rc = exact_eval_trunk(e, rows, V, e->feat, stream))) return rc;
  if ((rc = star_batch_row0(e->feat, offs, B, V, F, 1, d->leaf, s))) return rc;
  // 3. the standard tail on the leaf rows; 4. the layers; 5. / 6. output_transform and the heads
  char* tail_ws = static_cast<char*>(e->ws) + layer_bytes;
  const size_t tail_bytes = e->ws_bytes - layer_bytes;
  if ((rc = exact_eval_tail(e, d->leaf, nullptr, B, pi, v, nullptr, nullptr, tail_ws, tail_bytes,
                            s)))
    return rc;
  if ((rc = star_exact_layers(e->feat, offs, B, V, F, d->H, d->L, d->layers, d->x0, e->ws, s)))
    return rc;
  return exact_eval_tail(e, nullptr, d->x0, B, nullptr, nullptr, gpi, gv, tail_ws, tail_bytes, s);
}
