/* libaz_hip.so — C-ABI of the MI355X (gfx950) board-evaluation hot path of
 * andrpac/alphazero-gnn: the Connect4/TicTacToe conv trunk + policy/value heads,
 * the GNN message-passing layers of gnn_utils.py, their backward pass and Adam.
 *
 * Conventions
 *   - Every pointer except the ones documented as host pointers is a DEVICE pointer
 *     (HBM), caller-allocated.  No entry point allocates, frees or synchronises, so a
 *     caller may capture them into a hipGraph.
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).
 *   - All arithmetic is fp32 (the reference runs torch fp32: SURVEY.md §0.8); GEMM-shaped
 *     work runs on v_mfma_f32_32x32x2_f32, everything else on the VALU.
 *   - Return value: AZ_OK (0) or a negative AZ_E* code; az_last_error() explains it.
 *   - Layouts are the reference's: nn.Linear weights [out][in] row-major, conv weights
 *     [Cout][Cin][3][3], features the NCHW flatten c*n*n + x*n + y
 *     (connect4/Connect4Net.py:42-49).
 *
 * Each entry point names the reference interface it replaces (path:line in the
 * reference tree).  The Python binding (ctypes) is alphazero-gnn_amd/azhip/_lib.py;
 * INTEGRATION.md shows the reference-side binding.
 */
#ifndef AZ_HIP_H
#define AZ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AZ_ABI_VERSION 2

#define AZ_OK 0
#define AZ_EINVAL (-1)     /* bad shape / null pointer / misaligned buffer */
#define AZ_ELAUNCH (-2)    /* a kernel launch failed (hipGetLastError) */
#define AZ_EDEVICE (-3)    /* no gfx950 device / HIP runtime error */

#define AZ_ACT_NONE 0
#define AZ_ACT_RELU 1
#define AZ_ACT_SIGMOID 2
#define AZ_ACT_TANH 3
#define AZ_ACT_DRELU 4     /* backward of ReLU: v * (G[i][j] > 0), G = saved activation */

int az_abi_version(void);
const char* az_last_error(void);
/* Checks that the current HIP device is a gfx950 (MI355X); returns AZ_OK or AZ_EDEVICE. */
int az_check_device(void);
/* Zero-copy host staging: fine-grained pinned host memory mapped at the same address on the
 * device (a kernel may read / write it directly; host sees device stores after a stream
 * synchronise).  Returns NULL on failure (az_last_error says why).  No reference counterpart:
 * it replaces the .cpu() / torch.FloatTensor round trips of the batch-1 predict
 * (connect4/Connect4GNN.py:59-84) with in-place reads and writes by the kernels. */
void* az_host_alloc(size_t bytes);
int az_host_free(void* p);

/* ---------------------------------------------------------------------------------
 * Dense fp32 GEMM with fused epilogue:  C = epi(op(A) . op(B))     (MFMA 32x32x2 f32;
 * M <= 8 with a K-major B dispatches to a weight-streaming GEMV kernel).
 * Replaces every nn.Linear of the path (gnn_utils.py:11-28,101-105, Connect4Net.py:21-25,
 * TicTacToeNet.py:21-26) and, with the transposed layouts, their weight/input gradients.
 *   A(i,k) = a_kmajor ? A[r(i)*lda + k] : A[k*lda + i]      r(i) = a_rows ? a_rows[i] : i
 *            (k >= K0 reads A2[r(i)*lda2 + k-K0] when A2 != NULL: concatenation [A | A2]
 *             along K, i.e. torch.cat([t, agg], dim=1) of gnn_utils.py:31,68)
 *   B(k,j) = b_kmajor ? B[j*ldb + k] : B[q(k)*ldb + j]       q(k) = b_rows ? b_rows[k] : k
 *            (b_kmajor = nn.Linear weight [N][K]; b_rows gathers rows of an N-major B)
 *   v      = act(sum_k A(i,k) B(k,j) + bias[j])     (AZ_ACT_DRELU: v * (G[i*ldg+j] > 0))
 *   C2[i*ldc2 + j] = v                                        when C2 != NULL
 *   v      = R ? R[c(i)*ldr + j] + (G ? G[i*ldg + j] : 1) * v : v   (gated residual,
 *            gnn_utils.py:71)
 *   C[c(i)*ldc + j] = v + beta * C[c(i)*ldc + j]             c(i) = c_rows ? c_rows[i] : i
 * ws/ws_bytes: optional device workspace; when the tile grid cannot fill the GPU the K loop is
 * split over workgroups and the fp32 partial slabs (splits*M*N*4 bytes) are reduced in a
 * fixed order (results are deterministic run to run).
 * Requirements: K % 4 == 0 when an operand is K-major; lda, lda2, ldb % 4 == 0 and 16-byte
 * aligned A/A2/B; K0 % 4 == 0; a_rows only with a_kmajor, b_rows only with !b_kmajor;
 * round_up(M, 4) <= lda when !a_kmajor; round_up(N, 4) <= ldb when !b_kmajor.
 * --------------------------------------------------------------------------------- */
typedef struct az_gemm_desc {
  int M, N, K;
  const float* A; int lda; int a_kmajor;
  const float* A2; int lda2; int K0;
  const int* a_rows;
  const float* B; int ldb; int b_kmajor;
  const int* b_rows;
  const float* bias;
  int act;
  const float* R; int ldr;
  const float* G; int ldg;
  float beta;
  float* C; int ldc;
  const int* c_rows;
  float* C2; int ldc2;
  void* ws; size_t ws_bytes;
} az_gemm_desc;

int az_gemm_f32(const az_gemm_desc* d, void* stream);

/* MFMA products per fp32 product that az_gemm_f32 runs for a plain K-major M x N x K GEMM with
 * ws_bytes of workspace: 3 = the fp16 form (each operand row scaled by a power of two and split
 * into two fp16 terms, three products on v_mfma_f32_32x32x16_f16: M > 64, K >= 1024, N >= 256,
 * room for A's row scales), 6 = the bf16 form (three bf16 terms, six products), 1 = an fp32
 * MFMA tile, 0 = the fp32 GEMV (M <= 8).  For rooflines and reports; no GPU work. */
int az_gemm_form(int M, int N, int K, size_t ws_bytes);

/* ---------------------------------------------------------------------------------
 * Connect4Net trunk, connect4/Connect4Net.py:42-49 (== Connect4GNNWrapper.extract_features,
 * connect4/Connect4GNN.py:31-46 in eval mode): conv1 3x3 p1 + ReLU -> conv2 3x3 p1 + ReLU ->
 * NCHW flatten, fused in one kernel (conv1 in LDS, conv2 as an implicit GEMM on MFMA 16x16x4).
 *   boards  int8 [B][7][7] in {-1,0,1} (axis 0 = column x, axis 1 = row y)
 *   feat    fp32 [B][3136]
 * --------------------------------------------------------------------------------- */
int az_c4_trunk_fwd(const int8_t* boards, int B,
                    const float* conv1_w, const float* conv1_b,
                    const float* conv2_w, const float* conv2_b,
                    float* feat, void* stream);

/* 3x3 conv (stride 1, padding `pad` in {0,1}) + ReLU on NCHW input; `in` is int8 boards
 * [B][H][W] (Cin must be 1) when in_int8 != 0, else fp32 [B][Cin][H][W].
 * TicTacToeNet conv1..conv3, tictactoe/TicTacToeNet.py:33-35. */
int az_conv3x3_relu_fwd(const void* in, int in_int8, int B, int Cin, int H, int W,
                        const float* w, const float* b, int Cout, int pad,
                        float* out, void* stream);

/* Policy/value heads: logits = hp . wp^T + bp  -> log_softmax;  v = tanh(hv . wv^T + bv).
 * Connect4GNN.py:48-57 (hp = hv = features, K = 3136) and the last layers of
 * TicTacToeGNN.py:36-45 (hp = relu(fc1), hv = relu(fc2), K = 512).  A <= 32.
 *   logp [B][A], pi [B][A] = exp(logp) (may be NULL), v [B].
 * ws: device scratch of az_heads_ws_bytes(B, K, A) bytes (per-chunk partial dot products,
 * summed in a fixed order). */
size_t az_heads_ws_bytes(int B, int K, int A);
int az_heads_fwd(const float* hp, int ldhp, const float* hv, int ldhv, int B, int K,
                 const float* wp, const float* bp, int A, const float* wv, const float* bv,
                 float* logp, float* pi, float* v, void* ws, size_t ws_bytes, void* stream);

/* Connect4 trunk and policy/value heads in one call: az_c4_trunk_fwd then az_heads_fwd on the
 * feature rows (Connect4Net.py:42-60; Connect4GNN.py:48-57), bit-identical to that pair.  For
 * B <= 320 and A <= 8 it is ONE launch (the heads read the features from the trunk's LDS tile);
 * otherwise the two launches, with ws >= az_heads_ws_bytes(B, 3136, A).  feat [B][3136] is
 * written either way; boards may be az_host_alloc memory (read in place). */
int az_c4_trunk_heads_fwd(const int8_t* boards, int B, const float* conv1_w, const float* conv1_b,
                          const float* conv2_w, const float* conv2_b, const float* wp,
                          const float* bp, int A, const float* wv, const float* bv, float* feat,
                          float* logp, float* pi, float* v, void* ws, size_t ws_bytes,
                          void* stream);

/* The whole Connect4 leaf evaluation of MCTS.search (MCTS.py:169-174 via Connect4GNN.py:59-120:
 * predict and predict_with_gnn of the same boards) as ONE host call with direct launches:
 * trunk + standard heads (az_c4_trunk_heads_fwd), then output_transform + heads on the same
 * features (az_transform_heads_fwd).  Outputs are bit-identical to those calls.  Built for the
 * batch-1 path, where a hipGraph replay costs more host time than these 4 launches. */
typedef struct az_c4_eval {
  const float* conv1_w; const float* conv1_b; const float* conv2_w; const float* conv2_b;
  const float* fc_policy_w; const float* fc_policy_b; const float* fc_value_w;
  const float* fc_value_b;
  int A;                                   /* actions (fc_policy rows) */
  const float* ot0_w; const float* ot0_b;  /* output_transform.0 [3136][3136], [3136] */
  const float* ot2_w; const float* ot2_b;  /* output_transform.2; all four NULL: no GNN tail */
  int max_B;                               /* capacity of the scratch below */
  float* feat; float* hidden; float* y;    /* device [max_B][3136] each (hidden/y: GNN only) */
  float* logp; float* glogp;               /* device [max_B][A] */
  void* ws; size_t ws_bytes;               /* >= az_transform_heads_ws_bytes(max_B, 3136, A) */
  /* Optional (both NULL: four launches).  The batch <= 2 evaluation in ONE launch
   * (c4_leaf_kernel, az_gemm.hip): sync = device int[4096], zeroed once by the caller and left
   * zero by every launch; err = host-visible int (az_host_alloc) the launch sets to 1 if its
   * in-kernel hand-over timed out -- the outputs are then invalid: zero sync and *err, and call
   * again without them.  One evaluation at a time per sync buffer. */
  int* sync; int* err;
} az_c4_eval;
/* v != NULL: standard heads into pi [B][A] (may be NULL) and v [B];  gv != NULL: the GNN tail
 * into gpi / gv.  boards, pi, v, gpi, gv may be az_host_alloc memory.  With v == NULL (the
 * batched predict_with_gnn alone) and registered output_transform weights, the trunk writes
 * output_transform.0's operand already split for the fp16-form GEMM into the last
 * az_transform_heads_ws_bytes-sized region of e->ws; the GNN tail runs as
 * az_transform_heads_fwd with y = NULL (e->y is not written for B > 8), so the outputs are
 * bit-identical to az_c4_trunk_fwd + az_transform_heads_fwd(y = NULL).  Above 64 rows that tail
 * is ONE GEMM (output_transform.0) and one kernel that sums its split-K slabs, applies bias and
 * ReLU and runs the heads composed with output_transform.2 on the rows (az_transform_heads_fwd
 * below); up to 64 rows both GEMMs run.  Both v and gv above 320 rows (predict_both): the same
 * hand-off, and the trunk kernel that writes the split operand also forms the standard heads from
 * the rows in its LDS tile -- bit-identical to az_heads_fwd on feat.  e->feat and e->hidden are
 * scratch: above 64 rows, when output_transform.0 takes the pre-split operand for certain
 * (registered weights, their planes cached) and nothing else reads the fp32 feature rows, they
 * are not written, and the hidden rows are not written when output_transform.0 leaves split-K
 * slabs (the fused kernel keeps them in registers). */
int az_c4_eval_fwd(const az_c4_eval* e, const int8_t* boards, int B, float* pi, float* v,
                   float* gpi, float* gv, void* stream);

/* Connect4Net trunk on an n x n board with n in {4, 5, 6, 8} (connect4/Connect4Net.py:42-49 with
 * Connect4Game(board_size), connect4/Connect4Game.py:123; the 7x7 board is az_c4_trunk_fwd):
 * conv1 3x3 p1 + ReLU -> conv2 3x3 p1 + ReLU -> NCHW flatten in ONE launch, one workgroup per
 * board, conv1's plane and the feature row in LDS.  Every output is the fmaf chain of
 * az_conv3x3_relu_fwd ((ci, kh, kw) order, out-of-range taps skipped, + bias, ReLU), so feat is
 * bit-identical to the two az_conv3x3_relu_fwd calls.
 *   boards  int8 [B][n][n] in {-1,0,1} (may be az_host_alloc memory)
 *   feat    fp32 [B][64 n^2], 16-byte aligned; conv2_w 16-byte aligned */
int az_c4n_trunk_fwd(const int8_t* boards, int B, int n, const float* conv1_w,
                     const float* conv1_b, const float* conv2_w, const float* conv2_b,
                     float* feat, void* stream);
/* The same launch followed, in the same workgroup, by the policy/value heads of the board's
 * feature row read from LDS (Connect4Net.py:42-60; Connect4GNN.py:48-57): ONE launch at every B,
 * no workspace, bit-identical to az_c4n_trunk_fwd + az_heads_fwd(K = 64 n^2).  feat may be NULL
 * (the rows are then not stored); pi may be NULL; logp [B][A], v [B]; A <= 32. */
int az_c4n_trunk_heads_fwd(const int8_t* boards, int B, int n, const float* conv1_w,
                           const float* conv1_b, const float* conv2_w, const float* conv2_b,
                           const float* wp, const float* bp, int A, const float* wv,
                           const float* bv, float* feat, float* logp, float* pi, float* v,
                           void* stream);

/* The whole Connect4 leaf evaluation of MCTS.search (MCTS.py:169-174 via Connect4GNN.py:59-120:
 * predict and predict_with_gnn of the same boards) on an n x n board, n in {4, 5, 6, 8}, as ONE
 * host call with direct launches: az_c4n_trunk_heads_fwd (the heads formed only when v is asked
 * for, feat stored only for the GNN tail), then az_transform_heads_fwd(y = NULL) on feat.  One
 * launch for v alone, four with gv.  At every B the outputs are bit-identical to
 * az_conv3x3_relu_fwd x 2, az_heads_fwd and az_transform_heads_fwd(y = NULL) called one by one.
 * Up to 8 rows both output_transform layers are GEMVs whose per-output chain does not depend on
 * the number of rows and the heads run one workgroup per row, so a row of a batch of <= 8 is
 * bit-identical to the same board evaluated alone. */
typedef struct az_c4n_eval {
  const float* conv1_w; const float* conv1_b; const float* conv2_w; const float* conv2_b;
  const float* fc_policy_w; const float* fc_policy_b; const float* fc_value_w;
  const float* fc_value_b;
  int A;                                   /* actions (fc_policy rows), <= 32 */
  const float* ot0_w; const float* ot0_b;  /* output_transform.0 [F][F], [F] */
  const float* ot2_w; const float* ot2_b;  /* output_transform.2; all four NULL: no GNN tail */
  int max_B;                               /* capacity of the scratch below */
  float* feat; float* hidden; float* y;    /* device [max_B][F] (hidden: GNN only; y: not used,
                                              may be NULL) */
  float* logp; float* glogp;               /* device [max_B][A] */
  void* ws; size_t ws_bytes;               /* GNN tail: >= az_c4n_eval_ws_bytes(max_B, n, A);
                                              without one ws may be NULL */
  int n;                                   /* board side: 4, 5, 6 or 8 */
  int F;                                   /* 64 n^2 */
} az_c4n_eval;
/* Workspace of a descriptor with a GNN tail (az_transform_heads_ws_bytes(max_B, 64 n^2, A), so
 * every GEMM plan is the one the call on its own gets).  0 for a shape az_c4n_eval_fwd rejects. */
size_t az_c4n_eval_ws_bytes(int max_B, int n, int A);
/* v != NULL: standard heads into pi [B][A] (may be NULL) and v [B];  gv != NULL: the GNN tail
 * into gpi / gv; at least one of them.  boards, pi, v, gpi, gv may be az_host_alloc memory.
 * 1 <= B <= max_B.  A bad shape (n outside {4, 5, 6, 8} -- 7 is az_c4_eval_fwd's --, A > 32,
 * F != 64 n^2, B), a null pointer or a small workspace returns AZ_EINVAL before anything is
 * launched. */
int az_c4n_eval_fwd(const az_c4n_eval* e, const int8_t* boards, int B, float* pi, float* v,
                    float* gpi, float* gv, void* stream);

/* Connect4Net trunk on a rectangular board of nx columns and ny rows, (nx, ny) in {(7, 6), (6, 5),
 * (5, 4), (8, 7)} -- the standard Connect4 board and its nearest relatives (Connect4Game(board_size
 * = nx, rows = ny); square boards are az_c4_trunk_fwd / az_c4n_trunk_fwd).  The network reads the
 * board as a [1][nx][ny] image (Connect4Net.py:43), so the convolutions run with H = nx, W = ny and
 * feature c * nx*ny + x * ny + y is channel c at column x, row y.  conv1 3x3 p1 + ReLU -> conv2 3x3
 * p1 + ReLU -> NCHW flatten in ONE launch, one workgroup per board, conv1's plane and the feature
 * row in LDS; feat is bit-identical to two az_conv3x3_relu_fwd(H = nx, W = ny) calls.
 *   boards  int8 [B][nx][ny] in {-1,0,1} (may be az_host_alloc memory)
 *   feat    fp32 [B][64 nx ny], 16-byte aligned; conv2_w 16-byte aligned */
int az_c4r_trunk_fwd(const int8_t* boards, int B, int nx, int ny, const float* conv1_w,
                     const float* conv1_b, const float* conv2_w, const float* conv2_b,
                     float* feat, void* stream);
/* The same launch followed, in the same workgroup, by the policy/value heads of the board's
 * feature row read from LDS: ONE launch at every B, no workspace, bit-identical to
 * az_c4r_trunk_fwd + az_heads_fwd(K = 64 nx ny).  feat may be NULL (the rows are then not
 * stored); pi may be NULL; logp [B][A], v [B]; A <= 32. */
int az_c4r_trunk_heads_fwd(const int8_t* boards, int B, int nx, int ny, const float* conv1_w,
                           const float* conv1_b, const float* conv2_w, const float* conv2_b,
                           const float* wp, const float* bp, int A, const float* wv,
                           const float* bv, float* feat, float* logp, float* pi, float* v,
                           void* stream);

/* az_c4n_eval_fwd for the rectangular boards above: the whole leaf evaluation (predict and
 * predict_with_gnn of the same boards) as ONE host call with direct launches --
 * az_c4r_trunk_heads_fwd (the heads formed only when v is asked for, feat stored only for the GNN
 * tail), then az_transform_heads_fwd(y = NULL) on feat.  One launch for v alone, four with gv.  At
 * every B the outputs are bit-identical to az_conv3x3_relu_fwd x 2, az_heads_fwd and
 * az_transform_heads_fwd(y = NULL) called one by one, and a row of a batch of <= 8 is
 * bit-identical to the same board evaluated alone.  The fields are az_c4n_eval's with nx, ny in
 * place of n. */
typedef struct az_c4r_eval {
  const float* conv1_w; const float* conv1_b; const float* conv2_w; const float* conv2_b;
  const float* fc_policy_w; const float* fc_policy_b; const float* fc_value_w;
  const float* fc_value_b;
  int A;                                   /* actions (fc_policy rows), <= 32 */
  const float* ot0_w; const float* ot0_b;  /* output_transform.0 [F][F], [F] */
  const float* ot2_w; const float* ot2_b;  /* output_transform.2; all four NULL: no GNN tail */
  int max_B;                               /* capacity of the scratch below */
  float* feat; float* hidden; float* y;    /* device [max_B][F] (hidden: GNN only; y: not used,
                                              may be NULL) */
  float* logp; float* glogp;               /* device [max_B][A] */
  void* ws; size_t ws_bytes;               /* GNN tail: >= az_c4r_eval_ws_bytes(max_B, nx, ny, A);
                                              without one ws may be NULL */
  int nx; int ny;                          /* columns, rows: (7, 6), (6, 5), (5, 4) or (8, 7) */
  int F;                                   /* 64 nx ny */
} az_c4r_eval;
/* Workspace of a descriptor with a GNN tail (az_transform_heads_ws_bytes(max_B, 64 nx ny, A)).
 * 0 for a shape az_c4r_eval_fwd rejects. */
size_t az_c4r_eval_ws_bytes(int max_B, int nx, int ny, int A);
/* v != NULL: standard heads into pi [B][A] (may be NULL) and v [B];  gv != NULL: the GNN tail
 * into gpi / gv; at least one of them.  boards, pi, v, gpi, gv may be az_host_alloc memory.
 * 1 <= B <= max_B.  A bad shape ((nx, ny) outside the four above -- a square (n, n) is named as
 * az_c4_eval_fwd's or az_c4n_eval_fwd's board --, A > 32, F != 64 nx ny, B), a null pointer or a
 * small workspace returns AZ_EINVAL before anything is launched. */
int az_c4r_eval_fwd(const az_c4r_eval* e, const int8_t* boards, int B, float* pi, float* v,
                    float* gpi, float* gv, void* stream);

/* TicTacToeNet trunk, tictactoe/TicTacToeNet.py:33-36 (== TicTacToeGNNWrapper.extract_features,
 * TicTacToeGNN.py:25-34): conv1 3x3 p1 + ReLU -> conv2 3x3 p1 + ReLU -> conv3 3x3 p0 + ReLU ->
 * NCHW flatten in ONE launch, one workgroup per board, both intermediate planes in LDS.  Every
 * output is the fmaf chain of az_conv3x3_relu_fwd ((ci, kh, kw) order, out-of-range taps skipped,
 * + bias, ReLU), so feat is bit-identical to the three az_conv3x3_relu_fwd calls.
 *   boards  int8 [B][n][n] in {-1,0,1}, n in {3, 4, 5} (may be az_host_alloc memory)
 *   feat    fp32 [B][128 (n-2)^2] */
int az_ttt_trunk_fwd(const int8_t* boards, int B, int n, const float* conv1_w,
                     const float* conv1_b, const float* conv2_w, const float* conv2_b,
                     const float* conv3_w, const float* conv3_b, float* feat, void* stream);

/* The whole TicTacToe leaf evaluation of MCTS.search (MCTS.py:169-174 via TicTacToeGNN.py:47-110:
 * predict and predict_with_gnn of the same boards) as ONE host call with direct launches, no
 * launch waiting on another inside a kernel:
 *   az_ttt_trunk_fwd;  h1 = relu(fc1 feat), h2 = relu(fc2 feat);  az_heads_fwd(h1, h2)   (v)
 *   hidden = relu(ot0 feat);  y = ot2 hidden;  h1 / h2 of y;  az_heads_fwd(h1, h2)       (gv)
 * Up to 8 rows, fc1 and fc2 -- and output_transform.0 when both v and gv are asked for -- share
 * one launch (two / three weight streams over the same rows, each output the GEMV arithmetic
 * az_gemm_f32 has at M <= 8): 4 launches for v, 6 for gv, 6 for both.  That arithmetic does not
 * depend on the number of rows, so a row of a batch of <= 8 is bit-identical to the same board
 * evaluated alone.  Above 8 rows every linear layer is az_gemm_f32 on the rest of the workspace.
 * At every B the outputs are bit-identical to az_conv3x3_relu_fwd x 3, az_gemm_f32 and az_heads_fwd
 * called one by one (the eager path was found row-invariant at 2..8 rows, so no shape needs a
 * weaker statement). */
typedef struct az_ttt_eval {
  const float* conv1_w; const float* conv1_b; const float* conv2_w; const float* conv2_b;
  const float* conv3_w; const float* conv3_b;
  const float* fc1_w; const float* fc1_b;  /* [512][F], [512] */
  const float* fc2_w; const float* fc2_b;
  const float* fc_policy_w; const float* fc_policy_b;  /* [A][512], [A] */
  const float* fc_value_w; const float* fc_value_b;    /* [1][512], [1] */
  int n;                                   /* board side, 3..5 */
  int A;                                   /* actions (fc_policy rows), <= 32 */
  int F;                                   /* 128 (n-2)^2 */
  const float* ot0_w; const float* ot0_b;  /* output_transform.0 [F][F], [F] */
  const float* ot2_w; const float* ot2_b;  /* output_transform.2; all four NULL: no GNN tail */
  int max_B;                               /* capacity of the scratch below */
  float* feat;                             /* device [max_B][F] */
  float* h1; float* h2;                    /* device [max_B][512] each */
  float* hidden; float* y;                 /* device [max_B][F] each (GNN tail only) */
  float* logp; float* glogp;               /* device [max_B][A] */
  void* ws; size_t ws_bytes;               /* >= az_ttt_eval_ws_bytes(max_B, n, A) */
} az_ttt_eval;
/* Workspace for the descriptor: the heads' partials and, above 8 rows, room for every split-K
 * plan az_gemm_f32 makes for these layers (so its plans are those of a large workspace).
 * 0 for a shape az_ttt_eval_fwd rejects. */
size_t az_ttt_eval_ws_bytes(int max_B, int n, int A);
/* v != NULL: standard heads into pi [B][A] (may be NULL) and v [B];  gv != NULL: the GNN tail
 * into gpi / gv; at least one of them.  boards, pi, v, gpi, gv may be az_host_alloc memory.
 * 1 <= B <= max_B.  A bad shape (n outside 3..5, A > 32, F != 128 (n-2)^2, B), a null pointer
 * or a small workspace returns AZ_EINVAL before anything is launched. */
int az_ttt_eval_fwd(const az_ttt_eval* e, const int8_t* boards, int B, float* pi, float* v,
                    float* gpi, float* gv, void* stream);

/* ---------------------------------------------------------------------------------
 * Batch-invariant evaluation (config key batch_invariant): a board's outputs are the
 * same bits whatever rides in the batch with it.  No reference counterpart: the reference evaluates
 * one board per call, which is what these entry points make every batch size equal to.
 *
 * az_gemm_exact_f32: C = act(A W^T + bias), both operands K-major fp32 (the forward nn.Linear:
 * A [M][K] row stride lda, W [N][K] row stride ldw, C [M][N] row stride ldc), fp32 accumulation on
 * v_mfma_f32_32x32x2_f32.  The arithmetic is the contract:
 *   - K is cut into S contiguous segments; S and the cut points are a function of (N, K) only,
 *     reported by az_gemm_exact_plan (HOST function, no GPU work; seg_len receives S <=
 *     AZ_EXACT_MAX_SEGMENTS lengths that sum to K);
 *   - each segment is one chain acc = fmaf(a[k], w[k], acc) in ascending k, starting from +0;
 *   - the segment sums are added in ascending order with plain fp32 adds, then bias[j] is added
 *     (when bias != NULL), then the activation (AZ_ACT_NONE or AZ_ACT_RELU) is applied.
 * M sizes the launch (the grid, and blocks of 1 / 2 / 4 waves for <= 32 / <= 64 / more rows) and
 * masks loads and stores, nothing else: row i's bits do not depend on M or on i, and a CPU loop over
 * the plan with a correctly rounded fmaf reproduces every value (a result of -0 may come out as
 * +0).  No atomics.  Rows past M / N and k past K contribute nothing whatever
 * the memory behind the operands holds (they are zeroed in LDS, not loaded).
 * M >= 0 (0: nothing to do), N % 4 == 0, K % 4 == 0; lda, ldw, ldc % 4 == 0; A, W, bias, C and ws
 * 16-byte aligned.  ws >= az_gemm_exact_ws_bytes(M, N, K): room for the S segment sums of a call
 * whose tile grid alone cannot fill the GPU (0 for a call that needs none, or a rejected shape).
 * --------------------------------------------------------------------------------- */
#define AZ_EXACT_MAX_SEGMENTS 16
int az_gemm_exact_plan(int N, int K, int* segments, int* seg_len);
size_t az_gemm_exact_ws_bytes(int M, int N, int K);
int az_gemm_exact_f32(const float* A, int lda, const float* W, int ldw, const float* bias, int act,
                      float* C, int ldc, int M, int N, int K, void* ws, size_t ws_bytes,
                      void* stream);

/* az_gemm_exact_f32 with the epilogues of the GNN node update, arguments in a descriptor.  The
 * segment chain and the plan are az_gemm_exact_f32's (az_gemm_exact_plan(N, K)); after "segment
 * sums in ascending order, then bias" comes ONE of
 *   act              AZ_ACT_NONE, AZ_ACT_RELU or AZ_ACT_SIGMOID (1 / (1 + expf(-v)));
 *   gated residual   R and G non-NULL, act = AZ_ACT_NONE: C[i][j] = fmaf(G[i*ldg+j], v, R[i*ldr+j]),
 *                    one rounding;
 * and with W2 non-NULL the launch is PAIRED: a second weight matrix [N][K] (row stride ldw), bias2,
 * act2 and output C2 (row stride ldc) share the A operand and the launch.  The plan is that of ONE
 * product, so C and C2 hold the bits of two separate calls.  No gated residual on a paired call.
 * Row i's bits depend on row i of A (and of R, G) and the weights only: not on M, not on i, not on
 * whether the call ran spread over segments or direct.  Shapes, strides and alignment as
 * az_gemm_exact_f32; ldr, ldg >= N and % 4 == 0; R, G, W2, bias2, C2 16-byte aligned.
 * ws >= az_gemm_exact_ex_ws_bytes(M, N, K, paired). */
typedef struct az_gemm_exact_desc {
  int M; int N; int K;
  const float* A; int lda;
  const float* W; int ldw;
  const float* bias; int act;
  float* C; int ldc;
  const float* W2; const float* bias2; int act2; float* C2;   /* the paired product, or all 0 */
  const float* R; int ldr; const float* G; int ldg;           /* the gated residual, or all 0 */
  void* ws; size_t ws_bytes;
} az_gemm_exact_desc;
size_t az_gemm_exact_ex_ws_bytes(int M, int N, int K, int paired);
int az_gemm_exact_ex(const az_gemm_exact_desc* d, void* stream);

/* The leaf evaluation of az_c4_eval_fwd / az_c4n_eval_fwd / az_c4r_eval_fwd / az_ttt_eval_fwd, for
 * the same networks, as ONE host call whose launch sequence is the same at B = 1 and B = 4096:
 * the board's fused trunk (az_c4_trunk_fwd, az_c4n_trunk_fwd, az_c4r_trunk_fwd, az_ttt_trunk_fwd),
 * every nn.Linear the reference computes as az_gemm_exact_f32 -- fc1 / fc2 (TicTacToe),
 * output_transform.0 and output_transform.2 as two real GEMMs, no composed heads -- and the
 * policy / value heads one workgroup per row.  Every row of pi, v, gpi, gv is bit-identical to the
 * same board evaluated alone or at any other position of any other batch. */
#define AZ_EXACT_C4 0
#define AZ_EXACT_TTT 1
typedef struct az_eval_exact {
  int game;                                /* AZ_EXACT_C4 or AZ_EXACT_TTT */
  int nx; int ny;                          /* columns, rows (TicTacToe: nx = ny = n) */
  int A;                                   /* actions (fc_policy rows), <= 32 */
  int F;                                   /* Connect4: 64 nx ny; TicTacToe: 128 (n-2)^2 */
  const float* conv1_w; const float* conv1_b; const float* conv2_w; const float* conv2_b;
  const float* conv3_w; const float* conv3_b;          /* TicTacToe only */
  const float* fc1_w; const float* fc1_b;  /* TicTacToe only: [512][F], [512] */
  const float* fc2_w; const float* fc2_b;
  const float* fc_policy_w; const float* fc_policy_b;  /* [A][F] (TicTacToe: [A][512]), [A] */
  const float* fc_value_w; const float* fc_value_b;
  const float* ot0_w; const float* ot0_b;  /* output_transform.0 [F][F], [F] */
  const float* ot2_w; const float* ot2_b;  /* output_transform.2; all four NULL: no GNN tail */
  int max_B;                               /* capacity of the scratch below */
  float* feat;                             /* device [max_B][F] */
  float* h1; float* h2;                    /* device [max_B][512] each (TicTacToe only) */
  float* hidden; float* y;                 /* device [max_B][F] each (GNN tail only) */
  float* logp; float* glogp;               /* device [max_B][A] */
  void* ws; size_t ws_bytes;               /* >= az_eval_exact_ws_bytes(max_B, game, nx, ny, A) */
} az_eval_exact;
/* 0 for a shape az_eval_exact_fwd rejects. */
size_t az_eval_exact_ws_bytes(int max_B, int game, int nx, int ny, int A);
/* v != NULL: standard heads into pi [B][A] (may be NULL) and v [B];  gv != NULL: the GNN tail
 * into gpi / gv; at least one of them.  boards int8 [B][nx][ny]; boards, pi, v, gpi, gv may be
 * az_host_alloc memory.  0 <= B <= max_B (0: nothing to do; a caller with more rows calls again
 * on the next max_B rows, which invariance makes the same result).  A board without a fused
 * trunk, A > 32, a wrong F, B > max_B, a null pointer or a small workspace returns AZ_EINVAL with
 * a message before anything is launched. */
int az_eval_exact_fwd(const az_eval_exact* e, const int8_t* boards, int B, float* pi, float* v,
                      float* gpi, float* gv, void* stream);

/* ---------------------------------------------------------------------------------
 * FrozenLakeNet (frozenlake/FrozenLakeNet.py:253-335): a leaf is a list of n = 1..5 node boards
 * (the board itself, then the next state of every valid action), S = N*N floats each:
 *   h_j  = relu(fe2 relu(fe0 x_j))                       feature_extractor, per node, hidden 128
 *   r_1  = relu(c (W_1 sum_j h_j + n b_1))               GNN layer 1 under the all-ones adjacency
 *   r_l  = relu(c n (W_l r_{l-1} + b_l))   l = 2..L      (every node row is the same from here on)
 *   pi = softmax(policy_head r_L),  v = tanh(value_head r_L)
 * with c = fp32(n^-1/2) * fp32(n^-1/2), the entry of the symmetrically normalised adjacency
 * (FrozenLakeNet.py:55-74).  Only node 0's row reaches the heads, and it equals every other row.
 * --------------------------------------------------------------------------------- */
#define AZ_FL_MAX_NODES 5
#define AZ_FL_MAX_LAYERS 4
#define AZ_FL_HIDDEN 128
/* One pointer per tensor in state_dict order; the same struct holds weights or their gradients. */
typedef struct az_fl_params {
  float* fe0_w; float* fe0_b;              /* feature_extractor.0 [128][S], [128] */
  float* fe2_w; float* fe2_b;              /* feature_extractor.2 [E][128], [E] */
  float* gnn_w[AZ_FL_MAX_LAYERS];          /* gnn_layers.i.W.weight [E][E]; entries >= L unused */
  float* gnn_b[AZ_FL_MAX_LAYERS];          /* gnn_layers.i.W.bias [E] */
  float* policy_w; float* policy_b;        /* policy_head [A][E], [A] */
  float* value_w; float* value_b;          /* value_head [1][E], [1] */
} az_fl_params;
typedef struct az_fl_eval {
  int S;                                   /* cells, N*N with N = 2..8 (<= 64) */
  int E;                                   /* embedding_dim, 64 or 128 */
  int L;                                   /* gnn_layers, 1..4 */
  int A;                                   /* actions, 4 */
  int H;                                   /* hidden size of the feature extractor, 128 */
  int max_B;                               /* most leaves one call may carry */
  az_fl_params w;                          /* weights; fe2_w and gnn_w need 16-byte alignment */
} az_fl_eval;
/* Bytes of device workspace az_fl_grads needs for max_B leaves (az_fl_eval_fwd keeps its
 * intermediates in LDS and needs none); 0 for a shape the entry points reject. */
size_t az_fl_eval_ws_bytes(int max_B, int S, int E, int L);
/* predict of B leaves in ONE launch, one workgroup per leaf: nodes f32 [B][5][S] (rows at and
 * beyond counts[b] are never read), counts i32 [B] in 1..5 (a value outside is clamped into it),
 * pi [B][A], v [B].  Every output is a fixed-order fmaf chain over that leaf's nodes and the
 * weights; no atomics, nothing shared between leaves: row b is bit-identical to the same leaf
 * evaluated alone at every B.  nodes / counts / pi / v may be az_host_alloc memory.  ws is unused
 * and may be NULL.  A null descriptor, B outside 1..max_B, S / E / L / A / H out of range or a
 * null pointer returns AZ_EINVAL before any HIP call. */
int az_fl_eval_fwd(const az_fl_eval* e, const float* nodes, const int* counts, int B, float* pi,
                   float* v, void* ws, void* stream);
/* Gradients of FrozenLakeNet.train's loss (FrozenLakeNet.py:157-160) over a batch of B leaves,
 *   loss = -1/B sum_b sum_a tpi[b][a] log(max(pi[b][a], 1e-8)) + 1/B sum_b (v[b] - tv[b])^2,
 * into one buffer per parameter (g, overwritten) and *loss (device).  Where pi < 1e-8 the clamp
 * passes no gradient (unlike az_heads_loss_bwd, which differentiates log-softmax).  dlogits
 * (nullable, [B][A]) receives dloss/dlogits.  Two launches: per-leaf forward + backward to the
 * layer deltas (in ws), then one grid that sums delta^T input over leaves in leaf order for every
 * weight (and the loss in a block of its own); no atomics, so two calls give equal bits.
 * ws >= az_fl_eval_ws_bytes(max_B, S, E, L). */
int az_fl_grads(const az_fl_eval* e, const float* nodes, const int* counts, int B,
                const float* target_pi, const float* target_v, const az_fl_params* g, float* loss,
                float* dlogits, void* ws, size_t ws_bytes, void* stream);
/* torch.nn.utils.clip_grad_norm_ (FrozenLakeNet.py:166): the L2 norm over all n <= 16 buffers
 * (bufs / sizes are HOST arrays of device pointers and element counts) into *total_norm (device),
 * then every element times min(1, max_norm / (norm + 1e-6)).  One block sums the squares in fp64
 * in a fixed order; a second launch scales. */
int az_clip_grad_norm(float* const* bufs, const int64_t* sizes, int n, float max_norm,
                      float* total_norm, void* stream);

/* Per-row GNN evaluation tail: output_transform then the heads, i.e. gnn_utils.py:115 (in the
 * 1-row form of Connect4GNN.py:108-111, where the layers are the identity, gnn_utils.py:35-36)
 * followed by Connect4GNN.py:48-57 -- the batched predict_with_gnn after extract_features:
 *   hidden = relu(x W0^T + b0);  y = hidden W2^T + b2;  logp = log_softmax(y wp^T + bp);
 *   pi = exp(logp) (may be NULL);  v = tanh(y wv^T + bv).
 * x, hidden, y: [B][F]; W0, W2: [F][F] (nn.Linear layout); wp [A][F]; wv [1][F]; A <= 32.
 * When the second GEMM is split over K, its slab reduction, bias, the store of y and the heads'
 * dot products run in one pass (y is not re-read); results equal az_gemm_f32 + az_heads_fwd
 * bit for bit.  ws: >= az_heads_ws_bytes(B, F, A) rounded up to 256 B; az_transform_heads_ws_bytes
 * leaves room for the split-K slabs (a smaller workspace only limits the K split).
 * y may be NULL when only the heads are wanted (the evaluators): y is then never written.
 * For A <= 8 and B > 64 it is never computed either: the heads are linear in y, so
 *   logits = hidden Wc^T + bc,  Wc = [wp; wv] W2  ((A + 1) x F),  bc = [wp; wv] b2 + [bp; bv],
 * with Wc / bc accumulated in fp64 and rounded once to fp32 (compose_heads_kernel).  They are
 * cached per weight generation when W2, b2, wp, bp, wv and bv all lie in registered storage
 * (az_weights_register; az_weights_changed covers the heads' weights too) and composed per call
 * into the workspace otherwise -- the same kernels, so the same bits.  output_transform.2 then
 * costs a 9-row product instead of a B-row GEMM: when output_transform.0 leaves split-K slabs,
 * ONE kernel sums them in slab order, adds b0, applies ReLU (the plain reduce's arithmetic: the
 * hidden rows keep their bits) and runs the heads on the rows in registers; when it leaves none
 * (stream-K batches) the standard heads kernel reads the fp32 hidden rows.  The choice depends
 * only on B, A, y == NULL and the workspace (az_transform_heads_ws_bytes holds the per-call
 * Wc), never on registration.  Other shapes with y == NULL (B <= 64, A > 8) keep the earlier
 * forms: on the fp16-form split-K tiles every block folds its tile of y into per-row dot products
 * with wp / wv and heads_tiles_finalize_kernel sums them in tile order, else y is formed in
 * workspace scratch (az_transform_heads_ws_bytes includes it).  y == NULL results are the same
 * function to fp32 rounding, not bit-identical to the y != NULL path (tests/test_gpu_kernels.py
 * and tests/test_gpu_composed_heads.py bound it). */
size_t az_transform_heads_ws_bytes(int B, int F, int A);
/* Its second half alone: y = x W^T + b, then the heads of y (same fusion, same workspace). */
int az_linear_heads_fwd(const float* x, int B, int F, const float* w, const float* b,
                        const float* wp, const float* bp, int A, const float* wv, const float* bv,
                        float* y, float* logp, float* pi, float* v, void* ws, size_t ws_bytes,
                        void* stream);
int az_transform_heads_fwd(const float* x, int B, int F, const float* w0, const float* b0,
                           const float* w2, const float* b2, const float* wp, const float* bp,
                           int A, const float* wv, const float* bv, float* hidden, float* y,
                           float* logp, float* pi, float* v, void* ws, size_t ws_bytes,
                           void* stream);

/* ---------------------------------------------------------------------------------
 * GNN message passing (gnn_utils.py:5-74) over a destination-sorted CSR graph.
 * The reference's star (row 0 = destination, rows 1..N-1 = sources) is the CSR with
 * rowptr = [0, N-1, N-1, ...], col = [1..N-1]; the synthetic grid has one segment per node.
 * --------------------------------------------------------------------------------- */
typedef struct az_graph {
  int V, E;
  const int* rowptr;    /* [V+1] */
  const int* col;       /* [E] source node of edge e (sorted by destination) */
  const int* edge_dst;  /* [E] destination node of edge e */
  int D;                /* number of destinations with >= 1 in-edge */
  const int* dst_rows;  /* [D] those destinations (ascending) */
  /* backward only (may be NULL for forward use): */
  const int* src_rowptr;  /* [V+1] reverse CSR by source */
  const int* src_edges;   /* [E] edge ids grouped by source (ascending within a source) */
  const int* dst_index;   /* [V] compact destination index, -1 when no in-edge */
  int max_deg;            /* max in-degree; only picks kernels, forward and backward: an
                             understated value is slower, never wrong (edges are not dropped) */
  int band;               /* max |src - dst| over the edges when the caller knows it, else 0.
                             Eval-mode layers on F = 64, H = 128 graphs with 0 < band <= 32 (the
                             row-major grid: 32) run the band kernel (az_gnn_layer_infer); a
                             source outside the claimed band takes a slow path, never wrong */
} az_graph;

typedef struct az_gnn_layer_w {     /* GNNLayer parameters, state_dict order */
  const float* att_w1; const float* att_b1;   /* attention.0  [H][2F], [H] */
  const float* att_w2; const float* att_b2;   /* attention.2  [1][H],  [1] */
  const float* upd_w1; const float* upd_b1;   /* update_net.0 [F][2F], [F] */
  const float* upd_w2; const float* upd_b2;   /* update_net.2 [F][F],  [F] */
  const float* gate_w; const float* gate_b;   /* gate.0       [F][2F], [F] */
} az_gnn_layer_w;

typedef struct az_gnn_layer_grads { /* gradients, same layout as az_gnn_layer_w (written) */
  float* att_w1; float* att_b1; float* att_w2; float* att_b2;
  float* upd_w1; float* upd_b1; float* upd_w2; float* upd_b2;
  float* gate_w; float* gate_b;
} az_gnn_layer_grads;

/* alpha[e] = sigmoid(w2 . relu(P[dst(e)][2q] + P[col(e)][2q+1] + b1) + b2)
 * the factored attention MLP of GNNLayer.compute_attention (gnn_utils.py:30-32,48-55):
 * W1 [t; x] = W1[:, :F] t + W1[:, F:] x, so both halves are projected once per NODE.
 * P [V][2H] (row stride ldp) interleaves them: P[v][2q] = W1[q, :F].x_v,
 * P[v][2q+1] = W1[q, F:].x_v, which is exactly the GEMM x . W1'^T with W1 [H][2F] read as
 * [2H][F] (row stride F).  H % 2 == 0. */
int az_gnn_attn_score_fwd(const az_graph* g, const float* P, int ldp, int H,
                          const float* b1, const float* w2, const float* b2,
                          float* alpha, void* stream);

/* agg[d] = sum_{e in seg(d)} a'_e x[col(e)],  a' = a / sum(a) when sum(a) > 0
 * (gnn_utils.py:57-65), for the D destinations g->dst_rows (D == V means every row);
 * other rows of agg are not written.  Edges are summed in CSR order (deterministic).
 * x, agg: [V][F] with row strides ldx, ldagg; F % 4 == 0. */
int az_gnn_aggregate_fwd(const az_graph* g, const float* x, int ldx, int F,
                         const float* alpha, float* agg, int ldagg, void* stream);

/* One full GNNLayer.forward (gnn_utils.py:34-74) generalised per destination:
 * x_out[d] = x[d] + sigmoid(Wg[x_d;agg_d]+bg) * (Wu2 relu(Wu1[x_d;agg_d]+bu1)+bu2) for the D
 * destinations, x_out[v] = x[v] for every other row (a 1-row GNNLayer input is returned
 * unchanged, gnn_utils.py:35-36).  x_out may not alias x.  `ws` is a device workspace of
 * az_gnn_layer_ws_bytes() bytes; when `save` is non-NULL the activations the backward
 * pass needs are kept in it (see az_gnn_layer_bwd). */
size_t az_gnn_layer_ws_bytes(int V, int E, int D, int F, int H);
int az_gnn_layer_fwd(const az_graph* g, const float* x, int F, int H, const az_gnn_layer_w* w,
                     float* x_out, void* ws, size_t ws_bytes, void* stream);

/* Inference form of az_gnn_layer_fwd (eval mode: same function, nothing kept for a backward
 * pass).  F == 64, H == 128:
 *  - 0 < g->band <= 32 (node-ordered band graphs: the synthetic grid, config 5): ONE band
 *    kernel launch (after a 221 KB weight split into ws): per 64-destination tile, projections,
 *    attention scores, normalised aggregation, gate / update MLPs and the gated residual in LDS /
 *    registers on fp32-accurate bf16x3 MFMAs; x and the source projection of each node are read /
 *    computed once, in a rolling window (gnn_utils.py:30-74);
 *  - else 0 < g->max_deg <= 4: ONE source-projection GEMM (Ps = x W1[:, F:]^T, [V][H] in ws) plus
 *    ONE fused kernel per 64-destination tile;
 *  - other shapes run az_gnn_layer_fwd.
 * ws >= az_gnn_layer_infer_ws_bytes(g, F, H). */
size_t az_gnn_layer_infer_ws_bytes(const az_graph* g, int F, int H);
int az_gnn_layer_infer(const az_graph* g, const float* x, int F, int H, const az_gnn_layer_w* w,
                       float* x_out, void* ws, size_t ws_bytes, void* stream);
/* The network's LAST layer followed by output_transform (gnn_utils.py:87-117 in eval mode:
 * y = output_transform(GNNLayer(x)), output_transform = Linear + ReLU + Linear on every row).
 * On band graphs (see az_gnn_layer_infer) ONE launch: the tile's layer output never leaves LDS
 * and only y is written.  Otherwise az_gnn_layer_infer into ws, then az_mlp2_fwd.
 * ot_w0 / ot_w2: [F][F] nn.Linear weights; y may not alias x.
 * ws >= az_gnn_layer_ot_infer_ws_bytes(g, F, H). */
size_t az_gnn_layer_ot_infer_ws_bytes(const az_graph* g, int F, int H);
int az_gnn_layer_ot_infer(const az_graph* g, const float* x, int F, int H,
                          const az_gnn_layer_w* w, const float* ot_w0, const float* ot_b0,
                          const float* ot_w2, const float* ot_b2, float* y, void* ws,
                          size_t ws_bytes, void* stream);
/* The two launches of the fused path, separately (profiling / callers that keep Ps):
 * Ps [V][H] = x W1[:, F:]^T, then the fused layer kernel given Ps (copies non-destination rows
 * of x to x_out first when D < V).  Fused shapes only (AZ_EINVAL otherwise). */
int az_gnn_source_proj_fwd(const az_graph* g, const float* x, int F, int H,
                           const az_gnn_layer_w* w, float* Ps, void* ws, size_t ws_bytes,
                           void* stream);
int az_gnn_layer_fused_fwd(const az_graph* g, const float* x, const float* Ps, int F, int H,
                           const az_gnn_layer_w* w, float* x_out, void* stream);

/* GNNLayer's gated node update on its own (gnn_utils.py:18-28 gate / update_net, :67-74), for a
 * caller that computes the attention and the aggregation itself (SURVEY §8b
 * az_gnn_node_update_fwd).  The destinations are dst_rows[0..D) -- the rows the reference's
 * destination mask selects; D == V with dst_rows NULL means every row:
 *   c = [x_d ; agg_d],  gate = sigmoid(Wg c + bg),  u1 = relu(Wu1 c + bu1),  u = Wu2 u1 + bu2,
 *   x_out[d] = x[d] + gate * u,  x_out[v] = x[v] on every other row.
 * x, agg, x_out: [V][F] (agg read on the destination rows only); x_out may not alias x;
 * F % 16 == 0.  gate_w / upd_w1: [F][2F], upd_w2: [F][F] (nn.Linear layout).
 * save: [3][D][F] written (gate, u1, u), read by az_gnn_node_update_bwd.
 * ws >= az_gnn_node_update_ws_bytes(D, F).  The same GEMMs, in the same order, as the update
 * inside az_gnn_layer_fwd. */
size_t az_gnn_node_update_ws_bytes(int D, int F);
int az_gnn_node_update_fwd(const float* x, const float* agg, int V, int F, int D,
                           const int* dst_rows, const float* gate_w, const float* gate_b,
                           const float* upd_w1, const float* upd_b1, const float* upd_w2,
                           const float* upd_b2, float* x_out, float* save, void* ws,
                           size_t ws_bytes, void* stream);

/* output_transform, gnn_utils.py:101-105,115: y = W2 relu(W0 x + b0) + b2 on M rows.
 * hidden: [M][F] scratch (kept for the backward pass); ws: optional split-K workspace. */
int az_mlp2_fwd(const float* x, int M, int F, const float* w0, const float* b0,
                const float* w2, const float* b2, float* hidden, float* y,
                void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * GNN leaf evaluation over the leaf's children.  The reference's GNNLayer.forward is written for
 * "row 0 is the target state, the other rows are path states" (gnn_utils.py:38-43), and
 * Connect4Net.predict documents `neighbor_states` as an "optional list of neighboring states for GNN
 * enhancement" (Connect4Net.py:110); FrozenLakeNet.predict builds that neighbourhood, the board plus
 * the next state of every valid action.  These entry points evaluate such stars at inference.
 * --------------------------------------------------------------------------------- */
#define AZ_STAR_MAX_NODES 9    /* a leaf and up to 8 children */
#define AZ_STAR_MAX_STARS 8
#define AZ_STAR_MAX_LAYERS 4
#define AZ_STAR_HIDDEN 128     /* attention.0's hidden width in the networks (gnn_utils.py:12) */
/* The layer stack of PolicyValueGNN in eval mode (gnn_utils.py:34-74, 109-112) on B small stars.
 *   x       star b: counts[b] rows of F floats at x + b * ldstar; row 0 the leaf, rows 1.. its
 *           neighbours in the caller's order.  Rows at or beyond counts[b] are never read.
 *   counts  int [B], mapped host memory or HBM; the kernels clamp a value into [1, 9] themselves
 *   x0      [B][F]: row 0 of each star after L layers (only row 0 changes in a layer, so no other
 *           row is written anywhere).  May not alias x.
 * A one-row star passes unchanged, x0[b] = x[b][0] bit for bit (gnn_utils.py:35-36).  The weights
 * are sigmoid(attention(.)) and are divided by their sum only when the sum is > 0
 * (gnn_utils.py:58-59): with every weight underflowed to 0 the aggregate is 0.
 * Four launches per layer: attention.0 factored per node (W1 [t; x] = W1[:, :F] t + W1[:, F:] x)
 * with blocks that own 16 hidden units x 256 columns of one star, so its weights come from HBM
 * once and not once per node; the attention weights and the aggregate per star; gate.0 and update_net.0 on
 * [t; agg] as one paired GEMV grid over the B row 0s; update_net.2 with the gated residual
 * t + g * u.  Every output is a fixed-order fp32 fmaf chain, no atomics, nothing shared between
 * stars: star b's row does not depend on B or on the other stars of the call, and two calls give
 * equal bits.
 * 1 <= B <= 8 (B == 0: nothing to do), F % 4 == 0, H % 2 == 0, 0 <= L <= 4, ldstar >= F and
 * ldstar % 4 == 0; x, x0, ws and the weight matrices 16-byte aligned; anything else returns
 * AZ_EINVAL with a message before any launch.  ws >= az_gnn_star_infer_ws_bytes(B, F, H, L)
 * (0 for a rejected shape). */
size_t az_gnn_star_infer_ws_bytes(int B, int F, int H, int L);
int az_gnn_star_infer(const float* x, int ldstar, const int* counts, int B, int F, int H, int L,
                      const az_gnn_layer_w* layers, float* x0, void* ws, size_t ws_bytes,
                      void* stream);

/* The same layer stack on ANY number of stars of any size, packed: the batched route of lock-step
 * self-play with gnn_neighbors (hundreds of leaves per round), where the node update is dense
 * matrix products rather than weight streaming.
 *   x       [V][F], the packed feature rows of B stars; never written, never copied
 *   offs    int [B+1] in HBM (or mapped host memory), ascending, offs[0] = 0, offs[B] = V: star b is
 *           rows offs[b] .. offs[b+1]-1, its first row the leaf, the rest its neighbours in the
 *           caller's order.  Any star size >= 1 (TicTacToe 3x3: up to 10 rows, 5x5: up to 26).
 *   x0      [B][F]: row 0 of each star after L layers.  May not alias x.
 * Semantics are az_gnn_star_infer's: weights sigmoid(attention(.)), divided by their sum only when
 * the sum is > 0 (all 0: the aggregate is 0), summed and aggregated in neighbour order; a one-row
 * star returns its row bit for bit at every L (L = 0 included).
 * Per layer: attention.0 factored per node as ONE K-major product of the V rows with att_w1 read
 * as [2H][F] (from layer 1 on a second B-row product for the updated row 0s); one kernel that forms
 * the weights, their sum, the aggregate and the operand row TA[b] = [t | agg] ([B][2F]; HBM-bound:
 * (n-1) F 4 bytes read and 2 F 4 bytes written per star); gate.0 and update_net.0 as two plain
 * K-major GEMMs on TA (K = 2F); update_net.2 (K = F) with the gated-residual epilogue.  All
 * products go through az_gemm_f32's dispatch, so which tile serves which B is its business: a
 * row is within 1e-5 of az_gnn_star_infer's but NOT bit-identical to it, and may differ between
 * values of B.  Two identical calls give equal bits (no atomics, fixed summation orders).
 * B >= 1 (B == 0: nothing to do), V >= B, F % 16 == 0, H % 4 == 0, 0 <= L <= 4; x, x0, ws and the
 * weight matrices 16-byte aligned.  A bad shape, a null or misaligned pointer or a short workspace
 * returns AZ_EINVAL with a message before any launch; so does a non-ascending offs when offs is
 * host memory (az_host_alloc / pinned) -- offs in HBM is clamped into the V rows by the kernels.
 * ws >= az_gnn_star_batch_ws_bytes(B, V, F, H, L) (0 for a rejected shape). */
size_t az_gnn_star_batch_ws_bytes(int B, int V, int F, int H, int L);
int az_gnn_star_batch_infer(const float* x, const int* offs, int B, int V, int F, int H, int L,
                            const az_gnn_layer_w* layers, float* x0, void* ws, size_t ws_bytes,
                            void* stream);

/* predict_with_gnn of a Connect4 leaf with its neighbourhood (Connect4GNN.py:86-120 on the star
 * [board] + neighbor_states: extract_features, PolicyValueGNN.forward, the heads of row 0) as ONE
 * host call with direct launches: the board's fused trunk (az_c4_trunk_fwd for 7x7,
 * az_c4n_trunk_fwd for 4x4, 5x5, 6x6 and 8x8, az_c4r_trunk_fwd for 7x6, 6x5, 5x4 and 8x7) on the
 * 9 board slots of every star, az_gnn_star_infer on the feature rows, then
 * az_transform_heads_fwd(y = NULL) on the B row 0s.  Another board shape returns AZ_EINVAL. */
typedef struct az_c4_star_eval {
  const float* conv1_w; const float* conv1_b; const float* conv2_w; const float* conv2_b;
  const float* fc_policy_w; const float* fc_policy_b; const float* fc_value_w;
  const float* fc_value_b;
  int A;                                   /* actions (fc_policy rows), <= 32 */
  const float* ot0_w; const float* ot0_b;  /* output_transform.0 [F][F], [F] */
  const float* ot2_w; const float* ot2_b;  /* output_transform.2 */
  int nx; int ny;                          /* columns, rows */
  int F;                                   /* 64 nx ny */
  int L;                                   /* GNN layers, 0..4 */
  az_gnn_layer_w layers[AZ_STAR_MAX_LAYERS];   /* entries >= L unused */
  int max_B;                               /* most stars one call may carry, <= 8 */
  float* feat;                             /* device [max_B * 9][F] */
  float* x0; float* hidden;                /* device [max_B][F] each */
  float* glogp;                            /* device [max_B][A] */
  void* ws; size_t ws_bytes;               /* >= az_c4_star_eval_ws_bytes(max_B, nx, ny, A, L) */
} az_c4_star_eval;
/* 0 for a shape az_c4_star_eval_fwd rejects. */
size_t az_c4_star_eval_ws_bytes(int max_B, int nx, int ny, int A, int L);
/* boards int8 [B][9][nx ny] in the project's [column][row] order (slot i of star b is its row i; a
 * slot at or beyond counts[b] may hold anything: its features are never read), counts int [B],
 * gpi [B][A] (may be NULL), gv [B].  boards, counts, gpi and gv may be az_host_alloc memory.
 * 0 <= B <= min(max_B, 8) (0: nothing to do).  A row is bit-identical to the same star evaluated
 * alone.  A bad shape, a null pointer or a small workspace returns AZ_EINVAL before any launch. */
int az_c4_star_eval_fwd(const az_c4_star_eval* e, const int8_t* boards, const int* counts, int B,
                        float* gpi, float* gv, void* stream);

/* TicTacToe stars: a leaf of an n x n board has up to n^2 children, so a star has up to 10 / 17 /
 * 26 rows at n = 3 / 4 / 5 -- more than the 9 row slots az_gnn_star_infer is built around. */
#define AZ_TTT_STAR_MAX_NODES 26   /* a 5x5 leaf and its 25 children */
/* The layer stack of PolicyValueGNN in eval mode (gnn_utils.py:34-74, 109-112) on B <= 8 PACKED
 * stars of 1 .. 26 rows: az_gnn_star_infer's arithmetic on az_gnn_star_batch_infer's layout.
 *   x       [V][F], the packed feature rows of the B stars; never written
 *   offs    int [B+1], mapped host memory or HBM, ascending, offs[0] = 0, offs[B] = V: star b is
 *           rows offs[b] .. offs[b+1]-1, its first row the leaf, the rest its neighbours in the
 *           caller's order
 *   x0      [B][F]: row 0 of each star after L layers.  May not alias x.
 * A one-row star passes unchanged bit for bit at every L (gnn_utils.py:35-36), L = 0 is the gather
 * of the first rows, the weights are divided by their sum only when the sum is > 0
 * (gnn_utils.py:58-59) and the neighbours are summed in the caller's order.
 * Four launches per layer, the B row 0s being the rows of one weight-streaming GEMV pass:
 * attention.0 factored per node, blocks owning 16 hidden units x 256 columns of one star, a wave
 * taking rows wave, wave + 4, .. (up to 7 per wave); the attention weights and the aggregate per
 * star (26 H floats of LDS); gate.0 and update_net.0 on [t; agg] as one paired GEMV grid;
 * update_net.2 with the gated residual t + g * u.  Every output is a fixed-order fp32 fmaf chain,
 * no atomics, nothing shared between stars: star b's row does not depend on B, on its position in
 * the pack or on the other stars' sizes, and two calls give equal bits.
 * 1 <= B <= 8 (B == 0: nothing to do), B <= V <= 26 B, F % 4 == 0, H == AZ_STAR_HIDDEN,
 * 0 <= L <= 4; x, x0, ws and the weight matrices 16-byte aligned; anything else returns AZ_EINVAL
 * with a message before any launch; so does an offs in host memory (az_host_alloc / pinned) that
 * does not ascend from 0 to V in steps of 1 .. 26 -- offs in HBM is clamped into the V rows and
 * to 26 rows per star by the kernels.  ws >= az_gnn_star_packed_infer_ws_bytes(B, F, H, L)
 * (0 for a rejected shape). */
size_t az_gnn_star_packed_infer_ws_bytes(int B, int F, int H, int L);
int az_gnn_star_packed_infer(const float* x, const int* offs, int B, int V, int F, int H, int L,
                             const az_gnn_layer_w* layers, float* x0, void* ws, size_t ws_bytes,
                             void* stream);

/* predict_with_gnn of a TicTacToe leaf with its neighbourhood (TicTacToeGNN.py:47-110 on the star
 * [board] + neighbor_states: extract_features TicTacToeGNN.py:25-34, PolicyValueGNN.forward
 * gnn_utils.py:107-116, apply_policy_value_heads TicTacToeGNN.py:36-45 on row 0) as ONE host call
 * with direct launches: az_ttt_trunk_fwd on the V packed boards, az_gnn_star_packed_infer on the
 * feature rows, then on the B row 0s the GNN tail of az_ttt_eval_fwd at <= 8 rows
 * (output_transform.0 + ReLU, output_transform.2, fc1 / fc2 in one launch, az_heads_fwd). */
typedef struct az_ttt_star_eval {
  const float* conv1_w; const float* conv1_b; const float* conv2_w; const float* conv2_b;
  const float* conv3_w; const float* conv3_b;
  const float* fc1_w; const float* fc1_b;  /* [512][F], [512] */
  const float* fc2_w; const float* fc2_b;
  const float* fc_policy_w; const float* fc_policy_b;  /* [A][512], [A] */
  const float* fc_value_w; const float* fc_value_b;    /* [1][512], [1] */
  const float* ot0_w; const float* ot0_b;  /* output_transform.0 [F][F], [F] */
  const float* ot2_w; const float* ot2_b;  /* output_transform.2 */
  az_gnn_layer_w layers[AZ_STAR_MAX_LAYERS];   /* entries >= L unused */
  int n;                                   /* board side, 3..5 */
  int A;                                   /* actions (fc_policy rows), <= 32 */
  int F;                                   /* 128 (n-2)^2 */
  int L;                                   /* GNN layers, 0..4 */
  int max_B;                               /* most stars one call may carry, <= 8 */
  float* feat;                             /* device [max_B * 26][F] */
  float* x0; float* hidden; float* y;      /* device [max_B][F] each */
  float* h1; float* h2;                    /* device [max_B][512] each */
  float* glogp;                            /* device [max_B][A] */
  void* ws; size_t ws_bytes;               /* >= az_ttt_star_eval_ws_bytes(max_B, n, A, L) */
} az_ttt_star_eval;
/* 0 for a shape az_ttt_star_eval_fwd rejects. */
size_t az_ttt_star_eval_ws_bytes(int max_B, int n, int A, int L);
/* rows int8 [V][n][n] packed stars, offs int32 [B+1] (star b = boards offs[b] .. offs[b+1]-1, the
 * first the leaf; 1 .. 26 boards each), gpi [B][A] (may be NULL), gv [B]; rows, offs, gpi and gv
 * may be az_host_alloc memory.  0 <= B <= min(max_B, 8) (0: nothing to do), B <= V <= 26 B.  A
 * star's outputs are bit-identical to the same star evaluated alone or elsewhere in another pack.
 * A bad shape, a null or misaligned pointer, a small workspace or a bad host offs returns
 * AZ_EINVAL before any launch. */
int az_ttt_star_eval_fwd(const az_ttt_star_eval* e, const int8_t* rows, const int* offs, int B,
                         int V, float* gpi, float* gv, void* stream);

/* Batch-invariant star evaluation (config key batch_invariant with gnn_neighbors).
 *
 * az_gnn_star_batch_exact_infer: az_gnn_star_batch_infer's arguments, offs checks, shape limits
 * and semantics (L = 0 gather and one-row stars included) with every product an exact GEMM: per
 * layer P = x W1'^T (M = V, N = 2H, K = F; from layer 1 on also Pt over the B updated row 0s), the
 * same weights-and-aggregate kernel, gate.0 and update_net.0 as ONE paired az_gemm_exact_ex launch
 * on TA = [t | agg] (K = 2F; sigmoid -> gate, ReLU -> u1), update_net.2 with the gated-residual
 * epilogue (R = TA's t half, G = gate).  x0[b] is a function of star b's rows and the weights
 * only: the same bits at any B, V, position and packing, spread or direct.  Within 1e-5 of
 * az_gnn_star_batch_infer, not bit-identical to it.
 * ws >= az_gnn_star_batch_exact_ws_bytes(B, V, F, H, L) (0 for a rejected shape; monotonic in B and
 * V, so a workspace sized for a capacity serves every smaller call). */
size_t az_gnn_star_batch_exact_ws_bytes(int B, int V, int F, int H, int L);
int az_gnn_star_batch_exact_infer(const float* x, const int* offs, int B, int V, int F, int H,
                                  int L, const az_gnn_layer_w* layers, float* x0, void* ws,
                                  size_t ws_bytes, void* stream);

/* predict + predict_with_gnn(board, neighbor_states) of B leaves with their neighbourhoods as ONE
 * host call, for every board az_eval_exact_fwd serves, with the same launch sequence at B = 1 and
 * B = 4096: the board's fused trunk on the V packed rows, the gather of every star's row 0, the
 * standard tail on the B leaf rows exactly as az_eval_exact_fwd runs it, the exact layer stack
 * (az_gnn_star_batch_exact_infer), output_transform.0 / .2 as two exact GEMMs, the heads.
 * A star's four output rows are the same bits alone, at any position of any pack and across
 * calls; pi, v of star b equal az_eval_exact_fwd's pi, v of its leaf board; gpi, gv of a one-row
 * star equal az_eval_exact_fwd's gpi, gv of that board. */
typedef struct az_star_eval_exact {
  az_eval_exact e;        /* game, shape, trunk / heads / output_transform weights (all of them);
                             e.max_B: most stars a call may carry; e.feat: device [max_V][F];
                             e.h1, e.h2, e.hidden, e.y, e.logp, e.glogp: [max_B] rows as there;
                             e.ws >= az_star_eval_exact_ws_bytes(max_B, max_V, game, nx, ny, A, L, H) */
  int L; int H;           /* GNN layers 0..4, attention.0's hidden width */
  az_gnn_layer_w layers[AZ_STAR_MAX_LAYERS];   /* entries >= L unused */
  int max_V;              /* most packed rows a call may carry, >= max_B */
  float* leaf; float* x0; /* device [max_B][F] each */
} az_star_eval_exact;
/* 0 for a shape az_star_eval_exact_fwd rejects (a board without a fused trunk among them). */
size_t az_star_eval_exact_ws_bytes(int max_B, int max_V, int game, int nx, int ny, int A, int L,
                                   int H);
/* rows int8 [V][nx][ny] packed stars, offs int32 [B+1] (star b = rows offs[b] .. offs[b+1]-1, row
 * 0 the leaf), pi [B][A] and gpi [B][A] (each may be NULL), v [B], gv [B]; rows, offs and the
 * outputs may be az_host_alloc memory.  0 <= B <= max_B, B <= V <= max_V (B == 0: nothing to do).
 * A bad shape, a null pointer, a short workspace or a non-ascending host offs returns AZ_EINVAL
 * with a message before any launch. */
int az_star_eval_exact_fwd(const az_star_eval_exact* e, const int8_t* rows, const int* offs, int B,
                           int V, float* pi, float* v, float* gpi, float* gv, void* stream);

/* ---------------------------------------------------------------------------------
 * Backward pass (Connect4GNN.py:150-156,187-197 / TicTacToeGNN.py:217-264), deterministic:
 * every reduction runs in a fixed order, no float atomics.
 * --------------------------------------------------------------------------------- */
/* d loss / d logits and d loss / d tanh-input of the value head for
 * l = -sum(pi*logp)/B_norm + sum((z-v)^2)/B_norm (Connect4GNN.py:150-152).
 * loss_rows (nullable): [B][2] per-row (policy, value) loss terms. */
int az_heads_loss_bwd(const float* logp, const float* v, const float* target_pi,
                      const float* target_v, int B, int A, int B_norm, float* dlogits,
                      float* dvpre, float* loss_rows, void* stream);
/* Heads backward: dwp/dbp/dwv/dbv (nullable as a group) and dhp/dhv (nullable as a pair;
 * dhv == dhp sums both heads into one buffer, the Connect4 case hp == hv).
 * ws >= az_colsum_ws_bytes(B, A+1) bytes when weight grads are requested. */
int az_heads_bwd(const float* dlogits, const float* dvpre, const float* hp, int ldhp,
                 const float* hv, int ldhv, int B, int K, const float* wp, int A,
                 const float* wv, float* dwp, float* dbp, float* dwv, float* dbv,
                 float* dhp, int lddhp, float* dhv, int lddhv, void* ws, size_t ws_bytes,
                 void* stream);
/* out[j] = beta*out[j] + sum_i X[i][j] (bias gradients), fixed-order two-pass reduce. */
size_t az_colsum_ws_bytes(int R, int C);
int az_colsum(const float* X, int R, int C, int ldx, float* out, float beta, void* ws,
              size_t ws_bytes, void* stream);
/* Dropout (Connect4Net.py:52, F.dropout semantics y = x * keep / (1-p)): a counter-based
 * keep mask (mask[i] = 1 with probability 1-p, reproducible from `seed`), and y = mask ? x*scale : 0
 * (forward with scale = 1/(1-p); backward on the gradient with the same mask). */
int az_dropout_mask(uint8_t* mask, int64_t n, double p, uint64_t seed, void* stream);
int az_mask_scale(const float* x, const uint8_t* mask, float scale, int64_t n, float* y,
                  void* stream);
/* Conv trunk backward helpers (3x3, stride 1; pad in {0,1}):
 *   dz[b*HW+p][c] = dy[b][c*HW+p] * (mask ? mask*scale : 1) * (y > 0)   NCHW -> position-major
 *   cols[(b,y,x)][c*9+kh*3+kw] = in[b][c][y+kh-pad][x+kw-pad]           row stride ldc >= 9C
 *   dz[(b,y,x)][c] = sum_{kh,kw} dcols[(b,y-kh+pad,x-kw+pad)][c*9+kh*3+kw] * (a[b][c][y][x] > 0)
 * With them a conv layer's grads are GEMMs: dW = dz^T cols, db = colsum(dz),
 * dcols = dz W (then col2im for the layer below). */
int az_nchw_drelu_to_pm(const float* dy, const float* y, const uint8_t* mask, float scale,
                        int B, int C, int HW, float* dz, void* stream);
int az_im2col3x3(const void* in, int in_int8, int B, int C, int H, int W, int pad, int ldc,
                 float* cols, void* stream);
int az_col2im3x3_drelu(const float* dcols, int ldc, const float* a, int B, int C, int H, int W,
                       int pad, float* dz, void* stream);
/* GNNLayer backward (gnn_utils.py:34-74, per destination) from the activations the forward
 * kept in fwd_ws: writes dx [V][F] (input gradient) and every parameter gradient in `gr`.
 * The graph must carry the reverse CSR (src_rowptr/src_edges/dst_index). */
size_t az_gnn_layer_bwd_ws_bytes(int V, int E, int D, int F, int H);
int az_gnn_layer_bwd(const az_graph* g, const float* x, int F, int H, const az_gnn_layer_w* w,
                     const void* fwd_ws, const float* dout, float* dx,
                     const az_gnn_layer_grads* gr, void* ws, size_t ws_bytes, void* stream);
/* az_gnn_node_update_fwd's backward: from dout [V][F] and the forward's `save`:
 *   dx [V][F]   = dout on every row, + d/dx_d of the update on the destination rows;
 *   dagg [V][F] = d/dagg_d on the destination rows (other rows are not written);
 * and the six parameter gradients (written, same layout as the weights).
 * ws >= az_gnn_node_update_bwd_ws_bytes(D, F). */
size_t az_gnn_node_update_bwd_ws_bytes(int D, int F);
int az_gnn_node_update_bwd(const float* x, const float* agg, int V, int F, int D,
                           const int* dst_rows, const float* gate_w, const float* upd_w1,
                           const float* upd_w2, const float* save, const float* dout, float* dx,
                           float* dagg, float* d_gate_w, float* d_gate_b, float* d_upd_w1,
                           float* d_upd_b1, float* d_upd_w2, float* d_upd_b2, void* ws,
                           size_t ws_bytes, void* stream);
/* Training on child stars: az_gnn_star_batch_infer's layer stack on packed stars keeping what the
 * backward needs, and that backward.  x [V][F], offs [B+1], layers and x0 [B][F] are
 * az_gnn_star_batch_infer's, with the same semantics (weights sigmoid(attention(.)), divided by
 * their sum only when it is > 0, summed and aggregated in neighbour order; a one-row star returns
 * its row bit for bit).  The rows are float64-accurate like that call's but not its bits.
 *   save   per layer (az_gnn_star_batch_save_bytes in all): P [V][2H] = x W1'^T (W1 read as
 *          [2H][F]: [v][2q] target half, [v][2q+1] source half); Pt [B][2H], the same of the
 *          updated row 0s (written from layer 1 on); TA = [t | agg] [B][2F]; gate, u1, u [B][F];
 *          the raw weights a [V] (0 at a star's first row) and their sums s [B]
 *   ws     az_gnn_star_batch_train_ws_bytes, one size for both calls; nothing in it is carried
 *          from the forward to the backward
 * az_gnn_star_batch_bwd takes dx0 [B][F] = d loss / d x0 and WRITES every tensor of grads[0..L).
 * Only row 0 of a star changes in a layer and x is an input here (the trunk is frozen in the GNN
 * step), so no gradient with respect to x is formed: between layers only dt [B][F] flows.  Per
 * layer, last first: the gated residual (du = dt g, dg = dt u g (1 - g), both 0 for a one-row
 * star, whose dt passes through); update_net.2, update_net.0 and gate.0 as transposed products
 * over the B rows with az_colsum biases; d[t | agg] = du1 Wu1 + dg Wg, its first half added into
 * dt, its second half dagg; one kernel per star (the F-long dots dagg . x_j, (n-1) F 4 bytes per
 * star, the normalisation and sigmoid backward, the hidden-unit gradients into dP [V][2H] and, from
 * layer 1 on, the target half into dPt [B][2H], per-star partials of attention.2 and
 * attention.0.bias); d attention.0.weight = dP^T x (+ dPt^T t from layer 1 on); dt += dPt W1'.
 * A batch of one-row stars writes zeros; a two-row star adds exactly zero to attention.*.
 * No atomics, fixed orders: two identical calls give equal bits.
 * Shapes and alignment as az_gnn_star_batch_infer, and H <= 1024; dx0 16-byte aligned, every
 * gradient pointer non-null, the matrices 16-byte aligned.  A bad shape, a null or misaligned
 * pointer, a short save or ws, or a non-ascending host offs returns AZ_EINVAL with a message
 * before any launch.  B == 0 returns AZ_OK. */
size_t az_gnn_star_batch_save_bytes(int B, int V, int F, int H, int L);
size_t az_gnn_star_batch_train_ws_bytes(int B, int V, int F, int H, int L);
int az_gnn_star_batch_fwd_train(const float* x, const int* offs, int B, int V, int F, int H, int L,
                                const az_gnn_layer_w* layers, float* x0, void* save,
                                size_t save_bytes, void* ws, size_t ws_bytes, void* stream);
int az_gnn_star_batch_bwd(const float* x, const int* offs, int B, int V, int F, int H, int L,
                          const az_gnn_layer_w* layers, const void* save, size_t save_bytes,
                          const float* dx0, const az_gnn_layer_grads* grads, void* ws,
                          size_t ws_bytes, void* stream);
/* output_transform backward (gnn_utils.py:101-105): dW2, db2, dW0, db0, dh (scratch [M][F])
 * and dx (nullable).  ws >= az_colsum_ws_bytes(M, F) (+ split-K room). */
int az_mlp2_bwd(const float* x, int M, int F, const float* w0, const float* w2,
                const float* hidden, const float* dy, float* dx, float* dw0, float* db0,
                float* dw2, float* db2, float* dh, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * torch.optim.Adam step (defaults of Connect4GNN.py:132-133: betas (0.9,0.999), eps 1e-8,
 * no weight decay, no amsgrad) over one flat fp32 parameter buffer:
 *   m = lerp(m, g, 1-b1); v = b2 v + (1-b2) g^2;
 *   p -= (lr / (1-b1^t)) m / (sqrt(v) / sqrt(1-b2^t) + eps)          (t = step >= 1)
 * --------------------------------------------------------------------------------- */
int az_adam_f32(float* p, const float* g, float* m, float* v, int64_t n,
                double lr, double beta1, double beta2, double eps, int step, void* stream);
/* The same call under SURVEY §8b's name (reference: torch.optim.Adam.step, Connect4GNN.py:187-197). */
int az_adam_step(float* p, const float* g, float* m, float* v, int64_t n,
                 double lr, double beta1, double beta2, double eps, int step, void* stream);

/* ---------------------------------------------------------------------------------
 * Loss metrics of B rows of network outputs against their targets, summed over the rows into
 * acc[AZ_METRICS_N] (doubles on the device; a mean is acc[k] / acc[AZ_METRICS_ROWS]):
 *   AZ_METRICS_CE    -sum_a t log p     policy cross-entropy (train()'s l_pi times B)
 *   AZ_METRICS_SE    (tv - v)^2         value squared error  (train()'s l_v times B)
 *   AZ_METRICS_TOP1  argmax p == argmax t, ties to the lowest index on both sides
 *   AZ_METRICS_ENT   -sum_a p log p     policy entropy
 *   AZ_METRICS_TENT  -sum_a t log t     target entropy
 *   AZ_METRICS_ROWS  B
 * p [B][ldp] (ldp >= A) holds probabilities (is_log = 0) or log-probabilities (is_log = 1); v,
 * target_v [B]; target_pi [B][A]; 1 <= A <= 32.  A term with t == 0 is exactly 0 whatever p is;
 * log p is never taken below log(FLT_MIN), so p == 0 under t > 0 adds the finite -t log(FLT_MIN),
 * and p == 0 adds 0 to the entropy: no NaN or inf from zeros.  The per-row terms are formed in
 * fp32 and summed over the rows in fp64 in a fixed order without atomics (per-block sums into ws,
 * then one block adds them in block order), so two identical calls give equal bits.
 * accumulate != 0 adds the sums to what acc holds, so a chunked pass needs one device-to-host read
 * at its end and no host synchronisation; otherwise acc is overwritten.  B == 0 is valid: acc is
 * left as it is when accumulating and zeroed otherwise.  ws >= az_policy_value_metrics_ws_bytes(B,
 * A) bytes, 8-byte aligned (may be NULL when B == 0).  A bad shape, a null pointer or a
 * misaligned acc / ws returns AZ_EINVAL before any launch.
 * --------------------------------------------------------------------------------- */
#define AZ_METRICS_CE 0
#define AZ_METRICS_SE 1
#define AZ_METRICS_TOP1 2
#define AZ_METRICS_ENT 3
#define AZ_METRICS_TENT 4
#define AZ_METRICS_ROWS 5
#define AZ_METRICS_N 6
size_t az_policy_value_metrics_ws_bytes(int B, int A);
int az_policy_value_metrics(const float* p, int ldp, int is_log, const float* v,
                            const float* target_pi, const float* target_v, int B, int A,
                            double* acc, int accumulate, void* ws, void* stream);

/* Parameters changed: every cached per-row weight scale and fp16 weight plane of the fp16 GEMM
 * form (az_gemm_f32's large K-major GEMMs on registered weights, below) is recomputed before its
 * next use.  The cache is keyed by the weight pointer and shape, so a caller that writes
 * registered weights any way other than az_adam_f32 (which calls it) -- an optimizer step of its
 * own, loading a checkpoint, copying buffers -- must call it before the next GEMM on them.
 * A missed call is NOT a precision loss: above 64 rows the GEMM multiplies by the cached planes,
 * i.e. it returns the PREVIOUS weights' result.  It covers more than GEMM operands: the heads
 * composed with output_transform.2 (az_transform_heads_fwd with y = NULL) are cached the same
 * way and depend on fc_policy / fc_value weights and biases and on output_transform.2's bias, so
 * a write to any registered parameter needs the call.  (azhip/params.py FlatParams calls it for the
 * torch-side writes that bump the buffer's version counter -- in-place ops on the parameter
 * tensors -- and from copy_flat_ / weights_changed().  Writes through `.data`, and collectives
 * that write parameter views in place (dist.broadcast / all_reduce), do not bump it: such a
 * path must call FlatParams.weights_changed() itself.) */
int az_weights_changed(void);

/* Parameter storage: [base, base + bytes) holds weights whose values change only where
 * az_weights_changed() says so.  Only weights inside a registered range have their fp16-form
 * row scales and pre-split planes cached (az_gemm_f32's large K-major GEMMs: W split once per
 * weight update instead of in every tile); any other weight pointer gets its scales computed per
 * call, since a pointer alone says nothing about the values behind it.  Registering or
 * unregistering also invalidates every cache entry; unregistering waits for the device and frees
 * the entries of weights inside the range (8 N K bytes each).  The Python parameter store
 * (azhip/params.py FlatParams) registers its flat buffer. */
int az_weights_register(const void* base, size_t bytes);
int az_weights_unregister(const void* base);

#ifdef __cplusplus
}
#endif
#endif /* AZ_HIP_H */
