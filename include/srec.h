/* libsrec_hip.so - C ABI of the MI355X (gfx950) session-recommendation training hot path.
 *
 * The reference (SpaceLearner/SessionRec-pytorch) has no FFI: its hot path is Python calling
 * DGL / PyTorch CUDA ops.  Each entry point below names the reference call site(s) whose
 * arithmetic it replaces; the host-side mirror (sessionrec-pytorch_amd/) binds them with ctypes
 * (see INTEGRATION.md for the stub a maintainer of the reference would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (outputs pre-allocated), fp32 /
 *     int32 unless noted; the library allocates nothing and never synchronises;
 *   - `stream` is a hipStream_t (pass the framework's current stream; NULL = default stream);
 *   - row-major matrices with an explicit leading dimension `ld_*` (floats); d, ld multiples of 4,
 *     base pointers 16-byte aligned (float4 / 1 KiB-per-wave coalesced rows);
 *   - `dyn*` (nullable) points at an int32 in device memory holding the LIVE extent of a
 *     capacity-padded dimension, so one captured hipGraph serves batches of any size:
 *     effective n = min(n_cap, *dyn); rows in [n, n_cap) are written as zeros by producers;
 *   - return 0 on success, a hipError_t value or SREC_BAD_ARG (1001) otherwise.
 */
#ifndef SREC_H
#define SREC_H
#include "srec_hg.h"
#include "srec_ens.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SREC_BAD_ARG 1001

/* ---- dense linear algebra on the matrix cores (v_mfma_f32_32x32x2_f32, exact fp32) ----------------
 * C[m,n] = alpha * sum_k A(m,k) B(n,k) + beta*C[m,n] + bias[n];  A(m,k)=A[m*a_rs+k*a_cs], same for B.
 * dyn_mode: 0 none, 1 clamps M, 2 clamps K.  ws (nullable): ws_floats of scratch for split-K slabs.
 * Replaces nn.Linear fwd/bwd: srgnn.py:66-68,124  lessr.py:16-17,59-62,94-100,164  msgifsr.py:114-116,202
 * gatconv.py:157,282-283; GRU input/hidden projections srgnn.py:15, msgifsr.py:25. */
int srec_gemm_f32(const float* A, int a_rs, int a_cs, const float* B, int b_rs, int b_cs, float* C, int ldc,
                  const float* bias, int M, int N, int K, const int* dyn, int dyn_mode, float alpha, float beta,
                  float* ws, long ws_floats, void* stream);

/* bf16-operand variant (v_mfma_f32_32x32x16_bf16, fp32 accumulate): A [M,K], B [N,K] fp32 in HBM, rounded to
 * bf16 while staged into LDS; K % 32 == 0; dyn (nullable) clamps M.  The reduced-precision path BASELINE
 * config C3 names; same call sites as srec_gemm_f32 (forward and backward-data products). */
int srec_gemm_bf16_nt(const float* A, int lda, const float* B, int ldb, float* C, int ldc, const float* bias, int M,
                      int N, int K, const int* dyn, float alpha, float beta, float* ws, long ws_floats, void* stream);

/* bf16-operand weight-gradient product: C[N,K] = alpha * A[Mred,N]^T B[Mred,K] + beta*C (dW = dY^T X of every
 * nn.Linear backward: autograd of F.linear at e.g. msgifsr.py:77-79, gatconv.py:166-175); operands are transposed
 * to reduction-contiguous bf16 while staged into LDS; dyn (nullable) clamps the reduction rows. N % 4 == K % 4 == 0. */
int srec_gemm_bf16_tn(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int Mred, int N, int K,
                      const int* dyn, float alpha, float beta, float* ws, long ws_floats, void* stream);

/* ---- fused full-catalog scoring + softmax-CE (score_ce.hip) -----------------------------------------
 * z[b,v] = cs[v] * <sr_b, E_v> (cs NULL -> 1).  Replaces sr @ E^T, log(softmax), nll_loss:
 * srgnn.py:145-147  niser.py:149-156  lessr.py:182-183  msgifsr.py:276-309,321  train.py:99 (+ backward). */
int srec_ce_plan(int B, int V, int d, int* n_item_tiles, int* n_ranges);
/* ws_stats: 2*n_item_tiles*B floats.  Outputs lab_logit[B], lse[B], lossvec[B], loss[1]. */
int srec_score_ce_fwd(const float* sr, int ld_sr, const float* E, int ld_e, const float* cs, const int* labels,
                      int B, int V, int d, const int* dynB, float* ws_stats, float* lab_logit, float* lse,
                      float* lossvec, float* loss, void* stream);
/* ws_dsr: n_ranges*B*d floats.  gscale (nullable): upstream d loss (with ga / gc given it multiplies them: no 1 / B).  Outputs dE[V,d] (every row), dsr[B,d].
 * parts: bit0 = dE kernel, bit1 = d sr kernels (3 = both), bit2 = accumulate into dE.  ga/gc (nullable): per-session coefficients
 * dS[b,v] = (ga[b] softmax[b,v] - gc[b] [v==label_b]) cs[v] for losses built from (lse_b, z[b,label_b]), e.g. the
 * order-fusion mixture of msgifsr.py:311-317. */
int srec_score_ce_bwd(const float* sr, int ld_sr, const float* E, int ld_e, const float* cs, const int* labels,
                      const float* lse, const float* gscale, const float* ga, const float* gc, int B, int V, int d,
                      const int* dynB, float* dE, int ld_de, float* ws_dsr, float* dsr, int parts, void* stream);
/* log-probabilities (B,V): the (B,num_items) tensor every reference model's forward() returns. */
int srec_score_logp(const float* sr, int ld_sr, const float* E, int ld_e, const float* cs, const float* lse, int B,
                    int V, int d, const int* dynB, float* logp, long ld_logp, void* stream);

/* bf16-operand variant of the fused scoring (score_ce_bf16.hip; BASELINE config C3 "bf16"): same call sites as
 * srec_score_ce_fwd/bwd.  srec_bf16_prepare rounds rows [R,d] fp32 (RNE) into a row-major copy dst16 [Rp, d_pad] (zero for
 * rows >= live R / columns >= d; Rp % 128 == 0; d <= 256, d % 4 == 0; d_pad from srec_ce_plan_bf16) and, when dstT16 != NULL,
 * a transposed copy [d_pad, Rp] (no longer read by the scoring kernels: pass NULL); call it once per step for the table and
 * once per head for the session vectors.
 * ws_stats >= 2 * n_stat_slabs * B floats, ws_dsr >= n_ranges * B * d floats.  Soft-max statistics, exp and all
 * accumulation stay fp32; dE / dsr are fp32.  The backward runs both parts in one launch (parts bits as above;
 * bit3 = leave the d-sr partial slabs in ws_dsr unreduced); it reads only the row-major copies (ET16 is ignored and may be
 * NULL: the transposed MFMA fragments are taken from the row-major LDS image by ds_read_b64_tr_b16; ws_de: see
 * srec_ce_de_split below, NULL = no session split). */
int srec_bf16_prepare(const float* src, int ld, int R, const int* dynR, int d, void* dst16, void* dstT16, int Rp,
                      void* stream);
int srec_ce_plan_bf16(int B, int V, int d, int* n_stat_slabs, int* n_ranges, int* d_pad);
int srec_score_ce_fwd_bf16(const void* sr16, int Bp, const void* E16, int Vp, const float* cs, const int* labels,
                           int B, int V, int d, const int* dynB, float* ws_stats, float* lab_logit, float* lse,
                           float* lossvec, float* loss, void* stream);
int srec_score_ce_bwd_bf16(const void* sr16, float* ws_de, int Bp, const void* E16, const void* ET16, int Vp,
                           const float* cs, const int* labels, const float* lse, const float* gscale, const float* ga,
                           const float* gc, int B, int V, int d, const int* dynB, float* dE, int ld_de, float* ws_dsr,
                           float* dsr, int parts, void* stream);
/* Session split of the backward's item tiles (round 6; the step a rank of an N-GPU job runs scores N x 512 sessions against V / N
 * table rows: few item tiles, each streaming N x the sessions - train.py:94-101 sharded): srec_ce_de_split(B, V, d, &split): workgroups
 * per item tile at this shape (1 = none).  The caller may pass ws_de (nullable) >= split x V x d floats and the split in `parts`
 * bits 8 - 15: workgroup (tile, s) then writes slab s, and the slabs are summed in order into dE (added to it with parts bit 2)
 * by one more launch.  Needs ld_de == d == d_pad. */
int srec_ce_de_split(int B, int V, int d, int* split);

/* ---- embedding rows (rowops.hip) --------------------------------------------------------------------
 * gather: nn.Embedding lookup srgnn.py:133 niser.py:133 lessr.py:168 msgifsr.py:247.
 * scatter_add_sorted: its backward as a deterministic segmented sum (items[u] distinct, pos grouped by ptr). */
int srec_gather_rows(const float* src, int ld_src, const int* idx, float* out, int ld_out, int n_cap,
                     const int* dyn, int d, void* stream);
/* backward of the last-node pick x[last] (srgnn.py:140 niser.py:140 lessr.py:177; `last` non-negative and strictly ascending,
 * one entry per session): dst [nrows, d] = zeros with dst[idx[j]] = g[j] for the live j < *dyn - every row written, no
 * separate zero fill */
int srec_expand_rows_sorted(const float* g, int ld_g, const int* idx, int n_cap, const int* dyn, int nrows, int d,
                            float* dst, int ld_dst, void* stream);
int srec_scatter_add_sorted(const float* g, int ld_g, const int* items, const int* ptr, const int* pos, float* dst,
                            int ld_dst, int u_cap, const int* dyn, int d, int accumulate, void* stream);
/* the lookup with its feature dropout fused (msgifsr.py:247 `dropout(embedding(iid))`): out[r, c] *= mask(r * d + c), mask =
 * 1 / (1 - p) with probability 1 - p else 0, from a counter-based hash keyed by (seed, *counter, salt) - counter (nullable) is a
 * device int that is constant within a training step and changes between steps (the optimizer's step count).  The backward
 * re-derives the same mask while it sums the gradient rows (g must be contiguous: ld_g == d). */
int srec_gather_rows_drop(const float* src, int ld_src, const int* idx, float* out, int ld_out, int n_cap, const int* dyn,
                          int d, float p, int seed, const int* counter, int salt, void* stream);
int srec_scatter_add_sorted_drop(const float* g, int ld_g, const int* items, const int* ptr, const int* pos, float* dst,
                                 int ld_dst, int u_cap, const int* dyn, int d, int accumulate, float p, int seed,
                                 const int* counter, int salt, void* stream);
int srec_scatter_add_sorted_ex(const float* g, int ld_g, const int* items, const int* ptr, const int* pos, float* dst,
                               int ld_dst, int u_cap, const int* dyn, int d, int accumulate, float p, int seed,
                               const int* counter, int salt, const float* projW, int ld_w, float* radial, void* stream);
/* srec_scatter_add_sorted_ex (radial NULL) as the FIRST level of a two-level lookup gradient whose second level the optimizer's
 * row pass performs (srec_adam_rows_lookup): wavefront u < min(*stamp_dyn, stamp_cap) also writes slot[stamp_items[u]] = u + 1
 * (stamp_items[u] < 0 skipped; slot int32 [table rows], zero before and zeroed again by the row pass).  stamp_cap <= u_cap. */
int srec_scatter_add_sorted_stamp(const float* g, int ld_g, const int* items, const int* ptr, const int* pos, float* dst,
                                  int ld_dst, int u_cap, const int* dyn, int d, int accumulate, float p, int seed,
                                  const int* counter, int salt, const int* stamp_items, int stamp_cap, const int* stamp_dyn,
                                  int* slot, void* stream);
/* row-sharded lookup backward (the nn.Embedding gradient of srgnn.py:133 / msgifsr.py:247 when the table is sharded over the
 * ranks): dst[rel[q], :] += rows[q, :] for every request q < w ucap with rel[q] >= 0, the requests of ALL w <= 16 ranks in one launch
 * and - an item may be requested by several ranks - added per item in rank order (the bits of w rank-by-rank
 * srec_scatter_add_sorted calls).  ids [w ucap] = the requests' global item ids, ascending inside each rank's list of ucap (-1
 * padding behind them); rows [w ucap, d] dense.  radial (nullable) as in srec_scatter_add_sorted_ex. */
int srec_add_rows_ranks(const float* rows, int d, const int* rel, const int* ids, int w, int ucap, float* dst, int ld_dst,
                        const float* projW, int ld_w, float* radial, void* stream);
/* Embedding(max_norm) in-place renorm, idx distinct or NULL (= all rows): lessr.py:126 msgifsr.py:162 */
int srec_renorm_rows(float* W, int ld, const int* idx, int n_cap, const int* dyn, int d, float max_norm,
                     void* stream);
/* out[v] = scale / norm(E_v); eps_mode 0: max(norm,eps) (F.normalize), 1: norm+eps (niser.py:151) */
/* the renorm of every row (max_norm > 0; <= 0: none) + the bf16 operand copy dst16 [>= n, Dp] (Dp >= d, Dp % 4 == 0,
 * columns d .. Dp zero) of the table the bf16 scoring kernels read, in one pass (d <= 1024) */
int srec_renorm_rows_bf16(float* W, int ld, int n, int d, float max_norm, void* dst16, int Dp, void* stream);
int srec_row_invnorm(const float* W, int ld, int n, int d, int eps_mode, float eps, float scale, float* out,
                     void* stream);
/* row L2 normalisation of node / session features: niser.py:135,142,148  msgifsr.py:253,263,273 */
int srec_normalize_fwd(const float* X, int ld_x, float* Y, int ld_y, float* inv, int n_cap, const int* dyn, int d,
                       int eps_mode, float eps, void* stream);
/* the same + a bf16 copy dst16 [>= n_cap, Dp] of the normalised rows (zero rows past the live count; columns d .. Dp are
 * not written): the session-vector operand of srec_score_ce_*_bf16 without a conversion pass of its own */
int srec_normalize_fwd_bf16(const float* X, int ld_x, float* Y, int ld_y, float* inv, int n_cap, const int* dyn, int d,
                            int eps_mode, float eps, void* dst16, int Dp, void* stream);
int srec_normalize_bwd(const float* Y, int ld_y, const float* dY, int ld_dy, const float* inv, float* dX, int ld_dx,
                       int n_cap, const int* dyn, int d, void* stream);
/* the same for np <= 4 row blocks of different tensors normalised into ONE stacked matrix Y [sum n_p, d] (MSGIFSR: the
 * per-order features of msgifsr.py:253 feed the batched MSHGNN layer stacked) - one launch instead of np + a concatenation.
 * X / dX / dyn: HOST arrays of np device pointers (dyn entries nullable), ld / n: HOST int arrays. */
int srec_normalize_group_fwd(int np, const void* X, const int* ld, const int* n, const void* dyn, float* Y, int ld_y,
                             float* inv, int d, int eps_mode, float eps, void* stream);
int srec_normalize_group_bwd(int np, const void* dX, const int* ld, const int* n, const void* dyn, const float* Y, int ld_y,
                             const float* dY, int ld_dy, const float* inv, int d, void* stream);
/* out [n, da + db] = [a | b]: the feature-axis concatenation in front of fc_sr (srgnn.py:143, msgifsr.py:270-272) */
int srec_cat_cols(const float* a, int lda, int da, const float* b, int ldb, int db, int n, float* out, void* stream);
/* chain rule of the catalog-row normalisation on the dense dE: G_v -= e_v <e_v, G_v> */
int srec_rownorm_project(const float* W, int ld_w, const float* cs, float inv_scale, float* G, int ld_g, int n, int d,
                         void* stream);
/* deferred form of the projection: the scoring backward leaves dE unprojected, later additions to it (lookup gradients)
 * record their radial part radial[v] += <W_v, l_v> (srec_scatter_add_sorted_ex), and either this call or the optimizer's row pass
 * (srec_adam_rows_proj) applies G_v -= W_v (<W_v, G_v> - radial[v]) inv_v^2 and clears radial */
int srec_rownorm_project_radial(const float* W, int ld_w, const float* cs, float inv_scale, float* G, int ld_g, int n, int d,
                                float* radial, void* stream);
/* out[c] (+)= sum_r w[r, c/D] * X[r,c] (wgt NULL -> plain column sums: bias / fc_e / attention-vector
 * gradients).  Two deterministic stages; ws = 128*ncol floats of scratch (16-byte aligned). */
int srec_col_sum(const float* X, int ld, const float* wgt, int H, int D, int n_cap, const int* dyn, int ncol,
                 float* out, int accumulate, float* ws, void* stream);

/* Static per-session budgets of the one-wavefront-per-session / per-destination kernels (LDS arrays): nodes of one session in
 * a read-out (srec_seg_attn_*), node degree per relation (srec_gat_*, srec_hg_*), in-degree in LESSR's shortcut graph
 * (srec_sgat_*).  HOST pointers (nullable).  The reference has no such limit (DGL's degree buckets grow with the data,
 * collate.py:87-217 builds any session length); the host mirror checks every batch against these when it is collated and
 * raises instead of truncating (ops.check_limits). */
int srec_limits(int* max_session_nodes, int* max_degree, int* max_degree_sgat);

/* Batch intake of a replayed step (graph.GraphedTrainStep._stage; replaces the `x.to(device)` of the reference's
 * prepare_batch, /root/reference/src/utils/train.py:26-30, for capacity-padded batches): dst [n] (device) = src [n] int32 words
 * read by a kernel from page-locked HOST memory (or device memory); both 16-byte aligned.  Ordered on `stream`. */
int srec_copy_words(const int* src, int* dst, long n, void* stream);
/* the same INSIDE a captured step: the source of this replay is looked up in a mailbox of M entries {address lo, address hi,
 * words, expected counter} in page-locked host memory at index *counter % M (counter: the optimizer's device-side step count),
 * so no copy command precedes the graph launch; *err (device) = 1 when the entry's expected counter differs. */
int srec_copy_words_mailbox(const int* mailbox, int M, const int* counter, int* dst, long cap, int* err, void* stream);

/* ---- per-session kernels (segops.hip): one wavefront per session ------------------------------------
 * attention readout core: srgnn.py:79-86 niser.py:77-84 lessr.py:106-113 msgifsr.py:139-146 */
int srec_seg_attn_fwd(const float* U, int ld_u, const float* Vq, int ld_v, const float* we, const float* X, int ld_x,
                      const int* seg, int B, const int* dynB, int h, int D, float* alpha, float* out, int ld_out, void* stream);
int srec_seg_attn_bwd(const float* dout, int ld_do, const float* X, int ld_x, const float* alpha, const float* U,
                      int ld_u, const float* Vq, int ld_v, const float* we, const int* seg, int B, const int* dynB,
                      int h, int D, int n_cap, float* dX, int ld_dx, float* dU, int ld_du, float* dVq, int ld_dv,
                      float* dwe_part, int ld_dw, void* stream);
/* (bu, nullable: bias of the U product added inside, sigmoid(U + bu + Vq[b]) - msgifsr.py:114-115 puts the bias on fc_u;
 * out_hi / out_lo [B, ld16] and dU16 [2][n_cap, h] / dV16, dW16 [2][B, h], nullable: bf16 hi / lo splits of the outputs, the
 * operand copies of the 3-term split products of the read-out head - csrc/split16.hip; dU may be NULL when dU16 is given) */
/* out_i = h_i + mean_{session(i)} f  (msgifsr.py:86-89) */
int srec_seg_mean_add_fwd(const float* H, int ld_h, const float* F, int ld_f, const int* seg, int B, const int* dynB,
                          int D, float* out, int ld_out, void* stream);
int srec_seg_mean_add_bwd(const float* dout, int ld_do, const int* seg, int B, const int* dynB, int D, float* dF,
                          int ld_df, void* stream);

/* ---- MSGIFSR message passing (gat.hip): multi-head GAT over one relation, layout [N,H,D] ------------
 * gatconv.py:267-311 via msgifsr.py:58-64,74-89.  el/er [N,H]; A, DP [E,H] indexed by edge id;
 * in_ptr/in_idx = in-edge CSR of the destinations, out_ptr/out_idx = out-edge CSR of the sources. */
int srec_head_dot(const float* X, int ld, const float* a, int n_cap, const int* dyn, int H, int D, float* out,
                  void* stream);
int srec_gat_agg_fwd(const float* Fs, int ld_s, const float* el, const float* er, const int* in_ptr,
                     const int* in_idx, const int* esrc, int nd_cap, const int* dyn_nd, int H, int D, float slope,
                     float* A, float* rst, int ld_r, void* stream);
int srec_gat_bwd_dst(const float* dR, int ld_r, const float* Fs, int ld_s, const float* el, const float* er,
                     const float* A, const int* in_ptr, const int* in_idx, const int* esrc, int nd_cap,
                     const int* dyn_nd, int H, int D, float slope, float* DP, float* der, void* stream);
int srec_gat_bwd_src(const float* dR, int ld_r, const float* A, const float* DP, const float* attn_l,
                     const int* out_ptr, const int* out_idx, const int* edst, int ns_cap, const int* dyn_ns, int H,
                     int D, float* dFs, int ld_s, float* del, const float* der, const float* attn_r, void* stream);
int srec_head_outer(const float* wgt, const float* a, int n_cap, const int* dyn, int H, int D, float* out, int ld,
                    void* stream);
/* h_v = max_head(sum_i R_i + bias + nres*x): msgifsr.py:78-85 (+ identity residual / bias of gatconv.py:306-311).
 * rsts is a HOST array of n_rst (<= 8) device pointers. */
int srec_head_combine_fwd(const float* const* rsts, int n_rst, int ld_r, const float* x, int ld_x, const float* bias,
                          float nres, int n_cap, const int* dyn, int H, int D, float* out, int ld_o,
                          unsigned char* arg, void* stream);
int srec_head_combine_bwd(const float* dout, int ld_o, const unsigned char* arg, int n_cap, const int* dyn, int H,
                          int D, float* dR, int ld_r, void* stream);

/* ---- GRU gate math (gru.hip): msgifsr.py:25,42 (k-gram GRU), srgnn.py:15,45 (GRUCell) -----------------
 * GI/GH = input/hidden projections [n,3d] (r,z,n); GH NULL => h_prev = 0 and gh = bhh. */
int srec_gru_pointwise_fwd(const float* GI, int ld_gi, const float* GH, int ld_gh, const float* bhh, const float* Hp,
                           int ld_hp, int n_cap, const int* dyn, int d, float* Hn, int ld_hn, float* gates,
                           void* stream);
int srec_gru_pointwise_bwd(const float* dHn, int ld_dh, const float* gates, const float* GH, int ld_gh,
                           const float* bhh, const float* Hp, int ld_hp, int n_cap, const int* dyn, int d, float* dGI,
                           int ld_dgi, float* dGH, int ld_dgh, float* dHp, int ld_dhp, void* stream);
/* out = 0.5*mean_t X[n,t,:] + 0.5*Hl  (msgifsr.py:37,45), X contiguous [n,k,d] */
int srec_gram_combine_fwd(const float* X, const float* Hl, int ld_h, int n_cap, const int* dyn, int k, int d,
                          float* out, int ld_o, void* stream);
int srec_gram_combine_bwd(const float* dout, int ld_o, int n_cap, const int* dyn, int k, int d, float* dX, float* dHl,
                          int ld_h, void* stream);

/* SRGNN weighted-mean neighbour aggregation (srgnn.py:21-29,36-41): coef[e] = w_e / sum of w into the same
 * endpoint; out[v] = sum_{e in list(v)} coef[e] X[other[e]].  (ptr, idx) = in-edge CSR with other = esrc for
 * the graph, out-edge CSR with other = edst for the reversed graph; the backward is the same kernel on the
 * opposite CSR. */
int srec_edge_coef(const int* ptr, const int* idx, const int* ew, int n_cap, const int* dyn, float* coef,
                   void* stream);
int srec_edge_agg(const float* X, int ld_x, const int* ptr, const int* idx, const int* other, const float* coef,
                  int n_cap, const int* dyn, int D, float* out, int ld_o, void* stream);

/* ---- LESSR (bn.hip, gruseq.hip, sgat.hip) -------------------------------------------------------------
 * BatchNorm1d lessr.py:12,32,56,66,90,105,162,179 (ws = 64*D floats); PReLU lessr.py:140,149,159 (ws = 32*D).
 * srec_bn_fwd_train: training mode in two launches - batch statistics over the live rows, y, mean / biased var [D] for the
 * backward, and nn.BatchNorm1d's buffer updates (running_mean / running_var with the unbiased variance, nbt =
 * num_batches_tracked (int64) += 1; all three nullable).  srec_bn_apply_fwd: eval mode (given statistics). */
int srec_bn_fwd_train(const float* X, int ld_x, int n_cap, const int* dyn, int D, const float* gamma, const float* beta,
                      float eps, float momentum, float* rmean, float* rvar, long long* nbt, float* mean, float* var,
                      float* Y, int ld_y, float* ws, void* stream);
int srec_bn_apply_fwd(const float* X, int ld_x, const float* mean, const float* var, float eps, const float* gamma,
                      const float* beta, int n_cap, const int* dyn, int D, float* Y, int ld_y, void* stream);
int srec_bn_bwd(const float* dY, int ld_dy, const float* X, int ld_x, const float* mean, const float* var, float eps,
                const float* gamma, int training, int n_cap, const int* dyn, int D, float* dX, int ld_dx,
                float* dgamma, float* dbeta, float* ws, void* stream);
int srec_prelu_fwd(const float* X, int ld_x, const float* a, int n_cap, const int* dyn, int D, float* Y, int ld_y,
                   void* stream);
/* da NULL: the 32 chunk partials of d a stay in ws [32][D] for the caller to sum (srec_sum_slabs_multi, a 'tall' task) */
int srec_prelu_bwd(const float* dY, int ld_dy, const float* X, int ld_x, const float* a, int n_cap, const int* dyn,
                   int D, float* dX, int ld_dx, float* da, float* ws, void* stream);
/* EOPA: per node GRU over in-neighbours in edge-id order (lessr.py:20-27,35).  GI [Nsrc,3D] = ft W_ih^T + b_ih;
 * Whh [3D,D] as stored, WhhT [D,3D] k-major copy (read only when D > 32, else nullable: W_hh is held in registers);
 * gates [E,3D], Hprev/ghn [E,D], dGIe/dGHe [E,3D] by edge id. */
int srec_gru_seq_fwd(const float* GI, int ld_gi, const float* Whh, const float* WhhT, const float* bhh,
                     const int* in_ptr, const int* in_idx, const int* esrc, int n_cap, const int* dyn, int D,
                     float* neigh, int ld_n, float* gates, float* Hprev, float* ghn, void* stream);
int srec_gru_seq_bwd(const float* dneigh, int ld_dn, const float* Whh, const float* gates, const float* Hprev,
                     const float* ghn, const int* in_ptr, const int* in_idx, int n_cap, const int* dyn, int D,
                     float* dGIe, float* dGHe, void* stream);
/* SGAT: e = fc_e(sigmoid(q_u + k_v)), softmax over in-edges, sum a v_u (lessr.py:68-74).  A [E], dQe [E,Hh]. */
int srec_sgat_fwd(const float* Q, int ld_q, const float* K, int ld_k, const float* we, const float* Vf, int ld_v,
                  const int* in_ptr, const int* in_idx, const int* esrc, int n_cap, const int* dyn, int Hh, int Do,
                  float* A, float* out, int ld_o, void* stream);
int srec_sgat_bwd_dst(const float* dout, int ld_o, const float* Q, int ld_q, const float* K, int ld_k,
                      const float* we, const float* Vf, int ld_v, const float* A, const int* in_ptr,
                      const int* in_idx, const int* esrc, int n_cap, const int* dyn, int Hh, int Do, float* dQe,
                      float* dK, int ld_dk, float* dwe_part, int ld_dw, void* stream);
int srec_sgat_bwd_src(const float* dout, int ld_o, const float* A, const float* dQe, const int* out_ptr,
                      const int* out_idx, const int* edst, int n_cap, const int* dyn, int Hh, int Do, float* dQ,
                      int ld_dq, float* dVf, int ld_dv, void* stream);

/* ---- optimizer (adam.hip): torch.optim.Adam + coupled L2, train.py:70-75,101 ------------------------
 * hyper (device, 8 floats) = {lr/(1-b1^t), beta1, beta2, eps, weight_decay, 1-beta1, 1-beta2, sqrt(1-b2^t)} */
/* row-sharded item table: global ids (int64; -1 = padding) -> local row of the shard [lo, lo + n_loc) or -1 */
int srec_localize_idx(const long long* idx, long n, long lo, int n_loc, int* out, void* stream);
/* int32 ids (padded batches); zero (nullable): n - zero_from floats cleared by the same launch (the label-logit array of the sharded
 * forward: idx = (requested ids | labels) of one exchange, the labels from zero_from on) */
int srec_localize_idx32(const int* idx, long n, long lo, int n_loc, int* out, float* zero, long zero_from, void* stream);

/* inv[p] = u for the positions p = pos[ptr[u] .. ptr[u+1]) of item u < U (uniq_ptr / uniq_pos of a FlatBatch), -1 elsewhere */
int srec_inverse_index(const int* ptr, const int* pos, int U, int n, int* inv, void* stream);
/* row-sharded scoring: st [w, 2, B] = per-shard (log-sum-exp, label logit) gathered from the w ranks -> global lse [B],
 * label logit [B] and loss = mean over the LIVE sessions of (lse - lab).  lab_all (nullable, int64 [B]): the gathered
 * global labels, < 0 marking the capacity padding of a rank's batch (left out of the mean); gw (nullable, [B]):
 * d loss / d (lse_b - lab_b) = 1 / n_live on live sessions, 0 on padding - the ga / gc of srec_score_ce_bwd*. */
int srec_merge_stats(const float* st, int w, int B, const long long* lab_all, float* lse, float* lab, float* loss,
                     float* gw, void* stream);
int srec_merge_stats32(const float* st, int w, int B, const int* lab_all, float* lse, float* lab, float* loss,
                       float* gw, void* stream);        /* int32 labels */

int srec_adam_flat(float* p, const float* g, float* m, float* v, long n, const float* hyper, int use_wd,
                   void* stream);
/* step scalars on the DEVICE: *counter += 1, then hyper[8] = {lr/(1-b1^t), b1, b2, eps, wd, 1-b1, 1-b2, sqrt(1-b2^t)}
 * in double from cfg = double[5] {lr, beta1, beta2, eps, weight_decay} (torch.optim.Adam's host arithmetic,
 * train.py:70-75).  Makes a captured / pipelined optimizer step independent of host timing. */
int srec_adam_hyper(int* counter, const void* cfg, float* hyper, void* stream);
/* ... for n <= 16 (counter, cfg, hyper) slots in one launch; the three arguments are HOST arrays of n device pointers.
 * Loss tap (tap_ring nullable): the slot whose counter is tap_counter stores *tap_src - the step's loss, train.py:99-104
 * reads it after every step - into tap_ring[(steps taken before this one) % tap_n], so that a replayed step's loss survives
 * the next replay without a copy command between two graph launches.  skip (nullable, device int32: the err flag of
 * srec_copy_words_mailbox): non-zero = this step ran on a stale batch - the counters advance, the scalars written make every
 * Adam kernel of the step the identity (parameters and moments keep their bits), the loss slot reads NaN. */
int srec_adam_hyper_multi(int n, const void* counter, const void* cfg, const void* hyper, const int* tap_counter,
                          const float* tap_src, float* tap_ring, int tap_n, const int* skip, void* stream);
/* one launch for many small tensors (MT per launch, csrc/adam.hip: 88; any nt, launched MT at a time): desc = HOST
 * srec_adam_multi_desc below; the pointers travel by value in the kernel arguments (nothing staged in device memory; a
 * captured hipGraph bakes them into the node) */
typedef struct srec_adam_multi_desc {
    int nt;                    /* number of tensors */
    const int* use_wd;         /* [nt] apply the group's weight decay (0 for bias / batch_norm / activation, train.py:18) */
    const long* numel;         /* [nt] */
    float* const* p;           /* [nt] parameters ... */
    const float* const* g;     /* ... gradients ... */
    float* const* m;           /* ... exp_avg ... */
    float* const* v;           /* ... exp_avg_sq (device pointers, 4-B aligned; float4 path when all four are 16-B aligned) */
} srec_adam_multi_desc;
int srec_adam_multi(const void* desc, const float* hyper, void* stream);
/* item table, one wavefront per row.  max_norm > 0: Embedding(max_norm) renorm of the updated row (lessr.py:126,
 * msgifsr.py:162) - written back when renorm_write != 0, otherwise W keeps the plain Adam result (the reference
 * renormalises at the start of the NEXT forward) and only cs_out (nullable; = cs_scale / norm of the row as that forward
 * will see it: niser.py:151, msgifsr.py:279) reflects it.  dst16 (nullable; d <= 1024): bf16 copy [n, Dp] of the rows as
 * written - with renorm_write = 1 this pass leaves the table exactly as the next forward's stand-alone renorm + operand-copy
 * pass (srec_renorm_rows_bf16) would, which then need not run. */
int srec_adam_rows(float* W, const float* G, float* M, float* V, int n, int d, int ld, const float* hyper,
                   int use_wd, float max_norm, int renorm_write, float* cs_out, float cs_scale, int eps_mode,
                   float cs_eps, void* dst16, int Dp, void* stream);
int srec_adam_rows_proj(float* W, const float* G, float* M, float* V, int n, int d, int ld, const float* hyper, int use_wd,
                        float max_norm, int renorm_write, float* cs_out, float cs_scale, int eps_mode, float cs_eps,
                        const float* proj_cs, float proj_inv_scale, float* radial, void* dst16, int Dp, void* stream);
/* srec_adam_rows (proj_cs NULL) / srec_adam_rows_proj with the second level of a two-level lookup gradient folded in: row i
 * with u = slot[i] != 0 first adds s = sum of part[cptr[u - 1] .. cptr[u]) (dense rows of d floats, in piece order) to its
 * gradient and, with radial, <W_i, s> to radial[i] - the bits of srec_scatter_add_sorted_ex(part, .., accumulate = 1) followed by
 * the plain row pass - then clears slot[i].  G itself is NOT updated.  u_cap = entries of cptr - 1, n_part = rows of part. */
int srec_adam_rows_lookup(float* W, const float* G, float* M, float* V, int n, int d, int ld, const float* hyper, int use_wd,
                          float max_norm, int renorm_write, float* cs_out, float cs_scale, int eps_mode, float cs_eps,
                          const float* proj_cs, float proj_inv_scale, float* radial, void* dst16, int Dp, int* slot,
                          const float* part, const int* cptr, int u_cap, int n_part, void* stream);
/* the table's row pass and ONE multi-tensor launch (desc: at most 88 tensors, stepped with multi_hyper) as one launch of two
 * workgroup ranges; proj_cs / radial nullable as in srec_adam_rows / _proj, slot NULL: no lookup (part, cptr ignored).  The
 * bits of the two launches apart. */
int srec_adam_rows_multi(float* W, const float* G, float* M, float* V, int n, int d, int ld, const float* hyper, int use_wd,
                         float max_norm, int renorm_write, float* cs_out, float cs_scale, int eps_mode, float cs_eps,
                         const float* proj_cs, float proj_inv_scale, float* radial, void* dst16, int Dp, int* slot,
                         const float* part, const int* cptr, int u_cap, int n_part, const void* desc, const float* multi_hyper,
                         void* stream);

/* ---- MSGIFSR MSHGNN layer, all relations of both HeteroGraphConvs in one batched pass (hgat.hip) ------------------
 * Replaces msgifsr.py:70-89 (conv1(g) + conv2(reverse g), relation sum, head max, + session mean) around the fc GEMMs
 * of the GAT modules; `desc` points to a host srec_hg_desc (srec_hg.h).
 *   fwd: the caller has filled P[m] = x[rows of m] fc_m^T (p16 SREC_HG_FOLDED: and run srec_hg_fold); writes out[NT, D] = max_h(sum_rel rst + bias + n_rel x) +
 *        session mean of x, arg[NT, D] (winning head), and the saved A / eL / eR.
 *   bwd: g = d out; writes dx = n_rel g + session-mean term (the caller then accumulates dP[m] fc_m into it), dP[m],
 *        d_attn_l / d_attn_r / d_bias of every module.  ws: srec_hg_ws_floats() floats of scratch. */
int srec_hg_ws_floats(const void* desc, long* n_floats);
int srec_hg_fwd(const void* desc, const float* x, int ld_x, float* out, int ld_out, unsigned char* arg, void* stream);
/* the weight-only part of srec_hg_fwd on its own: V[m] (attention vectors folded into fc_m, gatconv.py:285-292 as a product over x)
 * and the per-type bias sums of desc.  srec_hg_fwd runs it itself unless SREC_HG_FOLDED in desc.p16 says it was done since the weights
 * last changed - by this call or by the step's prologue launch: */
int srec_hg_fold(const void* desc, void* stream);
/* desc: HOST srec_step_prep_desc (srec_hg.h): fold + bf16 weight copies + GRU / head fragment copies + mailbox intake, one launch
 * in front of a step (each of them a ~5 us graph node of its own otherwise; utils/train.py:94-101 is the step) */
int srec_step_prep(const void* desc, void* stream);
/* feature-dropout glue of a layer call in one pass each (GATConv feat_drop, gatconv.py:268-283): masks from the counter-based
 * hash of srec_gather_rows_drop (one mask per conv) and cnt [2, rows] (relation instances of the conv into each row): ms = mask / (1-p),
 * xc = x * ms (the convs' dropped inputs), rm = cnt0 ms0 + cnt1 ms1, xres = x * rm (summed identity residuals);
 * backward: dx += (sum_s t[0][s]) * ms0 + (sum_s t[1][s]) * ms1 (the convs' masked data gradients, t [2, S, n]: S partial sums
 * per conv, one per GAT module projecting the row's node type). */
/* ... and, in the same launch, the attention-dropout multipliers (gatconv.py:300) mk [na] = 0 or 1 / (1 - pa) (pa = 0: none) */
int srec_hg_drop_prep(const float* x, const float* cnt, int rows, int D, float p, int seed, const int* counter, int salt,
                      float* ms, float* xc, float* rm, float* xres, float pa, long na, float* mk, void* stream);
/* ... and, in the same pass, xc16 [2, rows, D] = bf16(xc): the operand copy the bf16 projection GEMM reads */
int srec_hg_drop_prep16(const float* x, const float* cnt, int rows, int D, float p, int seed, const int* counter, int salt,
                        float* ms, float* xc, float* rm, float* xres, float pa, long na, float* mk, void* xc16, void* stream);
/* live-source rows of every projection block of desc (HOST srec_hg_desc; only its topology is read): lists = HOST array of n_blocks
 * device pointers, lists[b] [ncap of the block's type] int32 <- ascending type-local rows u < *dyn_n with an out-edge
 * (out_ptr[i][u + 1] > out_ptr[i][u]) in at least one instance i whose SOURCE block is b; counts [n_blocks] (device) <- their
 * numbers.  A projection row is read only through the source index of such an edge (srec_hg_fwd / srec_hg_bwd), so the projection
 * GEMM may skip every row that is not listed (srec_gemm16_nt_rows).  One workgroup per block; at most 4 source instances per block. */
int srec_hg_live_rows(const void* desc, const void* lists, int* counts, void* stream);
/* ... srec_hg_drop_prep16 with srec_hg_live_rows(desc, lists, counts) as one more workgroup range of its launch */
int srec_hg_drop_prep16_live(const float* x, const float* cnt, int rows, int D, float p, int seed, const int* counter, int salt,
                             float* ms, float* xc, float* rm, float* xres, float pa, long na, float* mk, void* xc16,
                             const void* desc, const void* lists, int* counts, void* stream);
/* ... srec_hg_drop_prep (xc16 / desc + lists + counts nullable: else as _prep16 / _prep16_live) on rows that are formed in the same
 * pass: Y [rows, D] = the row-normalised X_p stacked, inv [rows] their 1 / norm - arguments and results of srec_normalize_group_fwd
 * (np <= 4 HOST arrays, sum nrow_p == rows; D <= 256: one wavefront per row).  Y is the x of the layer call. */
int srec_hg_drop_prep_norm(int np, const void* X, const int* ld, const int* nrow, const void* dyn, float* Y, float* inv, int eps_mode,
                           float eps, const float* cnt, int rows, int D, float p, int seed, const int* counter, int salt, float* ms,
                           float* xc, float* rm, float* xres, float pa, long na, float* mk, void* xc16, const void* desc,
                           const void* lists, int* counts, void* stream);
/* (ms of srec_hg_drop_prep / _prep16 is nullable: srec_hg_drop_merge with ms = NULL recomputes the masks from p / seed / counter /
 * salt, the mask tensor is then neither written nor read) */
int srec_hg_drop_merge(const float* t, int S, const float* ms, long n, float* dx, float p, int seed, const int* counter,
                       int salt, void* stream);
/* feature-dropout calls: SREC_HG_LATE_DX in desc.p16 makes srec_hg_bwd leave dx alone; after the caller's backward-data GEMMs
 * srec_hg_pre_merge writes the whole d x in one pass (the pre-fill of srec_hg_bwd + srec_hg_drop_merge: one kernel, one pass
 * over dx less); t [2, S, NT, D] as for srec_hg_drop_merge, masks recomputed from desc.rm_* */
int srec_hg_pre_merge(const void* desc, const float* g, int ld_g, const float* t, int S, float* dx, int ld_dx, void* stream);
int srec_hg_bwd(const void* desc, const float* x, int ld_x, const float* g, int ld_g, const unsigned char* arg, float* dx,
                int ld_dx, float* ws, void* stream);
/* The layer with its caller's L2 normalisations inside its own launches (node kernels only: H == 8, D % 8 == 0, D <= 256, at most 8
 * relation instances into a type; anything else is SREC_BAD_ARG).  Each writes every byte, with the same value, that the pair of calls
 * it stands for writes.
 *   srec_hg_fwd_exit = srec_hg_fwd + srec_norm_perm_pick_fwd without the un-normalised out: allf [NT, D] / invr [NT] in per-session
 *     order (cat_inv [NT]: stacked row -> concatenated row, -1 = capacity padding; there are as many concatenated as stacked rows),
 *     the left D columns of pout[k] [B, .] (row stride ld_p[k]) = the normalised output row pick[k][b] (zeros for b >= *dynB or
 *     a negative pick).  B = desc.B is the length of every pick list.  HOST arrays of npick <= 4.
 *   srec_hg_bwd_exit = srec_norm_perm_pick_bwd + srec_hg_bwd: g [NT, D] is an OUTPUT, formed from g_allf (row stride ld_ga) and the
 *     pick gradients g_pick[k] [B, D] (row stride ld_gp[k], entries nullable) by the score-gradient launch.
 *   srec_hg_pre_merge_norm = srec_hg_pre_merge + srec_normalize_group_bwd without the stacked dx: the layer's x is Y [NT, D], the
 *     normalised rows of one raw tensor per node type (inv [NT] their 1 / norm); dX[t] [ncap[t], D] (row stride ld[t]; HOST arrays of
 *     n_types entries) receives the gradient of type t's raw rows. */
int srec_hg_fwd_exit(const void* desc, const float* x, int ld_x, unsigned char* arg, const int* cat_inv, float* allf, float* invr,
                     int npick, const void* pick, const void* pout, const int* ld_p, int eps_mode, float eps, void* stream);
int srec_hg_bwd_exit(const void* desc, const float* x, int ld_x, float* g, int ld_g, const unsigned char* arg, float* dx, int ld_dx,
                     float* ws, const int* cat_inv, const float* allf, const float* invr, const float* g_allf, int ld_ga, int npick,
                     const void* pick, const void* g_pick, const int* ld_gp, void* stream);
int srec_hg_pre_merge_norm(const void* desc, const float* g, int ld_g, const float* t, int S, const float* Y, const float* inv,
                           const void* dX, const int* ld, void* stream);

/* grouped, K-segmented bf16-operand GEMM (gemm_group_bf16.hip): up to 8 problems C_p [M,N] (+)= sum_s opA(A_ps) opB(B_ps)
 * in one launch.  desc: host srec_gemm_group (srec_hg.h).  mode 0: A [M,K], B [N,K] (nn.Linear forward); 1: A [M,K],
 * B [K,N] reduction-major, segments summed (backward-data over several modules); 2: A [K,M], B [K,N] both
 * reduction-major (weight gradient; dyn clamps the reduction).  dyn clamps the output rows in modes 0 / 1. */
int srec_gemm_group_bf16(const void* desc, int mode, void* stream);

/* grouped exact-fp32 GEMM (csrc/gemm.hip): desc = srec_gemm_f32_group (srec_hg.h), every problem as srec_gemm_f32.  One
 * launch for all tiles of all problems (+ one reduce launch when a long-K problem was k-split into slabs of ws).
 * Replaces the chain of cuBLAS calls of the attention read-out / session-vector head (msgifsr.py:127-146,272-279;
 * srgnn.py:73-88,123-127) and their backward. */
int srec_gemm_f32_group_run(const void* desc, float* ws, long ws_floats, void* stream);
/* ... with the slab sums of the plain split problems (alpha 1, beta 0, no bias, no row clamp: weight gradients) left
 * to the caller where the caller allows it (slab_n[p] != 0 ON ENTRY): slab_off[p] = float offset of problem p's slabs in ws (-1:
 * finished by the call), slab_n[p] = their count, each M N floats (dense), to be summed into C[p] (srec_sum_slabs_multi_ld when ldc != N).  ws must be
 * private to the call until that sum has run. */
int srec_gemm_f32_group_run_defer(const void* desc, float* ws, long ws_floats, long* slab_off, int* slab_n, void* stream);
/* bf16-in-HBM grouped GEMMs (gemm16.hip): the GAT fc projections and their backward (gatconv.py:166-175,282-283) with every
 * operand already stored as bf16 - LDS-DMA staging, no conversion pass.  desc: host srec_gemm16_group (srec_hg.h, up to 16
 * problems per launch).
 *   srec_gemm16_nt: C_p [M, N] (+)= sum_s A_ps [M, K] B_ps [N, K]^T; K % 32 == 0, lda / ldb % 8 == 0; c16 = bf16 output;
 *                   dyn clamps the output rows (rows past it: zeros when beta == 0 or c16).
 *   srec_gemm16_tn: C_p [M, N] = beta C_p + sum_s sum_{m < min(K, *dyn)} A_ps [m, M] B_ps [m, N]  (weight gradients: the
 *                   reduction runs over rows; both operands row-major as stored, M / N % 8 == 0), fp32 output.
 *   srec_rows_bf16: dst16 [n, d] = bf16(src [n, d]), zero rows past *dyn.
 *   srec_weights_bf16: n <= 8 matrices W_i [R_i, C_i] fp32 -> bf16 copy and transposed bf16 copy [C_i, R_i] in one launch;
 *                   W / W16 / WT16 are HOST arrays of n device pointers (WT16 entries may be NULL), R / Cc HOST int arrays. */
int srec_gemm16_nt(const void* desc, void* stream);
/* srec_gemm16_nt over row lists: rows = HOST array of np device pointers (a NULL entry: that problem takes all rows).  Problem p
 * computes the rows rows[p][0 .. *dyn[p]) of C_p only - ascending int32 row numbers < M, dyn[p] = the list's device count - from the
 * same rows of A_p; every other row of C_p is left unwritten, a listed row gets the bytes srec_gemm16_nt gives it.  bf16 output
 * with SREC_G16_KEEP_DEAD only (the forward projections over the live-source rows of srec_hg_live_rows). */
int srec_gemm16_nt_rows(const void* desc, const void* rows, void* stream);
int srec_gemm16_tn(const void* desc, void* stream);
/* two srec_gemm16_tn launches as ONE: the problems of desc_a (family A) and of desc_b (family B), np_a + np_b <= SREC_G16_MAXP, equal
 * beta; every output tile gets the bytes the launch of its own desc gives it.  Each family's tiles are dealt to the XCDs in runs of
 * their own, the tile order within a family is that of srec_gemm16_tn; family A takes the low workgroup indices (it starts first)
 * unless b_first != 0. */
int srec_gemm16_tn2(const void* desc_a, const void* desc_b, int b_first, void* stream);
int srec_rows_bf16(const float* src, int ld, int n, const int* dyn, int d, void* dst16, void* stream);
/* out [C, n] = sum_r part [C, R, n] in fixed order (the row-split weight-gradient products of one module), n % 4 == 0 */
int srec_sum_slabs(const float* part, int C, int R, long n, float* out, void* stream);
int srec_weights_bf16(int n, const void* W, const void* W16, const void* WT16, const int* R, const int* Cc, void* stream);
/* MSGIFSR after its last MSHGNN layer in ONE launch each way (csrc/rowops.hip): F.normalize of every node row
 * (msgifsr.py:260-263), the per-session concatenation of all orders' nodes (msgifsr.py:135, perm = cat_perm of the FlatBatch)
 * and the last-node picks (filter_nodes, msgifsr.py:264): allf [n_cap, D], invr [n_cap] = 1 / norm, pout_k [B, D].
 * pick / pout / ld_p / g_pick / ld_gp / row0 / ncap / dyn_n are HOST arrays.  The backward writes EVERY row of dx [n_rows, D] (capacity padding as zeros). */
int srec_norm_perm_pick_fwd(const float* x, int ld_x, const int* perm, int n_cap, const int* dyn_t, int D, int eps_mode,
                            float eps, float* allf, float* invr, int npick, int B, const int* dyn_b, const void* pick,
                            const void* pout, const int* ld_p, void* stream);
int srec_norm_perm_pick_bwd(const float* allf, const float* invr, const float* g_allf, int ld_g, const int* perm, int n_cap,
                            const int* cat_seg, int B, const int* dyn_b, int D, int npick, const void* pick, const void* g_pick,
                            const int* ld_gp, float* dx, int ld_dx, int nt, const int* row0, const int* ncap, const void* dyn_n,
                            int n_rows, void* stream);
/* k-gram GRU of the SemanticExpander, all orders per launch (grux.hip; msgifsr.py:25,32-45): desc = host
 * srec_gru_step_desc (srec_hg.h).  d % 4 == 0 and 256 % (d / 4) == 0. */
int srec_gru_step_fwd(const void* desc, void* stream);
int srec_gru_step_bwd(const void* desc, void* stream);
/* forward of ALL time steps in one launch (csrc/gruf.hip; d = 128 / 256): desc = HOST srec_gru_fused_desc (srec_hg.h);
 * srec_gru_wfrag: n <= 8 GRU weights W_i [3 d, d] fp32 -> fragment-major bf16 copies dst_i [3 d d] (W, dst: HOST arrays of
 * device pointers), the B operands the fused forward streams */
int srec_gru_fused_fwd(const void* desc, void* stream);
int srec_gru_wfrag(int n, const void* W, const void* dst, int d, void* stream);
/* backward of all time steps in one launch (csrc/grufb.hip): desc = HOST srec_gru_fused_bwd_desc; srec_gru_wfrag_t: the
 * fragment-major weight copies for its backward-data products (B operand = W [3 d, d] itself, reduction over its rows) */
int srec_gru_fused_bwd(const void* desc, void* stream);
/* nodes per workgroup (16 / 32) both use for np problems of n[p] nodes; bias_part of the backward holds one row [6 d] per
 * workgroup: sum_p ceil(n[p] / nodes) rows */
int srec_gru_fused_nodes(int np, const int* n, int d, int* nodes);
/* mixed launches (round 6): with 16-node workgroups and every k[p] <= 4, the problems - in LAUNCH order: longest k first, as both
 * launchers sort them - whose workgroups hold 32 nodes instead, so that one launch is at most one workgroup per CU (bit p of
 * *mask; the shortest problems first, never those of the longest order - their 16-node kernel batches the input projections; 0 = none).  A workgroup of the fused kernels owns a CU and lives as long as its weight
 * stream whatever its node count: the bench batches (250 - 280 live 16-node tiles on 256 CUs) ran a second round on ~45 % of the
 * steps.  bias_part keeps one row per 16 nodes: a 32-node workgroup writes row 2 t and zeroes row 2 t + 1. */
int srec_gru_fused_wide(int np, const int* n, const int* k, int* mask);
/* waves per workgroup (4 / 8) of both and of the fragment-major weight copies for hidden size d */
int srec_gru_fused_waves(int d, int* waves);
int srec_gru_wfrag_t(int n, const void* W, const void* dst, int d, void* stream);
/* both copies of the same weights in one launch */
int srec_gru_wfrag_both(int n, const void* W, const void* dst_fwd, const void* dst_bwd, int d, void* stream);
/* out[p] [ncol] = column sums of part[p] [rows[p], ncol] for np <= 4 problems in one launch (the GRU bias gradients from the
 * per-block partial rows of srec_gru_step_bwd); part / out: HOST arrays of np device pointers, rows: HOST int array */
int srec_gru_bias_final(int np, const void* part, const int* rows, int ncol, const void* out, void* stream);
/* np <= 32 outputs out_i [n_i] = sum_r part_i [R_i, n_i] in one launch (row-split weight gradients); HOST arrays.  tall
 * (nullable HOST array): tall_i != 0 = few columns summed over hundreds of rows (the GRU bias partials of srec_gru_fused_bwd
 * / srec_gru_step_bwd, what srec_gru_bias_final does as a launch of its own).  Column tasks: n_i % 4 == 0, both pointers
 * 16-byte aligned; tall tasks are scalar (any n_i, any alignment).  With R_i = 1 a task is a copy: the row-sharded path fills
 * its gradient-bucket arenas with it (dist.VocabParallel._bucket_fill: gradients that did not land in their slot, zeros for
 * parameters without a gradient on this rank, the flag tail) - no torch.cat in the rank step. */
int srec_sum_slabs_multi(int np, const void* part, const int* R, const long* n, const void* out, const int* tall,
                         void* stream);
/* ... with strided destinations: w_i > 0 = out_i is a block of w_i columns in rows of stride ld_i floats (a column slice of a
 * weight gradient: the concat-free linear layers); w, ld: HOST int arrays, both or neither nullable */
int srec_sum_slabs_multi_ld(int np, const void* part, const int* R, const long* n, const void* out, const int* tall,
                            const int* w, const int* ld, void* stream);
/* ... and with the optimizer's step-scalar role (srec_adam_hyper_multi, arguments as there) in one more workgroup of the same launch:
 * the end-of-backward sums of a captured step and the Adam scalars need nothing of each other (one ~6 us graph node less) */
int srec_sum_slabs_multi_hyper(int np, const void* part, const int* R, const long* n, const void* out, const int* tall,
                               const int* w, const int* ld, int nh, const void* counter, const void* cfg, const void* hyper,
                               const int* tap_counter, const float* tap_src, float* tap_ring, int tap_n, const int* skip,
                               void* stream);

/* ---- evaluation: K best items per session without the (B, V) score matrix (topk.hip) -----------------------------
 * Replaces `logits = model(...); logits.topk(20)` of train.py:36-55 for models whose score is one soft-max
 * (ranking by z[b,v] = cs[v] * <sr_b, E_v>): out_val [B,K] descending, out_idx [B,K] int32 item ids, ties towards
 * the lower id.  K <= 32, d % 4 == 0; ws: srec_score_topk_ws() bytes. */
int srec_score_topk_ws(int B, int V, int K, long* bytes);
int srec_score_topk(const float* sr, int ld_sr, const float* E, int ld_e, const float* cs, int B, int V, int d, int K,
                    float* out_val, int* out_idx, void* ws, void* stream);

/* ---- serving and evaluation: THE SERVED SCORE and its operands (score_pass.h) ----------------------------------------------
 * Every entry point of the sections below scores the rows of one table under the same score, and takes its operands as ONE
 * host struct, `const void* served` -> srec_served (the convention of srec_head_fwd(const void* desc, ...); the pointers
 * inside are DEVICE pointers; the struct is read during the call only):
 *   s[b,v]  = logsumexp_{c<C}( cs[v] * <sr_c[b], E_v> + off[c,b] ),  off = off_in if v is in listed[b,:] else off_ex
 *             (C == 1: s = z + off, no exp / log)
 *   s'[b,v] = s[b,v] + bias[group[b] * ld_bias + v]     the BIASED served score: one more operand, added AFTER the mixture
 * (msgifsr.py:281-321: order fusion, repeat / explore gate, also where the score mixes several soft-maxes).
 * Layouts: sr: C blocks [B, d] (row stride ld_sr, block stride comp_stride); E [V, d] (row stride ld_e); cs [V]; off_ex /
 * off_in [C, B] (NULL = 0); listed [B, L] global item ids, -1 = empty slot, every id at most once per session (NULL / L = 0:
 * none; L > 0 with listed == NULL is taken as L = 0); id_lo: global id of local row 0 (row-sharded tables).  cs / off_* /
 * listed / bias / group nullable.  Limits: 1 <= C <= 4, d % 4 == 0, d <= 1024, 0 <= L <= 64, ids below 2^31 (id_lo + V <=
 * INT_MAX; srec_score_rank, which never forms such an id, does not ask for it); fp32 MFMA, no (B, V) tensor.
 * listed_mode SREC_LISTED_SCORE: an item of listed[b,:] scores with off_in; SREC_LISTED_DROP: an item of listed[b,:] is not
 * eligible for session b and off_in is ignored.
 * bias - a log-prior correction, a boost or a penalty; -INFINITY means "item v is not in the catalogue for this call".  fp32,
 * indexed by the LOCAL row like cs (a row shard passes the pointer to its first column and the full row stride ld_bias), G
 * rows; group [B] picks the row of every session, group == NULL means row 0 for every session and is legal only with G == 1
 * (ld_bias is not read then).  bias == NULL (the plain call carries G = 1 and group = NULL beside it; a G > 1
 * with its group is accepted and not read) IS the unbiased case of every entry point, bit for bit, the same kernel instances.  NaN or +INFINITY in bias and a group id outside [0, G) are the CALLER's
 * error: nothing here looks for them, the kernels assume neither occurs (a group id is held inside [0, G), nothing else is
 * promised for it).  An all-zero bias returns the ids and (by ==) the values of the unbiased call.
 * ELIGIBLE: a (session b, row v) pair with v in [0, V) of this call (global id id_lo + v, a row shard), unless the item is
 * listed under SREC_LISTED_DROP or its bias is -INFINITY (eligibility is tested by itself: an eligible item that merely scores
 * -INFINITY is still eligible).
 * Every entry point returns SREC_BAD_ARG for served == NULL, ahead of everything; then 0 and no launch for B <= 0, ahead of
 * every other check of the descriptor.  Nonzero and no launch for: sr or E not aligned to 16 bytes, ld_sr / ld_e /
 * comp_stride not multiples of 4, d % 4 != 0, V, d, C or L out of range, id_lo < 0, ids that do not fit (above), a listed_mode
 * other than the two; G < 1; group == NULL with G > 1; bias != NULL with ld_bias < V and G > 1; bias or group not aligned to 4
 * bytes.  The *_ws functions take the shape alone. */
#define SREC_LISTED_SCORE 0
#define SREC_LISTED_DROP 1
typedef struct srec_served {
    const float* sr; int ld_sr; long comp_stride;   /* the session vectors */
    const float* E; int ld_e;                       /* the table */
    const float* cs;                                /* the column scale */
    const float* off_ex; const float* off_in;
    const int* listed; int L; int listed_mode;
    long id_lo;
    int B, V, d, C;
    const float* bias; long ld_bias;
    const int* group; int G;
} srec_served;

/* ---- evaluation: rank of the label among ALL items, any cutoff, mixtures of soft-maxes too (rank.hip) ---------------
 * Replaces `logits = model(...); logits.topk(20)` of train.py:36-55 by the one integer every HR / MRR / NDCG @k is a function
 * of.  The score is s of the served score; the rank kernels know neither a bias nor SREC_LISTED_DROP: a descriptor with
 * bias != NULL or listed_mode != SREC_LISTED_SCORE is refused (SREC_BAD_ARG), never ignored.
 * labels[b] global id (< 0: rank -1).  rank[b] = # local rows v with id_lo + v != labels[b] and
 * (s > target[b] or (s == target[b] and id_lo + v < labels[b])): ties towards the lower id, as srec_score_topk.
 * target [B]: written here (the label's score where this table owns the label, else 0) unless target_given.  Ranks and
 * targets of disjoint row shards add up; rank == NULL runs the target pass alone (a shard's share, ahead of that sum). */
int srec_score_rank_ws(int B, int V, int d, int C, int L, long* bytes);
int srec_score_rank(const void* served, const int* labels, float* target, int target_given, int* rank, void* ws,
                    void* stream);

/* ---- serving: the K best ELIGIBLE items per session under the biased served score (recommend.hip) -----------------------
 * out_val [B, K] fp32 descending (the biased scores), out_idx [B, K] int32 global ids id_lo + row; ties towards the lower id
 * (srec_score_topk, srec_score_rank); a session with fewer than K eligible rows gets (-INFINITY, -1) in the remaining slots,
 * so K > V is allowed - an ineligible item (listed and dropped, bias -INFINITY) is NEVER returned, while an eligible item that
 * merely scores -INFINITY still precedes an unfilled slot.  1 <= K <= SREC_SELECT_MAXK.  The output is a pure function of the
 * inputs (no atomics; lists are ordered by (value descending, id ascending), never by arrival).
 * floor fp32 [B], nullable (the floor of srec_score_cutoff): a (session b, row v) pair is additionally INELIGIBLE when
 * s'[b,v] < floor[b] - the test is on the biased served score, before temperature and noise.  floor == NULL IS the call
 * without a floor, bit for bit (the same kernel instances).  A session whose kept set is smaller than K ends in
 * (-INFINITY, -1) slots.  floor aligned to 4 bytes.
 * ws: srec_score_select_ws() bytes (per-range partial lists), with or without a bias or a floor.  Nonzero and no launch,
 * beyond the descriptor's reasons: K out of range, a NULL output or ws, floor misaligned. */
#define SREC_SELECT_MAXK 128
int srec_score_select_ws(int B, int V, int d, int C, int L, int K, long* bytes);
int srec_score_select(const void* served, int K, const float* floor, float* out_val, int* out_idx, void* ws, void* stream);

/* ---- serving: the score of GIVEN items per session (score_items.hip) ---------------------------------------------------
 * Replaces `logits = model(...); logits.gather(1, items)` (msgifsr.py:306-321 / srgnn.py:145-147) for re-ranking, allow-lists,
 * sampled-negative evaluation and lists longer than SREC_SELECT_MAXK: out[b,m] (fp32 [B, M]) is the biased served score at
 * the global id items[b * ld_items + m].  ld_items == 0: one list of M ids shared by all sessions.  Per slot: an id < 0
 * (padding) gives -INFINITY; a row outside [id_lo, id_lo + V) belongs to another shard and gives 0.0f without any read of the
 * table OR of the bias, so the results of disjoint row ranges ADD UP (as the targets of srec_score_rank), to the bits of one
 * device; the shard that owns the id adds the bias, and -INFINITY stays -INFINITY; SREC_LISTED_SCORE: an item of listed[b,:]
 * scores with off_in; SREC_LISTED_DROP: the shard that owns it gives -INFINITY (off_in is ignored).  Duplicate ids in a list
 * are legal and scored independently.  The output is a pure function of the inputs: the summation order depends on (d, C)
 * alone, no atomics, no workspace.  Nonzero and no launch, beyond the descriptor's reasons: ld_sr < d or ld_e < d, M < 1,
 * 0 < ld_items < M, items or out NULL or not aligned to 4 bytes. */
int srec_score_items(const void* served, const int* items, long ld_items, int M, float* out, void* stream);

/* ---- serving: the log-normaliser of the served score over the ELIGIBLE catalogue (score_norm.hip) -----------------------
 * out[b] (fp32 [B]) = logsumexp over the eligible rows v of s'[b,v]: an item whose bias is -INFINITY does not contribute;
 * SREC_LISTED_SCORE: an item of listed[b,:] contributes with off_in; SREC_LISTED_DROP: it does not contribute and off_in is
 * ignored.  A session without an eligible row (or whose eligible rows all score -INFINITY) gives exactly -INFINITY, never NaN.
 * Subtracting out[b] from off_ex[:, b] and off_in[:, b] renormalises what srec_score_select / srec_score_items return:
 * logsumexp_c(z_c + off_c - Z) = s - Z.  The disjoint row ranges of shards combine by log-sum-exp of their results.
 * No (B, V) tensor, no float atomics: one (max, sum) pair per (item range, session) in ws, folded in range order - the
 * output is a pure function of the inputs.  ws: srec_score_norm_ws() bytes.  Nonzero and no launch, beyond the descriptor's
 * reasons: a NULL out or ws. */
int srec_score_norm_ws(int B, int V, int d, int C, int L, long* bytes);
int srec_score_norm(const void* served, float* out, void* ws, void* stream);

/* ---- serving: DRAW K distinct items per session from the served distribution (recommend.hip, NOISE instances) ------------
 * The selection of srec_score_select over the SAMPLED key of every eligible (session b, row v) pair,
 *   key[b,v] = s'[b,v] * inv_temperature + g(seed, q[b], id_lo + v),
 * inv_temperature = 1 / T > 0 and finite, q[b] = session_keys[b] (any 32-bit value; NULL: the row index b), g independent
 * Gumbel(0, 1) noise.  By the Gumbel-top-k identity the K best keys, in order, are a draw WITHOUT replacement (Plackett-Luce)
 * from p(v) ~ exp(s'[b,v] / T) over the eligible rows.  out_key [B, K] fp32 descending, out_idx [B, K] int32 global ids in
 * draw order; ties towards the lower id; (-INFINITY, -1) slots where fewer than K rows are eligible; K <= SREC_SELECT_MAXK;
 * floor as in srec_score_select (NULL: no floor, the same kernel instances); ws: srec_score_sample_ws() bytes.
 * The noise is counter-based - a pure function of (seed, q, GLOBAL id), csrc/sample_noise.h; nothing (B, V)-sized exists:
 *   h32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16       (32-bit, "lowbias32")
 *   skey = h32(lo ^ h32(q * 0x9E3779B9 + hi * 0x85EBCA6B + 0x165667B1))      lo / hi: the 32-bit words of seed; per session
 *   h    = h32(skey ^ ((unsigned)gid * 0x9E3779B1 + 0x7F4A7C15))             per pair; a bijection of gid for a fixed session
 *   w    = fminf(fmaf((float)h, 0x1p-32f, 0x1p-33f), 0x1.fffffep-1f)         in (0, 1)
 *   g    = -logf(-log1pf(-w))                                                in [-2.82, 22.9], always finite
 * so a call is reproducible, a session's draw does not depend on the batch it is in (give it the same key), and the lists
 * of disjoint row shards - every shard with its id_lo - merge by (key, id) to the bits of the single-device call.
 * Nonzero and no launch for the reasons of srec_score_select, for inv_temperature that is not positive and finite
 * (zero, negative, infinite, NaN) and for session_keys not aligned to 4 bytes.
 * srec_sample_uniform: HOST function, no GPU - h_out / w_out [n_b, n_v] (either may be NULL, not both) are h and w of the
 * formula for the keys session_keys[0 .. n_b) (NULL: 0 .. n_b - 1) and the global ids ids[0 .. n_v) (NULL: 0 .. n_v - 1):
 * the stream pinned for tests and for users who restate a draw. */
int srec_score_sample_ws(int B, int V, int d, int C, int L, int K, long* bytes);
int srec_score_sample(const void* served, int K, float inv_temperature, unsigned long long seed, const int* session_keys,
                      const float* floor, float* out_key, int* out_idx, void* ws, void* stream);
int srec_sample_uniform(unsigned long long seed, const int* session_keys, int n_b, const int* ids, int n_v,
                        unsigned* h_out, float* w_out);

/* ---- serving: TRUNCATED sampling - a per-session score cutoff found without the (B, V) matrix (score_cutoff.hip); its
 * result is the floor operand of srec_score_select / srec_score_sample ---------------------------------------------------
 * Per session b, over the eligible rows and the biased served score s'[b,v] of the descriptor.  m_b = the largest eligible
 * s';  w_v = exp((s'_v - m_b) * inv_t) and W_b = sum of w_v over the eligible rows;  inv_t = 1 / T is the temperature the
 * draw will use.
 * Three criteria, each optional, each evaluated on the FULL eligible distribution (not one after the other):
 *   top_k (integer >= 1, any size - not limited to SREC_SELECT_MAXK; 0 = absent): tau_k = the k-th largest eligible s',
 *     counting multiplicity; with fewer than k eligible rows it is -INFINITY.
 *   top_p (0 < p < 1; p >= 1 = absent): tau_p = the largest eligible score value t with  sum_{s' >= t} w >= p * W  - the last
 *     value of the shortest descending prefix that reaches p.  Items tied with that value are all inside: the kept set is a
 *     function of a VALUE alone, ids never break a tie at the boundary.
 *   min_p (0 < q <= 1): tau_q = m_b - min_gap, in fp32.  The host computes min_gap = -T ln q in double and rounds it once
 *     to fp32; it is a scalar like inv_temperature.  min_gap = +INFINITY = absent.
 * Outputs: floor[b] fp32 = the largest of the criteria given, -INFINITY when none is given;  count[b] int32 = #{eligible,
 * s' >= floor};  log_kept[b] fp32 = log(sum_{s' >= floor} w / W), always <= 0;  top[b] fp32 = m_b.
 * A session with nothing eligible gives (-inf, 0, -inf, -inf).  A session whose eligible rows all score -inf gives floor =
 * -inf, count = the number of eligible rows and log_kept = 0.  Never NaN.  An eligible row scoring -inf has weight 0 and is
 * counted only under floor = -inf.  -0.0 is canonicalised (the comparisons are on s' + 0.0f).  NaN scores are the caller's
 * error, as elsewhere.
 * No (B, V)-sized tensor, no float atomics; the outputs are a pure function of the inputs, do not depend on the item-range
 * split of a launch, and disjoint row shards combine to THE BITS of the single-device result.  The cutoff compares the same
 * fp32 s' the select / sample kernels form (score_tile.h, SCORE_PASS_ITEM_SCORE), so the boundary item passes its own floor.
 * How: s' + 0.0f maps to an order-preserving 32-bit key (sign bit flipped for s' >= 0, all bits for s' < 0), searched by
 * radix, 8 bits per pass of the catalogue (SREC_CUTOFF_PASSES = 4 passes, numbered 0 .. 3: the key is then known to the bit).  Pass j builds,
 * per session, a 256-bin histogram over digit j of the eligible pairs whose higher digits equal the session's prefix: COUNTS
 * for top_k, MASS for top_p (the two searches keep separate prefixes).  Mass is fixed-point INTEGER, x = (u64)(w * 2^44),
 * w in fp32 (expf), clamped to 1: integer sums are order-free, so per-range partials and shards add exactly (quantum 2^-44:
 * the truncation loses at most V * 2^-44 < 1e-6 of W >= 1 for V <= 2^24).  A bin sum of more than 2^19 items would not fit
 * 64 bits, so a workgroup never covers more, and outside the workgroup a sum travels as TWO int64 limbs (sum of x mod 2^32,
 * sum of x >> 32; value = hi * 2^32 + lo, 128-bit arithmetic where they are read).  The pass-0 total is W.  The target of
 * top_p: p is taken as P / 2^32, P = round(p * 2^32) held in [1, 2^32 - 1], and "mass >= p W" is the exact integer test
 * mass * 2^32 >= P * W.  After the 4 passes one more pass (the TAIL: the same kernel, the bin is "s' + 0.0f >= floor")
 * gives count, kept mass and W for the final floor - uniform over the criteria and their combination - and
 * log_kept = (float) log((double) kept / (double) W) (0 where W = 0 and count > 0).
 * Shards all-reduce integers between the passes, so the ABI is pass-granular:
 *   hist  int64 [B][3][256]: counts, mass limb lo, mass limb hi of one pass - ZEROED by the pass entry points, then added to
 *         with integer atomics (empty bins are skipped); SUM over shards.
 *   state int64 [B][SREC_CUTOFF_STATE]: prefix of the top_k search, of the top_p search, count above, mass above (lo, hi),
 *         W (lo, hi), flags (1: fewer than k eligible rows, 2: W = 0) - written by advance, the same on every shard.
 *   top   fp32 [B]: m_b, from the K = 1 selection (srec_score_select; MAX over shards) - needed ahead of pass 0.
 * srec_score_cutoff_hist (pass 0 .. 3) reads top and state (pass 0: state is not read); srec_score_cutoff_advance (pass
 * 0 .. 3, no table access, one workgroup per session) scans the summed bins from the top, fixes the next digit of either
 * search and, at pass 3, writes floor (and top[b] + 0.0f back into top); pass = SREC_CUTOFF_PASSES does that last step alone
 * (neither top_k nor top_p given: no histogram is needed).  srec_score_cutoff_tail fills hist bins 0 (below) and 1 (kept);
 * srec_score_cutoff_finish turns the summed tail bins into count and log_kept.  No host synchronisation anywhere.
 * srec_score_cutoff chains everything on one device: ws = srec_score_cutoff_ws() bytes (hist, state and the K = 1 selection's
 * scratch).
 * All return nonzero and do not launch for the reasons of srec_score_select, for inv_temperature not positive and
 * finite, top_k < 0, top_p <= 0 or NaN, min_gap < 0 or NaN, pass out of range, a NULL top / state / hist / floor / output. */
#define SREC_CUTOFF_PASSES 4
#define SREC_CUTOFF_STATE 8
int srec_score_cutoff_ws(int B, int V, int d, int C, int L, long* bytes);
int srec_score_cutoff_hist(const void* served, float inv_temperature, int top_k, float top_p, int pass, const float* top,
                           const long long* state, long long* hist, void* stream);
int srec_score_cutoff_advance(int B, int pass, int top_k, float top_p, float min_gap, const long long* hist,
                              long long* state, float* top, float* floor, void* stream);
int srec_score_cutoff_tail(const void* served, float inv_temperature, const float* top, const float* floor, long long* hist,
                           void* stream);
int srec_score_cutoff_finish(int B, const long long* hist, int* count, float* log_kept, void* stream);
int srec_score_cutoff(const void* served, float inv_temperature, int top_k, float top_p, float min_gap, float* floor,
                      int* count, float* log_kept, float* top, void* ws, void* stream);

/* ---- serving: top-N lists BEYOND SREC_SELECT_MAXK - collect what the cutoff keeps, then order it (select_many.hip) ---------
 * The K best eligible items per session under the biased served score for 1 <= K <= SREC_SELECT_MANY_MAXK, the contract of
 * srec_score_select (descending values, ties towards the lower id, (-INFINITY, -1) once the eligible rows run out), without
 * the (B, V) matrix and without a running list in LDS.  floor = the floor of srec_score_cutoff(top_k = K) at temperature 1
 * over the same descriptor (over the WHOLE catalogue for a row shard), whose count[b] is exactly the number of pairs the
 * collect pass finds for session b: both form s' through the same tile product.  count exceeds K only by rows that tie with
 * the K-th.  An eligible row that merely scores -INFINITY is collected (and counted) only under floor = -INFINITY, i.e. when
 * the session has fewer than K eligible rows; it then precedes the unfilled slots with value -INFINITY and its own id.
 * srec_score_select_many_collect: one pass over the table.  Every eligible (session b, row v) pair with !(s'[b,v] < floor[b])
 *   - the test of srec_score_select's floor - is appended as (s', id_lo + v) to row b of buf_val (fp32) / buf_idx (int32),
 *   both [B, cap]; n int32 [B] is ZEROED here and counts the pairs with integer atomics, one returned atomic per (workgroup,
 *   session, 128-item chunk) that has any.  A pair whose slot would be >= cap is counted and not written: n[b] > cap tells the
 *   caller that the row is incomplete.  The ORDER inside a row is arrival order and means nothing; the SET is a pure function
 *   of the inputs.  No float atomics.
 * srec_score_select_many_order: no table access, one workgroup per session.  Sorts the first min(n[b], cap) pairs of row b by
 *   (value descending, id ascending) - distinct keys, so the output is a pure function of the set - and writes the first K
 *   to out_val / out_idx [B, K], (-INFINITY, -1) behind them.  Values come back as s' + 0.0f (-0.0 is canonicalised, as in
 *   srec_score_cutoff).  cap <= SREC_SELECT_MANY_SORT pairs (64 KB of 64-bit keys in LDS); a caller with more pairs in a row
 *   (more than SORT - K rows tie with the K-th) orders the buffer by other means.
 * The lists of disjoint row shards - every shard with its id_lo, the floor of the whole catalogue - merge by (value, id) to the
 * bits of the single-device call.  Both return SREC_BAD_ARG and do not launch for: (collect) the descriptor's reasons, cap < 1,
 * a NULL or misaligned floor / buffer / n; (order) K outside 1 .. SREC_SELECT_MANY_MAXK, cap < 1, cap > SREC_SELECT_MANY_SORT,
 * a NULL or misaligned n / buffer / output.  No workspace. */
#define SREC_SELECT_MANY_MAXK 4096
#define SREC_SELECT_MANY_SORT 8192
int srec_score_select_many_collect(const void* served, const float* floor, int cap, float* buf_val, int* buf_idx, int* n,
                                   void* stream);
int srec_score_select_many_order(int B, int cap, const int* n, const float* buf_val, const int* buf_idx, int K, float* out_val,
                                 int* out_idx, void* stream);

/* ---- evaluation of what is SERVED: the eligible rows ahead of a given label under the biased served score (rank_served.hip) --
 * The rank of the label among what a user is shown - under a bias, allow / deny lists, exclude-seen and a truncation floor -
 * which srec_score_rank refuses to compute; srec_score_rank is unchanged.  No (B, V) tensor.
 * labels [B] int32 global ids; target [B] fp32 = the label's biased served score, exactly what srec_score_items returns for it
 * (bias included, -INFINITY for a dropped or out-of-catalogue item, shard results summed): an INPUT, there is no target pass.
 * ahead[b] (int32 [B]) = the number of local rows v for which ALL of these hold:
 *   (b, v) is ELIGIBLE (above);  id_lo + v != labels[b] - the label is left out by id, never by its score;
 *   !(s'[b,v] < floor[b]) when floor != NULL - the floor of srec_score_cutoff, as srec_score_select tests it;
 *   s'[b,v] > target[b], or s'[b,v] == target[b] and id_lo + v < labels[b] - ties towards the lower id, as everywhere.
 * labels[b] < 0 writes 0.  ahead is WRITTEN, not accumulated (zeroed on the stream by the call).  Counts of disjoint row shards
 * add up; a label another shard owns keeps its order relative to every local id (no global id is formed as an int, so ids
 * need not fit one: the exemption of srec_score_rank).  SREC_LISTED_SCORE and SREC_LISTED_DROP are both resolved INSIDE the
 * pass - no fix-up pass, so the count is exact for the scores the pass forms: with labels[b] = out_idx[b,j] and target[b] =
 * out_val[b,j] of srec_score_select over the same operands, ahead[b] == j.  Whether the label itself could be shown is the
 * CALLER's test (target == -INFINITY, or target < floor[b]): the count does not look at it.
 * bias == NULL is the unbiased case; floor == NULL runs the same kernel instances as a floor of -INFINITY; a descriptor without
 * a list (L == 0) runs instances with the list machinery compiled out - the same scores, the same counts.  Integer atomics
 * only: the output is a pure function of the inputs.  ws: srec_score_ahead_ws() bytes (a token: nothing is kept there).
 * Nonzero and no launch, beyond the descriptor's reasons: labels, target or ahead NULL; labels, target, floor or ahead not
 * aligned to 4 bytes. */
int srec_score_ahead_ws(int B, int V, int d, int C, int L, long* bytes);
int srec_score_ahead(const void* served, const int* labels, const float* target, const float* floor, int* ahead, void* ws,
                     void* stream);

/* ---- ... for M given items per session in ONE pass: where several targets stand among what is served (rank_served_many.hip) --
 * Rest-of-session evaluation (every remaining item of a session is relevant) and "where would these items land?".
 * items [B, M] int32 global ids, row stride ld_items; an entry < 0 is an EMPTY slot; every id appears at most once per row.
 * target [B, M] fp32, row stride ld_items: the items' own served values s' - what srec_score_items returns for them, summed over
 * row shards.  floor [B] or NULL.  1 <= M <= SREC_AHEAD_MAXT.  For a live slot (b, j) with u = items[b,j], t = target[b,j]:
 *   ahead[b,j] = N[b,j] + A[b,j]                                                              (int32 [B, M], contiguous)
 *   N[b,j] = #{ local rows v : (b, v) ELIGIBLE (above), id_lo + v is NOT one of items[b,:], !(s'[b,v] < floor[b]),
 *               s'[b,v] > t  or (s'[b,v] == t and id_lo + v < u) }                                           - the pass
 *   A[b,j] = #{ i != j live : items[b,i] != u, target[b,i] > -INFINITY, !(target[b,i] < floor[b]),
 *               target[b,i] > t or (target[b,i] == t and items[b,i] < u) }            - the targets among themselves
 * An empty slot gives 0.  A is added only with among_targets != 0 (a row shard passes 0: A needs no table and is added once).
 * The session's own targets are left out of the pass BY ID and ordered among themselves by their GIVEN values - the rule of
 * srec_score_ahead for its one label: round-off between the gather kernel's and the pass's summation orders cannot make a
 * target count against itself, two targets never both count as ahead of each other, and the shown targets of a session get
 * pairwise distinct ranks in (value descending, id ascending) order.  N is a sum over disjoint row ranges (row shards add up).
 * With M == 1 the result is srec_score_ahead's, bit for bit.  Duplicate ids in a row are the caller's error: they do not fault,
 * the result for those columns is unspecified; so is a NaN among the target values, for its session (no fault either).  ahead is WRITTEN (zeroed on the stream by the call); integer atomics only: a
 * pure function of the inputs.  A bias, a grouped bias, SREC_LISTED_DROP, a floor and ids beyond int32 are accepted.
 * ws: srec_score_ahead_many_ws() bytes (a token).  Nonzero and no launch, beyond the descriptor's reasons: M outside
 * 1 .. SREC_AHEAD_MAXT; ld_items < M; items, target or ahead NULL; items, target, floor or ahead not aligned to 4 bytes. */
#define SREC_AHEAD_MAXT 64
int srec_score_ahead_many_ws(int B, int V, int d, int C, int L, int M, long* bytes);
int srec_score_ahead_many(const void* served, const int* items, const float* target, long ld_items, int M, const float* floor,
                          int among_targets, int* ahead, void* ws, void* stream);

/* ---- serving and evaluation of ENSEMBLES: the served score over SEVERAL tables in one pass (ensemble.hip) ------------------
 * A probability-averaged ensemble ("soft voting": p(v) = sum_m w_m p_m(v)) is the served score with one table, one width and
 * one column scale PER COMPONENT; log w_m is folded into the member's offsets by the caller:
 *   s[b,v]  = logsumexp_{c<C}( cs[c][v] * <sr[c][b], E[c][v]> + off[c,b] ),  off = off_in if v is in listed[b,:] under
 *             SREC_LISTED_SCORE, else off_ex                                       (C == 1: s = z + off, no exp / log)
 *   s'[b,v] = s[b,v] + bias[group[b] * ld_bias + v]
 * `const void* desc` -> srec_served_multi (include/srec_ens.h, with SREC_ENS_MAXCOMP = 8; a HOST struct of DEVICE pointers,
 * read during the call only).  Per component c < C
 * (arrays of extent SREC_ENS_MAXCOMP; entries >= C are not read): sr[c] [B, d[c]] (row stride ld_sr[c]), E[c] [V, d[c]] (row
 * stride ld_e[c]), cs[c] [V] or NULL (= 1), d[c].  Every other member means exactly what it means in srec_served: off_ex /
 * off_in [C, B] (NULL = 0), listed [B, L] / L / listed_mode, id_lo, B, V, bias / ld_bias / group / G; ELIGIBLE is the rule
 * stated there, unchanged.  Component c's raw dot product is the tile product of the single-table pass over (sr[c], E[c]),
 * to the bit; with C == 1 both entry points return what srec_score_select / srec_score_ahead (floor == NULL) return, to the
 * bit.  For C > 1 the components are folded in index order into a running (max, sum) pair, so the value may differ from
 * srec_served's three-pass mixture in the last bits; a component at -INFINITY contributes nothing, all of them give -INFINITY.
 * Limits: 1 <= C <= SREC_ENS_MAXCOMP; per component those of srec_served: d[c] % 4 == 0, 0 < d[c] <= 1024, sr[c] / E[c]
 * aligned to 16 bytes, ld_sr[c] / ld_e[c] multiples of 4; 0 <= L <= 64; id_lo + V <= INT_MAX (srec_ens_select).  fp32 only;
 * no floor, no noise, no row-sharded session tiles (id_lo serves a table shard as before).
 * srec_ens_select: the contract of srec_score_select without `floor`: out_val [B, K] descending, out_idx [B, K] global ids,
 *   ties towards the lower id, (-INFINITY, -1) once the eligible rows run out (K > V is legal), 1 <= K <= SREC_SELECT_MAXK;
 *   a pure function of the inputs, no atomics.  ws: srec_ens_select_ws() bytes.
 * srec_ens_ahead: the contract of srec_score_ahead without `floor`: ahead[b] = the number of eligible local rows v with
 *   id_lo + v != labels[b] and (s' > target[b], or s' == target[b] and id_lo + v < labels[b]); labels[b] < 0 gives -1; target
 *   is always the caller's; counts of disjoint row ranges add up; with (labels, target) = (out_idx[:, j], out_val[:, j]) of
 *   srec_ens_select over the same operands, ahead[b] == j.  ahead is WRITTEN; integer atomics only.  ws: srec_ens_ahead_ws()
 *   bytes (a token).
 * Both return SREC_BAD_ARG for desc == NULL, then 0 and no launch for B <= 0.  Nonzero and no launch for every reason of
 * srec_served (per component where the member is per component), for C out of range, for a NULL sr[c] or E[c] with c < C,
 * and for the reasons of srec_score_select / srec_score_ahead beyond the descriptor.  The *_ws functions take shapes alone
 * (d_max: the widest component). */
int srec_ens_select_ws(int B, int V, int d_max, int C, int L, int K, long* bytes);
int srec_ens_select(const void* desc, int K, float* out_val, int* out_idx, void* ws, void* stream);
int srec_ens_ahead_ws(int B, int V, int d_max, int C, int L, long* bytes);
int srec_ens_ahead(const void* desc, const int* labels, const float* target, int* ahead, void* ws, void* stream);

/* ---- serving: diversified top-N - greedy MMR re-rank of a pool, and intra-list diversity (diversify.hip) ------------------
 * Per session a pool of M slots; slot i has a row index row[b * M + i] into the row source X (fp32, n_rows rows of d columns,
 * leading dimension ld_x) and a value s[b * M + i].  A slot whose row index is < 0 or >= n_rows is UNFILLED: X is never read
 * for it and it is never picked.
 *   sim(i, j) = <X_i, X_j> / (max(|X_i|, 1e-12) * max(|X_j|, 1e-12))        a zero row: 0 to everything, never NaN
 *   for t = 0 .. K-1:  m_t(i) = s[i] - theta * pen_t(i) over the filled slots not yet picked; pen_0 = 0, and for t >= 1
 *     pen_t(i) = max of sim(i, j) over the slots j picked so far - the raw maximum, not clamped at 0.  The pick is the slot
 *     with the largest m_t, ties to the lower slot.
 * pick [B, K] int32: the slot numbers in pick order, -1 once the filled slots run out.  val [B, K]: s[pick], copied and not
 * recomputed (the pool's own bits), -INFINITY in the tail.  mmr [B, K] (nullable): the winning m_t, -INFINITY in the tail.
 * ild [B] (nullable): 1 - mean_{a<b} sim(pick_a, pick_b) over the filled picks, 0 with fewer than two.
 * theta (the diversity weight) is finite and >= 0; theta == 0 gives m_t = s[i] whatever the rows hold, so equal values come
 * back as the first K filled slots in slot order.  The similarity does not depend on a positive per-row factor (the column
 * scale cs of the scoring calls), so there is no cs argument.
 * One workgroup per session, no atomics, no workspace: a session's result is the same bits in any batch.
 * SREC_BAD_ARG and no launch unless 1 <= K <= M <= SREC_SELECT_MAXK, d % 4 == 0, 0 < d <= 1024, ld_x % 4 == 0, ld_x >= d,
 * X 16-byte aligned, n_rows >= 0, theta finite and >= 0 (not negative, NaN or infinite), X / row / s / pick / val non-null. */
int srec_diversify(const float* X, int ld_x, long n_rows, const int* row, const float* s, int B, int M, int K, int d,
                   float theta, int* pick, float* val, float* mmr, float* ild, void* stream);

/* ---- serving: per-category caps on an ordered pool - "at most caps[c] items of category c in the list" (cap_select.hip) ----
 * Per session an ORDERED pool of P slots: ids[b * P + i] a global item id, s[b * P + i] its value (what srec_score_select /
 * srec_score_select_many_order wrote).  A slot is FILLED iff 0 <= ids < n_items; anything else is an unfilled slot, never
 * dereferenced and never picked.  c_i = category[ids[b * P + i]] (category: int32 [n_items]); c_i < 0 or c_i >= G: the item
 * has no category and is always accepted - caps (int32 [G]) and the counters are never indexed with it.  Otherwise the slot
 * is accepted iff the number of EARLIER filled slots of the session with the same category is < caps[c_i] (which equals
 * "earlier accepted ones < cap": the greedy over a partition matroid, the optimum); caps[c] <= 0: category c is never shown.
 * Duplicate ids in a pool each count.
 * pick [B, K] int32: the slot numbers of the first K accepted slots in slot order, -1 once they run out.  val [B, K]: s[pick]
 * copied bit for bit, -INFINITY in the tail.  kept [B] = min(K, number accepted).  scanned [B]: the pool slots consumed - the
 * index after the K-th accepted slot, or P when fewer than K were accepted; slots at or past it are not part of the result.
 * One workgroup per session, integer logic only, no atomics, no workspace: a session's result is the same bits in any batch.
 * SREC_BAD_ARG and no launch unless 1 <= K <= P <= SREC_CAP_MAXP, 1 <= G <= SREC_CAP_MAXG (64 KB of int32 counters in LDS
 * beside the chunk state), n_items >= 0, every pointer non-null and aligned to 4 bytes.  B <= 0 returns 0. */
#define SREC_CAP_MAXP 4096
#define SREC_CAP_MAXG 16384
int srec_cap_select(const int* ids, const float* s, int B, int P, int K, const int* category, long n_items, const int* caps,
                    int G, int* pick, float* val, int* kept, int* scanned, void* stream);

/* ---- serving: per-session hide / boost lists merged into an ordered pool (personal.hip) -----------------------------------
 * "Never show this user these items, lift those": a sparse list per session instead of a dense [B, V] bias.  If M items of a
 * session change their value, its new top-K is the top-K of (the old top-(K + M) without those items) and (those items with
 * their new values): no catalogue pass, one merge per session.
 * Per session an ORDERED pool of P slots: pool_ids[b * P + i], pool_s[b * P + i] - what srec_score_select /
 * srec_score_select_many_order wrote.  A slot is FILLED iff pool_ids >= 0; unfilled slots may stand anywhere and are skipped;
 * the filled ones are in served order (value descending, id ascending), which the kernel relies on.
 * The list: M slots, items[b * M + j] >= 0 is a FILLED slot (int32 global id; ids are only compared, never used as an index).
 * An id met again in a later slot of the session is ignored: the first slot wins.  t_j = base[b * M + j] + bias[b * M + j],
 * one fp32 add; bias == NULL: every listed item is hidden, t_j = -INFINITY.  base is what srec_score_items returns for the
 * slot.  A listed item is a CANDIDATE iff t_j > -INFINITY (a -INFINITY base - seen, filtered - stays out whatever the bias).
 * A filled pool slot SURVIVES iff its id is in no filled list slot of the session, whatever the list says about it.
 *   hit [B]: the filled pool slots that did not survive.
 *   ids_out / val_out [B, K]: the first K of survivors and candidates by (value descending, id ascending), floats compared as
 *     the select kernels do (-0.0 == +0.0, no NaN); val_out is the survivor's pool_s copied bit for bit, or t_j; the tail is
 *     (-1, -INFINITY).  src [B, K] (may be NULL): i for pool slot i, P + j for list slot j, -1 in the tail.
 *   kept [B]: the filled output slots, min(K, survivors + candidates).
 * With hit[b] <= P - K, or the pool's last slot unfilled, the output is the exact top-K of the adjusted catalogue: anything
 * outside the pool scores at or below its last slot, and K survivors stand at or above that.  P = K + M always suffices.
 * One workgroup per session, no atomics, no workspace: a session's result is the same bits in any batch.
 * SREC_BAD_ARG and no launch unless 1 <= P <= SREC_CAP_MAXP, 1 <= M <= SREC_PERSONAL_MAXM, 1 <= K <= SREC_CAP_MAXP, pool_ids /
 * pool_s / items / base / ids_out / val_out / hit / kept non-null, every given pointer aligned to 4 bytes.  B <= 0 returns 0. */
#define SREC_PERSONAL_MAXM 1024
int srec_personal_merge(const int* pool_ids, const float* pool_s, int B, int P, const int* items, const float* base,
                        const float* bias, int M, int K, int* ids_out, float* val_out, int* src, int* hit, int* kept, void* stream);

/* ---- serving: calibrated slates - the greedy re-rank of a pool towards a target category distribution (calibrate.hip; Steck,
 * "Calibrated Recommendations", RecSys 2018).  The soft counterpart of the caps above; plain arguments, no workspace.
 * Per session a pool of M <= SREC_SELECT_MAXK slots: ids[b * M + i] a global item id and s[b * M + i] its value, as
 * srec_score_select wrote them.  A slot is FILLED iff 0 <= ids < n_items; anything else is never dereferenced and never
 * picked.  c_i = category[ids[b * M + i]] (category: int32 [n_items]); c_i < 0: the item has no category.
 * The target: T <= SREC_CALIB_MAXT pairs (tcat[b * T + j], tw[b * T + j]) of a CATEGORY id (not an item id) and a weight;
 * tcat < 0 or tw <= 0 is an empty pair, duplicates add up; T == 0 (tcat, tw may be NULL): no target.  Category ids are only
 * compared, never used as an index: there is no upper bound on them.
 * P_c = the sum of the weights of category c, S = {c : P_c > 0}, W = sum_{c in S} P_c.  W > 0: p_c = P_c / W; otherwise the
 * session has NO TARGET and its calibration term is 0.
 * After some picks n_c is the number of picks of category c and N the number of picks with ANY category >= 0, in S or not
 * (uncategorised picks count nowhere);
 *   KL(n, N) = sum_{c in S} p_c log(p_c / ((1 - a) n_c / max(N, 1) + a p_c)),   a = smooth in (0, 1) (Steck: 0.01).
 * Greedy, t = 0 .. K-1: for every filled slot i not yet picked let (n', N') be the state with the slot added (unchanged when
 * c_i < 0) and m_t(i) = (1 - w) s_i - w KL(n', N'), w = weight in [0, 1]; the pick is the largest m_t, ties to the LOWER slot.
 * w == 0: m = s_i exactly, the target is not looked at.  s_i == -INFINITY: m = -INFINITY, never NaN (also at w == 1).  No
 * target: KL = 0.  m depends on a slot only through s_i and its category: the calibration term is formed once per distinct
 * category, so two slots with the same s that share a category, or are both outside S, or both uncategorised, get the same
 * bits (and the lower slot wins).
 * pick [B, K] int32: the slot numbers in pick order, -1 once the filled slots run out.  val [B, K]: s[pick] copied bit for
 * bit, -INFINITY in the tail.  obj [B, K] (may be NULL): the winning m_t rounded to fp32, -INFINITY in the tail.  kl [B] (may
 * be NULL): KL of the final picks rounded to fp32, 0 without a target.
 * The sums of the weights, the calibration term and m_t are formed and compared in DOUBLE (weight and smooth are widened): a
 * float64 loop on the host gives the same picks wherever its best two candidates differ by more than double round-off.
 * One workgroup per session, no atomics, no workspace: a session's result is the same bits in any batch.
 * SREC_BAD_ARG and no launch unless 1 <= K <= M <= SREC_SELECT_MAXK, 0 <= T <= SREC_CALIB_MAXT, n_items >= 0, 0 <= weight <= 1,
 * 0 < smooth < 1 (NaN fails both), ids / s / category / pick / val non-null, tcat / tw non-null when T > 0, every pointer
 * aligned to 4 bytes.  B <= 0 returns 0. */
#define SREC_CALIB_MAXT 128
int srec_calibrate(const int* ids, const float* s, int B, int M, int K, const int* category, long n_items, const int* tcat,
                   const float* tw, int T, float weight, float smooth, int* pick, float* val, float* obj, float* kl, void* stream);

/* ---- fused read-out head (headf.hip): msgifsr.py:124-155 (AttnReadout.forward) + :269-273 (fc_sr, F.normalize) for all live
 * orders in ONE launch, a group of SREC_HEAD_SESSIONS sessions per workgroup; replaces the {U, Vq} GEMM / srec_seg_attn_fwd /
 * {s} GEMM / split-K sum / srec_normalize_fwd chain of the grouped head in bf16 mode (d = 128 / 256).  desc: HOST
 * srec_head_desc (srec_hg.h).  srec_head_wfrag: n <= SREC_HEAD_MAXW fp32 matrices W_i [rows_i, cols_i] (HOST arrays of
 * device pointers / ints) -> hi / lo fragment-major bf16 operand copies dst_i [2 rows_i cols_i] of W_i (trans_i = 0) or W_i^T
 * (trans_i = 1), once per optimizer step. */
int srec_head_wfrag(int n, const void* W, const void* dst, const int* rows, const int* cols, const int* trans, void* stream);
int srec_head_fwd(const void* desc, void* stream);
/* per-session half of the head's backward (normalise-backward, d cat product, attention read-out backward); desc: HOST
 * srec_head_bwd_desc (srec_hg.h) */
int srec_head_bwd(const void* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif
