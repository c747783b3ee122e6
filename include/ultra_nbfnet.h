/*
 * ultra_nbfnet.h -- C ABI of the dense layer epilogues around rspmm (libultra_amd.so).
 *
 * These replace the torch op chains of the reference layer on the hot path; operands are plain fp32
 * device pointers, kernels are enqueued on `stream` (hipStream_t as void*), status codes as in
 * ultra_rspmm.h.  Built for the shapes of the shipped ULTRA checkpoints (hidden dim 64); other shapes
 * return ULTRA_ERR_UNSUPPORTED and the host layer keeps using its generic path.
 */
#ifndef ULTRA_NBFNET_H
#define ULTRA_NBFNET_H

#include <stdint.h>

#include "ultra_rspmm.h"    /* ultra_explain_edits (ultra_beam_search_edit_rows_batch) */

#ifdef __cplusplus
extern "C" {
#endif

#define ULTRA_CONV_LAYER_NORM 1
#define ULTRA_CONV_RELU 2
#define ULTRA_CONV_RESIDUAL 4
#define ULTRA_LAYER0_MAX 8      /* ultra_nbf_layer0 only: max aggregate instead of sum (layers.py:206-207) */
#define ULTRA_LAYER0_ONLY_FILL 16   /* ... only the constant rows (they depend on the layer's parameters alone: relation, src_rows,
                                       src_values, weight may be NULL) -- e.g. on a side stream, beside the relation model */
#define ULTRA_LAYER0_SKIP_FILL 32   /* ... only the special rows, into an output the caller has filled with ULTRA_LAYER0_ONLY_FILL */

/*
 * GeneralizedRelationalConv.update (/root/reference/ultra/layers.py:233-240) fused with the residual
 * of the Bellman-Ford loop (/root/reference/ultra/models.py:158-160):
 *     out = [x +] relu( LayerNorm_eps( W . cat[x, agg] + b ) )
 * x, agg, out: (rows, 64) contiguous; weight (64, 128) row-major = linear.weight; bias (64) may be NULL;
 * ln_weight / ln_bias (64) required with ULTRA_CONV_LAYER_NORM.  out may not alias x or agg.
 * `flags`: ULTRA_CONV_LAYER_NORM | ULTRA_CONV_RELU | ULTRA_CONV_RESIDUAL; any other bit is ULTRA_ERR_INVALID (the
 * measurement switch 256 of tools/conv_probe.py is accepted only by a library built with -DULTRA_CONV_DEBUG=1).
 */
int32_t ultra_conv_update(const void *x, const void *agg, const void *weight, const void *bias, const void *ln_weight,
                          const void *ln_bias, void *out, int64_t rows, int32_t input_dim, int32_t output_dim, float eps,
                          int32_t flags, void *stream);

/*
 * Backward of ultra_conv_update for the fine-tuning path (autograd of /root/reference/ultra/layers.py:233-240; in the
 * reference: cat, addmm, native_layer_norm, relu and add nodes).  Nothing but x and agg has to be kept from the forward:
 * the pre-activation is recomputed on the matrix cores.
 *     grad_x, grad_agg (rows, 64); grad_weight (64, 128); grad_bias / grad_ln_weight / grad_ln_bias (64) may be NULL.
 * `flags`: ULTRA_CONV_LAYER_NORM | ULTRA_CONV_RELU | ULTRA_CONV_RESIDUAL; any other bit is ULTRA_ERR_INVALID and nothing
 * is launched or written.  The timing switches 256 / 512 / 1024 (skip one matrix product) and 2048 (clock ticks into the
 * workspace) give wrong gradients and exist only in a library built with -DULTRA_CONV_BWD_DEBUG=1 (tools/conv_bwd_probe.py).
 * workspace: ultra_conv_update_backward_workspace(rows) bytes of device memory (the
 * pre-activation gradient and the per-workgroup partial sums; combined in a fixed order -- no atomics, gradients are
 * reproducible run to run).  Gradients OVERWRITE their destinations.
 */
int64_t ultra_conv_update_backward_workspace(int64_t rows);
int32_t ultra_conv_update_backward(const void *x, const void *agg, const void *grad_out, const void *weight, const void *bias,
                                   const void *ln_weight, const void *ln_bias, void *grad_x, void *grad_agg, void *grad_weight,
                                   void *grad_bias, void *grad_ln_weight, void *grad_ln_bias, void *workspace,
                                   int64_t workspace_bytes, int64_t rows, int32_t input_dim, int32_t output_dim, float eps,
                                   int32_t flags, void *stream);

/*
 * Readout of EntityNBFNet.forward (/root/reference/ultra/models.py:166-170, 202-209):
 *     feature = cat[hidden, query]; score = mlp.2( relu( mlp.0( feature.gather(t_index) ) ) )
 * in the reference's operation order: mlp.0 = one k-ascending fmaf chain per hidden unit over the 64 node features and
 * then the 64 query features, bias added after the chain (the concatenated feature is never materialised: the query half
 * of the chain reads query[sample]); mlp.2 = nn.Linear(128, 1), a GEMV on the reference's CPU path whose association of
 * the 128 products belongs to the host BLAS and is passed in as a PROGRAM (order_dev, at most 640 int32 words on the device;
 * ultra_amd/host_order.py recovers it from the BLAS of the running process):
 *     [n_stage, then one header per stage: L (lanes, power of two <= 16), carry (0/1), (offset_p, groups_p) for p < L,
 *      then the element area]: lane p's elements start at word offset_p (a multiple of 4) and fill groups_p groups of
 *     eight, the last one padded with the element 128, which multiplies zeros
 *     lane p: v = (p == 0 && carry) ? previous stage's result : 0;  v = fma(hid[k], w2[k], v) for its k in order
 *             (an element written k + 256: v = v + fl(hid[k] * w2[k]), for host code that does not fuse);
 *     fold: v[p] += v[p + L/2]; v[p] += v[p + L/4]; ...; stage result v[0];  score = last result + b2.
 * order_dev == NULL: one chain, k ascending.  Every product of every stage must appear exactly once.
 * hidden (batch, num_node, 64) contiguous; query (batch, 64); t_index (batch, n_cand) int64 node ids or NULL for
 * all-tail (n_cand == num_node, identity); w1 = mlp.0.weight (128, 128) row-major, b1 = mlp.0.bias (128);
 * w2 = mlp.2.weight (128); b2 = mlp.2.bias (1); score (batch, n_cand).
 */
int32_t ultra_readout(const void *hidden, const int64_t *t_index, const void *w1, const void *query, const void *b1,
                      const void *w2, const void *b2, const int32_t *order_dev, int64_t order_len, void *score, int64_t batch,
                      int64_t num_node, int64_t n_cand, int32_t hidden_dim, int32_t feature_dim, void *stream);

/*
 * Batch prologue of EntityNBFNet.forward (/root/reference/ultra/models.py:190-197 with
 * /root/reference/ultra/base_nbfnet.py:79-86) in one pass over triples = (batch, n_cand, 3) int64 [h, t, r]:
 *   side[b] = 1 if row b keeps its head fixed (tail candidates), 0 if it keeps its tail fixed (head candidates, turned
 *             into a tail query with the inverse relation r + num_direct_rel);
 *   h0[b], r0[b] = source node / query relation of row b after that conversion;
 *   valid[b] = 1 iff row b shares its source node and its relation (the reference's two asserts), else 0  (int32 [batch]).
 * rel_first (optional, int64 [batch]): row b's relation as given, triples[b, 0, 2] -- the relation model's query
 * (/root/reference/ultra/models.py:20).  One workgroup per row: no scratch, any number of prologues may run concurrently.
 * ultra_readout_batch is ultra_readout reading the candidate node straight from `triples` (column 1 or 0 by side[b]).
 */
int32_t ultra_batch_prologue(const int64_t *triples, int64_t batch, int64_t n_cand, int64_t num_direct_rel, int64_t *h0,
                             int64_t *r0, int32_t *side, int32_t *valid, int64_t *rel_first, void *stream);
/* ultra_batch_prologue with one more output for the training step (rows of a few hundred candidates): cand (batch, n_cand)
 * int64 = the candidate nodes of the converted rows, new_t_index of /root/reference/ultra/base_nbfnet.py:84 (the tail where
 * side[b] = 1, the head otherwise).  cand may be NULL. */
int32_t ultra_batch_prologue_rows(const int64_t *triples, int64_t batch, int64_t n_cand, int64_t num_direct_rel, int64_t *h0,
                                  int64_t *r0, int32_t *side, int32_t *valid, int64_t *rel_first, int64_t *cand, void *stream);
int32_t ultra_readout_batch(const void *hidden, const int64_t *triples, const int32_t *side, const void *w1, const void *query,
                            const void *b1, const void *w2, const void *b2, const int32_t *order_dev, int64_t order_len,
                            void *score, int64_t batch, int64_t num_node, int64_t n_cand, int32_t hidden_dim,
                            int32_t feature_dim, void *stream);

/*
 * The NBFNet boundary condition (/root/reference/ultra/models.py:59-66, 135-141): out (batch, num_node, dim) fp32,
 * out[b, n, :] = values[b, :] if n == rows[b] else 0; values (batch, dim) or NULL for all-ones (RelNBFNet's query).
 * One pass, no memset (hipGraph friendly).  dim a multiple of 4.
 */
int32_t ultra_onehot_rows(void *out, const int64_t *rows, const void *values, int64_t batch, int64_t num_node, int64_t dim,
                          void *stream);

/*
 * Dynamic edge dropout of the training step (/root/reference/ultra/base_nbfnet.py:54-77) as a 0/1 vector instead of a
 * filtered copy of the graph: keep[e] = 0 where edge e equals one of the listed (easy) edges, else 1.  Edges are compared
 * through the mixed-radix key of the reference's edge_match (tasks.py:7-39): key = (head * num_node + tail) * num_rel +
 * type, or head * num_node + tail when type == NULL (`remove_one_hop`).  easy_key_sorted: the n_easy <= 8192 keys of the
 * edges to drop, ascending (duplicates allowed).  keep: (num_edge) fp32.
 */
int32_t ultra_edge_keep_mask(const int64_t *head, const int64_t *tail, const int64_t *type, int64_t num_edge,
                             const int64_t *easy_key_sorted, int64_t n_easy, int64_t num_node, int64_t num_rel, void *keep,
                             void *stream);
/*
 * The same vector straight from the batch's triples (base_nbfnet.py:57-59 builds the list: every (h, t, r) of the batch and
 * its inverse (t, h, r + inverse_offset), inverse_offset = num_relations / 2): h, t, r point at the first of n_triple <= 4096
 * int64 ids each, `stride` elements apart (3 for the columns of a contiguous (batch, n, 3) tensor, 1 for separate vectors).
 * Every workgroup hashes the 2 n_triple keys into a table in LDS and looks each of its edges up: no list, no sort.
 * type == NULL / r == NULL (`remove_one_hop`): keys of (head, tail) alone.  Same keys, same result as ultra_edge_keep_mask.
 */
int32_t ultra_easy_edge_keep(const int64_t *head, const int64_t *tail, const int64_t *type, int64_t num_edge, const int64_t *h,
                             const int64_t *t, const int64_t *r, int64_t n_triple, int64_t stride, int64_t num_node,
                             int64_t num_rel, int64_t inverse_offset, void *keep, void *stream);
/*
 * One keep ROW per sample (leave-one-out verification of stated facts): keep[s, e] = 0 where edge e is triple s -- (h_s, t_s,
 * r_s) -- or its inverse (t_s, h_s, r_s + inverse_offset), else 1: the easy edges of base_nbfnet.py:57-59 for the single triple
 * s, where ultra_easy_edge_keep marks their union over the batch.  Same operands and keys as ultra_easy_edge_keep (type == NULL
 * / r == NULL: `remove_one_hop`, keys of (head, tail) alone, both directions).  keep: (n_sample, keep_stride) fp32, keep_stride
 * >= num_edge; every element [s, 0:num_edge) is written and the padding of a row is left alone.  All duplicates of an edge
 * go; a triple that is not in the graph gives a row of ones.  One launch: the 2 n_sample keys are staged in LDS and every thread
 * compares its edge, loaded once, with all of them -- no atomics, no memset, no allocation, no host synchronisation, so the call
 * records into a hipGraph (the rows feed ultra_rspmm_forward_masked_samples).  n_sample > 1024: ULTRA_ERR_UNSUPPORTED;
 * keep_stride < num_edge or a negative size: ULTRA_ERR_INVALID -- both decided before any pointer is looked at.  n_sample == 0 or
 * num_edge == 0: ULTRA_OK, nothing launched.
 */
int32_t ultra_leave_one_out_keep(const int64_t *head, const int64_t *tail, const int64_t *type, int64_t num_edge, const int64_t *h,
                                 const int64_t *t, const int64_t *r, int64_t n_sample, int64_t stride, int64_t num_node,
                                 int64_t num_rel, int64_t inverse_offset, void *keep, int64_t keep_stride, void *stream);
/*
 * ultra_easy_edge_keep for batches of ANY size (pre-training: 64 x 513 triples): the same operands and the same keep vector,
 * the 2 n_triple keys hashed into an open-addressing table in global memory instead of LDS.  `workspace` holds the table:
 * at least ultra_easy_edge_keep_table_workspace(n_triple) bytes of device memory (a power of two of >= 2 slots per key, 8 B
 * each; -1 for a negative n_triple), 16-byte aligned.  Enqueues three kernels on `stream` (clear, insert, probe); no memset, no
 * allocation, no host synchronisation, so the call records into a hipGraph.  Keys below zero are skipped, as in
 * ultra_easy_edge_keep.
 */
int64_t ultra_easy_edge_keep_table_workspace(int64_t n_triple);
int32_t ultra_easy_edge_keep_table(const int64_t *head, const int64_t *tail, const int64_t *type, int64_t num_edge,
                                   const int64_t *h, const int64_t *t, const int64_t *r, int64_t n_triple, int64_t stride,
                                   int64_t num_node, int64_t num_rel, int64_t inverse_offset, void *workspace,
                                   int64_t workspace_bytes, void *keep, void *stream);

/*
 * Boundary condition of EntityNBFNet (/root/reference/ultra/models.py:131-141) with the query gather fused:
 *     query_out[b, :] = table[b, pick[b], :]            (query = relation_representations[arange(batch), r_index])
 *     out[b, n, :]    = query_out[b, :] if n == rows[b] else 0
 * table (batch, table_rows, dim) contiguous fp32; rows, pick int64 [batch]; dim a multiple of 4.
 * out may be NULL: then only query_out (and qbias_out) are produced and the boundary stays in closed form for
 * ultra_rspmm_forward_point / ultra_nbf_layer0.
 * Optionally (w1, b1, qbias_out all non-NULL) the same launch also emits the readout's per-sample bias
 *     qbias_out[b, f] = b1[f] + sum_k w1[f, dim + k] * query_out[b, k]      w1 (2 dim, 2 dim) = mlp.0.weight, f < 2 dim
 * (a per-sample folding of the readout's query half; the readout kernels of ABI 4 run the chain through the query
 * themselves and no longer take it).
 */
int32_t ultra_query_boundary(void *out, void *query_out, const int64_t *rows, const void *table, const int64_t *pick,
                             int64_t batch, int64_t num_node, int64_t table_rows, int64_t dim, const void *w1, const void *b1,
                             void *qbias_out, void *stream);

/*
 * The relation_projection MLPs of all entity layers (/root/reference/ultra/layers.py:80, applied to the relation
 * representations set by /root/reference/ultra/models.py:184-185) in one launch:
 *     out[l, r, :] = w2[l] . relu(w0[l] . x[r, :] + b0[l]) + b2[l]
 * x (rows, 64); w0, w2 (n_layer, 64, 64) = the stacked nn.Linear weights [out][in]; b0, b2 (n_layer, 64);
 * out (n_layer, rows, 64).  dim must be 64.
 */
int32_t ultra_relation_projection(const void *x, const void *w0, const void *b0, const void *w2, const void *b2, void *out,
                                  int64_t rows, int32_t n_layer, int32_t dim, void *stream);

/*
 * The same products with every layer's parameters where they live (n_layer host arrays of device pointers: w0[l], w2[l] (64, 64)
 * row-major [out][in]; b0[l], b2[l] (64)) -- the training step, whose parameters change every step, needs no stacked copies.
 */
int32_t ultra_relation_projection_layers(const void *x, const void *const *w0, const void *const *b0, const void *const *w2,
                                         const void *const *b2, void *out, int64_t rows, int32_t n_layer, int32_t dim, void *stream);

/*
 * Backward of ultra_relation_projection_layers for all layers in three launches (csrc/relproj_bwd.hip):
 *     grad_x (rows, 64) = sum_l ((grad_out[l] W2_l) * [h_l > 0]) W0_l,      h_l = relu(x W0_l^T + b0_l) recomputed
 *     grad_w2[l] = grad_out[l]^T h_l,  grad_b2[l] = column sums of grad_out[l],  grad_w0[l] = gh_l^T x,  grad_b0[l] = column sums of gh_l
 * grad_out: n_layer device pointers to (rows, 64) fp32; grad_w0 / grad_w2 stacked (n_layer, 64, 64), grad_b0 / grad_b2 (n_layer, 64),
 * all written in full.  workspace: ultra_relation_projection_backward_workspace(rows, n_layer) bytes.  dim == 64, n_layer <= 8.
 * Fixed summation order (no atomics).
 */
int64_t ultra_relation_projection_backward_workspace(int64_t rows, int32_t n_layer);
int32_t ultra_relation_projection_backward(const void *x, const void *const *w0, const void *const *b0, const void *const *w2,
                                           const void *const *grad_out, void *grad_x, void *grad_w0, void *grad_b0, void *grad_w2,
                                           void *grad_b2, void *workspace, int64_t workspace_bytes, int64_t rows, int32_t n_layer,
                                           int32_t dim, void *stream);

/*
 * Filtered ranking without the (batch, N) mask (/root/reference/ultra/tasks.py:94-141):
 *     rank[q] = 1 + #{t : t not in known(q) and score[q, pos[q]] <= score[q, t]}
 *     num_negative[q] = n_cand - |known(q)|
 * known(q) = known_index[known_ptr[q] : known_ptr[q + 1]]: the de-duplicated ids of the query's known true
 * answers INCLUDING pos[q] (strict_negative_mask zeroes both, tasks.py:108-111).  score (batch, n_cand) fp32,
 * everything else int64, all device pointers.  Ties count against the positive exactly like tasks.py:137.
 */
int32_t ultra_filtered_rank(const void *score, const int64_t *pos_index, const int64_t *known_ptr,
                            const int64_t *known_index, int64_t batch, int64_t n_cand, int64_t *rank_out,
                            int64_t *num_negative_out, void *stream);
/* ... over the LIVE ids of rows of n_cand slots: the live-count rules of ultra_filtered_topk_live.  Only
 * ids below *n_live are counted, num_negative_out[q] = *n_live - |known(q)|; pos_index and the known ids are live.  NULL
 * n_live: ULTRA_ERR_INVALID. */
int32_t ultra_filtered_rank_live(const void *score, const int64_t *pos_index, const int64_t *known_ptr,
                                 const int64_t *known_index, int64_t batch, int64_t n_cand, int64_t *rank_out,
                                 int64_t *num_negative_out, const int64_t *n_live, void *stream);
/* ... over the ids that are ALIVE: the rules of ultra_filtered_topk_alive.  A retired t is skipped,
 * num_negative_out[q] = live - retired - |known(q)|; pos_index and the known ids are alive.  n_live may be NULL (every slot is
 * below the bound); NULL retired_bits or n_retired: ULTRA_ERR_INVALID.  rank_out is zeroed by a kernel, never a memset node. */
int32_t ultra_filtered_rank_alive(const void *score, const int64_t *pos_index, const int64_t *known_ptr,
                                  const int64_t *known_index, int64_t batch, int64_t n_cand, int64_t *rank_out,
                                  int64_t *num_negative_out, const int64_t *n_live, const uint32_t *retired_bits,
                                  const int64_t *n_retired, void *stream);

/*
 * Strict negative sampling (/root/reference/ultra/tasks.py:42-76, strict = True) for n_query positives, n_draw negatives each,
 * without the (batch, N) masks of tasks.py:94-130 and without the host round trip of nonzero():
 *     out[q, d] = the floor(rand[q, d] * count[q])-th entity id, ascending, that is neither a known answer of query q nor its
 *                 positive;   count[q] = num_node - |known(q) u {positive[q]}|            (= candidate[index] of tasks.py:57-61)
 * known(q) is the slice of sorted_keys with (anchor[q] * num_relation + relation[q]) * num_node <= key < ... + num_node, where
 * sorted_keys holds the graph's DISTINCT (anchor, relation, answer) triples as ascending int64 keys
 * (anchor * num_relation + relation) * num_node + answer -- built once per graph by the caller (tails of (head, relation) for the
 * tail half of a batch, heads of (tail, relation) for the head half).  rand: fp32 uniform draws in [0, 1), the caller's
 * (torch.rand in the reference's order, so the sampled ids are the reference's).  All device pointers; ids int64.
 */
int32_t ultra_strict_negatives(const int64_t *sorted_keys_dev, int64_t n_key, const int64_t *anchor_dev, const int64_t *relation_dev,
                               const int64_t *positive_dev, const void *rand_dev, int64_t n_query, int64_t n_draw, int64_t num_node,
                               int64_t num_relation, int64_t *out_dev, void *stream);

/*
 * The fine-tuning step's loss and its gradient in one launch (/root/reference/script/run.py:66-77):
 *     target = [1, 0, ..., 0];  l = binary_cross_entropy_with_logits(pred, target, reduction = none)
 *     w[:, 0] = 1;  w[:, 1:] = softmax(pred[:, 1:] / temperature)  (temperature > 0; a constant, as under run.py's no_grad)
 *                              or uniform_weight (= 1 / num_negative; temperature == 0)
 *     loss = mean_b( sum_i l w / sum_i w );   grad = d loss / d pred
 * pred, grad (rows, n) fp32 row-major; loss one fp32.  rows <= 4096, n >= 2.  Sums run in a fixed order (reproducible).
 */
int32_t ultra_ranking_loss(const void *pred, int64_t rows, int64_t n, float temperature, float uniform_weight, void *loss,
                           void *grad, void *stream);

/*
 * The readout of a training step on the candidates' rows (/root/reference/ultra/models.py:202-207: score = mlp(cat[hidden,
 * query]), mlp = Linear(128, 128), ReLU, Linear(128, 1)) and its backward -- one launch forward, two backward:
 *     h = relu([hid[b, j] ; query[b]] w1^T + b1)          score[b, j] = h . w2 + b2
 * hid (batch, n, 64), query (batch, 64), w1 (128, 128) = mlp.0.weight, b1 (128), w2 (128) = mlp.2.weight, b2 (1); all fp32.
 * forward writes h (batch * n, 128) for the backward and score (batch, n).  backward takes grad_score (batch, n) and writes
 * grad_hid (batch, n, 64), grad_query (batch, 64), grad_w1 (128, 128), grad_b1 (128), grad_w2 (128), grad_b2 (1); work: scratch of
 * ultra_readout_train_backward_workspace(batch, n) bytes.  Every sum has a fixed order (reproducible run to run).
 */
int32_t ultra_readout_train_forward(const void *hid, const void *query, const void *w1, const void *b1, const void *w2,
                                    const void *b2, void *h, void *score, int64_t batch, int64_t n, void *stream);
int64_t ultra_readout_train_backward_workspace(int64_t batch, int64_t n);
int32_t ultra_readout_train_backward(const void *grad_score, const void *h, const void *hid, const void *query, const void *w1,
                                     const void *w2, void *grad_hid, void *grad_query, void *grad_w1, void *grad_b1, void *grad_w2,
                                     void *grad_b2, void *work, int64_t work_bytes, int64_t batch, int64_t n, void *stream);

/*
 * Relation graph of a knowledge graph (/root/reference/ultra/tasks.py:144-199) on the GPU, as bit matrices.
 *   edge_index (2, num_edge) int64 [head; tail], edge_type (num_edge) int64 -- inverse edges already included;
 *   W = (num_relation + 31) / 32 words per bit row.
 * ultra_relation_graph_bits:  hbits / tbits (num_node * W words, ZEROED by the caller) receive, per entity, the set of
 *   relations it is head / tail of; adj (4 * num_relation * W words, zeroed) the four adjacency bit matrices
 *   [hh | tt | ht | th] (row = r1, bit = r2; tasks.py:186-189); row_counts (4 * num_relation int64) the edges per (type, row).
 * ultra_relation_graph_emit:  with row_offsets = the exclusive prefix sum of row_counts (type-major, row-minor) and
 *   total_edges their sum, writes the relation graph's edge_index (2, total_edges) / edge_type (total_edges) in the
 *   reference's order (hh, tt, ht, th blocks, each sorted by (row, col)).
 * ultra_relation_graph_dense_adjacency:  the same matrices as the byte adjacency of the reference-order layer kernel
 *   (ultra_nbf_dense_layer with ULTRA_LAYER_REFERENCE_ORDER): a_ex_out = ceil(R/16)^2 * 1024 bytes, layout
 *   [row tile 16][col chunk 16][lane = row % 16 + 16 type][col % 16] -- plan format straight from the device.
 */
int32_t ultra_relation_graph_bits(const int64_t *edge_index_dev, const int64_t *edge_type_dev, int64_t num_edge, int64_t num_node,
                                  int64_t num_relation, void *hbits_dev, void *tbits_dev, void *adj_dev, int64_t *row_counts_dev,
                                  void *stream);
int32_t ultra_relation_graph_emit(const void *adj_dev, const int64_t *row_offsets_dev, int64_t num_relation, int64_t total_edges,
                                  int64_t *edge_index_out_dev, int64_t *edge_type_out_dev, void *stream);
int32_t ultra_relation_graph_dense_adjacency(const void *adj_dev, int64_t num_relation, void *a_ex_out_dev, void *stream);
/*
 * ultra_relation_graph_bits_keep:  ultra_relation_graph_bits of the graph without the edges whose keep (num_edge fp32) is 0
 *   (the relation graph of a projection's graph after traversal dropout, ultraquery.py:217-219).
 * ultra_relation_graph_edge_keep:  for the edges (rel_edge_index (2, num_rel_edge), rel_edge_type) of a relation graph,
 *   keep_out[i] = 1 where adj (bits of any graph, e.g. the dropped one) holds the edge, else 0 -- the dropped relation graph as a
 *   0/1 vector over the static one's edges.
 */
int32_t ultra_relation_graph_bits_keep(const int64_t *edge_index_dev, const int64_t *edge_type_dev, const float *keep_dev,
                                       int64_t num_edge, int64_t num_node, int64_t num_relation, void *hbits_dev, void *tbits_dev,
                                       void *adj_dev, int64_t *row_counts_dev, void *stream);
int32_t ultra_relation_graph_edge_keep(const void *adj_dev, int64_t num_relation, const int64_t *rel_edge_index_dev,
                                       const int64_t *rel_edge_type_dev, int64_t num_rel_edge, float *keep_out_dev, void *stream);
/*
 * ultra_relation_graph_add_edges:  the bit sets of ultra_relation_graph_bits kept current while edges are ADDED.  hbits / tbits /
 *   adj hold the state of some edge list (as ultra_relation_graph_bits left it); afterwards they hold the state of that list with
 *   the given edges appended, word for word what ultra_relation_graph_bits computes for the concatenated list, and row_counts is
 *   refreshed for ultra_relation_graph_emit.  Cost: the given edges and the bit sets of their endpoints, not the graph.
 *   Launches, in stream order: a check of every index; the heads' and tails' relation bits; one wave per listed endpoint that
 *   applies the whole pair marking of that entity (a repeated endpoint repeats idempotent ORs); the row counts.
 *   changed (one int32 on the device, written whole by the call): bit 0 (value 1) -- a bit was added to adj; bit 1 (value 2) -- an
 *   index lies outside [0, num_node) / [0, num_relation): no index is dereferenced and hbits / tbits / adj stay as they were.
 *   The index values live on the device and the call neither waits for it nor allocates, so an index out of range is reported
 *   through `changed`; arguments the host can see (NULL pointers, negative sizes, num_node or num_relation <= 0, more than 2^20
 *   relations) answer ULTRA_ERR_INVALID with nothing launched.
 */
int32_t ultra_relation_graph_add_edges(const int64_t *edge_index_dev, const int64_t *edge_type_dev, int64_t num_edge, int64_t num_node,
                                       int64_t num_relation, void *hbits_dev, void *tbits_dev, void *adj_dev, int64_t *row_counts_dev,
                                       int32_t *changed_dev, void *stream);

/*
 * One layer of the path beam search behind BaseNBFNet.visualize (/root/reference/ultra/base_nbfnet.py:173-232), with the
 * reference's semantics under stable sorts and exact top-k keys:
 *   candidates of destination v: (e, b) for every in-edge e of v whose source is not `tail`, ascending edge id, then
 *   beam b < num_beam; value m = dist_in[src(e), b] + edge_grad[e] (one fp32 add); prev_rank = the smallest j with
 *   isclose(m(e, b), m(e, j)) (torch's default isclose); a candidate with the same (src, dst, type, prev_rank) as the one
 *   directly before it is dropped; the top num_beam survivors by value (descending, ties to the earlier candidate, -inf
 *   last) are kept, padded with the last one kept; a destination without candidates gets -inf and (0, 0, 0, 0).
 * Graph: a destination-major CSR whose slots keep ascending edge id within every row -- row_ptr (num_node + 1) int64,
 * csr_src / csr_type / csr_eid (num_edge) int32 -- and hub_rows (num_hub) int64: exactly the rows with more than
 * ULTRA_BEAM_HUB_DEGREE slots (served by a workgroup each).  edge_grad (num_edge) fp32 by edge id; dist_in / dist_out
 * (num_node, num_beam) fp32; back_edge_out (num_node, num_beam, 4) int64 [src, dst, type, prev_rank].  All device pointers;
 * one writer per output row, no atomics.  num_beam outside [1, ULTRA_BEAM_MAX]: ULTRA_ERR_UNSUPPORTED.
 */
#define ULTRA_BEAM_MAX 64
#define ULTRA_BEAM_HUB_DEGREE 256
int32_t ultra_beam_search_layer(const int64_t *row_ptr, const int32_t *csr_src, const int32_t *csr_type, const int32_t *csr_eid,
                                const int64_t *hub_rows, int64_t num_hub, int64_t num_node, int64_t num_edge,
                                const void *edge_grad, const void *dist_in, int64_t tail, int32_t num_beam, void *dist_out,
                                int64_t *back_edge_out, void *stream);

/*
 * ultra_beam_search_layer for num_sample independent searches over one graph: edge_grad (num_sample, num_edge), dist_in /
 * dist_out (num_sample, num_node, num_beam) fp32, back_edge_out (num_sample, num_node, num_beam, 4) int64, all contiguous,
 * and tails (num_sample) int64 ON THE DEVICE -- nothing is read on the host, so a chain of layers costs no
 * synchronisation.  Sample s is exactly ultra_beam_search_layer on slice s with tails[s], bit for bit: the sample is a grid
 * dimension of the same two kernels, so a layer is two launches whatever num_sample is.  A tail is only compared with
 * source ids (never an index): an entry outside [0, num_node) excludes no source; callers validate it where they hold it
 * on the host.  num_sample == 0: ULTRA_OK, nothing launched.  num_beam outside [1, ULTRA_BEAM_MAX]: ULTRA_ERR_UNSUPPORTED;
 * num_sample outside [0, 65535], a NULL operand or an empty graph: ULTRA_ERR_INVALID.
 */
int32_t ultra_beam_search_layer_batch(const int64_t *row_ptr, const int32_t *csr_src, const int32_t *csr_type,
                                      const int32_t *csr_eid, const int64_t *hub_rows, int64_t num_hub, int64_t num_node,
                                      int64_t num_edge, int64_t num_sample, const void *edge_grad, const void *dist_in,
                                      const int64_t *tails, int32_t num_beam, void *dist_out, int64_t *back_edge_out,
                                      void *stream);

/*
 * The beam search on (base graph, delta): called AFTER ultra_beam_search_layer_batch on the base CSR, on the same
 * stream and with the same dist_in / dist_out / back_edge_out, it recomputes every touched destination row of every sample
 * (edits->row_dev; ultra_explain_edits, ultra_rspmm.h) and overwrites it; no other row is written.  The candidate stream of
 * row v is the materialised graph's: the base slots in ascending edge id WITHOUT those whose (src, type) is a dead key of the
 * row (a binary search in the row's key range), then the row's added edges in ascending j; values dist_in[src, b] + grad with
 * grad = edge_grad[s, base edge id] or added_grad[s, j] (added_grad: (num_sample, added_grad_stride) fp32).  A dead slot is
 * skipped like a slot whose source is the sample's tail: it is never "the candidate directly before".  One workgroup of 16 waves
 * per (touched row, sample), the slice-and-merge of the hub kernel with the added edges as the tail of the last slice -- the
 * same scan, merge and write routines as the base launch.  The grid is capacity_rows x num_sample, the live row count is read
 * on the device: no host read.  Arguments as ultra_beam_search_layer_batch; edits == NULL or a NULL array: ULTRA_ERR_INVALID.
 */
int32_t ultra_beam_search_edit_rows_batch(const int64_t *row_ptr, const int32_t *csr_src, const int32_t *csr_type,
                                          const int32_t *csr_eid, int64_t num_node, int64_t num_edge, int64_t num_sample,
                                          const void *edge_grad, const ultra_explain_edits *edits, const void *added_grad,
                                          int64_t added_grad_stride, const void *dist_in, const int64_t *tails,
                                          int32_t num_beam, void *dist_out, int64_t *back_edge_out, void *stream);

/* ---- complex logical queries (UltraQuery) ----
 * ultra_symbolic_traversal: SymbolicTraversal.forward (ultraquery.py:280-298),
 *   t[b, v] = max(0, max{ h[b, u] : edge u -> v of type r_index[b] })   (0 where no such edge)
 * over a CSR keyed by (tail, relation): row_ptr (num_node + 1) int64; csr_src / csr_type (num_edge) int32, the in-edges of
 * every row sorted by relation.  r_index (batch) int64; h, t (batch, num_node) contiguous, fp32 (dtype 0) or fp64 (1).
 * Exact: the same bits as any other order of the max.
 *
 * ultra_answer_ranking: batch_evaluate (query_utils.py:284-325) under the stable descending order (u ahead of v iff
 * p_u > p_v, or p_u == p_v and u < v; NaN above every number).  pred (batch, num_node) fp32 contiguous; keep
 * (num_node) uint8 or NULL (a node with keep 0 scores -inf); answers: per query its easy answers by ascending id, then its hard ones (disjoint), at
 * [ans_ptr[b], ans_ptr[b + 1]); hard_ptr (batch) int64: where query b's hard ranks start in `ranking`; num_easy (batch)
 * int64.  A query with more than ULTRA_RANKING_LDS_ANSWERS answers (rounded up to a power of two P) works in
 * ws + ws_off[b] (4-byte words; 4 P words per such query).  Outputs: answer_ranking (sum of answers) int64, the 0-based
 * unfiltered position of every answer in list order; ranking (sum of hard answers) int64, 1 + #{non-answers ahead}.
 */
#define ULTRA_RANKING_LDS_ANSWERS 2048
int32_t ultra_symbolic_traversal(const int64_t *row_ptr, const int32_t *csr_src, const int32_t *csr_type, int64_t num_node,
                                 const int64_t *r_index, int64_t batch, int32_t dtype, const void *h, void *t, void *stream);
int32_t ultra_symbolic_traversal_keep(const int64_t *row_ptr, const int32_t *csr_src, const int32_t *csr_type,
                                      const float *keep_slot, int64_t num_node, const int64_t *r_index, int64_t batch, int32_t dtype,
                                      const void *h, void *t, void *stream);
int32_t ultra_answer_ranking(const void *pred, const uint8_t *keep, const int64_t *answers, const int64_t *ans_ptr,
                             const int64_t *hard_ptr, const int64_t *num_easy, const int64_t *ws_off, void *ws, int64_t batch,
                             int64_t num_node, int64_t *answer_ranking, int64_t *ranking, void *stream);

/* ---- the symbolic traversal of a CHANGING graph (csrc/traversal_edit_kernels.hip) ----
 * Added and retracted facts (rspmm.GraphDelta) in the TRAVERSAL's direction: the traversal writes t[b, v] for v = edge_index[1],
 * so the edits are keyed by the tail they point into.  Prepared at add() / remove() time into arrays of fixed address:
 *   row_dev       int32 [capacity_rows]      the distinct tails an added OR a removed edge points into, ascending
 *   count_dev     int32 [1]                  the live number of touched tails, read ON THE DEVICE
 *   add_ptr_dev   int32 [capacity_rows + 1]  added edges [ptr[k], ptr[k + 1]) point into row_dev[k]
 *   add_src_dev / add_type_dev   int32 [capacity_edges]  their (source, relation), sorted by (relation, source) within a tail
 *   dead_ptr_dev  int32 [capacity_rows + 1]  dead keys [ptr[k], ptr[k + 1]) belong to row_dev[k]; NULL: no tombstones at all
 *   dead_src_dev / dead_type_dev int32 [capacity_keys]   the DISTINCT dead (source, relation) keys, sorted by (relation, source)
 *                                            within a tail: EVERY base edge source -> tail of that relation is absent
 * ultra_symbolic_traversal_edit_rows is called on the output of ultra_symbolic_traversal (same CSR of the BASE graph, r_index,
 * h).  It OVERWRITES t[b, v] for the touched tails v, and nothing else, with
 *   max(0, max{h[b, u] : live base edge u -> v of type r_index[b]}, max{h[b, u] : added edge u -> v of type r_index[b]})
 * -- ultra_symbolic_traversal on the materialised graph, the same bits (a max has no order).  Tombstones never apply to the added
 * edges.  One wave per (touched tail, sample): the relation's base segment by the base kernel's two binary searches, scanned 64
 * slots a trip and combined by lane shuffles; the relation's dead keys are one sorted range, found by binary search, in which
 * every lane binary-searches its edge's source.  The grid is sized by (capacity_rows, batch) and a wave at or beyond *count_dev
 * ends at once: a launch recorded into a hipGraph serves every later content of the arrays.  No atomics, no allocation, no memset,
 * no host synchronisation.  fp32 (dtype 0) / fp64 (1).  A key is only compared, never used as an index; a touched tail outside
 * [0, num_node) is not written; a source outside [0, num_node) is left out, never dereferenced; ptr values are clamped to their
 * capacity.  A NULL operand, a dtype other than 0 / 1, negative capacities, batch outside [0, 65535] or num_node outside
 * (0, 2^31): ULTRA_ERR_INVALID, decided before any GPU call.  capacity_rows == 0 or batch == 0: ULTRA_OK, nothing launched.
 */
typedef struct {
    const int32_t *row_dev, *count_dev;
    const int32_t *add_ptr_dev, *add_src_dev, *add_type_dev;
    const int32_t *dead_ptr_dev, *dead_src_dev, *dead_type_dev;
    int64_t capacity_rows, capacity_edges, capacity_keys;
} ultra_traversal_edits;
int32_t ultra_symbolic_traversal_edit_rows(const int64_t *row_ptr, const int32_t *csr_src, const int32_t *csr_type,
                                           int64_t num_node, const ultra_traversal_edits *edits, const int64_t *r_index,
                                           int64_t batch, int32_t dtype, const void *h, void *t, void *stream);
/* ultra_symbolic_traversal_edit_rows_owned: the same launch over an overlay of facts ASSUMED per sample.
 *   owner_dev     int32 [capacity_edges]     parallel to add_src_dev: -1 = the edge is live in every sample; s in [0, batch) = in
 *                                            sample s only; any other value = nowhere.  Only compared, never used as an index.
 * Sample b's row is max(0, its live base edges, the added edges whose owner is -1 or b).  The dead keys apply to base edges only:
 * a retracted base fact that one sample assumes again is live for that sample.  EARLY-OUT, a contract: a (touched tail, sample)
 * pair is NOT written where the tail holds no dead key of relation r_index[b] and the relation's added range holds no edge live
 * for b -- the output of ultra_symbolic_traversal stands there.  The wave decides it from one strided pass over the added range,
 * before it reads the base segment.  Everything else -- the launch shape, the device-side count, the clamps, NULL dead_ptr_dev,
 * the argument checks -- is ultra_symbolic_traversal_edit_rows'; a NULL owner_dev is ULTRA_ERR_INVALID. */
int32_t ultra_symbolic_traversal_edit_rows_owned(const int64_t *row_ptr, const int32_t *csr_src, const int32_t *csr_type,
                                                 int64_t num_node, const ultra_traversal_edits *edits, const int32_t *owner_dev,
                                                 const int64_t *r_index, int64_t batch, int32_t dtype, const void *h, void *t,
                                                 void *stream);

/* ---- training UltraQuery ----
 * ultra_symbolic_traversal_keep: ultra_symbolic_traversal on the graph without its dropped edges; keep_slot (num_edge) fp32 in
 *   the CSR's slot order, 0 = absent.
 *
 * ultra_traversal_dropout: UltraQuery.traversal_dropout (ultraquery.py:34-83) as a keep vector over the static edge list.
 *   edge_index (2, num_edge) / edge_type (num_edge) int64; deg_out / deg_in (num_node) int32 degrees of the full graph;
 *   r_index (batch) int64 relations, sym (batch, num_node) fp32 (dtype 0) or fp64 (1) symbolic sets;
 *   inv(r) = r ^ 1 (inverse_rel_plus_one) or r -+ num_relation / 2;
 *     k(e) = #{b : r_b == type(e), sym[b, src(e)] != 0} + #{b : inv(r_b) == type(e), sym[b, dst(e)] != 0}
 *     keep[e] = 0 iff not (deg_out[src] <= 1 or deg_in[dst] <= 1) and ((k > 0 and u1[e] <= q[k]) or (more > 0 and u2[e] <= more))
 *   q (2 batch + 1) fp32, q[k] = 1 - (1 - ratio)^k; u1, u2 (num_edge) fp32 uniforms (u2 may be NULL when more_dropout <= 0);
 *   masks: scratch of 2 * num_relation * ultra_traversal_dropout_mask_words(batch) 32-bit words; keep (num_edge) fp32 out;
 *   k_out (num_edge) int32 out or NULL.  No atomics: the same bits on every run.
 *
 * ultra_query_loss: the query loss of run_query.py:94-114 and d loss / d pred in one launch.  pred, grad (rows, n) fp32,
 *   target (rows, n) uint8 (easy answers).  Positives weigh 1 / num_pos; negatives softmax(pred / temperature) over the
 *   row's negatives (a constant) or 1 / num_neg (temperature 0); loss = mean_b(sum l w / sum w), l = BCE with logits.
 *   work: rows + 1 32-bit words, the last one ZERO on entry (left zero).  Fixed summation order: reproducible.
 */
int64_t ultra_traversal_dropout_mask_words(int64_t batch);
int32_t ultra_traversal_dropout(const int64_t *edge_index, const int64_t *edge_type, int64_t num_edge, int64_t num_node,
                                int64_t num_relation, int32_t inverse_rel_plus_one, const int32_t *deg_out, const int32_t *deg_in,
                                const int64_t *r_index, int64_t batch, int32_t dtype, const void *sym, const float *q,
                                const float *u1, const float *u2, float more_dropout, void *masks, float *keep, int32_t *k_out,
                                void *stream);
int32_t ultra_query_loss(const void *pred, const uint8_t *target, int64_t rows, int64_t n, float temperature, void *work,
                         void *loss, void *grad, void *stream);

/* ---- serving link-prediction queries ----
 * ultra_filtered_topk: the k best candidates of every row of score (batch, n_cand) fp32 contiguous, leaving out the row's
 * known ids: known_index[known_ptr[b] : known_ptr[b + 1]], ascending and distinct within a row (the layout of
 * ultra_filtered_rank; no positive has to be listed); known_ptr == NULL: no filter.  The order is the stable descending sort:
 * score descending, equal scores by ascending id, every NaN above every number (NaNs tie with each other), -0.0 == +0.0.  A
 * filtered candidate is removed, not rescored: a genuine -inf is a candidate like any other, ranked last.
 *   ids_out (batch, k) int64; scores_out (batch, k) fp32, the stored bits of the selected scores (-0.0 stays -0.0, a NaN keeps
 *   its payload); count_out[b] = min(k, n_cand - |known(b)|); slots at or beyond the count hold id -1 and score -inf.
 * A row longer than ULTRA_TOPK_CHUNK is split over workgroups, each leaving at most k survivors in `workspace`
 * (ultra_filtered_topk_workspace(batch, n_cand, k) bytes of device memory, 8-byte aligned; -1 for arguments out of range); a
 * second launch merges any number of partial lists per row.  Exact and reproducible: the same bits on every run.  No
 * allocation, no memset, no host synchronisation: the call records into a hipGraph.
 * k outside [1, ULTRA_TOPK_MAX] or n_cand >= 2^31: ULTRA_ERR_UNSUPPORTED, decided before any pointer is looked at.  NULL score
 * or outputs, n_cand <= 0 or a workspace that is too small: ULTRA_ERR_INVALID, nothing is launched.  batch == 0: ULTRA_OK.
 */
#define ULTRA_TOPK_MAX 256      /* largest k */
#define ULTRA_TOPK_CHUNK 4096   /* candidates one workgroup selects from; a row longer than this is split */
int64_t ultra_filtered_topk_workspace(int64_t batch, int64_t n_cand, int32_t k);
int32_t ultra_filtered_topk(const void *score, const int64_t *known_ptr, const int64_t *known_index, int64_t batch,
                            int64_t n_cand, int32_t k, int64_t *ids_out, void *scores_out, int64_t *count_out, void *workspace,
                            int64_t workspace_bytes, void *stream);
/* ---- a growing graph: selection over the live ids of reserved rows ----
 * The _live twins of ultra_filtered_topk / ultra_filtered_above / ultra_filtered_rank take the arguments of their parents plus
 * n_live, a DEVICE pointer to one int64 with 1 <= *n_live <= n_cand.  n_cand is the number of SLOTS: the row stride of score,
 * the launch shape and the workspace size depend on (batch, n_cand) alone, and *n_live is read by the kernels, so a call recorded
 * into a hipGraph serves every later value.  An id >= *n_live is absent: its slot is never read (it may hold anything, a NaN or
 * +inf included) and it is never counted -- count_out[b] = min(k, *n_live - |known(b)|), size_out and num_negative_out count
 * live ids.  The known ids (and the positives of the rank) must be live.  The value is clamped on the device to [0, n_cand]
 * and never used to index past a row.  The same kernels serve the parents (n_live == NULL inside: every slot is live), whose
 * results keep their bits.  Errors: those of the parent, under the twin's name; a NULL n_live is ULTRA_ERR_INVALID. */
int32_t ultra_filtered_topk_live(const void *score, const int64_t *known_ptr, const int64_t *known_index, int64_t batch,
                                 int64_t n_cand, int32_t k, int64_t *ids_out, void *scores_out, int64_t *count_out,
                                 void *workspace, int64_t workspace_bytes, const int64_t *n_live, void *stream);
/* ---- retired entities: selection over the ids that are ALIVE, not just below a bound ----
 * The _alive entries take the arguments of their _live twins plus retired_bits, a DEVICE bitmap of ceil(n_cand / 32) uint32
 * words (id v is bit v & 31 of word v >> 5), and n_retired, a DEVICE pointer to one int64: the number of set bits below the
 * bound.  n_live may be NULL here: every slot is below the bound.  An id whose bit is set is ABSENT: never a key, a member or
 * a competitor -- whatever its score slot holds (a NaN, +inf) reaches no output.  Bits at ids >= *n_live are ignored.
 * *n_retired is clamped on the device to [0, live] and used only in the counts -- count_out[b] = min(k, live - retired -
 * |known(b)|), num_negative_out[q] = live - retired - |known(q)|; size_out never counts a retired id -- never as an index.  The
 * known ids and the positives of the rank must be alive.  The launch shapes, the workspace and the number of launches depend on
 * (batch, n_cand) alone and both operands are read by the kernels, so a call recorded into a hipGraph serves every later
 * retirement.  No global atomics beyond the rank's own, no memset, no allocation, no host wait.  The same kernels serve the
 * _live twins and the parents (retired_bits == NULL inside), whose results keep their bits.  Errors: those of the parent, under
 * the entry's name; NULL retired_bits or n_retired: ULTRA_ERR_INVALID, nothing is launched. */
int32_t ultra_filtered_topk_alive(const void *score, const int64_t *known_ptr, const int64_t *known_index, int64_t batch,
                                  int64_t n_cand, int32_t k, int64_t *ids_out, void *scores_out, int64_t *count_out,
                                  void *workspace, int64_t workspace_bytes, const int64_t *n_live, const uint32_t *retired_bits,
                                  const int64_t *n_retired, void *stream);

/* ---- compiled execution of complex logical queries ----
 * ultra_query_segment: what a batch of UltraQuery stack machines does between two projection calls, as one launch.  The
 * program arrays are device memory, int32: entry_depth, push_row, pop_row (batch each), op_ptr (batch + 1), ops
 * (op_ptr[batch] words).  stack (batch, 2, num_node) fp32 contiguous: slot d of sample b at ((b * 2 + d) * num_node).
 * Sample b, whose stack holds entry_depth[b] values on entry:
 *   1. push_row[b] >= 0: push row push_row[b] of push_src (push_rows, num_node);
 *   2. ops[op_ptr[b] : op_ptr[b + 1]] in order -- a word e >= 0 pushes the one-hot set of entity e (1.0 at e, 0.0 elsewhere),
 *      -1 replaces the two top values x (below) and y (top) by x AND y, -2 by x OR y, -3 replaces the top x by 1 - x;
 *   3. pop_row[b] >= 0: pop the top into row pop_row[b] of pop_dst (pop_rows, num_node).
 * A sample without work is not touched; only live slots are read and only changed slots that are still live are written.  An
 * op that would overflow or underflow the two slots, and a row outside push_rows / pop_rows, is skipped (the host compiler
 * refuses such programs).  logic 0 product: x * y, (x + y) - x * y; 1 godel: min, max, a NaN in either operand gives NaN;
 * 2 lukasiewicz: max(x + y - 1, 0), min(x + y, 1), NaN propagating -- each operation rounded as torch rounds it, no
 * contraction.  sym_stack / sym_push_src / sym_pop_dst: a second stack that runs the same program (the symbolic sets), or all
 * NULL.  push_src NULL (push_rows 0): nothing is pushed from it; pop_dst alike.
 * No LDS, no atomics, no allocation, no memset, no host synchronisation: the call records into a hipGraph.
 * stack_depth != 2, dtype != 0 (fp32) or num_node >= 2^31: ULTRA_ERR_UNSUPPORTED, decided before any pointer is looked at.
 * NULL program arrays or stack, batch outside [0, 65535], num_node <= 0, logic outside [0, 2], a buffer that disagrees with
 * its row count, symbolic buffers that do not mirror the neural ones: ULTRA_ERR_INVALID, nothing is launched.  batch == 0:
 * ULTRA_OK.
 *
 * ultra_nonzero_lists: per row of x (batch, n) fp32 contiguous the ids v with x[b, v] != 0 (a NaN counts, -0.0 does not: the
 * rule of ultra_traversal_dropout), ascending, at index_out[ptr_out[b] : ptr_out[b + 1]]; ptr_out (batch + 1) int64,
 * ptr_out[0] = 0 -- the layout ultra_filtered_topk and ultra_filtered_rank take.  counts: (batch) int64 of scratch.  Two
 * launches (counts per row; scan and fill), no atomics, no host synchronisation: the same integers on every run.
 * capacity (the ids index_out holds) < batch * n: ULTRA_ERR_INVALID, decided on the host.
 *
 * ultra_nonzero_lists_live: the lists over the LIVE ids of rows of n SLOTS -- the final symbolic sets of a
 * graph served with reserved rows, whose dead slots hold 1.0 after a negation.  The arguments of ultra_nonzero_lists plus n_live,
 * a DEVICE pointer to one int64 (the scalar the ultra_filtered_*_live entries read).  n stays the row stride of x; the launch
 * shape, counts, ptr_out and the capacity rule (capacity >= batch * n) depend on (batch, n) alone and *n_live is read by the
 * kernels, once per workgroup, so a call recorded into a hipGraph serves every later value.  An id >= *n_live is absent: its
 * slot is never loaded (it may hold anything, a NaN included) and it is never counted or listed.  The value is clamped on the
 * device to [0, n] and never used as an index.  The same two kernels serve ultra_nonzero_lists (n_live == NULL inside: every
 * slot is live), whose results keep their bits.  No memset node is recorded: for batch == 0 a one-thread kernel writes
 * ptr_out[0] = 0.  Errors: those of ultra_nonzero_lists, under this name; a NULL n_live is ULTRA_ERR_INVALID, decided before
 * any GPU call.
 *
 * ultra_nonzero_lists_alive: the lists of ultra_nonzero_lists_live with every RETIRED id left out -- the
 * final symbolic sets of a graph that retired entities, whose retired slots hold 1.0 after a negation in the middle of the id
 * range.  The arguments of ultra_nonzero_lists_live plus retired_bits, a DEVICE bitmap of at least ceil(n / 32) 32-bit words:
 * id v is bit v & 31 of word v >> 5 (the words the ultra_filtered_*_alive entries read).  n_live may be NULL here: every slot
 * is below the bound (a graph without reserved rows).  No retired count is taken: the lists do no count arithmetic.  The value
 * in a retired slot may be loaded but reaches neither a count nor a list, whatever it holds; a word none of whose ids is below
 * the clamped live count is not loaded and a bit at an id >= *n_live is never looked at.  The bitmap is read by the kernels at
 * run time and the launch shape depends on (batch, n) alone, so a call recorded into a hipGraph serves every later retirement.
 * The same two kernels (retired_bits == NULL inside: the twin and the parent, whose results keep their bits); no atomics, no
 * memset node (batch == 0: the one-thread kernel), no allocation, no host wait.  Errors: those of ultra_nonzero_lists, under this
 * name; retired_bits == NULL is ULTRA_ERR_INVALID ("ultra_nonzero_lists_alive: retired_bits is NULL"), decided before anything
 * is launched.
 */
int32_t ultra_query_segment(const int32_t *entry_depth, const int32_t *push_row, const int32_t *pop_row, const int32_t *op_ptr,
                            const int32_t *ops, int64_t batch, int64_t num_node, int32_t stack_depth, int32_t dtype,
                            int32_t logic, void *stack, const void *push_src, int64_t push_rows, void *pop_dst,
                            int64_t pop_rows, void *sym_stack, const void *sym_push_src, void *sym_pop_dst, void *stream);
int32_t ultra_nonzero_lists(const void *x, int64_t batch, int64_t n, int64_t *counts, int64_t *ptr_out, int64_t *index_out,
                            int64_t capacity, void *stream);
int32_t ultra_nonzero_lists_live(const void *x, int64_t batch, int64_t n, int64_t *counts, int64_t *ptr_out,
                                 int64_t *index_out, int64_t capacity, const int64_t *n_live, void *stream);
int32_t ultra_nonzero_lists_alive(const void *x, int64_t batch, int64_t n, int64_t *counts, int64_t *ptr_out,
                                  int64_t *index_out, int64_t capacity, const int64_t *n_live,
                                  const uint32_t *retired_bits, void *stream);

/* ---- serving answer sets ----
 * ultra_filtered_above: per row of score (batch, n_cand) fp32 contiguous every candidate above `threshold`, ranked.  id v is a
 * MEMBER of row b iff score[b, v] > threshold as an fp32 comparison: strict, a NaN is never a member, +inf is a member of any
 * threshold, and with threshold -inf everything but -inf and NaN is.  size_out[b] (batch) int64: the members among all n_cand
 * ids, counted BEFORE the filter.  The list of row b: the members not in known(b) (known_ptr / known_index: the layout of
 * ultra_filtered_topk; known_ptr == NULL: no filter), in the stable descending order -- score descending, equal scores by
 * ascending id, -0.0 == +0.0 -- at ids_out[ptr_out[b] : ptr_out[b + 1]] (int64) and scores_out (fp32, the STORED bits of the
 * listed scores: -0.0 stays -0.0; a filtered member is removed, never rescored); ptr_out (batch + 1) int64, ptr_out[0] = 0.
 * ids_out / scores_out hold `capacity` entries each; entries at or beyond ptr_out[batch] are unspecified.
 * Launches: counts per chunk of ULTRA_TOPK_CHUNK candidates; one scan; the survivors' keys sorted per chunk; ceil(log2(chunks))
 * merge levels.  The kernel boundary is the only synchronisation between workgroups, there are no global atomics (LDS atomics
 * only hand out slots before a sort), no allocation, no memset of the workspace (its initial contents do not matter) and no
 * host synchronisation; the number of launches depends on (batch, n_cand) alone, so the call records into a hipGraph.  Exact
 * and reproducible: the same bits on every run.
 * workspace: ultra_filtered_above_workspace(batch, n_cand) bytes of device memory, 8-byte aligned (offsets, counts and two key
 * buffers of batch * n_cand * 8 bytes each); -1 for batch outside [0, 65535] or n_cand outside [0, 2^31).
 * n_cand >= 2^31, a NaN or +inf threshold: ULTRA_ERR_UNSUPPORTED, decided before any pointer is looked at.  NULL score or
 * outputs, n_cand <= 0, batch outside [0, 65535], capacity < batch * n_cand (the rule of ultra_nonzero_lists: no overflow path
 * exists) or a workspace that is too small: ULTRA_ERR_INVALID, nothing is launched.  batch == 0: ULTRA_OK.
 */
int64_t ultra_filtered_above_workspace(int64_t batch, int64_t n_cand);
int32_t ultra_filtered_above(const void *score, const int64_t *known_ptr, const int64_t *known_index, int64_t batch,
                             int64_t n_cand, float threshold, int64_t *ptr_out, int64_t *ids_out, void *scores_out,
                             int64_t capacity, int64_t *size_out, void *workspace, int64_t workspace_bytes, void *stream);
/* ... over the live ids (the rules stated at ultra_filtered_topk_live): the workspace is that of ultra_filtered_above. */
int32_t ultra_filtered_above_live(const void *score, const int64_t *known_ptr, const int64_t *known_index, int64_t batch,
                                  int64_t n_cand, float threshold, int64_t *ptr_out, int64_t *ids_out, void *scores_out,
                                  int64_t capacity, int64_t *size_out, void *workspace, int64_t workspace_bytes,
                                  const int64_t *n_live, void *stream);
/* ... over the ids that are alive (the rules stated at ultra_filtered_topk_alive). */
int32_t ultra_filtered_above_alive(const void *score, const int64_t *known_ptr, const int64_t *known_index, int64_t batch,
                                   int64_t n_cand, float threshold, int64_t *ptr_out, int64_t *ids_out, void *scores_out,
                                   int64_t capacity, int64_t *size_out, void *workspace, int64_t workspace_bytes,
                                   const int64_t *n_live, const uint32_t *retired_bits, const int64_t *n_retired, void *stream);

/* ---- candidate sets: selection AMONG an allow list per row ----
 * The _among entries take the arguments of their parents plus, behind the known lists,
 *   among_span (batch, 2) int64, DEVICE: the candidates of row b are among_index[among_span[b][0] : among_span[b][1]];
 *   among_index int64, DEVICE: ids ascending and distinct within a span (the contract of the known lists).  Spans may be shared
 *     by rows, may overlap and may be empty (an inverted or negative span is empty);
 * and, behind n_cand, among_capacity: a HOST int64 in [1, 2^31), at least the longest span the call may meet.  It alone, with
 * batch, sizes the grids and the workspaces; the spans are read on the device and a span longer than among_capacity is cut to it
 * there: nothing is read past among_index[begin + among_capacity).
 * n_live, retired_bits and n_retired (the operands of the _live and _alive twins) are OPTIONAL operands of the same entry: NULL
 * n_live means every slot is live, NULL retired_bits that nothing is retired; n_retired is taken for symmetry and not read.
 *   An id v of row b's span is ELIGIBLE iff 0 <= v < live and its retired bit is clear, live = *n_live clamped to [0, n_cand],
 *   or n_cand.  An id that is not eligible is ABSENT: its score slot is never loaded and it is never counted, whatever the slot
 *   holds; a negative id or an id >= n_cand is never used as an index.  A list made earlier stays valid after a retirement and
 *   may name ids that only become live later.
 * ultra_filtered_topk_among: the eligible ids not in known(b), in the order of ultra_filtered_topk (score descending, equal
 *   scores by ascending id, NaN on top, -0.0 == +0.0); scores_out the stored bits; padding -1 / -inf.  count_out[b] =
 *   min(k, #{eligible, not known}), COUNTED by the kernels: every chunk of ULTRA_TOPK_CHUNK list positions writes its survivor
 *   count beside its partial list and the merge adds them.  workspace: ultra_filtered_topk_among_workspace(batch,
 *   among_capacity, k) bytes, 8-byte aligned; -1 out of range.  A row whose capacity fits one chunk is finished by the first
 *   launch.
 * ultra_filtered_above_among: members = the eligible ids with score > threshold (strict, fp32); size_out[b] counts them before
 *   the known filter; the list is the members not known, ranked, at ids_out[ptr_out[b] : ptr_out[b + 1]].  capacity >=
 *   batch * among_capacity or ULTRA_ERR_INVALID (no overflow path).  workspace: ultra_filtered_above_among_workspace(batch,
 *   among_capacity) bytes -- the layout of ultra_filtered_above_workspace over rows of among_capacity positions.
 * ultra_filtered_rank_among: rank_out[q] = 1 + #{t eligible, t not in known(q) : score[q, pos[q]] <= score[q, t]};
 *   num_negative_out[q] = #{t eligible, not in known(q)}.  pos[q] is in known(q) by the parent's contract and need not be in
 *   the span.  Both outputs are zeroed by a kernel and added to with integer atomics, one per wave: the rank's own counters.
 * The launch shapes, the workspace sizes and the number of launches depend on (batch, among_capacity) alone; no allocation, no
 * memset, no host wait, no other global atomics: a recorded call serves any later spans, list contents, live count and retired
 * set within the capacity.  Exact and reproducible.
 * Errors, in the parents' order: k outside [1, ULTRA_TOPK_MAX], n_cand >= 2^31, a NaN or +inf threshold: ULTRA_ERR_UNSUPPORTED,
 * decided before any pointer is looked at.  NULL among_span or among_index, among_capacity outside [1, 2^31), NULL score or
 * outputs, n_cand <= 0, a short or misaligned workspace, (above) batch outside [0, 65535] or a short capacity, (rank) NULL
 * pos_index or known_ptr: ULTRA_ERR_INVALID, nothing is launched.  batch == 0: ULTRA_OK. */
int64_t ultra_filtered_topk_among_workspace(int64_t batch, int64_t among_capacity, int32_t k);
int32_t ultra_filtered_topk_among(const void *score, const int64_t *known_ptr, const int64_t *known_index,
                                  const int64_t *among_span, const int64_t *among_index, int64_t batch, int64_t n_cand,
                                  int64_t among_capacity, int32_t k, int64_t *ids_out, void *scores_out, int64_t *count_out,
                                  void *workspace, int64_t workspace_bytes, const int64_t *n_live, const uint32_t *retired_bits,
                                  const int64_t *n_retired, void *stream);
int64_t ultra_filtered_above_among_workspace(int64_t batch, int64_t among_capacity);
int32_t ultra_filtered_above_among(const void *score, const int64_t *known_ptr, const int64_t *known_index,
                                   const int64_t *among_span, const int64_t *among_index, int64_t batch, int64_t n_cand,
                                   int64_t among_capacity, float threshold, int64_t *ptr_out, int64_t *ids_out, void *scores_out,
                                   int64_t capacity, int64_t *size_out, void *workspace, int64_t workspace_bytes,
                                   const int64_t *n_live, const uint32_t *retired_bits, const int64_t *n_retired, void *stream);
int32_t ultra_filtered_rank_among(const void *score, const int64_t *pos_index, const int64_t *known_ptr,
                                  const int64_t *known_index, const int64_t *among_span, const int64_t *among_index, int64_t batch,
                                  int64_t n_cand, int64_t among_capacity, int64_t *rank_out, int64_t *num_negative_out,
                                  const int64_t *n_live, const uint32_t *retired_bits, const int64_t *n_retired, void *stream);

/*
 * The best k (query, id, score) records over MANY queries: ultra_topk_pairs_merge folds the row-wise
 * answers of one batch into the running list of a whole call, in place.  All operands on the DEVICE:
 *   ids (batch, k_row) int64 and scores (batch, k_row) fp32, contiguous, as any ultra_filtered_topk* entry writes them: a slot
 *     with id < 0 is ABSENT; a slot with id >= 0 and score -inf is a genuine candidate.
 *   query_base (one int64): row b is query *query_base + b of the call.
 *   n_rows (one int64, or NULL: batch): read at run time and clamped to [0, batch]; rows at and beyond it are never loaded.
 *   min_score (one fp32, or NULL): a slot is a MEMBER iff score > *min_score as an fp32 comparison -- strict, a NaN is never
 *     a member (the rule of ultra_filtered_above).  NULL: every present slot is a member, NaNs included.  The rule is applied
 *     to the records of the running list as well as to the batch's.
 *   best_query (k) int64, best_id (k) int64, best_score (k) fp32, best_count (one int64): the running list.  On entry its first
 *     *best_count records (clamped to [0, k]) are present and nothing beyond them is read; on return it holds the first
 *     m = min(k, #members) members of [running list ; row 0 ; row 1 ; ...] in the order below, slots [m, k) hold -1 / -1 / -inf and
 *     *best_count = m.  best_score holds STORED bits (-0.0 and NaN payloads survive).  The running list must not overlap ids or
 *     scores.
 * Order: score descending, then query ascending, then id ascending; every NaN above every number (NaNs tie), -0.0 == +0.0 --
 * the stable descending torch.sort of the call's row lists laid end to end in query order.  The CALLER guarantees
 *   (1) every query of the batch (*query_base + b) is larger than every query in the running list, and
 *   (2) rows ascend within the batch (they do: row b is query *query_base + b), each row in the (score, id) order its
 *       selection wrote;
 * the position in [running list ; rows] then breaks every tie of scores the way (query, id) does, and the kernel ranks by
 * (score, position) alone.
 * One workgroup, one launch; no allocation, no memset, no global atomics, no host wait: a recorded call reads query_base,
 * n_rows, min_score and the count when it is replayed.  Exact and reproducible.
 * k or k_row outside [1, ULTRA_TOPK_MAX] or batch outside [0, 65535]: ULTRA_ERR_UNSUPPORTED; a NULL ids, scores, query_base or
 * running-list pointer: ULTRA_ERR_INVALID; both decided before any pointer is looked at.  batch == 0: ULTRA_OK, nothing is
 * launched (the running list is left as it is). */
int32_t ultra_topk_pairs_merge(const int64_t *ids, const void *scores, int64_t batch, int32_t k_row, const int64_t *query_base,
                               const int64_t *n_rows, const float *min_score, int64_t *best_query, int64_t *best_id,
                               void *best_score, int64_t *best_count, int32_t k, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ULTRA_NBFNET_H */
