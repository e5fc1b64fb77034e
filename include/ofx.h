/*
 * ofx.h -- C ABI of libofx.so: the MI355X (gfx950) kernels behind OctFusion's
 * denoising hot path.
 *
 * The reference (octree-nn/octfusion) has no FFI of its own: its boundary is
 * Python nn.Module forward() calls that bottom out in torch ops.  This header
 * is the C-ABI drop-in point *under* those modules: every entry point names the
 * reference code it replaces (paths relative to the reference tree).  All
 * pointers are DEVICE pointers unless the name ends in _host; `stream` is a
 * hipStream_t passed as void*.  Every function returns 0 (OFX_OK) or a
 * negative OFX_E* code; nothing throws, nothing allocates device memory,
 * nothing synchronises (safe under hipGraph capture) unless stated.
 *
 * Layouts: features are row-major fp32 [rows, C] with an explicit leading
 * dimension (floats); octree keys int64; children / indices int32.
 */
#ifndef OFX_H_
#define OFX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFX_OK 0
#define OFX_EINVAL (-1)   /* bad argument (shape / alignment / null)          */
#define OFX_ELAUNCH (-2)  /* HIP launch error (hipGetLastError != success)    */
#define OFX_ENODEV (-3)   /* no gfx950 device visible                         */

#define OFX_ACT_NONE 0
#define OFX_ACT_SILU 1
#define OFX_ACT_GELU 2

#define OFX_MAX_DEPTH 16

int ofx_version(void);
const char* ofx_status_string(int status);
/* 0 when a HIP device is present and is gfx950; OFX_ENODEV otherwise. */
int ofx_device_check(void);
/* sha256 (16 hex digits) of every source, header and compile flag this library was built from
 * (octfusion_amd/build.py); the Python binding refuses a library whose hash differs from the tree. */
const char* ofx_build_hash(void);

/* ------------------------------------------------------------------ fp16x3 range guard (precision 3, the default)
 * Operands travel as fp16 hi + lo pairs (22 significand bits).  What that covers and what it does not:
 *  - WEIGHTS are scaled at pack time by a per-tensor power of two so that max|w| lands in [2^14, 2^15) (the kernels
 *    multiply the accumulators by the inverse in the epilogue FMA that adds the bias anyway -- exact, free): every
 *    weight within 2^-18 of the tensor's largest keeps 22 bits, smaller ones an ABSOLUTE error of 2^-40 max|w| --
 *    fp32-class against the output whatever the tensor's own magnitude (a near-zero-initialised projection that
 *    learned 1e-4-scale weights is as exact as an O(1) one);
 *  - ACTIVATIONS are not scaled.  Below |x| ~ 2^-3 the lo half is a denormal fp16: an absolute error floor of
 *    2^-25 ~ 3e-8 per operand (relative 2^-22 above it).  Normalised activations (every GraphConv input that comes
 *    from a GroupNorm) are O(1): there the floor is fp32's own.  Beyond +-65504 an operand does NOT saturate: its
 *    halves become +-Inf and every product it enters is NaN, so an un-normalised operand outside the range (network
 *    inputs, pool / unpool outputs, the residual stream into the 1x1 skip convolutions) makes the result loudly
 *    non-finite instead of plausibly wrong.  words[0] += the operands ofx_planes_split found outside the range
 *    (exact count, diagnostics).  The caller checks finiteness of a stage's result and the word once per batch of
 *    launches (octfusion_amd.ops.raise_on_range_error) and re-runs in bf16x3 (precision 0: fp32's exponent range,
 *    16 significand bits).
 *  - GRADIENTS ride in the activation slot of every data-gradient contraction (ofx_graphconv_bwd_data,
 *    ofx_gridconv_bwd_data, ofx_gemm_f32 on dy) and are NOT O(1): the gradient of an MSE over 1e5..1e7 elements starts
 *    at 2 / numel, where the 3e-8 floor above is the whole value (measured: DESIGN.md section 4.3).  These entry
 *    points therefore expect dy normalised by a power of two so that max|dy| lies in [2^7, 2^8) -- 2^8 of headroom
 *    below 65504 for the weighted segment sums of the reverse graph -- and the caller multiplies dx by the inverse:
 *    octfusion_amd.ops.grad_pow2 (device-side amax -> frexp -> ldexp, no host synchronisation), applied by
 *    ops.graphconv_backward, backward.gridconv_backward, ops.linear_backward and ops.gemm_grad.  Exact both ways, so
 *    dx stays homogeneous in dy.  The weight-gradient contractions (ofx_*_bwd_weight, ofx_gemm_tn_f32) run on bf16
 *    pairs or exact fp32 (fp32's exponent range) and take dy as it is.
 * ofx_set_range_words: device pointer to >= 4 zeroed uint32 on the CURRENT device (NULL: counting off).  Sticky. */
int ofx_set_range_words(uint32_t* words);

/* Measurement aid (csrc/ofx_probe.hip; not on the operator path): the rate the matrix pipe SUSTAINS on the current
 * device with realistic fp16 hi / lo operand pairs from LDS and no memory traffic -- ~1.45 PFLOP/s at ~1.55 GHz on MI355X
 * against the 2.5 PFLOP/s data-sheet peak, which needs constant operands (power limit).  One launch of `steps`
 * 24-MFMA steps per wave, 8 waves per block, `blocks` blocks (0: one per compute unit); the caller times it.
 * flops = blocks * 8 * steps * 24 * 32768; ticks[0] = shader clocks block 0 spent in the loop. */
int ofx_probe_mfma_sustained(int steps, int blocks, float* sink, unsigned long long* ticks, void* stream);

/* ------------------------------------------------------------------ scans */
/* Exclusive prefix sum of n int32 values into out[0..n] (out[n] = total).
 * ws: workspace of at least ofx_scan_ws_bytes(n) bytes.
 * Replaces torch.cumsum uses in ocnn Octree.octree_split and
 * dual_octree.py:265-271 (remap_node_idx). */
size_t ofx_scan_ws_bytes(int64_t n);
int ofx_scan_i32(const int32_t* in, int32_t* out, int64_t n, void* ws, void* stream);

/* ---------------------------------------------------------------- octree
 * Own octree container ops (ocnn.octree.Octree is third-party and absent;
 * semantics per SURVEY.md 8c).  Call sites replaced:
 * utils/util_dualoctree.py:225-273 (split2octree_small/large),
 * ldm_diffusion_util.py:318-325 (create_full_octree),
 * graph_vae.py:205-208,236-244 (octree_split / octree_grow). */

/* keys[i] = (b << 48) | i_local, children[i] = i for a full layer of depth d. */
int ofx_octree_full_layer(int depth, int batch_size, int64_t* keys, int32_t* children,
                          void* stream);
/* children[i] = label[i] ? rank : -1, where rank = excl_scan(label != 0).
 * scan_out must hold n+1 int32 (scan_out[n] = number of non-empty nodes). */
int ofx_octree_split(const int32_t* label, int64_t n, int32_t* children, int32_t* scan_out,
                     void* ws, void* stream);
/* keys_child[8*c + o] = ((key & m48) << 3 | o) | (key >> 48 << 48) for every
 * parent with children[i] = c >= 0. */
int ofx_octree_grow(const int64_t* keys_parent, const int32_t* children_parent, int64_t n_parent,
                    int64_t* keys_child, int32_t* children_child, void* stream);
/* split_small [B,8,S,S,S] (S = 2^full_depth) -> labels of the full layer
 * (any channel > 0) -- util_dualoctree.py:233-238. */
int ofx_split_small_label0(const float* split, int batch_size, int full_depth,
                           int32_t* label, void* stream);
/* labels of the 8 children of every non-empty full-layer node:
 * label1[8*c + j] = split[b, j, x, y, z] > 0 -- util_dualoctree.py:242-246. */
int ofx_split_small_label1(const float* split, int batch_size, int full_depth,
                           const int32_t* children, int32_t* label1, void* stream);
/* split_large [n, 8] -> label0[i] = any(split[i,:] > 0); label1[8*c + j] =
 * split[i, j] > 0 for non-empty i -- util_dualoctree.py:258-269. */
int ofx_split_large_label0(const float* split, int64_t n, int32_t* label0, void* stream);
int ofx_split_large_label1(const float* split, int64_t n, const int32_t* children,
                           int32_t* label1, void* stream);
/* ocnn.nn.octree2voxel at the FULL layer followed by permute(0,4,1,2,3)
 * (graph_unet_lr.py:176-177): data [B*8^d, C] -> vox [B, C, S, S, S]. */
int ofx_octree2voxel_cf(const float* data, int64_t ld, int C, int batch_size, int depth,
                        float* vox, void* stream);
/* inverse gather (graph_unet_lr.py:179-181): vox [B, C, S,S,S] -> data [B*8^d, C]. */
int ofx_voxel2octree_cf(const float* vox, int C, int batch_size, int depth, float* data,
                        int64_t ld, void* stream);

/* ------------------------------------------------------------ dual octree
 * Neighbour graph of the dual octree (replaces DualOctree.__init__,
 * dense_graph, sparse_graph, relative_dir, add_self_loops, remap_node_idx,
 * add_node_type/keyd/mask, sort_edges, calc_batch_id:
 * models/networks/dualoctree_networks/dual_octree.py:19-409).
 *
 * The tree is passed as the depth-concatenated arrays the reference itself
 * builds (dual_octree.py:42-44): child_all / key_all of length ncum[depth+1],
 * plus leafrank_all = per-depth exclusive scan of (child < 0).  nnum_host and
 * nnum_nempty_host are HOST arrays of depth+1 entries.
 *
 * Graph nodes of depth d are numbered [leaves of full_depth..d-1 | all nodes
 * of d] (dual_octree.py:265-271).  Edges come out grouped by (row, dir)
 * segment, i.e. already in the reference's sort_edges order: seg_ptr has
 * N_d*7+1 entries, col has E_d entries.  dir: 0:+z 1:-z 2:+y 3:-y 4:+x 5:-x
 * 6:self. */
typedef struct {
  int depth, full_depth, batch_size;
  const int32_t* child_all;
  const int64_t* key_all;
  const int32_t* leafrank_all;
  const int64_t* nnum_host;
  const int64_t* nnum_nempty_host;
} ofx_tree_t;

/* Point cloud -> octree -- replaces ocnn `Octree.build_octree` + `merge_octrees` at the reference call sites
 * models/octfusion_model_union.py:198-212 and models/octfusion_model_vae.py:133-141, and the 'ND' input feature of
 * the VAE encoder (dual_octree.py:343-360).  The whole batch is built top-down from ONE sorted key array:
 *   _keys: key[i] = batch << 48 | morton(trunc((p + 1) * 2^(depth-1))) (coordinates clamped to the cube),
 *          idx[i] = i; batch_id NULL -> every point belongs to element batch_const;
 *   _sort: stable radix sort of the (key, idx) pairs (ws: ofx_points_sort_ws_bytes(n) bytes);
 *   _label_from_points: label[j] = 1 iff a point lies in the cell of node j of depth d (node_keys as in
 *          ofx_octree_grow: batch << 48 | morton_d), for ofx_octree_split;
 *   _point_features: per node of the finest depth, over its points in input order: feat [nnum,4] =
 *          (normalize(sum normals), dot(frac(mean scaled position) - 0.5, normal)), zero rows for empty nodes
 *          (16-B aligned); avg_points / avg_normals [nnum,3] optional (ocnn octree.points / octree.normals). */
size_t ofx_points_sort_ws_bytes(int64_t n);
int ofx_points_keys(const float* pts, int64_t ldp, const int32_t* batch_id, int batch_const, int64_t n, int depth,
                    int64_t* keys, int32_t* idx, void* stream);
int ofx_points_sort(const int64_t* keys_in, const int32_t* idx_in, int64_t n, int64_t* keys_out, int32_t* idx_out,
                    void* ws, size_t ws_bytes, void* stream);
int ofx_octree_label_from_points(const int64_t* sorted_keys, int64_t n_pts, const int64_t* node_keys, int64_t nnum,
                                 int depth_pts, int d, int32_t* label, void* stream);
int ofx_octree_point_features(const int64_t* sorted_keys, const int32_t* sorted_idx, int64_t n_pts, const float* pts,
                              int64_t ldp, const float* normals, int64_t ldn, const int64_t* node_keys, int64_t nnum,
                              int depth, float* feat, float* avg_points, float* avg_normals, void* stream);
/* per-depth leaf ranks: leafrank_all[ncum[t] + j] = #leaves before j at depth t.
 * ws: at least ofx_tree_leafrank_ws_bytes(max_d nnum[d]) bytes. */
size_t ofx_tree_leafrank_ws_bytes(int64_t max_nnum);
int ofx_tree_leafrank(const int32_t* child_all, const int64_t* nnum_host, int depth,
                      int32_t* leafrank_all, void* ws, void* stream);
/* node attributes of graph depth d: batch_id (key>>48), node_type (depth -
 * full_depth), keyd (key | depth<<58), node_mask (leaf, or all-true at d).
 * Any output may be NULL. */
int ofx_graph_nodes(const ofx_tree_t* tree, int d, int32_t* batch_id, uint8_t* node_type,
                    int64_t* keyd, uint8_t* node_mask, void* stream);
/* pass 1: seg_cnt[r*7 + dir] = number of neighbours of graph node r through
 * face dir (dir 6: 1 if the node has any neighbour). */
int ofx_graph_count(const ofx_tree_t* tree, int d, int32_t* seg_cnt, void* stream);
/* pass 2: col[seg_ptr[r*7+dir] ...] = neighbour ids (seg_ptr = excl. scan of seg_cnt). */
int ofx_graph_fill(const ofx_tree_t* tree, int d, const int32_t* seg_ptr, int32_t* col,
                   void* stream);
/* CSR -> the reference's COO view: row[e], dir[e] (int64) for edge_idx / edge_dir.  Any output may be NULL; col is
 * required only with col_out. */
int ofx_graph_expand(const int32_t* seg_ptr, int64_t n_nodes, const int32_t* col,
                     int64_t* row_out, int64_t* col_out, int64_t* dir_out, void* stream);
/* The table builders: ofx_graph_primary / _multi_flag / _primary_ext (declared with the GraphConv tables below),
 * ofx_graph_type_frac, ofx_graph_reverse_count / _fill, their weighted forms ofx_graph_*_w and the segment-keyed
 * ofx_seg_*_w.  Every pointer of these is required -- seg_ptr, col, w, rank, node_type and every output, multi_seg
 * included even when no segment is a multi-neighbour one (pass one spare element): a NULL returns OFX_EINVAL with
 * nothing launched.
 * nbr[r*7+dir] = the single neighbour of segment (r,dir), -1 if none, -2 if several. */
int ofx_graph_primary(const int32_t* seg_ptr, const int32_t* col, int64_t n_nodes, int32_t* nbr,
                      void* stream);
/* Reverse graph for the backward pass of GraphConv (autograd of index_select + scatter_mean,
 * models/networks/modules.py:205-213): reverse segment (c, dir) lists the forward edges with col == c in
 * direction dir; rev_row = their rows (sorted), rev_w = 1 / size of the forward segment (row, dir).
 * rev_cnt doubles as the fill cursor (it is zeroed and rewritten by _fill). */
int ofx_graph_reverse_count(const int32_t* seg_ptr, const int32_t* col, int64_t n_nodes, int32_t* rev_cnt,
                            void* stream);
int ofx_graph_reverse_fill(const int32_t* seg_ptr, const int32_t* col, int64_t n_nodes, const int32_t* rev_ptr,
                           int32_t* cursor, int32_t* rev_row, float* rev_w, void* stream);
/* weighted-graph variants of ofx_graph_primary / _multi_flag / _primary_ext: a segment counts as a single plain
 * source row only if it has one edge of weight exactly 1 (pointers: as for the table builders above) */
int ofx_graph_primary_w(const int32_t* seg_ptr, const int32_t* col, const float* w, int64_t n_nodes, int32_t* nbr,
                        void* stream);
int ofx_graph_multi_flag_w(const int32_t* seg_ptr, const float* w, int64_t n_nodes, int32_t* flag, void* stream);
int ofx_graph_primary_ext_w(const int32_t* seg_ptr, const int32_t* col, const float* w, int64_t n_nodes,
                            const int32_t* rank, int32_t* nbr_ext, int32_t* multi_seg, void* stream);
/* Backward of GraphConv (training path; autograd of models/networks/modules.py:194-220).
 * _bwd_data: dx [n, cin] = fused gather-GEMM of dy over the REVERSE graph (weighted segment sums) with the
 *   transposed weights WpT = ofx_pack_weights of W^T stacked over directions (K = 7*cout, N = cin, cin_pack =
 *   cout, nt = 0).  nbr_rev / nbr_ext_rev / multi_seg come from the _w table builders above; aux: scratch of
 *   (n_multi + 1) * ldy floats.  Without nbr_ext_rev, or with cout % 32 != 0 (or dy / ldy / aux not 16-B aligned),
 *   it takes the col path of ofx_graphconv_fwd: ws 16-B aligned with ws_bytes >= 588 * KpT, else OFX_EINVAL with
 *   nothing launched.
 * _bwd_weight: dWp [Kp, cout] = col_data^T @ dy in the PACKED k order of ofx_pack_weights (k = dir*cin + c,
 *   zero rows up to pad32(7*cin), then the 7*nt node-type rows), bf16 hi + lo pair MFMA (three products, ~16
 *   significand bits; exact fp32 MFMA under ofx_set_precision(1)), deterministic slice-ordered reduction.  ws holds
 *   the partial sums (and, for cin % 32 != 0, col-row chunks of >= 32 rows: a ws too small for either is
 *   OFX_EINVAL with nothing launched; a small ws only lowers the slice count / chunk size, never the result's
 *   accuracy class).  ofx_gridconv_bwd_weight likewise. */
int ofx_graphconv_bwd_data(const float* dy, int64_t ldy, int cout, int64_t n_nodes, const int32_t* nbr_rev,
                           const int32_t* rev_ptr, const int32_t* rev_row, const float* rev_w,
                           const int32_t* nbr_ext_rev, const int32_t* multi_seg, int64_t n_multi, float* aux,
                           const float* WpT, int64_t KpT, int cin, float* dx, int64_t ldx, void* ws, size_t ws_bytes,
                           void* stream);
int ofx_graphconv_bwd_weight(const float* x, int64_t ldx, int cin, int64_t n_nodes, const int32_t* nbr,
                             const int32_t* seg_ptr, const int32_t* col, const int32_t* nbr_ext,
                             const int32_t* multi_seg, int64_t n_multi, float* aux, const float* type_frac, int64_t ldt,
                             int nt_pad, const float* dy, int64_t ldy, int cout, float* dWp, int64_t Kp, void* ws,
                             size_t ws_bytes, void* stream);
/* Backward of DualOctreeGroupNorm (+ fused activation) -- training path, autograd of modules.py:291-326.
 * mean / rstd [B*C] are the forward statistics (ofx_gn_finalize).  sums [B*C*2] fp64 and coef [B*C*3] fp32 are
 * scratch.  Outputs dx [n, C], dgamma [C], dbeta [C]. */
int ofx_gn_backward(const float* x, int64_t ldx, const float* dy, int64_t ldy, int64_t n, int C,
                    const int32_t* batch_id, int batch_size, const float* count, int groups, float count_eps,
                    const float* mean, const float* rstd, const float* w, const float* bias, int act, double* sums,
                    float* coef, float* dx, int64_t lddx, float* dgamma, float* dbeta, void* stream);
/* out [K, N] = P^T Q for row-major P [rows, K], Q [rows, N] (weight gradients of the dense layers: dW = x^T dy).
 * K, N multiples of 4; bf16 hi + lo pair MFMA (exact fp32 MFMA under ofx_set_precision(1)), slice-ordered
 * (deterministic) reduction of the partials held in ws (at least K * N floats, else OFX_EINVAL). */
int ofx_gemm_tn_f32(const float* P, int64_t ldp, const float* Q, int64_t ldq, int64_t rows, int64_t K, int64_t N,
                    float* out, void* ws, size_t ws_bytes, void* stream);
/* Reverse tables for any tap table (the dense layers' 27-tap grid tables): nbr [n_out, ndir], valid sources in
 * [0, n_in); reverse CSR keyed by (source row, tap) with unit weights; and segment-generic versions of the
 * weighted table builders (nseg segments, sources in [0, n_src)). */
int ofx_table_reverse_count(const int32_t* nbr, int64_t n_out, int ndir, int64_t n_in, int32_t* rev_cnt, void* stream);
int ofx_table_reverse_fill(const int32_t* nbr, int64_t n_out, int ndir, int64_t n_in, const int32_t* rev_ptr,
                           int32_t* cursor, int32_t* rev_row, float* rev_w, void* stream);
int ofx_seg_primary_w(const int32_t* seg_ptr, const int32_t* col, const float* w, int64_t nseg, int32_t* nbr,
                      void* stream);
int ofx_seg_multi_flag_w(const int32_t* seg_ptr, const float* w, int64_t nseg, int32_t* flag, void* stream);
int ofx_seg_primary_ext_w(const int32_t* seg_ptr, const int32_t* col, const float* w, int64_t nseg, int64_t n_src,
                          const int32_t* rank, int32_t* nbr_ext, int32_t* multi_seg, void* stream);
/* Backward of the 27-tap grid convolution (torch autograd of nn.Conv3d(k=3, padding=1[, stride 2]) and of
 * nearest-upsample + conv: graph_unet_lr.py / modules.py:63-95).  WpT = ofx_pack_conv3d of weight.transpose(0,1);
 * dWp [pad32(27*cin), cout], row k = tap*cin + c.  _bwd_data's workspace rule is ofx_graphconv_bwd_data's
 * (col path: ws_bytes >= 588 * pad32(27*cout)). */
int ofx_gridconv_bwd_data(const float* dy, int64_t ldy, int cout, int64_t n_out, int64_t n_in, const int32_t* nbr_rev,
                          const int32_t* rev_ptr, const int32_t* rev_row, const float* rev_w,
                          const int32_t* nbr_ext_rev, const int32_t* multi_seg, int64_t n_multi, float* aux,
                          const float* WpT, int cin, float* dx, int64_t ldx, void* ws, size_t ws_bytes, void* stream);
int ofx_gridconv_bwd_weight(const float* x, int64_t ldx, int cin, int64_t n_in, int64_t n_out, const int32_t* nbr27,
                            const int32_t* nbr27_ext, const float* zero_row, const float* dy, int64_t ldy, int cout,
                            float* dWp, void* ws, size_t ws_bytes, void* stream);
/* Optimiser step of the training loop (octfusion_model_union.py:142, 478-487): torch.optim.AdamW's update
 * (step >= 1 is the 1-based step count) and the EMA of the weights (ldm_diffusion_util.py:38-54). */
int ofx_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, void* stream);
int ofx_ema_update(float* ema, const float* param, int64_t n, float beta, void* stream);
/* The same two updates for a whole list of tensors in a handful of launches (csrc/ofx_train.hip; the per-element
 * arithmetic is shared with the two entry points above, so the results are the same bits).  rows: a HOST array, read
 * before the call returns.  Per row: grad == NULL: no AdamW and no decay (torch's grad=None rule), EMA only;
 * ema == NULL: AdamW only; n == 0: skipped.  param / grad / moments / ema need no alignment (16-byte aligned rows take
 * the vector path).  The EMA reads the freshly updated parameter.  OFX_EINVAL: n < 0, step < 1, a NULL param with
 * n > 0, a gradient without both moments.  Nothing is launched when an argument is invalid. */
typedef struct OfxAdamRow {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  float* ema;
  int64_t n;
} OfxAdamRow;
int ofx_adamw_ema_multi(const OfxAdamRow* rows, int64_t n_rows, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int step, float ema_beta, void* stream);
/* Elements per work chunk of ofx_adamw_ema_multi (a row of n elements is cut into ceil(n / chunk) chunks). */
int ofx_adamw_ema_multi_chunk(void);
/* Rows per launch of ofx_adamw_ema_multi: a call over R rows with work launches ceil(R / rows) kernels (one more where
 * a slab would exceed 2^30 chunks). */
int ofx_adamw_ema_multi_rows(void);
/* MSE loss of the diffusion stages and its gradient without a host read: dy[i] = (y[i] - target[i]) * (float)(2.0 / n),
 * *loss_out (device double) = mean((double)diff * diff) with diff the fp32 difference.  partials: device workspace of
 * ofx_mse_grad_partials(n) doubles; the sum runs in a fixed order (no atomics): the same bits run to run.  n >= 1. */
int64_t ofx_mse_grad_partials(int64_t n);
int ofx_mse_grad(const float* y, const float* target, float* dy, double* partials, double* loss_out, int64_t n,
                 void* stream);
/* NeuralMPU SDF evaluation -- replaces NeuralMPU.__call__ / get_linear_pred / octree_linear_pts
 * (models/networks/dualoctree_networks/mpu.py:55-153), spmm / modulated_spmm (utils/spmm.py:12-61) and, with the
 * _grid entry, the sampling loop of calc_sdf (utils/util_dualoctree.py:99-118).
 * pts [n,4] fp32 = (x, y, z in [-1,1], batch id).  For every depth d in [depth_start, depth_end] the 8 cell
 * centres around the point that exist in the tree (and are leaves when d < depth_end) contribute
 * w = prod(1-|f|) * d^2/50 and w * (code[row] . [f*2/2^d, 1]); sdf = sum / (sum w + 1e-8);
 * mask[i] = 1 iff a centre of depth_end exists.  code rows: nodes of depth_start..depth_end concatenated
 * (row = index in depth d + sum_{l<d} nnum[l]), 16-B aligned.  mask may be NULL.
 * _grid: point q = head + i of the size^3 lattice (x slowest), coordinate = fl(fl(i*step) + bbmin). */
int ofx_mpu_eval(const ofx_tree_t* tree, int depth_start, int depth_end, const float* pts, int64_t n_pts,
                 const float* code, float* sdf, uint8_t* mask, void* stream);
int ofx_mpu_eval_grid(const ofx_tree_t* tree, int depth_start, int depth_end, const float* code, int size,
                      float step, float bbmin, int batch_index, int64_t head, int64_t count, float* sdf,
                      uint8_t* mask, void* stream);
/* NeuralMPU with gradients (training): replaces compute_mpu_gradients (loss.py:100-108), i.e. autograd of
 * get_linear_pred w.r.t. the query position with create_graph=True.  grad [n,3] = d sdf / d (x, y, z) with the
 * reference's conventions (floor detached, d|f|/df = +1 at f = 0: mpu.py:18-32).  _backward is the adjoint of
 * (sdf, grad) w.r.t. the code table: dcode [rows,4] += J^T (dsdf, dgrad) (fp32 atomics; the caller zeroes
 * dcode; either upstream pointer may be NULL = zeros). */
int ofx_mpu_eval_grad(const ofx_tree_t* tree, int depth_start, int depth_end, const float* pts, int64_t n_pts,
                      const float* code, float* sdf, float* grad, uint8_t* mask, void* stream);
int ofx_mpu_backward(const ofx_tree_t* tree, int depth_start, int depth_end, const float* pts, int64_t n_pts,
                     const float* code, const float* dsdf, const float* dgrad, float* dcode, void* stream);
/* VAE training losses, forward value + gradient w.r.t. the network output in one pass (loss.py:164-178).
 * sums are fp64 accumulators the caller zeroes.
 * _octree_ce (compute_octree_loss, loss.py:110-122): label = child[i] >= 0; sums[0] += sum of the 2-class cross
 *   entropies, sums[1] += number of rows whose argmax equals the label; dlogits (optional) =
 *   (softmax - onehot) * dscale (dscale = weight / n for the mean).
 * _sdf_reg_loss (sdf_reg_loss, loss.py:23-29): sums[0] += sum (grad - grad_gt)^2 over 3n, sums[1] +=
 *   sum (sdf - sdf_gt)^2; dsdf = 2 w_sdf (sdf - sdf_gt) / n, dgrad = 2 w_grad (grad - grad_gt) / (3n) (optional).
 * _kl_sample (DiagonalGaussianDistribution, distributions.py:24-46): params [n, 2E] = (mean | logvar), logvar
 *   clamped to [-30, 20]; z = mean + exp(logvar/2) * noise (noise NULL: the mean); kl_sum += sum of
 *   0.5 (mean^2 + var - 1 - logvar).  _bwd: dparams = d/dparams of (<dz, z> + kl_scale * sum kl). */
int ofx_octree_ce(const float* logits, int64_t ld, const int32_t* child, int64_t n, float dscale, double* sums,
                  float* dlogits, int64_t ldd, void* stream);
int ofx_sdf_reg_loss(const float* sdf, const float* grad, const float* sdf_gt, const float* grad_gt, int64_t n,
                     float w_sdf, float w_grad, double* sums, float* dsdf, float* dgrad, void* stream);
int ofx_kl_sample_fwd(const float* params, int64_t ld, const float* noise, int64_t n, int embed_dim, float* z,
                      double* kl_sum, void* stream);
int ofx_kl_sample_bwd(const float* params, int64_t ld, const float* noise, const float* dz, int64_t n,
                      int embed_dim, float kl_scale, float* dparams, int64_t ldp, void* stream);
/* Extended table for the branch-free kernel: flag[s] = segment s has > 1 neighbours;
 * with rank = exclusive scan of flag: nbr_ext[s] = neighbour id | N (none: zero row) |
 * N + 1 + rank[s] (several: pre-averaged row), multi_seg[rank[s]] = s. */
int ofx_graph_multi_flag(const int32_t* seg_ptr, int64_t n_nodes, int32_t* flag, void* stream);
int ofx_graph_primary_ext(const int32_t* seg_ptr, const int32_t* col, int64_t n_nodes,
                          const int32_t* rank, int32_t* nbr_ext, int32_t* multi_seg, void* stream);
/* type_frac[r, dir*nt + t] = fraction of (r,dir)'s neighbours with node_type t; row
 * pitch ld floats, columns >= 7*nt zero-filled up to ld.  This is the one-hot
 * half of GraphConv's col_data (modules.py:199-210), constant per doctree. */
int ofx_graph_type_frac(const int32_t* seg_ptr, const int32_t* col, const uint8_t* node_type,
                        int64_t n_nodes, int nt, float* type_frac, int64_t ld, void* stream);

/* ---------------------------------------------------------------- GEMM core
 * Packed weight layout Wp[(k/4) * N + n][4] (k padded to Kp, multiple of 32,
 * with zero rows).  ofx_pack_weights handles plain [K,N] (sk = N, sn = 1),
 * transposed nn.Linear [N,K] (sk = 1, sn = K) and -- when cin > 0 -- the
 * GraphConv row permutation: reference row dir*(cin+nt)+c (modules.py:174-176)
 * -> packed k = dir*cin + c for features, 7*cin + dir*nt + t for node types. */
/* Contraction precision (process-wide).  Modes 0 and 3 split activations and weights into 16-bit hi + lo halves and
 * run a*w = a_lo*w_hi + a_hi*w_lo + a_hi*w_hi on the 16-bit matrix pipe with fp32 accumulation, 16/3 x the fp32-MFMA
 * rate:
 *   3 = fp16x3 (DEFAULT since round 3): fp16 halves, 22 significand bits (operands beyond +-65504 saturate) --
 *       whole-step element-wise error at the level of the reference's own fp32 arithmetic;
 *   0 = bf16x3: bf16 halves, 16 significand bits, fp32's exponent range (~1e-5 per layer, 2e-3 element-wise through a
 *       whole step);
 *   1 = exact fp32 MFMA (v_mfma_f32_32x32x2_f32, bit-equal to an fma chain);
 *   2 = reduced precision: the planes GraphConv runs ONE fp16 MFMA per product (operands rounded to fp16, fp32
 *       accumulate; ~5e-4 per product), every other contraction in bf16 pairs.
 * Not thread-safe: set it before launching work, from the thread that launches.  Packed weights and operand planes are
 * mode-specific (re-pack after switching).
 * A packed-weight buffer holds the fp32 pack followed by the 16-bit hi|lo planes of the mode it was packed in:
 * ofx_packed_floats(Kp, N) floats in total. */
int ofx_set_precision(int mode);
int ofx_get_precision(void);
int64_t ofx_packed_floats(int64_t Kp, int64_t N);
int64_t ofx_packed_k(int64_t K);                       /* K rounded up to 32 */
int64_t ofx_graphconv_packed_k(int cin, int nt);       /* 7*cin + pad32(7*nt)  */
int ofx_pack_weights(const float* W, int64_t sk, int64_t sn, int64_t K, int64_t N,
                     int cin, int nt, float* Wp, int64_t Kp, void* stream);

/* out[orow(m), n] = sum_k A[arow(m), k] * W[k, n] + bias[n] + res[m, n]
 * a_rows / out_rows: optional int32 row maps (NULL = identity); a negative
 * out_rows entry skips the row.  Replaces torch mm / nn.Linear in
 * Downsample/Upsample (modules.py:391-395, 440-443), Conv1x1 (:332-339), the
 * time-embedding MLPs (graph_unet_hr.py:107-111). */
int ofx_gemm_f32(const float* A, int64_t lda, const int32_t* a_rows, int64_t M, int64_t K,
                 const float* Wp, int64_t Kp, int64_t N, const float* bias,
                 const float* res, int64_t ldr, float* out, int64_t ldc,
                 const int32_t* out_rows, void* ws, size_t ws_bytes, void* stream);
/* The same GEMM writing `out` as hi / lo pair planes (out_mode 2 = bf16 pairs, 3 = fp16 pairs; 0 = fp32 rows, i.e.
 * ofx_gemm_f32): needs N % 4 == 0, a 128-B aligned `out` with ldc % 32 == 0 and 16-B aligned res / bias / ws. */
int ofx_gemm_f32_planes(const float* A, int64_t lda, const int32_t* a_rows, int64_t M, int64_t K,
                        const float* Wp, int64_t Kp, int64_t N, const float* bias,
                        const float* res, int64_t ldr, float* out, int64_t ldc,
                        const int32_t* out_rows, void* ws, size_t ws_bytes, int out_mode, void* stream);

/* ---------------------------------------------------------------- GraphConv
 * Fused dual-octree graph convolution (modules.py:194-220 + scatter.py:42-66):
 *   out[r, :] = [ mean_{e in seg(r,dir)} x[col[e], :] for dir in 0..6 |
 *                 type_frac[r, :] ] @ W  + bias + emb[batch_id[r], :] + res[r, :]
 * The gather/segment-mean is done on the fly into LDS (col_data is never
 * written to HBM); the contraction runs on fp32 MFMA.  emb/batch_id fuse the
 * reference's per-batch-element time-embedding add (modules.py:754-758), res
 * the residual / skip add (:763).  type_frac may be NULL (nt <= 1).
 * nbr = ofx_graph_primary table (col path: any cin).  nbr_ext / multi_seg / aux
 * (scratch of (n_multi+1)*ldx floats: aux rows have the row pitch of x, of which the
 * first cin floats are written) enable the branch-free fast path when
 * cin % 32 == 0: a pre-pass averages the few multi-neighbour segments into aux, the
 * main kernel then gathers exactly one row per (row,dir).  ws: split-K workspace.
 * Col path (no nbr_ext, cin % 32 != 0, or x / ldx / aux not 16-B aligned): col_data rows
 * are materialised chunk by chunk in ws and contracted by the dense kernel, so ws is
 * REQUIRED there: 16-B aligned and ws_bytes >= 588 * Kp (128 col rows of Kp floats after
 * the 1/8 set aside for split-K / statistics partials), else OFX_EINVAL with nothing
 * launched; a larger ws only means fewer, larger chunks.
 * stats (optional, needs batch_id): the epilogue also accumulates the GroupNorm statistics
 * of the OUTPUT, stats[(b*stats_ld + n)*2 + {0,1}] += (v, v^2) in fp64 (caller zeroes it),
 * in the layout ofx_gn_finalize reads -- the consuming norm then skips ofx_gn_stats. */
int ofx_graphconv_fwd(const float* x, int64_t ldx, int cin, int64_t n_nodes,
                      const int32_t* nbr, const int32_t* seg_ptr, const int32_t* col,
                      const int32_t* nbr_ext, const int32_t* multi_seg, int64_t n_multi, float* aux,
                      const float* type_frac, int64_t ldt, int nt_pad,
                      const float* Wp, int64_t Kp, int cout, const float* bias,
                      const float* emb, int64_t lde, const int32_t* batch_id,
                      const float* res, int64_t ldr, float* out, int64_t ldc,
                      double* stats /* optional */, int64_t stats_ld,
                      void* ws, size_t ws_bytes, void* stream);

/* The two GraphConvs of a diffusion U-Net that are gathers, not contractions (csrc/ofx_narrow.hip), same operator
 * (modules.py:194-220), raw nn.Parameter weights W [7 * (cin + nt), cout] row-major (no packing):
 *  ofx_graphconv_narrow_in: the INPUT convolution (graph_unet_hr.py:116), cin <= 8 channels -> cout in {64, 128},
 *      7 * (cin + nt) <= 96, nt <= 8.  col_data of a 64-row block in LDS (node-type fractions counted from node_type
 *      [n] uint8, the per-node type of ofx_graph_nodes, while walking the neighbours), a lane owns 1-2 output columns
 *      with its weights in registers, exact fp32 FMA; `stats` as in ofx_graphconv_fwd (ws >= ceil(n / 64) * cout * 8
 *      bytes of partials).
 *  ofx_graphconv_narrow_out: the OUTPUT convolution (graph_unet_hr.py:205-209), C channels -> cout <= 8, as
 *      project-then-aggregate (scatter_mean and the weight product commute): the caller first computes the dense
 *      P = y @ Wd with Wd = ofx_narrow_out_pack(W) ([C, pw], Wd[c, dir * cout + o] = W[dir * (C + nt) + c, o], pw >= 7 cout
 *      zero-padded: 32 or 64 so that a row of P is whole 128-B lines), then this call gathers cout floats per edge:
 *      out[r, o] = sum_dir mean_{e in seg(r, dir)} P[col[e], dir * cout + o] + type_term[r, o], where
 *      type_term [n, cout] = ofx_narrow_out_type_term(...) = bias[o] + sum_{dir, t} type_frac[r, dir * nt + t] *
 *      W[dir * (C + nt) + C + t, o] is constant per (graph depth, weights) -- computed once per doctree, NULL = zero. */
int ofx_graphconv_narrow_in(const float* x, int64_t ldx, int cin, int64_t n_nodes, const int32_t* seg_ptr,
                            const int32_t* col, const uint8_t* node_type, int nt, const float* W, int cout,
                            const float* bias, const int32_t* batch_id, float* out, int64_t ldc,
                            double* stats /* optional */, int64_t stats_ld, void* ws, size_t ws_bytes, void* stream);
/* ofx_graphconv_narrow_in_tab (round 6): ofx_graphconv_narrow_in through the branch-free gather table -- nbr_ext [n, 7]
 * / multi_seg [n_multi] of ofx_graph_primary_ext; `aux` = scratch of (n_nodes + n_multi + 1) * (cin <= 4 ? 32 : 64) bytes
 * (16-B aligned) that a pre-pass fills with one record per gatherable id (x + node type of a row; x mean + node-type
 * counts of a multi-neighbour segment): a segment then costs one table entry + one aligned record.  One persistent launch of two
 * 512-thread blocks per CU; a block walks row groups with the next group's gathers in flight under the current
 * group's MFMAs and stores.  Same results as ofx_graphconv_narrow_in to fp32 rounding (the segment means of
 * multi-neighbour segments are taken before, not after, the weight product's inputs are staged: same arithmetic).
 * LIMIT (nt > 0): a record holds the node-type counts of its segment ONE BYTE PER TYPE, so no segment may hold more
 * than 255 rows of one node type -- a count of 256 reads back as 0 of that type and 1 of the next.  A coarse leaf
 * across a face from a cell refined four levels deeper has 4^4 = 256 neighbours of one type: the caller must send a
 * graph depth with a segment above 255 rows to ofx_graphconv_narrow_in (octfusion_amd.ops does, from
 * DualOctree.max_seg).  Not checked here: the segment sizes live on the device. */
int ofx_graphconv_narrow_in_tab(const float* x, int64_t ldx, int cin, int64_t n_nodes, const int32_t* seg_ptr,
                                const int32_t* col, const int32_t* nbr_ext, const int32_t* multi_seg, int64_t n_multi,
                                void* aux, const uint8_t* node_type, int nt, const float* W, int cout, const float* bias,
                                const int32_t* batch_id, float* out, int64_t ldc, double* stats /* optional */,
                                int64_t stats_ld, void* ws, size_t ws_bytes, void* stream);
int ofx_narrow_out_pack(const float* W, int C, int nt, int cout, int pw, float* Wd, void* stream);
int ofx_narrow_out_type_term(const float* type_frac, int64_t ldt, int nt, int64_t n_nodes, const float* W, int C,
                             int cout, const float* bias, float* type_term, void* stream);
int ofx_graphconv_narrow_out(const float* P, int64_t ldp, int cout, int64_t n_nodes, const int32_t* seg_ptr,
                             const int32_t* col, const float* type_term /* optional */, float* out, int64_t ldc,
                             void* stream);

/* ---------------------------------------------------------------- GraphConv on operand planes
 * Second implementation of the same operator (modules.py:194-220) for the layers that carry the step's
 * time: operands arrive PRE-SPLIT and are staged global -> LDS by DMA (csrc/ofx_gemm2.hip).
 *  "planes", mode 3 (fp16x3, the default precision) / mode 2 (bf16x3): every 32-channel chunk of a row is one
 *      128-B line [hi x 32 | lo x 32] of fp16 / bf16 halves, value = hi + lo: the bytes of the fp32 row, so a
 *      planes tensor aliases an fp32-shaped [rows, C] buffer (row pitch = fp32 pitch, C % 32 == 0);
 *  mode 1 (single-pass fp16, reduced precision, ofx_set_precision(2)): fp16 row-major, C % 64 == 0.
 * ofx_planes_split: fp32 -> planes (columns C..Cpad-1 zero-filled; in place allowed for modes 2 and 3).
 * ofx_planes_merge: planes -> fp32 (tests).
 * ofx_gn_apply_planes: ofx_gn_apply (modules.py:311-314 + fused SiLU/GELU) writing planes; `out` may be x
 *      itself in modes 2 and 3.  With aux != NULL (then out must not alias x) the same launch also writes the consuming
 *      GraphConv's aux rows (zero row + multi-neighbour means, from the CSR seg_ptr / col / multi_seg of that
 *      graph depth), and ofx_graphconv_fwd_planes is called with aux_ready = 1: one launch less per convolution.
 *      aux_plan (optional, with aux): which block writes which aux row -- int32 [mb + 1] ptr (mb = ceil(n / 64) blocks
 *      of 64 consecutive rows) | ptr[mb] aux row ids 1..n_multi grouped by the block that holds ALL their source rows |
 *      aux_left | aux_left leftover ids (sources in several blocks; always contains the zero row 0).  A block then
 *      writes its aux rows right after its own rows, from L1 / L2 instead of a second trip to HBM.
 * ofx_pack_weights_planes: GraphConv weights [7*(cin+nt'), cout] (element (k, n) at W[k*sk + n*sn]) ->
 *      [k tile][cout][128-B line], k order: 7*cin gathered channels direction-major, then the 7*nt node-type
 *      rows zero-padded to a whole tile; ofx_planes_packed_bytes() bytes.
 * ofx_graphconv_fwd_planes: as ofx_graphconv_fwd, with xp / aux / tfp planes (row pitches in BYTES, 128-B
 *      aligned bases and pitches), aux = scratch of aux_bytes >= (n_multi + 1) * ldx_bytes, tfp = planes of the
 *      type_frac slab padded to a whole chunk (NULL when nt <= 1; ldt_bytes >= 128 * ceil(7 nt / chunk), chunk = 32
 *      channels in modes 2 / 3 and 64 in mode 1, else OFX_EINVAL), W2 = packed planes weights.
 *      Any cout >= 1 and any 4-B aligned out / res / emb / bias with pitches >= cout are accepted; the float4 epilogue
 *      (and with it the persistent launch and the two-stage statistics) needs cout % 4 == 0, 16-B aligned out / res /
 *      emb / bias and ldc, ldr, lde % 4 == 0, everything else takes a scalar epilogue with fp64-atomic statistics.
 *      The launches read nothing outside the operands: rows [0, n_nodes) x cout floats of res at pitch ldr, cout floats
 *      of bias and of every emb row that batch_id names, n_nodes batch ids, the plane lines of xp / aux / tfp and the
 *      packed weights with their trailer; no readable slack is required behind any of them (nbr_ext under the
 *      persistent launch excepted, below).
 *      Two launch shapes (csrc/ofx_gemm3.hip, csrc/ofx_gemm2.hip):
 *      - persistent stream-K blocks (default when `sync` is given and the layer has >= 64 k-step units): as many
 *        blocks as the device holds at once, each owning an equal contiguous share of the (tile, k-step) sequence;
 *        tiles cut by a share boundary are combined in-launch through `ws` (raw fp32 accumulator pieces behind the
 *        statistics partials: <= (CUs * 2) * 64 KB) and `sync`: >= (2 * CUs + 1) uint32, ZERO on the first call,
 *        left zero by every launch.  The LAST word of the buffer (sync_bytes / 4 - 1, whatever the block count) is a
 *        sticky error flag: a bounded wait gave up (several seconds: a hung or pre-empted device).  While it is set
 *        every block of every later launch on this buffer returns at entry WITHOUT computing (a late contributor may
 *        still store into flag words the next launch believes to be zero), so the caller must check it once per batch
 *        of launches, clear the buffer and fall back to ofx_set_gconv_persistent(0).  One buffer (and one `ws`) per
 *        stream: launches that may run concurrently must not share them.  nbr_ext needs
 *        16 B of readable slack behind its last entry and a 16-B aligned base.  Deterministic: the pieces of a tile
 *        are added in ascending k order.
 *      - one tile per block (sync == NULL, tiny layers, ofx_set_gconv_persistent(0)): 256 / 128 x 128 tiles, no
 *        split-K, meant for layers with >= ~128 tiles. */
int ofx_planes_split(const float* x, int64_t ldx, int64_t n, int C, int Cpad, int mode, void* out,
                     int64_t ldo_bytes, void* stream);
int ofx_planes_merge(const void* planes, int64_t ldp_bytes, int64_t n, int C, int mode, float* out, int64_t ldo,
                     void* stream);
int ofx_gn_apply_planes(const float* x, int64_t ldx, int64_t n, int C, const int32_t* batch_id, const float* mean,
                        const float* rstd, const double* sums, const float* count, int groups, float eps,
                        float count_eps, const float* w, const float* bias, int act, int mode, void* out,
                        int64_t ldo_bytes, const int32_t* seg_ptr, const int32_t* col, const int32_t* multi_seg,
                        int64_t n_multi, void* aux /* optional */, const int32_t* aux_plan /* optional */,
                        int64_t aux_left, void* stream);
/* ofx_gn_apply_planes_oct (round 6): ofx_gn_apply_planes with aux rows, on the sibling-octet mapping -- the same
 * outputs (planes of act(GroupNorm(x)) + the consuming GraphConv's aux rows: modules.py:291-326 feeding :194-220).
 * A thread holds the eight rows of an "octet" (rows 8 o - shift .. 8 o - shift + 7; `shift` pads the coarse-leaf
 * prefix of the graph depth to a multiple of eight, so the octets of the depth-d part are sibling groups) for its
 * four channels in registers; an aux row whose sources all lie in one octet is a masked mean of registers.
 *   oct_ptr   int32 [n_oct + 1], n_oct = ceil((n + shift) / 8): entry range of every octet;
 *   oct_ent   int32 [n_own][2] (8-B aligned): (aux row id 1..n_multi, 8-bit mask of the octet's rows it averages);
 *   left_head int32 [n_left][4] (16-B aligned): every other aux row as (aux row id, first slot in left_src, number of
 *             sources, batch element); always contains the zero row (0, 0, 0, 0); n_own + n_left == n_multi + 1;
 *   left_src  int32: the source rows of the leftover aux rows, flattened (the CSR segment of each, in order).
 * Leftover rows are re-normalised from x by extra blocks interleaved with the main blocks.  mean / rstd from
 * ofx_gn_finalize, or both NULL with (sums, count, groups, eps, count_eps): finalised per block on the fly, as in
 * ofx_gn_apply -- for C / groups >= 2 only: a block that holds rows of a third batch element derives that element's
 * statistics assuming four consecutive channels span at most two groups, so C == groups without mean / rstd is
 * OFX_EINVAL (call ofx_gn_finalize first and pass its mean / rstd).  out must not alias x.  Host-side builder:
 * octfusion_amd/dual_octree.py DualOctree.oct_plan. */
int ofx_gn_apply_planes_oct(const float* x, int64_t ldx, int64_t n, int C, const int32_t* batch_id, const float* mean,
                            const float* rstd, const double* sums, const float* count, int groups, float eps,
                            float count_eps, const float* w, const float* bias, int act, int mode, void* out,
                            int64_t ldo_bytes, int64_t n_multi, void* aux, const int32_t* oct_ptr,
                            const int32_t* oct_ent, int64_t n_own, int shift, const int32_t* left_head,
                            const int32_t* left_src, int64_t n_left, void* stream);
/* Channel windows: ofx_gn_apply_planes / ofx_gn_apply_planes_oct / ofx_gn_finalize on the channels [c_lo, c_hi) of
 * the [n, C] tensor.  Every other argument is that of the full call (x, w, bias, mean, rstd, sums, out and aux are the
 * FULL tensor's pointers, groups the full tensor's group count): the launch writes the 128-B plane lines of the
 * window's chunks and the window's part of every aux row (aux pitch = ldo_bytes), reads the sums / mean / rstd of the
 * window's groups only, and computes every element exactly as the full call does -- so the calls on [c_lo, C) and
 * [0, c_lo) together leave the bytes of one full call.  c_lo and c_hi must be multiples of 32 (64 in mode 1) and of
 * C / groups, 0 <= c_lo < c_hi <= C: anything else is OFX_EINVAL. */
int ofx_gn_finalize_window(const double* sums, const float* count, int batch_size, int C, int groups, int c_lo,
                           int c_hi, float eps, float count_eps, float* mean, float* rstd, void* stream);
int ofx_gn_apply_planes_window(const float* x, int64_t ldx, int64_t n, int C, int c_lo, int c_hi,
                               const int32_t* batch_id, const float* mean, const float* rstd, const double* sums,
                               const float* count, int groups, float eps, float count_eps, const float* w,
                               const float* bias, int act, int mode, void* out, int64_t ldo_bytes,
                               const int32_t* seg_ptr, const int32_t* col, const int32_t* multi_seg, int64_t n_multi,
                               void* aux, const int32_t* aux_plan, int64_t aux_left, void* stream);
int ofx_gn_apply_planes_oct_window(const float* x, int64_t ldx, int64_t n, int C, int c_lo, int c_hi,
                                   const int32_t* batch_id, const float* mean, const float* rstd, const double* sums,
                                   const float* count, int groups, float eps, float count_eps, const float* w,
                                   const float* bias, int act, int mode, void* out, int64_t ldo_bytes, int64_t n_multi,
                                   void* aux, const int32_t* oct_ptr, const int32_t* oct_ent, int64_t n_own, int shift,
                                   const int32_t* left_head, const int32_t* left_src, int64_t n_left, void* stream);
/* rows per main block of ofx_gn_apply_planes: the granularity `aux_plan` is built for (the host-side plan builder,
 * octfusion_amd/dual_octree.py aux_plan, asks instead of assuming). */
int ofx_gn_apply_rows(void);
int64_t ofx_planes_packed_ktiles(int cin, int nt, int mode);
int64_t ofx_planes_packed_bytes(int cin, int nt, int cout, int mode);
int ofx_pack_weights_planes(const float* W, int64_t sk, int64_t sn, int cin, int nt, int cout, int mode, void* out,
                            void* stream);
int ofx_graphconv_fwd_planes(const void* xp, int64_t ldx_bytes, int cin, int64_t n_nodes, const int32_t* seg_ptr,
                             const int32_t* col, const int32_t* nbr_ext, const int32_t* multi_seg, int64_t n_multi,
                             void* aux, size_t aux_bytes, const void* tfp, int64_t ldt_bytes, int nt, const void* W2,
                             int cout, const float* bias, const float* emb, int64_t lde, const int32_t* batch_id,
                             const float* res, int64_t ldr, float* out, int64_t ldc, double* stats /* optional */,
                             int64_t stats_ld, void* ws, size_t ws_bytes, void* sync /* optional */, size_t sync_bytes,
                             int mode, int aux_ready, void* stream);
/* ofx_graphconv_fwd_planes with the number of compute units THIS launch's persistent schedule is planned for: 0 = the
 * process-wide value (ofx_set_gconv_cus), > 0 = that many whatever the process-wide value is (clamped to the device's
 * count; 1..7: OFX_EINVAL).  A launch planned for a subset leaves the other units to kernels on other streams -- and,
 * unlike the process-wide setter, says so per launch: "this stream 128, that stream all" inside one captured step. */
int ofx_graphconv_fwd_planes_cus(const void* xp, int64_t ldx_bytes, int cin, int64_t n_nodes, const int32_t* seg_ptr,
                                 const int32_t* col, const int32_t* nbr_ext, const int32_t* multi_seg, int64_t n_multi,
                                 void* aux, size_t aux_bytes, const void* tfp, int64_t ldt_bytes, int nt,
                                 const void* W2, int cout, const float* bias, const float* emb, int64_t lde,
                                 const int32_t* batch_id, const float* res, int64_t ldr, float* out, int64_t ldc,
                                 double* stats /* optional */, int64_t stats_ld, void* ws, size_t ws_bytes,
                                 void* sync /* optional */, size_t sync_bytes, int mode, int aux_ready, int cus,
                                 void* stream);
/* 1 (default): persistent launch (whole-tile rounds + a stream-K region) where the shape qualifies; 0: always one tile
 * per block; 2: persistent with pure stream-K (no whole-tile rounds) -- A/B knob, same values.  Anything else:
 * OFX_EINVAL. */
int ofx_set_gconv_persistent(int on);
/* ofx_gemm_planes (round 6): out[m, :] = A[row_tab[m, 0], :] @ W (+ bias) on the data path of the planes GraphConv
 * (persistent stream-K blocks, LDS-DMA staging, fp16x3 / bf16x3 MFMA; csrc/ofx_gemm3.hip with one "direction") -- the
 * reference's Upsample GEMM x[n, C] @ W.flatten(1) -> [n, 8 C] (modules.py:430-446, call site :458-467) for the
 * non-leaf rows of a graph depth.  ap: pair planes of A (mode 2 / 3; 128-B aligned rows); row_tab: int32 [M, 7], 16-B
 * aligned, + 16 B of readable slack: column 0 = the source row in [0, n_a) of output row m (the other six columns are
 * converted but never dereferenced: any row in [0, n_a)); W2 from ofx_pack_gemm_planes ((K / 32) * N * 128 + 128 bytes,
 * ofx_gemm_planes_packed_bytes); out fp32 rows, or with out_mode 2 / 3 pair planes (what the next GraphConv gathers).
 * ws / sync: the workspace and flag words of ofx_graphconv_fwd_planes (same protocol, same sticky error word).
 * Returns OFX_OK, a negative status, or 1 when the shape does not qualify (fewer than 8 k-steps of 32 channels, N < 128,
 * too few tiles, workspace too small): nothing was launched and the caller uses ofx_gemm_f32 / ofx_gemm_f32_planes. */
int64_t ofx_gemm_planes_packed_bytes(int K, int N, int mode);
int ofx_pack_gemm_planes(const float* W, int64_t sk, int64_t sn, int K, int N, int mode, void* out, void* stream);
int ofx_gemm_planes(const void* ap, int64_t lda_bytes, int64_t n_a, int64_t M, int K, const int32_t* row_tab,
                    const void* W2, int N, const float* bias, float* out, int64_t ldc, int out_mode, void* ws,
                    size_t ws_bytes, void* sync, size_t sync_bytes, int mode, void* stream);
/* Plan the persistent launches for at most `cus` compute units (0 = all of the device's; values above the device's
 * count are clamped to it), so that the launches of two lanes on two HIP streams can be resident side by side
 * (octfusion_amd/sampler.py: lanes; tools/two_half_probe.py).  Process-wide; affects launches issued or captured
 * afterwards.  OFX_EINVAL for 1..7. */
int ofx_set_gconv_cus(int cus);
/* The schedule ofx_graphconv_fwd_planes' persistent launch would use for n_rows x cout outputs and nkt k-steps per tile
 * (host only, no device work; cus > 0: plan for that many compute units): out[0..4] = blocks G, q, rem, region units U,
 * whole-tile rounds; out[5 .. 5 + G] = share boundaries of the stream-K region (k-step units, bound(0) = 0,
 * bound(G) = U; every piece between a boundary and a tile edge has >= 8 k-steps).  Returns G, 0 = not eligible. */
int ofx_gconv3_plan(int64_t n_rows, int cout, int nkt, int wm, int ni, int cus, int32_t* out, int64_t out_len);
/* block geometry of the planes kernel: 0 = automatic, 2 = 128 x 128 tiles (4 waves, two blocks per CU),
 * 4 = 256 x 128 tiles (8 waves, one block per CU) -- A/B knob.  Anything else: OFX_EINVAL. */
int ofx_set_gconv2_tile(int wm);

/* ---------------------------------------------------------------- dense grids
 * The nested dense U-Net (graph_unet_lr.py) in node-row layout: a full octree layer of
 * depth d is rows b*8^d + morton(x,y,z), so octree2voxel / the gather back
 * (graph_unet_lr.py:176-181) are identities and a 3x3x3 Conv3d is the same fused
 * gather-GEMM with 27 taps.
 * ofx_grid_conv_table: nbr27[row*27 + tap] (tap = (kx*3+ky)*3+kz); out-of-grid taps get
 *   `pad`: -1 for the col path, n_in (the zero row) for the branch-free kernel.
 *   mode 0: nn.Conv3d(k3,p1) at depth_out; mode 1: ConvDownsample (k3,s2,p1,
 *   modules.py:81-95) depth_out+1 -> depth_out; mode 2: ConvUpsample (nearest x2 then
 *   k3,p1, modules.py:63-78) depth_out-1 -> depth_out.
 * ofx_pack_conv3d: nn.Conv3d weight [cout,cin,3,3,3] -> packed k = tap*cin + c.
 * ofx_gridconv_fwd: out[r,:] = sum_tap x[nbr27[r,tap],:] @ W_tap + bias + emb[bid[r]] + res[r]
 *   (emb fuses ResnetBlock's time_mlp add, modules.py:507-511; res the skip, :513).
 *   cin % 32 == 0 with nbr27_ext and zero_row: the branch-free kernel.  Otherwise the col path of
 *   ofx_graphconv_fwd over nbr27: ws 16-B aligned with ws_bytes >= 588 * ofx_conv3d_packed_k(cin), else
 *   OFX_EINVAL with nothing launched.
 * ofx_attention: QKVAttention (modules.py:538-547) on rows; see csrc/ofx_dense.hip. */
int ofx_grid_conv_table(int mode, int depth_out, int batch_size, int32_t pad, int32_t* nbr27,
                        void* stream);
int64_t ofx_conv3d_packed_k(int cin);
int ofx_pack_conv3d(const float* W, int cin, int cout, float* Wp, void* stream);
int ofx_gridconv_fwd(const float* x, int64_t ldx, int cin, int64_t n_in, int64_t n_out,
                     const int32_t* nbr27 /* pad -1, may be NULL */,
                     const int32_t* nbr27_ext /* pad n_in, may be NULL */,
                     const float* zero_row /* >= cin zeros, 16-B aligned */,
                     const float* Wp, int cout, const float* bias, const float* emb, int64_t lde,
                     const int32_t* batch_id, const float* res, int64_t ldr, float* out,
                     int64_t ldc, void* ws, size_t ws_bytes, void* stream);
/* The same branch-free gather-GEMM with a caller-made table of ntap sources per output row (entries in [0, n_src];
 * n_src = the zero row): out[orow(r), :] = [ x[tab[r, 0], :] | ... | x[tab[r, ntap - 1], :] ] @ W + bias + res[r].
 * Downsample (modules.py:391-395) is this with tab[r, j] = 8 r + j, for an x whose row pitch is not its width (a column
 * slice of the skip-concatenation buffer) -- the reference's x.view(-1, 8 C) would have to copy.  cin % 32 == 0; W packed
 * as for ofx_gemm_f32 with K = ntap * cin; out_rows / out_mode as in ofx_gemm_f32_planes. */
int ofx_gather_gemm_f32(const float* x, int64_t ldx, int cin, int ntap, int64_t n_src, int64_t n_out, const int32_t* tab,
                        const float* zero_row, const float* Wp, int64_t Kp, int cout, const float* bias,
                        const float* res, int64_t ldr, float* out, int64_t ldc, const int32_t* out_rows, void* ws,
                        size_t ws_bytes, int out_mode, void* stream);
/* A/B knob: 0 keeps sequences of >= 256 tokens on the one-wave-per-32-queries attention kernel (default 1: the keys of a
 * 32-query tile are split over the four waves of a block). */
int ofx_set_attention_split(int on);
/* qkv [batch*T, 3*heads*ch] with row pitch ldq >= 3*heads*ch, out [batch*T, heads*ch] with pitch ldo >= heads*ch;
 * batch, T, heads >= 1 and 1 <= ch <= 128, else OFX_EINVAL with nothing launched.  K and V of one (batch, head) are
 * staged in LDS at a width CH = ch rounded up to 32, 64 or 128, so a launch is accepted only while
 *   2 * Tp * (CH + 4) * 4 bytes <= 160 KiB - 2 KiB,  Tp = T rounded up to a multiple of 32:
 * T <= 544 at ch <= 32, T <= 288 at ch <= 64, T <= 128 at ch <= 128; a longer sequence is OFX_EINVAL.  T >= 256 takes
 * the split-keys launch (see ofx_set_attention_split).  qkv is read in 16-byte pieces when ch % 4 == 0, ldq % 4 == 0 and
 * qkv is 16-byte aligned, one float at a time otherwise; the result does not depend on which. */
int ofx_attention(const float* qkv, int64_t ldq, int batch_size, int T, int heads, int ch,
                  float* out, int64_t ldo, void* stream);

/* Backward of ofx_attention (autograd of QKVAttention, modules.py:538-547): dqkv [rows, 3*C] in the layout of
 * qkv, from dout [rows, C].  rowstat: scratch of batch*heads*T*3 floats.  1 <= T <= 512 (a lane of the query-row
 * kernel keeps T / 64 <= 8 scores in registers): a longer sequence is OFX_EINVAL with nothing launched, whatever ch is --
 * narrower than the forward's envelope at ch <= 32 (T <= 544), wider at ch > 32 (forward: T <= 288, then 128).  ch >= 1
 * has no upper limit here (plain channel loops, no LDS stage per channel), where the forward refuses ch > 128.
 * Pitches: ldq, ldd >= 3*C, ldo >= C. */
int ofx_attention_bwd(const float* qkv, int64_t ldq, const float* dout, int64_t ldo, int batch_size, int T, int heads,
                      int ch, float* rowstat, float* dqkv, int64_t ldd, void* stream);

/* Stand-alone segment-mean gather: col_data[r, dir, :] (the reference's
 * `scatter_mean(x[col], row*7+dir)`, modules.py:208-210).  HBM-bound; used for
 * the gather roofline measurement and as a building block. */
int ofx_gather_mean(const float* x, int64_t ldx, int cin, int64_t n_nodes,
                    const int32_t* seg_ptr, const int32_t* col, float* col_data,
                    void* stream);

/* ---------------------------------------------------------------- GroupNorm
 * DualOctreeGroupNorm (modules.py:291-326): statistics per (batch element,
 * group) over all nodes of that element.
 *  stats:    sums[b, c, 0..1] += (sum x, sum x^2) in fp64 (zeroed inside).
 *  finalize: mean/rstd [B, C] fp32 with inv_count = 1/(count*cpg + count_eps) and
 *            centred variance; count_eps = eps reproduces the reference (:302),
 *            count_eps = 0 is torch.nn.GroupNorm (GroupNorm32, modules.py:26-28).
 *  apply:    out = act((x - mean[b]) * rstd[b] * w + bias);
 *            mean / rstd from ofx_gn_finalize -- or both NULL, then (sums, count, groups, eps, count_eps) and the
 *            launch finalises on the fly (same arithmetic, same bits; one launch less per norm). */
int ofx_gn_stats(const float* x, int64_t ldx, int64_t n, int C, const int32_t* batch_id,
                 int batch_size, double* sums, void* stream);
/* ofx_gn_stats without the zero-fill: accumulates into caller-zeroed `sums` (no memset node per statistics launch). */
int ofx_gn_stats_acc(const float* x, int64_t ldx, int64_t n, int C, const int32_t* batch_id, int batch_size,
                     double* sums, void* stream);
int ofx_gn_finalize(const double* sums, const float* count, int batch_size, int C, int groups,
                    float eps, float count_eps, float* mean, float* rstd, void* stream);
int ofx_gn_apply(const float* x, int64_t ldx, int64_t n, int C, const int32_t* batch_id,
                 const float* mean /* or NULL */, const float* rstd /* or NULL */, const double* sums /* if mean NULL */,
                 const float* count, int groups, float eps, float count_eps, const float* w, const float* bias,
                 int act, float* out, int64_t ldo, void* stream);

/* One-launch GroupNorm (+ activation) for layouts whose batch elements own `rows_per_batch` CONTIGUOUS rows (the
 * dense layers of the nested lr net; modules.py:26-28 GroupNorm32 with count_eps = 0): same arithmetic as
 * ofx_gn_stats + ofx_gn_finalize + ofx_gn_apply. */
int ofx_gn_fused_rows(const float* x, int64_t ldx, int rows_per_batch, int batch_size, int C, int groups, float eps,
                      float count_eps, const float* w, const float* bias, int act, float* out, int64_t ldo,
                      void* stream);

/* A/B knob: 1 (default) = 16-channel blocks for ofx_gn_fused_rows where the shape allows, 0 = one block per group */
int ofx_set_gn_rows16(int on);

/* ---------------------------------------------------------------- glue ops */
/* dst[dmap(i), 0:C] = src[smap(i), 0:C] for i < n (maps optional; negative skips). */
int ofx_rows_copy(const float* src, int64_t lds, const int32_t* smap, float* dst, int64_t ldd,
                  const int32_t* dmap, int64_t n, int C, void* stream);
/* ofx_rows_copy writing the destination rows as hi / lo pair planes (mode 2 / 3: the operand format of
 * ofx_graphconv_fwd_planes): C % 32 == 0, dst 128-B aligned, ldd % 32 == 0.  With ofx_gemm_f32_planes this lets the
 * pool / unpool of the U-Net (modules.py:409-423, 458-467) hand the following GraphConv its operand planes directly. */
int ofx_rows_copy_planes(const float* src, int64_t lds, const int32_t* smap, float* dst, int64_t ldd,
                         const int32_t* dmap, int64_t n, int C, int mode, void* stream);
/* y = act(x) elementwise over n floats. */
int ofx_act(const float* x, float* y, int64_t n, int act, void* stream);
/* sinusoidal embedding of t[B] (ldm_diffusion_util.py:171-191): out [B, dim]. */
int ofx_timestep_embedding(const float* t, int batch_size, int dim, float max_period,
                           float* out, void* stream);
/* LearnedSinusoidalPosEmb of the dense net (modules.py:550-563): out [B, 2 * half + 1] = [t, sin(2 pi t w), cos(2 pi t w)]. */
int ofx_learned_sinusoid(const float* t, const float* w, int batch_size, int half, float* out, void* stream);
/* Linear layer on M <= 16 rows (time / label embedding MLPs, per-block embedding projections; modules.py:754,
 * graph_unet_hr.py:253-257, graph_unet_lr.py:186-193): out = act_out(act_in(a) @ W^T + bias + res) with W [N, K] in
 * nn.Linear's own layout (no packing), exact fp32 FMA, one launch.  act_* = OFX_ACT_*; bias / res optional. */
int ofx_linear_small(const float* a, int64_t lda, int M, int K, const float* W, int64_t ldw, int N, const float* bias,
                     const float* res, int64_t ldr, int act_in, int act_out, float* out, int64_t ldo, void* stream);
/* DDIM eps-branch update (octfusion_model_union.py:345-350), coef on device:
 * coef = {alpha, sigma, alpha_next, sigma_next}; x updated in place; x0_out (optional)
 * receives x_start = (x - eps*sigma)/max(alpha,1e-8), which the reference hands to the next
 * step as x_self_cond. */
int ofx_ddim_eps_update(float* x, const float* eps, const float* coef, float* x0_out, int64_t n,
                        void* stream);
/* DDIM x0-branch update (:326-344): x = mean + sqrt(var) * noise with
 * coef = {alpha, c, alpha_next, sqrt(sigma_next^2 * c) or 0 when truncated}. */
int ofx_ddim_x0_update(float* x, const float* x0, const float* noise, const float* coef,
                       int64_t n, void* stream);

/* ------------------------------------------------------------------ marching cubes (csrc/ofx_mesh.hip)
 * Mesh export of the generate path (export_mesh, octfusion_model_union.py:435-468; create_mesh,
 * utils/util_dualoctree.py:120-142: skimage marching_cubes + trimesh on the host).  Input: sdf [batch, size, size,
 * size] fp32, x slowest (what the NeuralMPU sweep writes).  A corner is inside iff v < level (any finite level);
 * cells (i, j, k) with i, j, k < size - 1; the lattice boundary is not padded.
 * Vertices: one per lattice edge with exactly one inside endpoint, owned by its lower endpoint a, along +x / +y / +z
 * to b; index-space p = a + t (b - a), t = (level - v_a) / (v_b - v_a); stored as (p * step + bbmin) * scale
 * (the reference maps with step = (bbmax - bbmin) / size); ordered by owner linear index, then axis x, y, z.
 * Triangles: the project's own 256-case table (tools/gen_mc_table.py: ambiguous faces separate their inside corners,
 * so the mesh is closed away from the boundary), ordered by cell linear index then table order, int32 indices into the
 * shape's own vertices, (v1 - v0) x (v2 - v0) toward increasing values.  Output is bitwise reproducible (scans, no
 * atomic appends).  Limits: 2 <= size <= 512, 1 <= batch <= 65535 (the count pass puts the shape into the second grid
 * dimension, the emit pass launches per shape) and batch * size^3 * 5 <= INT32_MAX; ofx_mc_ws_bytes returns 0 outside
 * and ofx_mc_count / ofx_mc_emit OFX_EINVAL with nothing launched, as for a NULL pointer or a non-finite level.
 * t is plain fp32: corners exactly at `level` (and -0.0 at level 0.0) are outside; when v_b - v_a overflows to +-inf
 * (v_a = -3e38, v_b = 3e38), t is +-0 and the vertex is the owner point a.
 * ofx_mc_count: counts[b*3 + {0,1,2}] = vertices, triangles, cells with a non-finite corner of shape b (int64).
 * ofx_mc_emit: after the caller has read the counts back, writes shape b's vertices at verts + 3 * vert_off[b] and its
 * triangles at faces + 3 * tri_off[b] (offsets: int64 device arrays; the shapes' ranges may leave gaps, which are not
 * written); ws is the workspace of the count pass (its scans are read, its id map is written), so the two calls must
 * see the same sdf / level.
 * ofx_mc_table_host (host memory): tri_table [256 * 16] edge ids, -1 padded, ntri [256].  Corner c = dx*4 + dy*2 + dz,
 * edge e = axis*4 + k, k = the owner corner's coordinates on the other two axes (x, y, z order, high bit first). */
size_t ofx_mc_ws_bytes(int batch, int size);
int ofx_mc_count(const float* sdf, int batch, int size, float level, void* ws, int64_t* counts, void* stream);
int ofx_mc_emit(const float* sdf, int batch, int size, float level, float step, float bbmin, float scale, void* ws,
                const int64_t* vert_off, const int64_t* tri_off, float* verts, int32_t* faces, void* stream);
int ofx_mc_table_host(int8_t* tri_table, uint8_t* ntri);

/* ------------------------------------------------------------------ field meshing (csrc/ofx_fieldmesh.hip)
 * Marching cubes of the NeuralMPU field without a dense lattice (2 <= size <= 2048).  The lattice is
 * ofx_mpu_eval_grid's: coordinate fl(fl(i * step) + bbmin), SDF bit-equal to what that sweep writes.  It is cut into
 * bricks of 8^3 cells, nb = ceil((size - 1) / 8) per axis, brick (I, J, K) = linear index (I * nb + J) * nb + K; a
 * brick owns the cells [8I, min(8I + 8, size - 1)) per axis and holds the points [8I, min(8I + 8, size - 1)] (its
 * frame).  Per axis lo = cell(c(first point)), hi = cell(c(last point)), cell(c) = floor((c + 1) * 2^(de-1)) in fp32;
 * the brick is ACTIVE iff the box [lo - margin, hi + margin], clipped to [0, 2^de - 1], holds a node of the shape at
 * depth de = depth_end (empty or not); every brick is active when de <= full_depth.  The mesh is ofx_mc_emit's (same
 * inside test, interpolation, mapping, table and winding) restricted to the cells of active bricks: one vertex per
 * crossing lattice edge held by an active brick's frame, written by the lowest-indexed active brick that holds it,
 * ordered by (rank of that brick among the shape's active bricks, owner point (lx * 9 + ly) * 9 + lz in its frame,
 * axis); triangles ordered by (rank of the brick, cell (cx * 8 + cy) * 8 + cz, table order).  Scans only: bitwise
 * reproducible, and a shape's result does not depend on the other shapes of the call.
 * Shapes batch0 .. batch0 + batch - 1 of the tree are meshed; 1 <= batch <= 128.
 * ofx_fieldmesh_classify: fills cws (>= ofx_fieldmesh_classify_ws_bytes(batch, size) bytes, 16-byte aligned);
 *   counts[b*2 + {0,1}] = active bricks, bricks active at margin 0 ("seeds") of shape b (int64, device).
 * ofx_fieldmesh_count: n_bricks = the sum of the active-brick counts the caller read back, 1 <= n_bricks <= 2^26;
 *   ws >= ofx_fieldmesh_ws_bytes(n_bricks) bytes (4404 B per brick: its 729 samples, a 16-bit id map, list, counts,
 *   scans), 16-byte aligned; code as for ofx_mpu_eval_grid.
 *   counts[b*4 + {0,1,2,3}] = vertices, triangles, cells with a non-finite corner, leaks of shape b (int64, device),
 *   summed in int64.  The emit pass scans the call's vertex and triangle counts in int32: the caller must not call
 *   ofx_fieldmesh_emit unless the vertices of all shapes of the call together, and the triangles, are <= INT32_MAX.
 *   A leak is a crossing lattice edge that lies in a face shared by an active and an inactive brick.
 * ofx_fieldmesh_emit: after the caller has read the counts back, writes shape b's vertices at verts + 3 * vert_off[b]
 *   and its triangles at faces + 3 * tri_off[b] (offsets: int64 device arrays), from the same cws / ws.
 * OFX_EINVAL with nothing launched for a size, batch, depth, margin < 0, non-finite level / step / bbmin, step <= 0,
 * NULL or mis-aligned pointer outside the above; the ws_bytes functions return 0 there. */
size_t ofx_fieldmesh_classify_ws_bytes(int batch, int size);
size_t ofx_fieldmesh_ws_bytes(int64_t n_bricks);
int ofx_fieldmesh_classify(const ofx_tree_t* tree, int depth_end, int batch0, int batch, int size, float step,
                           float bbmin, int margin, void* cws, int64_t* counts, void* stream);
int ofx_fieldmesh_count(const ofx_tree_t* tree, int depth_start, int depth_end, const float* code, int batch0,
                        int batch, int size, float step, float bbmin, float level, const void* cws, int64_t n_bricks,
                        void* ws, int64_t* counts, void* stream);
int ofx_fieldmesh_emit(int batch, int size, float level, float step, float bbmin, float scale, const void* cws,
                       int64_t n_bricks, void* ws, const int64_t* vert_off, const int64_t* tri_off, float* verts,
                       int32_t* faces, void* stream);

/* ------------------------------------------------------------------ mesh components (csrc/ofx_mesh_cc.hip)
 * export_mesh's clean=True (models/octfusion_model_union.py:459-467; the same code in octfusion_model_vae.py:242-250):
 * trimesh.split(only_watertight=False), keep the component whose bounding box has the largest side.
 * tests/cc_oracle.py restates every function below with numpy / scipy.
 * Input: a batch mesh in the layout ofx_mc_emit writes -- verts [V, 3] fp32, faces [F, 3] int32 local to each shape,
 * vert_off / tri_off int64 [batch + 1] (ascending, from 0 to total_verts / total_faces).  Limits: batch >= 1 and
 * 1 <= total_verts, total_faces <= INT32_MAX (ofx_mesh_cc_ws_bytes returns 0 outside).  `ws` is one workspace of
 * ofx_mesh_cc_ws_bytes bytes shared by the calls on one mesh, in the order label, then table (+ stats) or select
 * (+ extract); `status` is two int32 the caller reads back with its counts: status[0] != 0 a capped union-find loop
 * gave up (the results are not to be used), status[1] != 0 a face index outside its shape's [0, n_verts) (bit 0) or
 * inconsistent offsets (bit 1) -- then no later pass touches the mesh or writes an output (_table, _stats, _select and
 * _extract read status[1] on the device and return OFX_OK with every output as the caller left it).
 * Two vertices are connected when a face uses both.  label[v] = the lowest vertex id of v's component within its shape
 * (a vertex that no face uses: itself); components with at least one face are numbered 0 .. K-1 by ascending label.
 * Everything is a function of the mesh alone (integer min / max atomics and scans, no atomic appends): bitwise
 * reproducible.
 * ofx_mesh_cc_label (:459, the split): range check, union-find (hook the larger root under the smaller, path halving,
 *   capped loops), flatten in a launch of its own.  label: int32 [V].
 * ofx_mesh_cc_table (:459): comp_of_vert int32 [V] (optional; -1 for an unused vertex) and comp_off int32
 *   [batch + 1], the offsets of the shapes' components in the dense numbering (comp_off[batch] = all components).
 * ofx_mesh_cc_stats (:461, the extents' inputs): after _table and the caller's readback of comp_off[batch] = n_comp,
 *   table int32 [n_comp, 8]: columns 0-2 / 3-5 the fp32 bits of the exact bounding-box min / max, 6 the vertex
 *   count, 7 the face count.  The order of the box is that of the bit patterns: -0.0 lies below +0.0 (a component
 *   holding both has min -0.0 and max +0.0), denormals and the infinities are ordinary values.  n_comp may be smaller
 *   than the true count: the first n_comp components are written and nothing else; n_comp == 0 writes nothing.
 * ofx_mesh_cc_select (:461-465): per shape the component with the largest max-axis extent (fp32 subtraction of the
 *   stored coordinates), a tie to the lowest label; winner_label int32 [batch] (-1: no face); keep_counts int64
 *   [3 * batch]: kept vertices, kept faces, components before cleaning.  Needs neither _table nor _stats.
 * ofx_mesh_cc_extract (:466): after the caller has read keep_counts back, writes shape b's kept vertices at out_verts +
 *   3 * new_vert_off[b] and kept faces, renumbered, at out_faces + 3 * new_tri_off[b], both in their original order
 *   (the shapes' ranges may leave gaps, which are not written); ws is the workspace ofx_mesh_cc_select left.
 * OFX_EINVAL with nothing launched for totals or a batch outside the limits or a NULL pointer (comp_of_vert excepted;
 * table may be NULL only with n_comp == 0). */
size_t ofx_mesh_cc_ws_bytes(int64_t total_verts, int64_t total_faces, int batch);
int ofx_mesh_cc_label(const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off, int batch,
                      int64_t total_verts, int64_t total_faces, int32_t* label, void* ws, int32_t* status,
                      void* stream);
int ofx_mesh_cc_table(const int32_t* faces, const int32_t* label, const int64_t* vert_off, const int64_t* tri_off,
                      int batch, int64_t total_verts, int64_t total_faces, int32_t* comp_of_vert, int32_t* comp_off,
                      void* ws, const int32_t* status, void* stream);
int ofx_mesh_cc_stats(const float* verts, const int32_t* faces, const int32_t* label, const int64_t* vert_off,
                      const int64_t* tri_off, int batch, int64_t total_verts, int64_t total_faces, int64_t n_comp,
                      int32_t* table, void* ws, const int32_t* status, void* stream);
int ofx_mesh_cc_select(const float* verts, const int32_t* faces, const int32_t* label, const int64_t* vert_off,
                       const int64_t* tri_off, int batch, int64_t total_verts, int64_t total_faces,
                       int32_t* winner_label, int64_t* keep_counts, void* ws, const int32_t* status, void* stream);
int ofx_mesh_cc_extract(const float* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off,
                        int batch, int64_t total_verts, int64_t total_faces, const int64_t* new_vert_off,
                        const int64_t* new_tri_off, float* out_verts, int32_t* out_faces, void* ws,
                        const int32_t* status, void* stream);

/* ------------------------------------------------------------------ mesh simplification (csrc/ofx_simplify.hip)
 * Vertex clustering with quadric-error placement (Lindstrom 2000): the decimation users of the reference run on the
 * host after export_mesh.  tests/simplify_oracle.py restates the rule with numpy; DESIGN.md section 4.16 derives it.
 * Input: a batch mesh in the layout of the component calls above (verts [V, 3] fp32, faces [F, 3] int32 local to each
 * shape, vert_off / tri_off int64 [batch + 1]).  Limits: batch >= 1, 1 <= total_verts < INT32_MAX,
 * 1 <= total_faces <= INT32_MAX / 3 (ofx_simplify_ws_bytes returns 0 outside).  `ws` is one workspace of
 * ofx_simplify_ws_bytes bytes shared by the two calls; `status` is two int32 the caller reads back with the counts:
 * status[0] != 0 a face index outside its shape's [0, n_verts) (bit 0) or inconsistent offsets (bit 1) -- checked
 * before any index is followed, and then no later pass touches the mesh; status[1] bit 0 a vertex needs a cell index
 * >= 1024 under cell_size, bit 1 a shape has a NaN or infinite vertex coordinate (in a vertex a face uses or not, under
 * `cells` and under cell_size alike); the outputs of the flagged shapes (counts columns 6 / 7) are not to be used,
 * those of the other shapes are what they would be alone.  Nothing allocates, nothing synchronises, no
 * floating-point atomics: the output is a function of each shape's own vertices and faces, bitwise reproducible, the
 * same alone or anywhere in a batch.
 * ofx_simplify_cluster: the grid is `cells` (1 .. 1024) cells along the longest side of each shape's bounding box, or,
 *   with cells == 0, cells of side cell_size (finite, > 0); 0 < reg <= 1 is the regulariser of the placement.  All
 *   arithmetic is fp64.  counts int64 [batch, 8]: occupied cells (clusters), kept vertices, kept faces, faces that
 *   collapsed (fewer than three different clusters), faces dropped as duplicates of an earlier face, 1 if the shape
 *   has a bad face index, 1 if it overflows the grid, 1 if it has a non-finite vertex (it is then left as a single
 *   cluster and never flagged as overflowing).  `stages` = ofx_simplify_stages() runs everything; a smaller value
 *   >= 1 stops after that many of {keys, vertex sort, incidence sort, solve, face pass} (for timing the split):
 *   status and the columns 5-7 are complete from stage 1 on, the columns 0-4 are 0 until the face pass has run.
 *   OFX_EINVAL with nothing launched (counts and status as the caller left them) for stages < 1 or >
 *   ofx_simplify_stages(), cells outside [0, 1024], cells == 0 with a cell_size that is not finite and > 0, reg
 *   outside (0, 1] or NaN, totals or a batch outside the limits, a NULL pointer.
 * ofx_simplify_extract: after the caller has read counts back, writes shape b's kept cluster positions (rounded once
 *   to fp32, in ascending (ix, iy, iz) cell order) at out_verts + 3 * new_vert_off[b] and its kept faces (input order,
 *   rotated so that the lowest cluster comes first, renumbered) at out_faces + 3 * new_tri_off[b] (the shapes'
 *   ranges may leave gaps, which are not written). */
int ofx_simplify_stages(void);
size_t ofx_simplify_ws_bytes(int64_t total_verts, int64_t total_faces, int batch);
int ofx_simplify_cluster(const float* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off,
                         int batch, int64_t total_verts, int64_t total_faces, int cells, double cell_size, double reg,
                         int stages, int64_t* counts, void* ws, int32_t* status, void* stream);
int ofx_simplify_extract(const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off, int batch,
                         int64_t total_verts, int64_t total_faces, const int64_t* new_vert_off,
                         const int64_t* new_tri_off, float* out_verts, int32_t* out_faces, void* ws,
                         const int32_t* status, void* stream);

/* ------------------------------------------------------------------ voxel meshes of octrees (csrc/ofx_voxmesh.hip)
 * The octree export of the generate path (export_octree, octfusion_model_union.py:403-422: the nodes of one depth
 * scattered into a dense float grid, then voxel2mesh / _voxel2mesh, ldm_diffusion_util.py:345-446, a Python loop over
 * the occupied voxels): one quad, as two triangles, for every face of an occupied cell whose neighbour is empty or
 * outside the grid.  tests/voxmesh_oracle.py restates the output with numpy.
 * Occupancy: R = 2^depth, 1 <= depth <= 9; one bitmask per shape, cell (x, y, z) = bit (x*R + y)*R + z (x slowest, the
 * order of np.where), kept in the workspace.  Two calls fill it:
 * ofx_voxmesh_mask_keys: clears the mask, then sets the cell of every key (int64 [n], what Octree.key(depth) holds:
 *   Morton code of depth levels, batch id from bit 48) whose batch id lies in [batch0, batch0 + batch).
 * ofx_voxmesh_mask_dense: occ [batch, R, R, R] fp32; a cell is occupied iff its value is finite and > threshold (a
 *   neighbour EQUAL to the threshold counts as empty; the reference emits no face toward it).
 * ofx_voxmesh_count: counts[b*2 + {0,1}] = quads, welded vertices (0 when !weld) of shape b (int64).  A shape has
 *   2 * quads triangles and, unwelded, 4 * quads vertices.
 * ofx_voxmesh_emit: after the caller has read the counts back, writes shape b's vertices at verts + 3 * vert_off[b]
 *   and its triangles at faces + 3 * tri_off[b] (offsets: int64 device arrays), int32 indices into the shape's own
 *   vertices.  Quads in ascending cell order, within a cell +z, -z, -x, +x, +y, -y, each with the reference's corner
 *   order and triangle pair (all wound outward).  Unwelded (the reference's arrays verbatim): four vertices per quad
 *   in its corner order.  Welded: every lattice corner a quad uses once, in ascending corner index
 *   (cx*(R+1) + cy)*(R+1) + cz.  Coordinates corner * (2 / R) - 1, exact in fp32.
 * Output is bitwise reproducible (popcounts and scans; the only atomics are the ORs into the bitmasks).  `weld` must be
 * the same for ws_bytes, count and emit.  Limits: 1 <= batch <= 65535 (the dense fill puts the shape into the second
 * grid dimension) and batch * R^3 * 24 <= INT32_MAX (ofx_voxmesh_ws_bytes returns 0 outside, which excludes depth 9;
 * the other entries return OFX_EINVAL with nothing launched, as for a NULL pointer, n < 0, batch0 < 0 or a NaN
 * threshold).  The offsets of _emit may leave gaps between the shapes' ranges, which are not written. */
size_t ofx_voxmesh_ws_bytes(int batch, int depth, int weld);
int ofx_voxmesh_mask_keys(const int64_t* keys, int64_t n, int batch0, int batch, int depth, void* ws, void* stream);
int ofx_voxmesh_mask_dense(const float* occ, int batch, int depth, float threshold, void* ws, void* stream);
int ofx_voxmesh_count(int batch, int depth, int weld, void* ws, int64_t* counts, void* stream);
int ofx_voxmesh_emit(int batch, int depth, int weld, void* ws, const int64_t* vert_off, const int64_t* tri_off,
                     float* verts, int32_t* faces, void* stream);

/* ------------------------------------------------------------------ evaluation metrics (csrc/ofx_metrics.hip)
 * The reference's metrics/ package (generate_pointclouds.py:14-37, evaluation_metrics.py:111-201, the CUDA extension
 * pytorch_structural_losses: nndistance.cu, approxmatch.cu:3-224).  Point clouds are [N, n, 3] fp32, the reference's
 * layout; tests/metrics_oracle.py restates every function in float64.
 * ofx_surface_sample: `batch` meshes concatenated -- verts [V, 3] fp32, faces [F, 3] int32 indices into the shape's
 * own vertices; offs (int64 device) = [vert_off[batch], vert_cnt[batch], face_off[batch], face_cnt[batch]];
 * total_faces = F; every shape needs >= 1 face and in-range indices (the caller checks).  Per shape: vertex bounding
 * box, and with normalize the vertices map to (v - box centre) * 2 / max extent (scale_to_unit_cube, padding 0);
 * triangles are drawn with probability |(B - A) x (C - A)| / sum (fp64 prefix per shape, fixed order), barycentrics
 * uniform with the u + w > 1 reflection.  The random numbers are r_d = ofx_metrics_hash(seed, id, i, d) for point i
 * of the shape with id = ids[b] (int64 device array, NULL: b), d = 0 triangle, 1 and 2 barycentrics: the output
 * out [batch, n, 3] is a pure function of the inputs (bitwise, any launch geometry).  ws: ofx_surface_sample_ws_bytes.
 * ofx_surface_sample_oriented: the same draw (same arguments, workspace and hash; `out` is bit-equal to
 * ofx_surface_sample's) plus normals [batch, n, 3]: the unit normal (B - A) x (C - A) / |.| of the triangle drawn for
 * each point, computed in fp64 from the un-normalised vertices (normalising scales and translates: same direction)
 * and rounded once to fp32.  A zero-area triangle has probability 0 and is never drawn; a shape whose total area is 0
 * is the caller's error (its normals are written as 0).  This is what the VAE encoder eats: Points(points, normals).
 * ofx_nn_matrix: d [na, nb] with d[i, j] = mean_p min_q |p - q|^2, p over a[i] ([na, n, 3]), q over b[j] ([nb, m, 3])
 * -- directed, so Chamfer is d_ab + d_ba^T (the reference's dl.mean + dr.mean); direct differences: a cloud against
 * itself gives exactly 0.  Any n, m >= 1.
 * ofx_emd_matrix: e [nx, ny] with e[i, j] = approxmatch cost (x[i] as xyz1, y[j] as xyz2) / n -- emd_approx_cuda of
 * evaluation_metrics.py:57-62: levels -4^j, j = 7 .. -1, three passes per level, Sum match * |p - q|; not symmetric.
 * Requires n == m <= OFX_EMD_MAX_POINTS (both clouds live in LDS); anything else is OFX_EINVAL. */
#define OFX_EMD_MAX_POINTS 2048
size_t ofx_surface_sample_ws_bytes(int batch, int64_t total_faces);
int ofx_surface_sample(const float* verts, const int32_t* faces, const int64_t* offs, const int64_t* ids, int batch,
                       int64_t total_faces, int n, uint64_t seed, int normalize, void* ws, float* out, void* stream);
int ofx_surface_sample_oriented(const float* verts, const int32_t* faces, const int64_t* offs, const int64_t* ids,
                                int batch, int64_t total_faces, int n, uint64_t seed, int normalize, void* ws,
                                float* out, float* normals, void* stream);
int ofx_nn_matrix(const float* a, int64_t na, int n, const float* b, int64_t nb, int m, float* d, void* stream);
int ofx_emd_matrix(const float* x, int64_t nx, const float* y, int64_t ny, int n, int m, float* e, void* stream);
/* the sampler's counter hash (host): splitmix64 steps h <- mix(h + 0x9E3779B97F4A7C15 * (x + 1)) over x = id, i, d */
uint64_t ofx_metrics_hash(uint64_t seed, int64_t shape, int64_t point, int draw);

/* ------------------------------------------------------------------ nearest-neighbour search (csrc/ofx_nnsearch.hip)
 * Exact brute-force search over `batch` ragged cloud pairs, concatenated as ofx_surface_sample concatenates meshes:
 * queries q [Q, 3] and targets t [T, 3] fp32; q_off, t_off [batch + 1] (int64 device) = where each pair's queries and
 * targets begin, q_off[0] = t_off[0] = 0 and the last entry the total.  Host-known sizes for the launch geometry:
 * total_q = Q, max_q / max_t = the largest query / target count of any pair (a pair larger than stated is not searched
 * in full).  Outputs dist2 [Q] fp32 and idx [Q] int32, idx local to the pair's target cloud.  tests/
 * recon_metrics_oracle.py restates the contract in float64.
 *   distance  |q - t|^2 = fma(dz, dz, fma(dy, dy, dx * dx)) from direct differences in fp32.  Every pair of points goes
 *     through that one code path: the value does not depend on which block, tile or slice saw it, and a cloud against
 *     itself gives exactly 0.
 *   tie rule  idx is the LOWEST index among the targets whose computed distance is minimal.
 *   purity    (dist2, idx) is a pure function of the inputs: bitwise equal across repeats and across any `splits`.
 *   edges     an empty target cloud gives dist2 = +inf, idx = -1; an empty query cloud writes nothing; batch == 0 or
 *     Q == 0 launches nothing and returns OFX_OK.  max_t > INT32_MAX, more than INT32_MAX blocks, a negative size or a
 *     NULL array that would be read or written: OFX_EINVAL, nothing launched.  Non-finite coordinates are the
 *     caller's error (a NaN distance is never the minimum).
 *   splits    the number of slices each pair's target cloud is cut into, every slice searched by blocks of its own.
 *     0 = automatic: ofx_nn_search_splits(batch, max_q, max_t) = enough slices for about 1024 blocks (four per CU of
 *     256), at most one per ofx_nn_search_tile() targets, at least 1 -- a single pair with few queries still fills the
 *     chip.  k >= 1 forces k slices (for comparing geometries).  Slices combine through a 64-bit unsigned minimum of
 *     (bits(dist2) << 32) | idx in ws (ofx_nn_search_ws_bytes(Q) bytes; may be NULL when one slice is used):
 *     non-negative floats order as their bit patterns, equal distances by index, so the tie rule holds.
 * A block searches ofx_nn_search_qpass() queries of one pair against one slice, in tiles of ofx_nn_search_tile(). */
int ofx_nn_search_qpass(void);
int ofx_nn_search_tile(void);
int ofx_nn_search_splits(int batch, int64_t max_q, int64_t max_t);
size_t ofx_nn_search_ws_bytes(int64_t total_q);
int ofx_nn_search(const float* q, const int64_t* q_off, const float* t, const int64_t* t_off, int batch,
                  int64_t total_q, int64_t max_q, int64_t max_t, int splits, void* ws, float* dist2, int32_t* idx,
                  void* stream);

/* ------------------------------------------------------------------ normals of raw point clouds (csrc/ofx_normals.hip)
 * Three stages over `batch` ragged clouds, concatenated: p [N, 3] fp32; off [batch + 1] (int64 device) = where each
 * cloud begins, off[0] = 0 and the last entry N.  Host-known sizes for the launch geometry: total = N, max_n = the
 * largest cloud (a cloud larger than stated is not processed in full).  tests/normals_oracle.py restates all three.
 * Common edges: batch == 0 or total == 0 launches nothing and returns OFX_OK; a negative size, k outside [1, 64],
 * batch > 65535, total > INT32_MAX, max_n outside [1, total] or a NULL array that would be read or written:
 * OFX_EINVAL, nothing launched.  Non-finite coordinates are the caller's error (no access leaves the arrays).
 * ofx_knn: exact k nearest neighbours of every point inside its own cloud.  idx [N, k] int32, local to the cloud,
 *   d2 [N, k] fp32.
 *   distance  fma(dz, dz, fma(dy, dy, dx * dx)) from direct fp32 differences, the expression of ofx_nn_search: a
 *     point against itself gives exactly 0.
 *   order     a row is ascending by (d2, idx).  The point itself is a candidate; ties go to the lowest index, so an
 *     exact duplicate with a lower index precedes the point itself.
 *   small     a cloud with fewer than k points fills the remaining slots with idx = -1, d2 = +inf.
 *   purity    (idx, d2) is a pure function of the inputs: bitwise equal across repeats, alone or in a batch, and for
 *     every `cells`.
 *   cells     each cloud is binned in a uniform grid of c^3 cells over its bounding cube (centred on the box centre,
 *     side = the largest extent); a query searches shells of cells around its own until its k-th distance lies below
 *     the squared distance to the unsearched cells, which keeps the result exact.  0 = automatic, per cloud of n
 *     points c = ofx_knn_cells(n) = clamp(floor(sqrt(n / 32)), 1, 64); c >= 1 forces c^3 cells for every cloud
 *     (c <= 128 and batch * c^3 < 2^30, else OFX_EINVAL); c = 1 is the brute-force sweep.  A cloud without extent
 *     uses one cell.
 *   ws        ofx_knn_ws_bytes(batch, total, max_n, cells) bytes (0 for arguments out of range).
 * ofx_pca_normals: from the valid (0 <= idx < n) neighbours of each row of idx [N, k], m of them: centroid and
 *   covariance (divided by m) in fp64 from the fp32 coordinates, summed in neighbour order; eigenvalues l0 <= l1 <= l2
 *   by a cyclic Jacobi of 8 sweeps in fp64; normals [N, 3] = the eigenvector of l0, normalised in fp64 and rounded
 *   once to fp32, then negated if its component of largest magnitude (lowest axis on ties, on the fp32 values) is
 *   negative; variation [N] = fl32(max(l0, 0) / (l0 + l1 + l2)).  m < 3, or an eigenvalue sum that is not positive:
 *   normal (0, 0, 0), variation 0, and degenerate [batch] int32 (zeroed by the call) counts the point.
 * ofx_orient_normals: a consistent outward sign, every cloud on its own.  n [N, 3] unoriented normals, idx [N, k]
 *   as ofx_knn writes it; per cloud lo [batch, 3], e [batch] fp32 (the corner and the side of the bounding cube,
 *   e > 0) and g [batch] int32 (cells per axis, 8 <= g <= max_g <= 128; max_g is host-known and sizes ws =
 *   ofx_orient_normals_ws_bytes(batch, total, max_g)); 1 <= steps <= 64, 0 <= rounds <= 64.
 *   grid      h = fl32(e / g); (g + 2)^3 cells with one border layer; c(x) = floor(fl32(fl32(x - lo) / h)) per axis.
 *     The cell of a point is clamp(c, 0, g - 1) + 1.  occupied = cells holding a point, dilated by the
 *     6-neighbourhood (the border layer included); exterior = the 6-connected set of non-occupied cells reachable from
 *     the non-occupied cells of the border layer.
 *   march     for s = 1 .. 2 steps: q = fl32(p + fl32(fl32(s * fl32(h / 2)) * n)); a = the first s at which c(q) + 1
 *     is outside [0, g + 1] on some axis (or not a number) or names an exterior cell, 2 steps + 1 if none; b likewise
 *     along -n.  sign = +1 if a < b, -1 if b < a, else 0 (undecided).
 *   votes     `rounds` double-buffered rounds: d_i = sum over the valid neighbours j of row i, in neighbour order, of
 *     s_j * ((n_j.x * n_i.x + n_j.y * n_i.y) + n_j.z * n_i.z) in fp64 from the fp32 components; s_i <- sign(d_i),
 *     unchanged when d_i = 0.
 *   outputs   out [N, 3] = -n where the final sign is -1, else n (an undecided point keeps the PCA sign); sign [N]
 *     int8 = the final sign (may be NULL); counts [batch, 4] int32 (zeroed by the call) = undecided_after_march,
 *     flipped_by_vote (marched sign non-zero and the final sign its opposite), undecided (final sign 0),
 *     degenerate (n = (0, 0, 0)).  All of it is a pure function of the inputs: the flood's result is a set. */
int ofx_knn_cells(int64_t n);
size_t ofx_knn_ws_bytes(int batch, int64_t total, int64_t max_n, int cells);
int ofx_knn(const float* p, const int64_t* off, int batch, int64_t total, int64_t max_n, int k, int cells, void* ws,
            int32_t* idx, float* d2, void* stream);
int ofx_pca_normals(const float* p, const int64_t* off, const int32_t* idx, int batch, int64_t total, int64_t max_n,
                    int k, float* normals, float* variation, int32_t* degenerate, void* stream);
size_t ofx_orient_normals_ws_bytes(int batch, int64_t total, int max_g);
int ofx_orient_normals(const float* p, const float* n, const int64_t* off, const int32_t* idx, int batch, int64_t total,
                       int64_t max_n, int k, const float* lo, const float* e, const int32_t* g, int max_g, int steps,
                       int rounds, void* ws, float* out, int8_t* sign, int32_t* counts, void* stream);

/* ------------------------------------------------------------------ SDF training samples (csrc/ofx_sdfdata.hip)
 * The reference's tools/repair_mesh.py sample_sdf (:293-334) and sample_occu (:358-375) on an SDF lattice
 * sdf [S, S, S] fp32, x slowest (the reference's sdf[x, y, z]); tests/sdfdata_oracle.py restates both with numpy.
 * fp16 outputs are uint16 bit patterns, rounded to nearest even once (numpy.astype).
 * ofx_sdf_sample_nodes: xyz [n_nodes, 3] int32 = the node coordinates of n_depths consecutive octree depths starting
 *   at depth_start, concatenated depth-major in node order; depth_off [n_depths + 1] (int64 device) = where each depth
 *   begins.  Candidate g = i*k + j, sample j of node i at depth d: p = fl32(fl32(node + u) * fl32(S * 2^-d)) with
 *   u = u[g, 0..2] (fp32 [n_nodes*k, 3]) or, u == NULL, u_c = (ofx_metrics_hash(seed, shape, g, c) >> 40) * 2^-24.
 *   Kept iff 0 <= p < S - 1 on every axis (so a sum fl32(node + u) that rounds up to the next integer at the last node
 *   is dropped, as in the reference).  Per kept sample, all in fp32 in the reference's order: xi = floor(p), the eight
 *   corners c = dx*4 + dy*2 + dz, weights ((1-|fx|) * (1-|fy|)) * (1-|fz|), sdf = their weighted sum for c = 0..7;
 *   gradient = (s4-s0+s5-s1+s6-s2+s7-s3, s2-s0+s3-s1+s6-s4+s7-s5, s1-s0+s3-s2+s5-s4+s7-s6) / (norm + 1e-8).
 *   Outputs, compacted in candidate order: points [., 3] = half(half(p / (S/2) - 1) * half(shape_scale)), grad [., 3],
 *   out_sdf [.] (each with room for n_nodes*k samples), *count (device int64) = samples kept.  Order comes from
 *   ballots and a scan over block counts (ws: ofx_sdf_sample_ws_bytes), never from atomics: with u == NULL the output
 *   is a pure function of the arguments, bitwise.  n_nodes == 0 launches nothing and writes count 0.  Limits:
 *   S >= 2, k >= 1, n_nodes * k < 2^31 - 256, depth_start + n_depths <= 31; otherwise OFX_EINVAL.
 * ofx_sdf_sample_occu: n points; u [n, 3] fp64 or, u == NULL, u_c = (ofx_metrics_hash(seed, shape, i, c) >> 11) * 2^-53.
 *   pu = u * ((S-1)/S), q = pu * S, trilinear value in fp64 over the fp32 corners (weights as above, the eight
 *   products summed pairwise).  points [n, 3] = half((pu - 0.5) * 2 * shape_scale); bits [ceil(n/8)] uint8 =
 *   numpy.packbits(value < 0): point i is bit 7 - i % 8 of byte i / 8, the last byte zero-padded. */
size_t ofx_sdf_sample_ws_bytes(int64_t n_nodes, int k);
int ofx_sdf_sample_nodes(const float* sdf, int S, const int32_t* xyz, int64_t n_nodes, const int64_t* depth_off,
                         int n_depths, int depth_start, int k, uint64_t seed, int64_t shape, const float* u,
                         float shape_scale, void* ws, uint16_t* points, uint16_t* grad, uint16_t* out_sdf,
                         int64_t* count, void* stream);
int ofx_sdf_sample_occu(const float* sdf, int S, int64_t n, uint64_t seed, int64_t shape, const double* u,
                        float shape_scale, uint16_t* points, uint8_t* bits, void* stream);

/* ------------------------------------------------------------------ mesh -> SDF lattice (csrc/ofx_mesh2sdf.hip)
 * The reference's offline mesh2sdf.compute call (tools/repair_mesh.py:150); tests/mesh2sdf_oracle.py restates the
 * contract in float64.  `batch` meshes concatenated as for ofx_surface_sample: verts [V, 3] fp32, faces [F, 3] int32,
 * 0-based into the shape's own vertices; vert_off / tri_off [batch + 1] (int64 device) = where each shape's vertices
 * and faces begin, the last entry the total.  sdf [batch, S, S, S] fp32, x slowest; lattice point (i, j, k) sits at
 * p = (2i/S - 1, 2j/S - 1, 2k/S - 1), the convention of ofx_mc_emit with bbmin -1, bbmax 1.  2 <= S <= 512.
 *   magnitude  |sdf| = the Euclidean distance from p to the nearest point of the nearest triangle, everywhere in the
 *     lattice: the closest point is evaluated in fp64 and rounded once.  A zero-area triangle is the segment or point
 *     it is.  Vertices may lie outside [-1, 1]^3.
 *   sign (signed_ != 0)  negative iff the number of triangles crossed by the ray from p towards -x (crossings with
 *     x <= x_i) is odd.  A triangle is crossed iff its yz-projection has non-zero area and contains (y, z) moved by
 *     (eps, eps^2): a zero of an edge function is resolved by -sign(dz), then sign(dy) of the edge, evaluated on one
 *     ordering of the edge's end points, so a crossing through a shared edge or vertex counts once.  Crossings with
 *     x < -1 count for the whole column, crossings right of the lattice for none.  signed_ == 0: the distance.
 *   status [batch] int32: non-zero, and that shape's lattice left unwritten, if a face index is outside [0, V_b) or
 *     a vertex used by a face is not finite; nothing is read through such an index.  A shape needs >= 1 face (the
 *     caller checks).
 *   The output is a pure function of the inputs, bitwise, alone or in a batch: minima and parities do not depend on
 *   order; atomics only count and assign bin slots.  ws: ofx_mesh_sdf_ws_bytes (0 for arguments out of range:
 *   batch in [1, 65535], total_verts >= 1, 1 <= total_faces < 2^31).  Bad arguments: OFX_EINVAL, nothing launched. */
size_t ofx_mesh_sdf_ws_bytes(int batch, int64_t total_verts, int64_t total_faces, int size);
int ofx_mesh_sdf(const float* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off, int batch,
                 int size, int signed_, float* sdf, void* ws, int32_t* status, void* stream);
/* Measurement aid (tools/mesh2sdf_probe.py; not on the operator path): device pointer to >= 3 zeroed uint64 on the
 * device the next ofx_mesh_sdf calls run on, NULL (the default): counting off, the plain kernel.  Per brick of 4^3
 * lattice points the distance pass adds: words[0] += bins searched, words[1] += triangles staged (members of those
 * bins), words[2] += triangles evaluated after the per-triangle box test (x 64 = point-triangle pairs).  Sticky. */
int ofx_mesh_sdf_set_counters(unsigned long long* words);

/* ------------------------------------------------------------------ point -> mesh queries (csrc/ofx_meshquery.hip)
 * Exact distance, nearest face and closest point of arbitrary points against triangle meshes: the search of
 * ofx_mesh_sdf off the lattice.  tests/meshquery_oracle.py restates the contract in float64.  Meshes concatenated as
 * for ofx_mesh_sdf (verts, faces, vert_off, tri_off); queries as for ofx_nn_search: q [Q, 3] fp32, q_off [batch + 1]
 * (int64 device) = where each shape's queries begin, the last entry Q = total_q.  A shape may have zero queries.
 * max_q = the largest query count of one shape (host-known; the grid is ceil(max_q / 64) x batch waves).
 *   dist [Q] fp32  the Euclidean distance from the query to the nearest point of the nearest triangle of its shape: the
 *     minimum over ALL the shape's triangles of the fixed fp64 expression of (point, triangle) that ofx_mesh_sdf
 *     minimises (the same code), rounded once.  At a query that is a lattice point the value is ofx_mesh_sdf's, bit
 *     for bit.  signed_ != 0: negated where the number of crossings with x_cross <= (double)q.x is odd -- the crossing
 *     rule, the x_cross expression and the edge tie rule of ofx_mesh_sdf (the same code); an open mesh gives the parity.
 *   face [Q] int32  the 0-based index, within the shape's own faces, of a triangle that attains the minimum: among the
 *     triangles whose computed squared distance is equal as doubles, the lowest index.
 *   point [Q, 3] fp32 (may be NULL)  the closest point on that triangle, evaluated once from the face's original
 *     vertices in fp64 with the pair's branches (the three edges as clamped segments, a later edge only if strictly
 *     nearer; the plane where the projection falls inside and is strictly nearer), rounded once.
 *   A query with a non-finite coordinate gets dist = NaN, face = -1, point = NaN; it does not enter its wave's box and
 *   changes no other query's result.
 *   status [batch] int32: non-zero, and that shape's outputs left unwritten, under the conditions of ofx_mesh_sdf (a
 *     face index outside [0, V_b), a non-finite vertex used by a face); nothing is read through such an index.  A
 *     shape needs >= 1 face (the caller checks).  The status words are written even when total_q == 0.
 *   bins: the grid size G per shape, 1 .. 16, or 0 = automatic: per shape the smallest G in 1 .. 16 with
 *     256 G^2 >= F_b (a surface meets about 3 G^2 bins: at most about 85 triangles per occupied bin).  The grid spans
 *     each shape's own bounding box (of the vertices its valid faces use), so a mesh may live in any frame.
 *   The output is a pure function of the inputs, bitwise: the same alone or in a batch, for any order of the queries
 *   and for any bins (bins and order only decide what is skipped, and every skip compares a lower bound with an upper
 *   bound, with a margin).  ws: ofx_mesh_query_ws_bytes (0 for arguments out of range: batch in [1, 65535],
 *   total_verts >= 1, 1 <= total_faces < 2^31, 0 <= total_q <= 2^30, bins in [0, 16]); it holds the binned triangles
 *   with their face index (40 bytes per face).  Bad arguments: OFX_EINVAL, nothing launched. */
size_t ofx_mesh_query_ws_bytes(int batch, int64_t total_verts, int64_t total_faces, int64_t total_q, int bins);
int ofx_mesh_query(const float* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off,
                   const float* q, const int64_t* q_off, int batch, int64_t total_q, int64_t max_q, int bins,
                   int signed_, float* dist, int32_t* face, float* point, void* ws, int32_t* status, void* stream);
/* Measurement aid (tools/meshquery_probe.py; not on the operator path), as ofx_mesh_sdf_set_counters: per wave of 64
 * queries the distance pass adds words[0] += bins searched, words[1] += triangles staged, words[2] += triangles
 * evaluated after the per-triangle box test (x 64 = point-triangle pairs).  NULL: counting off.  Sticky. */
int ofx_mesh_query_set_counters(unsigned long long* words);

/* ------------------------------------------------------------------ winding numbers (csrc/ofx_winding.hip)
 * The generalized winding number of arbitrary points around triangle meshes (Jacobson et al. 2013): the robust inside /
 * outside of meshes that are open, self-intersecting or nested, where ray parity means nothing.  The sibling of
 * ofx_mesh_query: meshes, queries, q_off, max_q, status, bins and every argument range are exactly its own.
 * tests/winding_oracle.py restates the contract in float64.
 *   The pair (query p, triangle), in fp64 with every operation rounded on its own: a, b, c = the vertices minus p;
 *     num = a . (b x c); den = ((|a| |b|) |c| + (a . b) |c|) + (b . c) |a|) + (c . a) |b|, dots as (x x + y y) + z z;
 *     the term is atan2(num, den) (van Oosterom and Strackee), and a sum S of terms counts as (2 S) / (4 pi) turns.
 *     A triangle whose fp64 (b - a) x (c - a) is exactly zero contributes nothing, in either mode.
 *   w [Q] fp32: the sum below, rounded once.  A query with a non-finite coordinate gets NaN and changes no other
 *     query's result; a shape with a non-zero status has its outputs left unwritten.
 *   beta == 0, exact: S = the terms of ALL the shape's triangles added in face-index order, starting from 0;
 *     w = (2 S) / (4 pi).  A pure function of (mesh, query), bitwise: the same alone or in a batch, for any order of
 *     the queries and for any bins -- the bins are not read and not built in this mode.
 *   beta > 0, far field (first order, after Barill et al. 2018): per non-empty bin k of the G^3 grid of ofx_mesh_query,
 *     over its triangles with a non-zero (b - a) x (c - a), in face-index order 64 at a time (the 64 values added in
 *     a fixed tree, the chunks in turn): N_k = sum of (b - a) x (c - a) / 2; centre_k = sum of area x centroid / sum of
 *     area, area = |(b - a) x (c - a)| / 2, centroid = ((a + b) + c) / 3; r_k = the largest distance from centre_k to
 *     a vertex of those triangles.  With d = centre_k - p, the bin is far for p iff |d| > beta r_k and then contributes
 *     (N_k . d) / (4 pi |d|^3); otherwise it contributes (2 S_k) / (4 pi), S_k = the terms of its triangles added in
 *     face-index order from 0.  w = the contributions added in bin-index order from 0.  The result depends on bins and
 *     beta, as the approximation does; it is bitwise the same from run to run, for any order of the queries and in any
 *     batch.  Putting a bin's faces in order costs the square of its size: choose bins so that bins stay small (the
 *     automatic rule does).
 *   beta: finite and >= 0.  ws: ofx_mesh_winding_ws_bytes (0 for arguments out of range, the ranges of
 *   ofx_mesh_query_ws_bytes).  Bad arguments: OFX_EINVAL, nothing launched.  No floating-point atomics. */
size_t ofx_mesh_winding_ws_bytes(int batch, int64_t total_verts, int64_t total_faces, int64_t total_q, int bins);
int ofx_mesh_winding(const float* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off,
                     const float* q, const int64_t* q_off, int batch, int64_t total_q, int64_t max_q, int bins,
                     float beta, float* w, void* ws, int32_t* status, void* stream);
/* Measurement aid (tools/winding_probe.py; not on the operator path), as ofx_mesh_query_set_counters but >= 4 zeroed
 * words: per wave of 64 queries words[0] += bins that were far for every query of the wave (never staged),
 * words[1] += triangles staged, words[2] += (query, triangle) pairs that entered a sum, words[3] += dipoles taken.
 * NULL: counting off.  Sticky. */
int ofx_mesh_winding_set_counters(unsigned long long* words);

/* ------------------------------------------------------------------ ray -> mesh casts (csrc/ofx_raycast.hip)
 * The first hit of arbitrary rays on triangle meshes, exact and bit-reproducible: the sibling of ofx_mesh_query.
 * tests/raycast_oracle.py restates the contract in float64.  Meshes concatenated as for ofx_mesh_query (verts, faces,
 * vert_off, tri_off); rays org [Q, 3] and dir [Q, 3] fp32 with ray_off [batch + 1] (int64 device) = where each shape's
 * rays begin, the last entry Q = total_q.  A shape may have zero rays.  max_q = the largest ray count of one shape.
 * A point of the ray is org + t dir: t is in units of |dir|, which is not normalised.
 *   The pair (ray, triangle), in fp64 with every operation rounded on its own (Woop, Benthin and Wald's watertight
 *     test): kz = the axis of the largest |dir| (the lowest index among equals), kx, ky the next two in cyclic order,
 *     swapped if dir[kz] < 0; Sx = dir[kx] / dir[kz], Sy = dir[ky] / dir[kz], Sz = 1 / dir[kz].  Per vertex P:
 *     A = P - org, x = A[kx] - Sx A[kz], y = A[ky] - Sy A[kz], z = Sz A[kz] -- one expression of (ray, vertex).
 *     U = det(Cx, By, Cy, Bx), V = det(Ax, Cy, Ay, Cx), W = det(Bx, Ay, By, Ax), det(a, b, c, d) = a b - c d with a
 *     correct sign (Kahan's fma form).  The ray meets the triangle iff U, V, W are all >= 0 or all <= 0 (two-sided),
 *     D = (U + V) + W != 0 (a triangle of zero area or seen edge-on never hits), and tmin <= (float)t <= tmax with
 *     (float)t finite, where t = ((U Az + V Bz) + W Cz) / D.
 *   t [Q] fp32  the minimum of t over ALL the shape's triangles the ray meets, rounded once; +inf for a miss.
 *   face [Q] int32  the lowest index among the triangles whose t is that minimum as doubles; -1 for a miss.
 *   point [Q, 3] fp32 (may be NULL)  ((U a + V b) + W c) / D of the winning face's original vertices a, b, c.
 *   cosn [Q] fp32 (may be NULL)  n . dir / (|n| |dir|), n = (b - a) x (c - a): negative where the ray meets the face
 *     from its front.  A miss gets NaN in point and cosn.
 *   A ray with a non-finite component or a zero direction gets t = +inf, face = -1, point = cosn = NaN and changes no
 *   other ray's result.
 *   status [batch], bins: as for ofx_mesh_query (same conditions, same grid rule; a shape with a non-zero status
 *     has its outputs left unwritten).  coherent != 0: consecutive rays are neighbours already (camera rays in 8 x 8
 *     pixel tiles) and are not sorted; else rays are ordered by shape, Morton code of the origin and octant of the
 *     direction.  tmin, tmax: not NaN; infinities are allowed.
 *   The output is a pure function of the inputs, bitwise: the same alone or in a batch, for any order of the rays, any
 *   bins and either value of coherent (they only decide what is skipped; every skip is a slab test of an inflated box,
 *   DESIGN.md 4.20).  ws: ofx_ray_cast_ws_bytes (0 for arguments out of range, the ranges of ofx_mesh_query_ws_bytes).
 *   Bad arguments: OFX_EINVAL, nothing launched. */
size_t ofx_ray_cast_ws_bytes(int batch, int64_t total_verts, int64_t total_faces, int64_t total_q, int bins);
int ofx_ray_cast(const float* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off,
                 const float* org, const float* dir, const int64_t* ray_off, int batch, int64_t total_q, int64_t max_q,
                 float tmin, float tmax, int bins, int coherent, float* t, int32_t* face, float* point, float* cosn,
                 void* ws, int32_t* status, void* stream);
/* Measurement aid (tools/raycast_probe.py; not on the operator path), as ofx_mesh_query_set_counters: per wave of 64
 * rays words[0] += bins visited (at least one lane passed the bin's slab test), words[1] += triangles staged,
 * words[2] += (ray, triangle) pairs evaluated after the per-triangle slab test.  NULL: counting off.  Sticky. */
int ofx_ray_cast_set_counters(unsigned long long* words);
/* The hits of a cast as an oriented point cloud, compacted in ray order (ballots and a scan over block counts, never
 * atomics): for every ray with face >= 0, points = org + (t + sigma g / |dir|) dir with g a standard normal from the
 * counter hash (ofx_metrics_hash's chain over seed, shape, the ray's index within its shape, draws 0 and 1; Box-Muller
 * in fp64; sigma == 0: no noise), normals = the hit face's unit normal turned against the ray.  out_off [batch + 1]
 * (int64 device): where each shape's points begin, the last entry the number of hits.  points / normals have room for
 * total_q rows.  t and face are the outputs of ofx_ray_cast on the same meshes and rays; a face index out of range
 * gives NaN rows.  ws: ofx_ray_scan_ws_bytes (0 for total_q outside [0, 2^30]). */
size_t ofx_ray_scan_ws_bytes(int64_t total_q);
int ofx_ray_scan(const float* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off,
                 const float* org, const float* dir, const int64_t* ray_off, int batch, int64_t total_q, const float* t,
                 const int32_t* face, float sigma, uint64_t seed, float* points, float* normals, int64_t* out_off,
                 void* ws, void* stream);

/* ------------------------------------------------------------------ mesh checks (csrc/ofx_meshcheck.hip)
 * Is a mesh sound: weld equal vertices, count what makes it closed, manifold and oriented, find the faces that
 * intersect other faces.  tests/meshcheck_oracle.py restates the contract in float64.  Meshes concatenated as for
 * ofx_mesh_query (verts, faces, vert_off, tri_off; batch in [1, 65535]); status [batch] int32 under its conditions: a
 * face index outside [0, V_b) or a non-finite vertex used by a face gives a non-zero word, that shape's outputs are
 * left unwritten and nothing is read through such an index.  A shape needs >= 1 face (the caller checks).  Limits of
 * _weld and _topology: 1 <= total_verts <= 2^30, 1 <= total_faces <= 2^30 / 3; of _selfx: those of ofx_mesh_query.  A
 * *_ws_bytes function returns 0 outside them; bad arguments give OFX_EINVAL with nothing launched.  No floating-point
 * atomics; integer atomics only count.  Every output is a pure function of each shape's own arrays, bitwise, alone or
 * anywhere in a batch, from run to run.
 *
 * ofx_mesh_weld: two vertices of a shape are equal iff their three coordinates are equal as fp32 values (-0 == +0);
 *   a vertex with a non-finite coordinate equals no other.  rep [V] int32 = the lowest index, within the shape, of
 *   the vertices equal to this one; distinct [batch] int64 = the number of representatives.  No tolerance.
 * ofx_mesh_weld_extract: after the caller has read `distinct` (and the status words) back.  With n_b the
 *   representatives of the shapes before b whose status is zero: out_verts [sum distinct, 3] holds shape b's
 *   representatives from row n_b on, in ascending index, with their stored bits; index [V] int32 = the new index,
 *   within the shape, of every vertex's representative; out_faces [F, 3] = the faces through index, same count and
 *   order (a face that has become degenerate stays).  rep and status are ofx_mesh_weld's; ws may be another buffer.
 *
 * ofx_mesh_topology: counts [batch, OFX_MESH_TOPOLOGY_K] int64, sums [batch, 2] fp64, edge_faces [F, 3] int32 (may
 *   be NULL).  A face with fewer than three different indices is index-degenerate: it is counted (column 0) and takes
 *   no part in anything else below, nor in ofx_mesh_selfx.  Over the other faces:
 *   1 edges         distinct unordered vertex pairs {face[k], face[(k + 1) % 3]};
 *   2 boundary      edges used by exactly 1 face;  3 non-manifold  edges used by 3 or more faces;
 *   4 inconsistent  edges used by exactly 2 faces that both walk them in the same direction;
 *   5 duplicate     faces whose vertex set equals that of a lower-indexed face, in either orientation (they still
 *                   count towards the edges);
 *   6 zero area     faces whose fp64 (b - a) x (c - a) is exactly zero, ofx_mesh_winding's rule;
 *   7 unreferenced  vertices that none of these faces uses;
 *   8 components    ofx_mesh_cc_label / _table's count (two vertices are connected when any face uses both); -1 for
 *                   every shape of the call if those passes refused it or gave up.
 *   edge_faces[f, k] = the number of faces on the edge leaving corner k of face f, negated where the edge is
 *   inconsistent; 0 for an index-degenerate face.
 *   sums: area = sum of |(b - a) x (c - a)| / 2 as 0.5 sqrt((nx nx + ny ny) + nz nz), volume = sum of
 *   (a . (b x c)) / 6, dots as (x x + y y) + z z, every operation in fp64 rounded on its own; index-degenerate faces
 *   add 0.  Added in face-index order 64 at a time (the 64 values in a fixed tree, the chunks in turn).
 *
 * ofx_mesh_selfx: partners [F] int32 = the number of other faces of its shape a face intersects, first [F] int32 =
 *   the lowest such face (-1: none), pairs [batch] int64 = sum of partners / 2.  max_faces = the largest face count
 *   of one shape (host-known: the grid); bins as for ofx_mesh_query (0 = its automatic rule, 1 .. 16; same grid).
 *   Faces i < j are a candidate pair iff neither is index-degenerate, neither has zero area (above) and their closed
 *   fp32 bounding boxes overlap -- the box test is part of the definition, so no culling can change an answer.
 *   Vertices are taken in the stored order of a face and the lower-indexed face is always "i".  All arithmetic is
 *   fp64 on the fp32 coordinates, every operation rounded on its own; n(T) = (b - a) x (c - a) with differences
 *   first, plane(T, x) = n(T) . (x - a), dots as above.  dom(T) = the axis of the largest |n(T)| component (the
 *   lowest among equals); the projection along it keeps axes dom + 1 and dom + 2 (mod 3) as (x, y); o2(p, q, r) =
 *   the sign of det(qx - px, ry - py, qy - py, rx - px), det(a, b, c, d) = a b - c d in Kahan's fma form (ms_det2),
 *   whose sign is exact.  With k vertex INDICES in common:
 *   k = 3  never a pair (duplicates are column 5 above).
 *   k = 2  with a the corner of i that j does not share, u and v the corners after it in i's cyclic order, b the
 *          corner of j that i does not share: iff plane(i, b) == 0 and, projected along dom(i), o2(u, v, a) ==
 *          o2(u, v, b) != 0 -- folded flat onto its neighbour.  Any other dihedral angle is no intersection.
 *   k = 1  iff the edge of i opposite the shared corner (the two corners after it, in order) meets j, or the same
 *          edge of j meets i.
 *   k = 0  iff an edge (corners 0-1, 1-2, 2-0) of i meets j, or one of j meets i.
 *   The edge p q meets the closed triangle T = a b c: sp, sq = the signs of plane(T, p), plane(T, q).  Equal and
 *   non-zero: no.  Both zero: projected along dom(T), iff p or q is inside (o2(a, b, x), o2(b, c, x), o2(c, a, x) all
 *   >= 0 or all <= 0) or p q crosses a b, b c or c a, where p q crosses r s iff d1 d2 <= 0 and d3 d4 <= 0 for d1 =
 *   o2(p, q, r), d2 = o2(p, q, s), d3 = o2(r, s, p), d4 = o2(r, s, q), except that four zeros (collinear) cross iff
 *   the closed intervals of the two segments overlap on the axis where |q - p| is larger (x on a tie).  Otherwise:
 *   with d = q - p, A = a - p, B = b - p, C = c - p, iff d . (A x B), d . (B x C), d . (C x A) are all >= 0 or all
 *   <= 0.  Touching counts: on an unwelded soup every neighbour is a partner.
 *   Not detected: bow-tie vertices; nothing is repaired.  ws holds the shared triangle bins (40 bytes per face). */
#define OFX_MESH_TOPOLOGY_K 9
size_t ofx_mesh_weld_ws_bytes(int batch, int64_t total_verts, int64_t total_faces);
int ofx_mesh_weld(const float* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off, int batch,
                  int64_t total_verts, int64_t total_faces, int32_t* rep, int64_t* distinct, void* ws, int32_t* status,
                  void* stream);
int ofx_mesh_weld_extract(const float* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off,
                          int batch, int64_t total_verts, int64_t total_faces, const int32_t* rep,
                          const int32_t* status, float* out_verts, int32_t* out_faces, int32_t* index, void* ws,
                          void* stream);
size_t ofx_mesh_topology_ws_bytes(int batch, int64_t total_verts, int64_t total_faces);
int ofx_mesh_topology(const float* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off,
                      int batch, int64_t total_verts, int64_t total_faces, int64_t* counts, double* sums,
                      int32_t* edge_faces, void* ws, int32_t* status, void* stream);
size_t ofx_mesh_selfx_ws_bytes(int batch, int64_t total_verts, int64_t total_faces, int bins);
int ofx_mesh_selfx(const float* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off, int batch,
                   int64_t max_faces, int bins, int32_t* partners, int32_t* first, int64_t* pairs, void* ws,
                   int32_t* status, void* stream);
/* Measurement aid (tools/meshcheck_probe.py; not on the operator path), as ofx_mesh_query_set_counters: per wave of 64
 * binned faces words[0] += bins visited (the bin's box meets the wave's), words[1] += triangles staged (members of
 * those bins), words[2] += ordered (face, face) pairs that passed the box test and reached the pair rule (every
 * unordered pair is judged from both sides).  NULL: counting off.  Sticky. */
int ofx_mesh_selfx_set_counters(unsigned long long* words);

/* ------------------------------------------------------------------ mesh as a graph, fairing, vertex normals
 * (csrc/ofx_meshsmooth.hip).  tests/smooth_oracle.py restates the contract in float64.  Meshes, status words, limits
 * and refusals as for the mesh checks above, with 1 <= total_verts <= 2^30 and 1 <= 6 total_faces <= 2^30.  A face
 * TAKES PART iff its shape's status is zero and its three indices differ; every other face, and a vertex no such face
 * uses (it may hold NaN), takes part in nothing.  A corner is 3 face + k (face local to the shape).  No atomics; every
 * floating-point sum below is fp64, every operation rounded on its own, in the order stated.  Every output is a pure
 * function of each shape's own arrays, bitwise, alone or anywhere in a batch, from run to run.  No host
 * synchronisation.  A refused shape has empty rows and corner lists; its vflags, normals and out rows are unwritten.
 *
 * ofx_mesh_adjacency: row_off [V + 1] int64 over the vertices of the whole call, row_off[0] = 0; nbr (room for
 *   6 total_faces) int32: row i = nbr[row_off[i] .. row_off[i + 1]) = the distinct vertices that share a face with i,
 *   as indices of the shape, ascending.  vflags [V] int32: bit 0 = a face uses the vertex, bit 1 = it ends an edge
 *   with exactly one face (boundary), bit 2 = it ends an edge with three or more.  corner_off [V + 1] int64 and
 *   corner [3 total_faces] int32 (both, or both NULL): the corners at vertex i, ascending.
 *
 * ofx_mesh_vertex_normals: normals [V, 3] fp32.  With a, b, c the face's vertices in stored order, n = (b - a) x
 *   (c - a) (differences first); a face with n exactly zero adds nothing.  The term of a corner at vertex p with the
 *   next and previous vertices q, r of its face, u = q - p, w = r - p:  mode 0 (area) n;  2 (uniform) n / |n|;
 *   1 (angle) (n / |n|) * atan2(|u x w|, u . w)  -- the division first, component by component; |x| =
 *   sqrt((x0 x0 + x1 x1) + x2 x2).  The terms are added in corner order; the sum s gives s / |s| rounded to fp32 once,
 *   or (0, 0, 0) when |s| is not positive.
 *
 * ofx_mesh_smooth: weights 0 uniform / 1 cotangent; boundary 0 fixed / 1 slide / 2 free; lambda, mu finite; iters
 *   in [0, 10000].  out [V, 3] fp32; out64 [V, 3] fp64 (may be NULL).  The state is fp64, the input widened exactly;
 *   an iteration is the half-step with s = lambda, then, unless mu == 0, the one with s = mu; a half-step sets, for
 *   every moving vertex i with a positive weight sum,
 *       p_i <- p_i + s * (A / W),  A = sum_j w_ij * (p_j - p_i),  W = sum_j w_ij,
 *   j over row i ascending, all p from before the half-step.  w_ij = 1 (uniform) or max(0, sum / 2) with sum = the
 *   cotangents, added in the order of i's corners, of the angle opposite the edge in every face on it: with o the
 *   face's third vertex, u = p_i - p_o, w = p_j - p_o, cot = (u . w) / |u x w|, or 0 when |u x w| is not positive;
 *   computed once, from the input.  A vertex moves iff a face uses it and, when it is a boundary vertex (bit 1):
 *   fixed -- never; slide -- with w_ij = 1 for the neighbours on a one-face edge and 0 for the others, whatever
 *   `weights`; free -- like any other.  out = the state rounded to fp32 once; a vertex that may not move (not used by
 *   a face, or fixed) keeps its input bits in out and has the widened input in out64.
 *   The launches: the adjacency, the rules, the weights, one per half-step, the rounding. */
size_t ofx_mesh_adjacency_ws_bytes(int batch, int64_t total_verts, int64_t total_faces);
int ofx_mesh_adjacency(const float* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off,
                       int batch, int64_t total_verts, int64_t total_faces, int64_t* row_off, int32_t* nbr,
                       int32_t* vflags, int64_t* corner_off, int32_t* corner, void* ws, int32_t* status, void* stream);
size_t ofx_mesh_vertex_normals_ws_bytes(int batch, int64_t total_verts, int64_t total_faces);
int ofx_mesh_vertex_normals(const float* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off,
                            int batch, int64_t total_verts, int64_t total_faces, int mode, float* normals, void* ws,
                            int32_t* status, void* stream);
size_t ofx_mesh_smooth_ws_bytes(int batch, int64_t total_verts, int64_t total_faces, int weights);
int ofx_mesh_smooth(const float* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off,
                    int batch, int64_t total_verts, int64_t total_faces, int weights, int boundary, double lambda,
                    double mu, int iters, float* out, double* out64, void* ws, int32_t* status, void* stream);

/* ------------------------------------------------------------------ rendering (csrc/ofx_render.hip)
 * Shaded views of triangle meshes for the reference's FID image sets (utils/render_utils.py:14-23, utils/render/):
 * a deterministic renderer of the project's own, parity with pyrender unpinned; tests/render_oracle.py
 * restates every stage, tests/render_ms_oracle.py the multisampled entries (1, 4 or 16 samples per pixel; the
 * one-sample entries are their samples = 1 case).
 * `batch` meshes concatenated as for ofx_surface_sample: verts [V, 3] fp32, faces [F, 3] int32,
 * 0-based into the shape's own vertices (the caller checks them); offs (int64 device) = [vert_off[batch],
 * vert_cnt[batch], face_off[batch], face_cnt[batch]]; max_verts / max_faces = the largest count of one shape.
 * cam [views, 24] fp64 (device): per view the view matrix (world -> camera) and then the pose (camera -> world), each
 * the top 3 x 4 rows, row-major; the pose is rigid.  The camera looks down -z, y up, aspect 1, tan_half_fov =
 * tan(yfov / 2); image row 0 is the top.  Every float64 operation is individually rounded, in the oracle's order.
 * ofx_render_project: norm [batch, 4] fp64 = (centre, scale) per shape: with normalize the centre of the bounding box
 *   and the largest distance of a vertex from it (min / max reductions only; non-finite vertices are left out; a shape
 *   without extent gets scale 1), else (0, 0, 0, 1).  Per (view, vertex), p = (v - centre) / scale, e = view * p,
 *   w = -e.z, f = 1 / tan_half_fov: sxy [views, V, 2] int32 = rint(((e.x f) / w + 1) * 128 size), rint((1 - (e.y f)
 *   / w) * 128 size) -- screen position in 1/256 pixel, pixel (i, j) has its centre at (256 i + 128, 256 j + 128);
 *   depth [views, V] fp64 = window depth ((zfar + znear) / (zfar - znear) + 1) / 2 - (zfar znear / (zfar - znear)) / w,
 *   affine in screen space.  A vertex with w < znear, a non-finite coordinate or a screen coordinate beyond +-2^26
 *   units (all written so that a NaN fails) gets sxy = (INT32_MIN, 0), depth 0: its triangles are dropped.
 * ofx_render_raster: keys [batch, views, size, size] uint64 = min over the triangles covering the pixel centre of
 *   (floor(depth * 2^32) clamped to [0, 2^32 - 1]) << 32 | face index; all ones where nothing covers.  A triangle with
 *   a dropped vertex covers nothing and adds 1 to dropped [batch, views] int32.  The vertices are ordered so that
 *   area2 = (b - a) x (c - a) > 0 (b and c swapped otherwise: both windings are drawn; area2 == 0 covers nothing).
 *   With E_ab(p) = (b.x - a.x)(p.y - a.y) - (b.y - a.y)(p.x - a.x) in int64, p is covered iff for each edge E > 0, or
 *   E == 0 and the edge is a left edge (b.y < a.y) or a top edge (b.y == a.y, b.x > a.x).  depth(p) = ((E_bc z_a +
 *   E_ca z_b) + E_ab z_c) / area2.  Resolution is a 64-bit atomic minimum: the result does not depend on order, and
 *   on equal quantised depth the lowest face index wins.  A triangle whose pixel box, clamped to the screen, holds
 *   more than big_px pixels goes to a list (ws: ofx_render_raster_ws_bytes) and is rasterised by a wave, the others
 *   by a thread: the keys do not depend on big_px.
 * ofx_render_sample_offsets: xy [samples, 2] int32 (host) = the sample positions of a pixel in 1/256 pixel from its
 *   origin (256 i, 256 j), samples in {1, 4, 16} (else OFX_EINVAL).  1: (128, 128), the centre.  4, the rotated grid:
 *   (96, 32), (224, 96), (32, 160), (160, 224).  16: 128 + 16 o, o = (1,1), (-1,-3), (-3,2), (4,-1), (-5,-2), (2,5),
 *   (5,3), (3,-5), (-2,6), (0,-7), (-4,-6), (-6,4), (-8,0), (7,-4), (6,7), (-7,-8): one sample in every one of the
 *   pixel's 16 columns and 16 rows.  The kernels use this table.
 * ofx_render_raster_ms: keys [batch, views, size, size, samples] uint64, the key of ofx_render_raster per sample:
 *   sample s of pixel (i, j) sits at p = (256 i + x_s, 256 j + y_s), and coverage (with its tie rule, the winding swap
 *   and the zero-area rule) and the depth are evaluated at p.  A triangle's pixel box takes in every pixel with a
 *   sample inside its bounding box; big_px counts pixels, not samples, and ws is that of ofx_render_raster.  dropped
 *   counts a triangle once per (shape, view).  samples = 1 is ofx_render_raster (the same code).
 * ofx_render_shade_ms: per pixel, every distinct face among the pixel's samples is shaded once as ofx_render_shade
 *   shades it, at the ray through the pixel's CENTRE (extrapolated on the face's plane where the centre is outside
 *   it), so a face's colour in a pixel does not depend on which samples it won; a sample's colour c_s is that colour
 *   clamped to [0, 1], or the background; image = floor(255 ((sum_s c_s) / samples) + 0.5), the sum in sample order
 *   in fp64.  samples = 1 is ofx_render_shade (the same code).
 * ofx_render_shade: image [batch, views, size, size, 3] uint8 = floor(255 clamp(c, 0, 1) + 0.5); c is the background
 *   where the key is all ones, else the flat two-sided glTF 2.0 metallic-roughness shading of the key's triangle under
 *   a directional, a point and a spot light at the camera (DESIGN.md 4.14 has the closed form).  params (host, 13
 *   fp64): base colour rgb, metallic, roughness, directional / point / spot intensity, spot angle scale and offset,
 *   background rgb.
 * Bad arguments: OFX_EINVAL, nothing launched.  Limits: batch * views <= 65535, size <= OFX_RENDER_MAX_SIZE,
 * V and F < 2^31. */
#define OFX_RENDER_MAX_SIZE 4096
int ofx_render_project(const float* verts, const int64_t* offs, int batch, int64_t total_verts, int64_t max_verts,
                       const double* cam, int views, int size, double tan_half_fov, double znear, double zfar,
                       int normalize, double* norm, int32_t* sxy, double* depth, void* stream);
size_t ofx_render_raster_ws_bytes(int views, int64_t total_faces);
int ofx_render_raster(const int32_t* faces, const int64_t* offs, int batch, int64_t total_verts, int64_t total_faces,
                      int64_t max_faces, int views, int size, const int32_t* sxy, const double* depth, int64_t big_px,
                      uint64_t* keys, int32_t* dropped, void* ws, void* stream);
int ofx_render_shade(const float* verts, const int32_t* faces, const int64_t* offs, int batch, const double* norm,
                     const double* cam, int views, int size, double tan_half_fov, const uint64_t* keys,
                     const double* params, uint8_t* image, void* stream);
int ofx_render_sample_offsets(int samples, int32_t* xy);
int ofx_render_raster_ms(const int32_t* faces, const int64_t* offs, int batch, int64_t total_verts, int64_t total_faces,
                         int64_t max_faces, int views, int size, int samples, const int32_t* sxy, const double* depth,
                         int64_t big_px, uint64_t* keys, int32_t* dropped, void* ws, void* stream);
int ofx_render_shade_ms(const float* verts, const int32_t* faces, const int64_t* offs, int batch, const double* norm,
                        const double* cam, int views, int size, int samples, double tan_half_fov, const uint64_t* keys,
                        const double* params, uint8_t* image, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OFX_H_ */
