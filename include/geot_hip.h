/*
 * geot_hip.h -- C ABI of libgeot_hip.so, the MI355X (gfx950) implementation of
 * GeoT's point-cloud sampling / grouping / interpolation hot path.
 *
 * Every entry point is a plain launcher: device pointers, sizes and a HIP
 * stream handle in, hipError_t (as int, 0 == hipSuccess) out.  No torch types,
 * no allocation, no host synchronisation, never exit(): safe to call from any
 * thread and to capture into a hipGraph.  `stream` is a hipStream_t passed as
 * void* (NULL = the legacy default stream).
 *
 * Each declaration cites the reference launcher / binding it replaces
 * (paths relative to the GeoT checkout).  Layouts: fp32 and int32 only, all
 * tensors contiguous, exactly as the reference's extensions require
 * (SURVEY.md section 8b).  Accumulating outputs (`*_grad`, FPS `temp`) must
 * arrive pre-filled (0 / 1e10) as in the reference; all other outputs are
 * written in full, so they may arrive uninitialised.
 *
 * Distances are un-contracted IEEE fp32, ((dx*dx)+(dy*dy))+(dz*dz), so integer
 * results are bit-identical to the CPU oracle (oracle/geot_oracle.c).
 */
#ifndef GEOT_HIP_H
#define GEOT_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define GEOT_ABI_VERSION 37
#define GEOT_KNN_KMAX_HEAP 1024    /* largest nsample of geot_knnquery_heap / geot_knnquery_heap_ws */
#define GEOT_KNN_KMAX_SORTED 4096  /* largest k of geot_knn_sorted / geot_knn_sorted_ws */
#define GEOT_NTM_MAX_C 32   /* largest class count of the geot_ntm_* entry points */
#define GEOT_CURVATURE_MAX_SCAN 16777216    /* geot_mesh_angle_defects / geot_scan_ball_sum: the most vertices of one scan (2^24) */
#define GEOT_MESH_NEIGHBOURS_LANE_ROW 64   /* geot_mesh_neighbours: the longest raw row (two entries per face at the vertex) one lane tidies */

/* ABI version / diagnostics. */
int geot_abi_version(void);
/* Which squared-distance arithmetic this build of the library uses (all index-producing ops):
 * 0 = un-contracted IEEE fp32 ((dx*dx)+(dy*dy))+(dz*dz) (default, libgeot_hip.so);
 * 1 = fma(dz,dz,fma(dy,dy,dx*dx)) (libgeot_hip_fma.so); 2 = fma(dz,dz,fma(dx,dx,dy*dy)) (libgeot_hip_fma_xy.so):
 * the two contractions nvcc -fmad=true may have made of the reference's source. */
int geot_distance_mode(void);
const char *geot_error_string(int hip_error);

/* ---- furthest point sampling -------------------------------------------
 * Dense batch.  Replaces
 *   pointnet2/_ext_src/src/sampling_gpu.cu:178-232 furthest_point_sampling_kernel_wrapper
 *     (bound as furthest_point_sampling, sampling.cpp:67-88): block_cap=512, skip_origin=1
 *   openpoints/cpp/pointnet2_batch/src/sampling_gpu.cu:218-260 (bound as
 *     furthest_point_sampling_wrapper, sampling.cpp:39-48):          block_cap=1024, skip_origin=0
 * xyz (b,n,3); temp (b,n) in/out, pre-filled 1e10; idxs (b,m) out.
 * block_cap selects the reference thread-block size whose reduction order
 * defines the tie rule; it is not our launch geometry. */
int geot_furthest_point_sampling(int b, int n, int m, const float *xyz, float *temp, int *idxs,
                                 int block_cap, int skip_origin, void *stream);

/* Offset-batched, optionally weighted.  Replaces
 *   pointops/src/sampling/sampling_cuda_kernel.cu:131-171 furthestsampling_cuda_launcher
 *   pointops/src/sampling/sampling_cuda_kernel.cu:309-349 furthestsampling_weights_cuda_launcher
 *   (declared extern "C" in pointops/src/sampling/sampling_cuda_kernel.h:9-29).
 * xyz (n_total,3); offset/new_offset (b) int32 inclusive prefix sums (device);
 * weights (n_total) or NULL; tmp (n_total) in/out, pre-filled 1e10;
 * idx (new_offset[b-1]) out, global indices.  n_max = largest segment. */
int geot_furthestsampling_offset(int b, int n_max, const float *xyz, const int *offset,
                                 const int *new_offset, const float *weights, float *tmp,
                                 int *idx, void *stream);

/* ---- gather ---------------------------------------------------------------
 * pointnet2/_ext_src/src/sampling_gpu.cu:25-33, 52-60
 * openpoints/cpp/pointnet2_batch/src/sampling_gpu.cu (gather_points_kernel_launcher_fast, _grad_) */
int geot_gather_points(int b, int c, int n, int m, const float *points, const int *idx, float *out,
                       void *stream);
int geot_gather_points_grad(int b, int c, int n, int m, const float *grad_out, const int *idx,
                            float *grad_points, void *stream);
/* The same gradient without float atomics (one writer per element, bit-reproducible): see geot_group_points_grad_ws.
 * workspace: geot_scatter_grad_ws_floats(b, c, n, m, 1, 0) floats of scratch. */
int geot_gather_points_grad_ws(int b, int c, int n, int m, const float *grad_out, const int *idx,
                               float *grad_points, float *workspace, void *stream);
/* Host-only (ABI 28): the form geot_gather_points, geot_group_points, geot_three_interpolate and
 * geot_three_interpolate_into launch for a table of m_table floats per (batch, channel) row and n_out_elems output
 * elements per row (m; npoints * nsample; n) -- 0 = nothing to launch, 1 = the plain register gather, 2 = the
 * table-in-LDS gather -- under the same GEOT_GATHER_IMPL as the launches and from the planner the four launchers call.
 * For 2, out receives the first n_out of: channels per workgroup, channel chunks, slices, elements per slice, LDS
 * bytes.  out is a HOST array. */
int geot_gather_plan(int b, int c, int m_table, long long n_out_elems, long long *out, int n_out);

/* ---- ball query -------------------------------------------------------------
 * pointnet2/_ext_src/src/ball_query_gpu.cu:49-57 query_ball_point_kernel_wrapper
 * openpoints/cpp/pointnet2_batch/src/ball_query_gpu.cu (ball_query_kernel_launcher_fast)
 * new_xyz (b,m,3), xyz (b,n,3) -> idx (b,m,nsample); written in full. */
int geot_ball_query(int b, int n, int m, float radius, int nsample, const float *new_xyz,
                    const float *xyz, int *idx, void *stream);
/* openpoints/cpp/pointops/src/ballquery/ballquery_cuda_kernel.cu:80-88 ballquery_launcher.
 * b = number of batch segments in offset/new_offset (the reference scans for it). */
int geot_ballquery_offset(int b, int m, float radius, int nsample, const float *xyz,
                          const float *new_xyz, const int *offset, const int *new_offset, int *idx,
                          void *stream);

/* ---- group (channels-first) -------------------------------------------------
 * pointnet2/_ext_src/src/group_points_gpu.cu:33-42, 69-78
 * openpoints/cpp/pointnet2_batch/src/group_points_gpu.cu (…_launcher_fast) */
int geot_group_points(int b, int c, int n, int npoints, int nsample, const float *points,
                      const int *idx, float *out, void *stream);
int geot_group_points_grad(int b, int c, int n, int npoints, int nsample, const float *grad_out,
                           const int *idx, float *grad_points, void *stream);

/* Same result as geot_group_points_grad / geot_three_interpolate_grad (up to fp32 summation order) WITHOUT float
 * atomics (geot_amd/csrc/tile_scatter.hip): the pairs of every tile of sources are sorted by target once per call, a
 * workgroup keeps the sums of (batch, 4 channels) x all targets in LDS and streams grad_out through it -- grad_out is
 * read once, every output element has one writer and one summation order: bit-reproducible, 3-4x faster.
 * workspace: geot_scatter_grad_ws_floats(b, c, targets, sources, slots, weighted) floats; contents irrelevant unless
 * geot_grad_ws_needs_zero says 1 (shapes the sorted form does not take -- more than 32768 targets per cloud -- fall
 * back to a channels-last atomic accumulation in the workspace, which must then arrive zero-filled). */
long long geot_scatter_grad_ws_floats(int b, int c, int m_targets, long long n_sources, int slots_per_source,
                                      int weighted);
int geot_group_points_grad_ws(int b, int c, int n, int npoints, int nsample, const float *grad_out,
                              const int *idx, float *grad_points, float *workspace, void *stream);
/* 0 when the *_grad_ws entry points only use their workspace as scratch for these sizes (gradient as a
 * gather over a reverse index), 1 when they accumulate in it and it must arrive zero-filled.  The answer is the form
 * the launch takes: query and launch share one planner that knows every limit of the two sorted forms.  A sorted form
 * that is still refused at launch (a workspace that is not 8-byte aligned, an LDS grant the device denies) falls back
 * to the accumulation, which then clears the workspace itself. */
int geot_grad_ws_needs_zero(int b, int c, int m_targets, long long n_sources, int slots_per_source);
/* Host-only (ABI 8): the form the *_grad_ws / _grad_out / _grad_from entry points take for these sizes -- 1 = the sorted
 * pair stream (tiles), 2 = the whole-row list walk (csr), 3 = the channels-last scatter with float atomics in the
 * workspace, 0 = nothing to launch -- under the same GEOT_GATHER_IMPL as the launches, and the form that is launched
 * (one dispatcher switches on this answer).  For 1, out receives the first
 * n_out of: channels per workgroup, sources per tile, tiles, pairs per tile, entry slots per tile, LDS bytes of the
 * scatter, LDS bytes of the sort, workspace words.  out is a HOST array. */
int geot_scatter_grad_plan(int b, int c, int m_targets, long long n_sources, int slots_per_source, int weighted,
                           long long *out, int n_out);
int geot_three_interpolate_grad_ws(int b, int c, int n, int m, const float *grad_out, const int *idx,
                                   const float *weight, float *grad_points, float *workspace,
                                   void *stream);
/* As geot_three_interpolate_grad_ws, for a grad_points (and a workspace) that arrive UNINITIALISED: every element
 * of grad_points is written.  Where one thread owns an output element (the reverse-index gather) the result is
 * stored instead of added: no zero-fill pass and no read of the old value, 12 % of the op at (8, 1536, 24000 ->
 * 8192).  Replaces the torch.zeros + accumulate of pointnet2_utils.py:147-165's backward. */
int geot_three_interpolate_grad_out(int b, int c, int n, int m, const float *grad_out, const int *idx,
                                    const float *weight, float *grad_points, float *workspace, void *stream);
/* PointnetFPModule front end (pointnet2/pointnet2_modules.py:619-626; openpoints' three_interpolation is the same
 * chain) without its temporaries.  geot_fp_weights: the inverse-distance weights from three_nn's SQUARED
 * distances, weight = r / ((r0 + r1) + r2), r = 1 / (sqrt(d2) + 1e-8), in one launch.  _into / _grad_from: the
 * interpolation writes (reads its gradient from) the first c channels of the wider (B, c + c_skip, n) tensor
 * that `torch.cat([interpolated, unknow_feats], dim=1)` would build; *_bstride = floats between batches there
 * (>= c * n).  Workspace of _grad_from as for _grad_ws. */
int geot_fp_weights(int b, int n, const float *dist2, float *weight, void *stream);
int geot_three_interpolate_into(int b, int c, int m, int n, const float *points, const int *idx,
                                const float *weight, float *out, long long out_bstride, void *stream);
int geot_three_interpolate_grad_from(int b, int c, int n, int m, const float *grad_out, long long grad_bstride,
                                     const int *idx, const float *weight, float *grad_points, float *workspace,
                                     void *stream);

/* Grid-accelerated variants of geot_knn_sorted / geot_three_nn (geot_amd/csrc/knn_grid.hip): identical
 * outputs, bit for bit, but only the cells around each query are visited (exact: the search widens until
 * the k-th distance is strictly inside the visited block).  workspace = geot_knn_grid_ws_bytes(b, nr)
 * bytes of 16-byte-aligned scratch (contents irrelevant on entry).  Falls back to the brute-force kernel
 * when workspace is NULL / too small or geot_knn_grid_eligible(b, nq, nr, k) is 0 (small problems, k > 64,
 * or GEOT_NN_IMPL=basic|wave in the environment; GEOT_NN_IMPL=grid forces the grid where it is valid).  A workspace
 * that would be used but is not 16-byte aligned is refused with hipErrorInvalidValue, nothing written (all three). */
long long geot_knn_grid_ws_bytes(int b, int nr);
/* geot_ball_query through the same grid (cells of edge >= 1.0001 radius; identical output). */
int geot_ball_grid_eligible(int b, int n, int m, float radius, int nsample);
int geot_ball_query_ws(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz,
                       int *idx, void *workspace, long long ws_bytes, void *stream);
int geot_knn_grid_eligible(int b, int nq, int nr, int k);
int geot_knn_sorted_ws(int b, int nq, int nr, int k, const float *query, const float *ref, int *idx,
                       float *dist2, void *workspace, long long ws_bytes, void *stream);
/* Host-only (ABI 18): the constants the grid searches run with, for tests that place inputs on either side of every
 * in-kernel branch.  Each returns 1 and fills the first n_out entries of its list when the matching *_eligible call
 * is 1, and returns 0 and leaves out alone otherwise; no kernel is started.  out is a HOST array.
 * geot_knn_grid_plan (up to 7): cells per axis aimed at, G = floor(sqrt(3 nr / (5 k))) clamped to 1..32; the most
 * cells per axis (32, also the grid of geot_spatial_order); the 64-record register slots of the threshold-select fast
 * path; the smallest and the largest k that take it; queries (waves) per workgroup; the largest cell whose points
 * geot_spatial_order returns in ascending index.
 * geot_ball_grid_plan (up to 3): the most cells per axis; the register slots; queries per workgroup.  The cell edge
 * is the cloud's largest extent / floor(extent / (1.0001f * radius)) cells, 1..32 of them per axis. */
int geot_knn_grid_plan(int b, int nq, int nr, int k, long long *out, int n_out);
int geot_ball_grid_plan(int b, int n, int m, float radius, int nsample, long long *out, int n_out);
int geot_three_nn_ws(int b, int n, int m, const float *unknown, const float *known, float *dist2, int *idx,
                     void *workspace, long long ws_bytes, void *stream);

/* BatchNorm (+ ReLU) on channels-first (b, c, l) tensors as streaming passes -- the conv1x1 -> BatchNorm -> ReLU
 * stages of SharedMLP (pointnet2/pytorch_utils.py:8-117) and of the mini-PointNet Encoder (transformer.py:106-136) in
 * training mode.  The O(c) arithmetic between the passes (mean / variance / running statistics / SyncBatchNorm's
 * all-reduce) is the caller's (geot_amd/fused_norm.py).
 *   geot_bn_slices      S = number of slices a row is cut into for the partial sums (<= 32)
 *   geot_bn_stats       partial (b,c,S,2) = per-slice (sum x, sum x^2)
 *   geot_bn_apply       out = x * scale[c] + shift[c], clamped at 0 when relu
 *   geot_bn_bwd_reduce  partial (b,c,S,2) = (sum g, sum g xhat), g = dz masked by [x*scale+shift > 0] when relu,
 *                       xhat = (x - mean[c]) * rstd[c]
 *   geot_bn_bwd_apply   dx = k0[c] * (g - c1[c] - xhat * c2[c])
 * and the PointnetFPModule front end (pointnet2_modules.py:619-640) with the first 1x1 convolution moved in front of
 * the interpolation:  y (b,c,n) = sum_t weight[.,t] A[:, idx[.,t]] + Wb (c,cs) skip (b,cs,n),  A (b,c,m) = W_a
 * known_feats from the caller's GEMM, cs <= 8; partial (b,c,S',2) = per-slice (sum y, sum y^2) for the BatchNorm
 * behind it (S' = geot_fp_front_slices).  Rows of A must fit the LDS (m <= 36864). */
/* The O(c) arithmetic between the passes as launches of its own (13 and 7 torch launches per layer otherwise:
 * 2.5 % of the configs[2] step), split where SyncBatchNorm all-reduces:
 *   geot_bn_sums      sums (c,2) fp64 = sum over b and S of partial (b,c,S,2), fixed order
 *   geot_bn_finalize  n = count_dev ? *count_dev (device double: the all-reduced element count) : count;
 *                     mean = sums0/n, var = max(sums1/n - mean^2, 0) in fp64; mean, rstd = 1/sqrt(var+eps) as fp32;
 *                     scale = gamma*rstd, shift = beta - mean*scale (gamma / beta NULL: 1 / 0); running_mean / _var
 *                     (NULL: not tracked) <- (1-eaf)*old + eaf*(mean | var*n/max(n-1,1))  (torch batch_norm semantics);
 *                     pre_bias (NULL: none): the statistics are those of y while the layer normalises y + pre_bias[c]
 *                     (a convolution bias in front of a batch-statistics BatchNorm cancels in the output: the caller
 *                     skips the add, only the running mean sees it)
 *   geot_bn_bwd_coef  g_beta, g_gamma = fp32 of local_sums (this rank's sum g, sum g xhat); c1, c2 = sums/n (0 if n == 0) */
int geot_bn_sums(int b, int c, int s, const float *partial, double *sums, void *stream);
/* geot_bn_stats and geot_fp_front write statistics records (b,c,S,4) = (s1, s2, pivot, count): sums of (x - pivot) and
 * (x - pivot)^2 around the slice's first element, so that |mean| >> std costs no digits; geot_bn_sums_shifted turns every
 * record back into (sum x, sum x^2) in fp64 and adds them: sums (c,2).  (geot_bn_sums: the plain (b,c,S,2) partials of
 * the backward reduce.) */
int geot_bn_sums_shifted(int b, int c, int s, const float *partial, double *sums, void *stream);
int geot_bn_finalize(int c, const double *sums, double count, const double *count_dev, double eps, double eaf,
                     const float *gamma, const float *beta, const float *pre_bias, float *running_mean,
                     float *running_var, float *mean, float *rstd, float *scale, float *shift, void *stream);
int geot_bn_bwd_coef(int c, const double *local_sums, const double *sums, double count, const double *count_dev,
                     float *g_gamma, float *g_beta, float *c1, float *c2, void *stream);
int geot_bn_slices(int b, int c, int l);
int geot_bn_stats(int b, int c, int l, const float *x, float *partial, void *stream);
int geot_bn_apply(int b, int c, int l, int relu, const float *x, const float *scale, const float *shift, float *out,
                  void *stream);
int geot_bn_bwd_reduce(int b, int c, int l, int relu, const float *x, const float *dz, const float *scale,
                       const float *shift, const float *mean, const float *rstd, float *partial, void *stream);
int geot_bn_bwd_apply(int b, int c, int l, int relu, const float *x, const float *dz, const float *scale,
                      const float *shift, const float *mean, const float *rstd, const float *k0, const float *c1,
                      const float *c2, float *dx, void *stream);
/* The same four passes over x + seg[.., e / n]: x (b,c,l) with l = G n columns in G segments of n, seg (b,c,G) a
 * per-(channel, segment) addend that is never added in memory (the Encoder's W_g pooled in front of its second
 * BatchNorm).  4 <= n <= 256, n % 4 == 0, l % n == 0, every tensor 16-byte aligned; S = geot_bn_slices(b,c,l), a slice
 * boundary may fall inside a segment.
 *   geot_bn_stats_seg       the (s1, s2, pivot, count) records of x + seg, as geot_bn_stats
 *   geot_bn_apply_seg       out = act((x + seg) * scale[c] + shift[c])
 *   geot_bn_bwd_reduce_seg  partial (b,c,S,2) fp64 = (sum g, sum g xhat) carried in fp64 from the first add, mask and xhat
 *                           from x + seg; geot_bn_sums_f64 adds them up as geot_bn_sums does the fp32 ones
 *   geot_bn_bwd_apply_seg   dx as geot_bn_bwd_apply, and dseg (b,c,G) = the sum of dx over each segment (one writer per
 *                           element, fixed order) */
int geot_bn_stats_seg(int b, int c, int l, int n, const float *x, const float *seg, float *partial, void *stream);
int geot_bn_apply_seg(int b, int c, int l, int n, int relu, const float *x, const float *seg, const float *scale,
                      const float *shift, float *out, void *stream);
int geot_bn_bwd_reduce_seg(int b, int c, int l, int n, int relu, const float *x, const float *seg, const float *dz,
                           const float *scale, const float *shift, const float *mean, const float *rstd, double *partial,
                           void *stream);
int geot_bn_sums_f64(int b, int c, int s, const double *partial, double *sums, void *stream);
int geot_bn_bwd_apply_seg(int b, int c, int l, int n, int relu, const float *x, const float *seg, const float *dz,
                          const float *scale, const float *shift, const float *mean, const float *rstd, const float *k0,
                          const float *c1, const float *c2, float *dx, float *dseg, void *stream);
/* relu(bn(W x)) for a thin first stage, x (j,l) with j <= 8 input rows, W (c,j): y = W x is never stored (the Encoder's
 * Conv1d(3, 128) -> BatchNorm -> ReLU).  y[c][e] = the fp64 dot product w[c] . x[:, e] rounded to fp32, by one device
 * function in every kernel that forms it, so forward and backward agree on every sign.
 *   geot_thin_moments        partial (S, j + j j) fp64 per slice of columns (S = geot_thin_moments_slices(l)): sums of
 *                            x' = x - p and of x' x'^T about the pivot p = x's first column
 *   geot_thin_bn_sums        mom (2 j + j j) fp64 = p, sum x', sum x' x'^T over all slices; sums (c,2) fp64 = (sum y,
 *                            sum y^2) rebuilt from w mom about q = w p, the input of geot_bn_finalize
 *   geot_thin_bn_apply       out (c,l) = act((y - mean[c]) * scale[c] + beta[c])
 *   geot_thin_bn_bwd_reduce  partial (c, S', 2 + j) fp64 = per slice (S' = geot_thin_bn_bwd_slices(c,l)) sum g, sum g xhat,
 *                            sum g x_j (all carried in fp64), g = dz masked by [(y - mean) scale + beta > 0] when relu; xhat of
 *                            the sums from the unrounded y, about the exact mean w (p + sum x' / l) when mom is given
 *                            (the statistics were this rank's alone), else (NULL) about mean[c]
 *   geot_thin_bn_bwd_sums    local (c,2) fp64 = sum g, sum g xhat (the input of geot_bn_bwd_coef); gx (c,j) fp64 = sum g x_j
 *   geot_thin_bn_wgrad       dw (c,j) = scale[c] (gx - c1[c] sum x_j - c2[c] sum xhat x_j) in fp64: c1, c2 = sums / n, sums
 *                            (c,2) fp64 = the (all-reduced) sum g, sum g xhat, n = count_dev ? *count_dev : count; the
 *                            sums over x from mom; xhat about the exact mean w (p + sum x' / l) when local_mean (the
 *                            statistics were this rank's alone), else about mean[c].  mom NULL or n == 0 (running
 *                            statistics): dw = scale gx */
int geot_thin_moments_slices(int l);
int geot_thin_moments(int j, int l, const float *x, double *partial, void *stream);
int geot_thin_bn_sums(int c, int j, int l, int s, const double *partial, const float *w, const float *x, double *mom,
                      double *sums, void *stream);
int geot_thin_bn_apply(int c, int j, int l, int relu, const float *w, const float *x, const float *mean, const float *scale,
                       const float *beta, float *out, void *stream);
int geot_thin_bn_bwd_slices(int c, int l);
int geot_thin_bn_bwd_reduce(int c, int j, int l, int relu, const double *mom, const float *w, const float *x, const float *dz,
                            const float *scale, const float *beta, const float *mean, const float *rstd, double *partial,
                            void *stream);
int geot_thin_bn_bwd_sums(int c, int j, int s, const double *partial, double *local, double *gx, void *stream);
int geot_thin_bn_wgrad(int c, int j, int l, int local_mean, const float *w, const double *mom, const double *gx,
                       const double *sums, double count, const double *count_dev, const float *scale, const float *mean,
                       const float *rstd, float *dw, void *stream);
/* Residual add + LayerNorm of the transformer blocks (transformer.py:41-104: x + drop_path(branch), then norm; the
 * position embedding added between blocks, :395-400) as one pass each way over row-major (rows, c) tensors,
 * c in {128, 256, 384, 512, 768, 1024} (geot_res_ln_supported):
 *   t = x + s[row / rows_per_sample] * y + extra   (y, s, extra may be NULL; s needs y),  z = LayerNorm(t; gamma, beta, eps)
 *   geot_res_ln       writes t (t_out NULL: not wanted), z, and the per-row mean / rstd
 *   geot_res_ln_grad  g = gt + LayerNorm'(gz) (gt / gz NULL: zero) = the gradient of x and of extra; gy_out (NULL: not
 *                     wanted) = s * g = the gradient of y; d gamma, d beta;  workspace: geot_res_ln_ws_floats floats. */
int geot_res_ln_supported(int c);
long long geot_res_ln_ws_floats(int rows, int c);
int geot_res_ln(int rows, int c, int rows_per_sample, float eps, const float *x, const float *y, const float *s,
                const float *extra, const float *gamma, const float *beta, float *t_out, float *z_out, float *mean,
                float *rstd, void *stream);
int geot_res_ln_grad(int rows, int c, int rows_per_sample, const float *gz, const float *gt, const float *t,
                     const float *mean, const float *rstd, const float *gamma, const float *s, float *g_out, float *gy_out,
                     float *dgamma, float *dbeta, float *workspace, void *stream);
/* Attention head split (transformer.py:70-72): the (b, n, 3, h, d) qkv projection -> out (3, b*h, n, d) = (q * scale, k,
 * v) contiguous for the batched GEMMs, d a multiple of 4; _grad: three (b*h, n, d) gradients (NULL: zero) back into
 * the (b, n, 3, h, d) gradient with d q scaled -- one launch each instead of a stack, a permuted copy and an
 * element-wise pass over the (b, h, n, n) score gradient.  Every pointer given (qkv, out; gq, gk, gv, grad_qkv) must be
 * 16-byte aligned: hipErrorInvalidValue otherwise. */
int geot_qkv_split(int b, int n, int h, int d, float scale, const float *qkv, float *out, void *stream);
int geot_qkv_split_grad(int b, int n, int h, int d, float scale, const float *gq, const float *gk, const float *gv,
                        float *grad_qkv, void *stream);
/* Gradient of a soft-max over the last dimension n in {64, 128, 256, 512, 1024} of row-major (rows, n): grad_in = y * (grad -
 * sum_j grad_j y_j) in one pass (the attention scores of transformer.py:75-77; torch runs grad * y as a pass of its own). */
int geot_softmax_grad(long long rows, int n, const float *grad, const float *y, float *grad_in, void *stream);
/* Poly-1 focal loss (openpoints/loss/build.py:183-258 Poly1FocalLoss; :799-892 Poly1FocalLoss_U_corr when `keep` is
 * given) on logits (b, c, n) with int64 class labels (b, n) -- no one-hot tensors, two launches forward, one backward:
 *   l = at * BCEwithlogits(x, y) * (1 - pt)^gamma + epsilon * (1 - pt)^(gamma + 1),  y = [label == c], pt = y p + (1-y)(1-p),
 *   at = alpha y + (1 - alpha)(1 - y) (alpha < 0: 1);  out2[0] = sum l / (b c n), or with keep (b, n) bytes:
 *   sum l keep / (c sum keep + 0.001);  out2[1] = 1 / that denominator (for _grad).  workspace: _ws_doubles doubles.
 *   _grad: grad_logits = upstream[0] * out2[1] * keep * dl/dx  (upstream: device scalar). */
long long geot_poly1_focal_ws_doubles(int b, int c, int n);
int geot_poly1_focal(int b, int c, int n, float alpha, float gamma, float epsilon, const float *logits,
                     const long long *labels, const unsigned char *keep, double *workspace, float *out2, void *stream);
int geot_poly1_focal_grad(int b, int c, int n, float alpha, float gamma, float epsilon, const float *logits,
                          const long long *labels, const unsigned char *keep, const float *out2, const float *upstream,
                          float *grad_logits, void *stream);
/* Class-weighted soft-max cross-entropy (ABI 17; openpoints/loss/build.py:913-925 Weight_CELoss, :928-938 Weight_CELoss_U
 * when `conf` is given) on logits (b, c, n), 1 <= c <= GEOT_NTM_MAX_C, with int64 labels (b, n) and class_weights (bw, c):
 *   w = mean over the bw rows (a sequential fp32 sum, one division);  per point  -w[y] * log_softmax(x)[y];
 *   out2[0] = sum / (b n) -- ignored points count in the denominator, the weights do not;  out2[1] = 1 / (b n).
 *   conf (b, n) fp32 (may be NULL): the point is ignored when !(conf >= thresh) (NaN: ignored), when y == 0 and when y == 255.
 *   Any other label outside [0, c) makes the loss NaN.  workspace: _ws_doubles doubles.  No atomics: the same bits every call.
 *   _grad: grad_logits = upstream[0] * out2[1] * w[y] * (softmax - onehot), exactly 0 at ignored points, written in full. */
long long geot_weighted_ce_ws_doubles(int b, int c, int n);
int geot_weighted_ce(int b, int c, int n, int bw, float thresh, const float *logits, const long long *labels,
                     const float *class_weights, const float *conf, double *workspace, float *out2, void *stream);
int geot_weighted_ce_grad(int b, int c, int n, int bw, float thresh, const float *logits, const long long *labels,
                          const float *class_weights, const float *conf, const float *out2, const float *upstream,
                          float *grad_logits, void *stream);
/* Poly-1 focal loss with a per-point factor (ABI 17; openpoints/loss/build.py:564-688 Poly1FocalLoss_U_T): l as in
 * geot_poly1_focal, beta[b,n] = conf[b,n] / t[b, y[b,n], n] with t (b, c, n) a second logits tensor, keep (b, n) bytes:
 *   out2[0] = sum l * beta * keep / (c sum keep + 0.001);  out2[1] = 1 / that denominator.  workspace: as geot_poly1_focal.
 *   _grad: grad_logits = upstream[0] * out2[1] * keep * beta * dl/dx;
 *          grad_t[b,c,n] = [c == y] * upstream[0] * out2[1] * keep * (-conf / t^2) * sum_c' l(x[b,c',n]);
 *   both written in full (0 where keep is 0 and, for grad_t, off the label channel). */
int geot_poly1_focal_beta(int b, int c, int n, float alpha, float gamma, float epsilon, const float *logits,
                          const long long *labels, const unsigned char *keep, const float *conf, const float *t,
                          double *workspace, float *out2, void *stream);
int geot_poly1_focal_beta_grad(int b, int c, int n, float alpha, float gamma, float epsilon, const float *logits,
                               const long long *labels, const unsigned char *keep, const float *conf, const float *t,
                               const float *out2, const float *upstream, float *grad_logits, float *grad_t, void *stream);
/* max over the n innermost elements of every row, x (rows, n) contiguous and 16-byte aligned, n a multiple of 4, <= 256:
 * out (rows), arg (rows) uint8 = the first maximum's slot (torch.max semantics); _grad writes dx (rows, n) in full.
 * (Encoder's max over a group's points, transformer.py:127-134; max over nsample of the SA modules.) */
int geot_segment_max(long long rows, int n, const float *x, float *out, unsigned char *arg, void *stream);
/* BatchNorm -> ReLU -> max over the n innermost elements of y (b, c, groups, n) without building the normalised tensor
 * (the last SharedMLP stage + max_pool2d of a SetAbstraction module in training mode, pointnet2_modules.py:57-66): the
 * affine map is monotone, so out = relu(scale_c sel + shift_c) with sel = the row's maximum (scale_c >= 0) or minimum;
 * sel and arg (slot of the first extremum) are kept for _grad:  dx_j = k0_c ([j == arg] gm - c1_c - xhat_j c2_c),
 * gm (b, c, groups) = the pooled output's gradient where the pre-activation was positive, c1 / c2 = the means of the
 * (sparse) gradient and of gradient * xhat (caller: geot_amd/fused_norm.py bn_relu_max).  n as geot_segment_max. */
int geot_bn_pool(int b, int c, int groups, int n, int relu, const float *y, const float *scale, const float *shift, float *out,
                 float *sel, unsigned char *arg, void *stream);
int geot_bn_pool_grad(int b, int c, int groups, int n, const float *y, const float *gm, const unsigned char *arg,
                      const float *mean, const float *rstd, const float *k0, const float *c1, const float *c2, float *dx,
                      void *stream);
/* out (rows) = the sum of every row, same shape rules: the gradient of a per-group term broadcast over the group's
 * points (Encoder, transformer.py:131-132: feature_global expanded over n) at streaming speed, fixed summation order. */
int geot_segment_sum(long long rows, int n, const float *x, float *out, void *stream);
/* out[r] (fp64) = sum of the n floats of row r, fixed order: the long few-row sums (1x1-conv bias gradients over (B, C, N),
 * per-channel input sums) without the semaphore memset torch's reduction issues (a memset node under capture). */
int geot_rowsum_f64(long long rows, int n, const float *x, double *out, void *stream);
/* partial (rows, S, j) = per-slice sums of a[row][.] * b[jj][.] for a (rows, l), b (j, l), j <= 8, S =
 * geot_rowdot_small_slices(rows, l): the weight gradient of a 1x1 convolution with a handful of input channels
 * (Encoder first_conv, transformer.py:110: Conv1d(3, 128) over all points of all groups), one streaming pass. */
/* out (cols) = column sums of the row-major x (rows, cols): the bias gradient of a Linear layer (fixed summation order;
 * workspace: geot_colsum_ws_floats floats). */
long long geot_colsum_ws_floats(int rows, int cols);
int geot_colsum(int rows, int cols, const float *x, float *out, float *workspace, void *stream);
int geot_rowdot_small_slices(int rows, int l);
int geot_rowdot_small(int rows, int l, int j, const float *a, const float *b, float *partial, void *stream);
int geot_segment_max_grad(long long rows, int n, const float *dy, const unsigned char *arg, float *dx, void *stream);
/* The backward of  out = max over every group's n columns of (W x)  from the max's sparse gradient (ABI 35,
 * csrc/max_conv.hip; Encoder, transformer.py:113 and :123-126: the 1x1 convolutions in front of the two group maxima):
 * W (co, ci), x (ci, g n) with group k owning columns k n .. k n + n - 1, dout (co, g) the gradient of out, arg (co, g) as
 * geot_segment_max wrote it for y = W x viewed (co, g, n).  All fp32, contiguous.
 *   _dgrad   dx (ci, g n):  dx[c, k n + j] = sum over the o with arg[o, k] == j of dout[o, k] W[o, c], ascending o;
 *            every element written exactly once, zeros included.
 *   _wgrad   dW (co, ci):   dW[o, c] = sum over k of dout[o, k] x[c, k n + arg[o, k]]: chunks of groups leave fp32
 *            partial sums in ws (geot_maxconv_ws_floats(co, ci, g, n) floats, contents on entry irrelevant), a finish
 *            kernel adds the chunks in ascending order in fp64 and rounds once.  The chunking depends on the shapes alone
 *            (GEOT_MAXCONV_CHUNK=<groups per chunk>, read per call by both, pins it for tests).
 * No float atomics, kernel launches only, bit-identical from call to call.  hipErrorNotSupported (nothing launched) unless
 * co <= 1024, ci % 4 == 0, 4 <= n <= 256, n % 4 == 0 and W, x, dx, ws, dW are 16-byte aligned; _ws_floats: -1. */
int geot_maxconv_dgrad(int co, int ci, int g, int n, const float *W, const float *dout, const unsigned char *arg, float *dx,
                       void *stream);
long long geot_maxconv_ws_floats(int co, int ci, int g, int n);
int geot_maxconv_wgrad(int co, int ci, int g, int n, const float *x, const float *dout, const unsigned char *arg, float *ws,
                       float *dW, void *stream);
int geot_fp_front_slices(int b, int c, int m, int n);
int geot_fp_front(int b, int c, int m, int n, int cs, const float *A, const int *idx, const float *weight,
                  const float *skip, const float *Wb, float *y, float *partial, void *stream);

/* ---- the same FP front end and its BatchNorm on POINT-MAJOR activations (B, N, C), csrc/channels_last.hip ----------
 * Behaviour replaced: three_interpolate + concat + the first Conv2d/BatchNorm2d/ReLU of PointnetFPModule.mlp
 * (pointnet2/pointnet2_modules.py:619-640, pointnet2/_ext_src/src/interpolate_gpu.cu:88-146) and its gradient.
 * A point's C channels are one contiguous row; the 1x1 convolutions on either side are GEMMs and take the layout as a
 * transpose flag, so nothing is transposed in memory.  Needs C % 4 == 0 and C <= 4096 (geot_cl_tiles() >= 0).
 *   geot_cl_tiles(batches, rows_per_batch, c)  rows T of the (T, 2, c) partial-sum buffer of a bn_*_cl reduction over
 *                      batches x rows_per_batch rows;  geot_fp_front_cl_tiles(b, c, n, cs): the same for fp_front_cl
 *   geot_fp_front_cl   y_cl (b,n,c) = sum_t weight[b,e,t] a_cl[b, idx[b,e,t], :] + wb (c,cs) skip (b,cs,n)[:, e];
 *                      partial (T,2,c) = per-tile (sum y, sum y^2); order (b,n) or NULL = the sequence in which a
 *                      workgroup takes its points (values do not depend on it; the partial sums' rounding does)
 *   geot_bn_stats_cl / _apply_cl / _bwd_reduce_cl / _bwd_apply_cl   as geot_bn_* above on (rows, c) row-major
 *   geot_bn_sums_cl    sums (c,2) fp64 = sum over the T tiles of partial (T,2,c), fixed order
 *   geot_rix_build     reverse index of idx (b,L,nt) with values in [0,m): per target the (source, weight) pairs in
 *                      ascending pair order, into ws (geot_rix_ws_ints ints); weight NULL = unit weights; order (b,m)
 *                      or NULL = the sequence in which the gather takes the targets (a permutation per cloud)
 *   geot_gather_rows_csr_cl   out_cl (b,m,c) = sum over the pairs of target j of weight * g_cl[b, source, :]
 *                      (the gradient of a point-major gather; one writer per row, fixed order: reproducible); `order`
 *                      must be the one the index was built with */
int geot_cl_tiles(int batches, long long rows_per_batch, int c);
int geot_fp_front_cl_tiles(int b, int c, int n, int cs);
int geot_fp_front_cl(int b, int c, int m, int n, int cs, const float *a_cl, const int *idx, const float *weight,
                     const float *skip, const float *wb, const int *order, float *y_cl, float *partial, void *stream);
int geot_bn_stats_cl(long long rows, int c, const float *x, float *partial, void *stream);
int geot_bn_apply_cl(long long rows, int c, int relu, const float *x, const float *scale, const float *shift, float *out,
                     void *stream);
int geot_bn_bwd_reduce_cl(long long rows, int c, int relu, const float *x, const float *dz, const float *scale,
                          const float *shift, const float *mean, const float *rstd, float *partial, void *stream);
int geot_bn_bwd_apply_cl(long long rows, int c, int relu, const float *x, const float *dz, const float *scale,
                         const float *shift, const float *mean, const float *rstd, const float *k0, const float *c1,
                         const float *c2, float *dx, void *stream);
int geot_bn_sums_cl(int tiles, int c, const float *partial, double *sums, void *stream);
/* statistics records: fp_front_cl and bn_stats_cl accumulate SHIFTED sums (around each tile's first row) and write
 * (tiles, 3, c) = (s1, s2, pivot) followed by `tiles` row counts = geot_cl_stat_floats(tiles, c) floats;
 * geot_bn_sums_shifted_cl rebuilds (sum x, sum x^2) per tile in fp64 and adds them up: sums (c,2) */
long long geot_cl_stat_floats(int tiles, int c);
int geot_bn_sums_shifted_cl(int tiles, int c, const float *partial, double *sums, void *stream);
long long geot_rix_ws_ints(int b, long long L, int m, int nt);
int geot_rix_build(int b, int L, int m, int nt, const int *idx, const float *weight, const int *order, int *ws,
                   long long ws_ints, void *stream);
int geot_gather_rows_csr_cl(int b, int c, int L, int m, int nt, const float *g_cl, const int *ws, const int *order,
                            float *out_cl, void *stream);
/* The backward of [fp_front_cl -> BatchNorm (+ ReLU)] in two passes instead of four, the gradient gy of the BatchNorm's
 * input never written:  geot_bn_bwd_reduce_skip_cl = geot_bn_bwd_reduce_cl + the sums sum g skip_k, sum xhat skip_k that
 * give grad_wb = sum_e gy_e skip_e once the means are known (partial (T, 2 + 2 cs, c), T = geot_cl_tiles(1, b n, c);
 * geot_bn_sums_k_cl adds the T tiles up: sums (c, K) fp64);  geot_gather_rows_csr_bn_cl = geot_gather_rows_csr_cl of
 * gy = scale (g - c1 - xhat c2), formed on the fly from the rows of y_cl and dz_cl. */
int geot_bn_sums_k_cl(int tiles, int c, int k, const float *partial, double *sums, void *stream);
int geot_bn_bwd_reduce_skip_cl(int b, int n, int c, int cs, int relu, const float *x, const float *dz, const float *scale,
                               const float *shift, const float *mean, const float *rstd, const float *skip, float *partial,
                               void *stream);
/* grad_wb (c, cs) = scale_c (S1 - c1_c S2 - c2_c S3) from sums_k (c, 2 + 2 cs) of the pass above, c1 / c2 of
 * geot_bn_bwd_coef and s2 (cs) fp64 = the sum of every skip channel over all points */
int geot_fp_skip_wgrad_cl(int c, int cs, const double *sums_k, const float *scale, const float *c1, const float *c2,
                          const double *s2, float *gwb, void *stream);
int geot_gather_rows_csr_bn_cl(int b, int c, int L, int m, int nt, int relu, const float *y_cl, const float *dz_cl,
                               const float *scale, const float *shift, const float *mean, const float *rstd, const float *c1,
                               const float *c2, const int *ws, const int *order, float *out_cl, void *stream);

/* EdgeConv tail = the rest of DGCNN_Propagation's layer behind the (linear) 1x1 convolution
 * (openpoints/models/backbone/transformer.py:366-379: Conv2d -> GroupNorm(groups) -> LeakyReLU(slope) ->
 * max over the k neighbours), fused.  With P = W_d x_k (b,c,nk) and Q = (W_q - W_d) x_q (b,c,nq) from the caller's
 * GEMMs, y[b,:,i,j] = P[b,:,idx[b,i,j]] + Q[b,:,i] is the convolution's output; out (b,c,nq) =
 * max_j LeakyReLU(GroupNorm(y)).  The (b,c,nq,k) tensor is never materialised.  Saved for the gradient: ysel
 * (b,c,nq) the selected y, ysum (b,c,nq) = sum_j y, jsel (b,c,nq) uint8 the selected slot, stats (b,groups,2) =
 * (mean, 1/sqrt(var+eps)).  _grad writes grad_p (b,c,nk), grad_q (b,c,nq), grad_gamma (c), grad_beta (c) in full
 * (no atomics: deterministic).  workspace: geot_edgeconv_ws_bytes() bytes of scratch, contents irrelevant.
 * Needs slope >= 0, c % groups == 0, k <= 255, b <= 65535, c <= 65535, b nq k and b nk <= 2^31 - 16, and rows that
 * fit the LDS (nk <= 38400, nq <= 17066): geot_edgeconv_eligible() tells; callers fall back to the composed ops
 * otherwise.  Any alignment of the arrays is taken (16-byte aligned idx with k = 4 takes the int4 index loads). */
int geot_edgeconv_eligible(int b, int c, int nq, int nk, int k, int groups);
long long geot_edgeconv_ws_bytes(int b, int c, int nq, int nk, int k);
/* Host-only (ABI 9): the launch plan of geot_edgeconv_gn_max[_grad[_rix]] for these sizes, from the function the
 * launches use.  Returns 1 and fills the first n_out of: forward channels per workgroup, forward slices, forward LDS
 * bytes, k == 4 instances (1/0), backward-reduce slices, dP channels per workgroup, dP slices, dP LDS bytes, dP lanes
 * per target (log2), floats per forward partial record, floats of the partials area, float offset of the backward's
 * per-group coefficients, byte offset of the reverse index, workspace bytes -- when the shape is eligible; returns 0
 * and leaves out alone otherwise.  out is a HOST array. */
int geot_edgeconv_plan(int b, int c, int nq, int nk, int k, int groups, long long *out, int n_out);
int geot_edgeconv_gn_max(int b, int c, int nq, int nk, int k, int groups, float eps, float slope, const float *P,
                         const float *Q, const int *idx, const float *gamma, const float *beta, float *out,
                         float *ysel, float *ysum, unsigned char *jsel, float *stats, void *workspace,
                         long long ws_bytes, void *stream);
int geot_edgeconv_gn_max_grad(int b, int c, int nq, int nk, int k, int groups, float slope, const float *P,
                              const float *Q, const int *idx, const float *gamma, const float *beta,
                              const float *ysel, const float *ysum, const unsigned char *jsel, const float *stats,
                              const float *grad_out, float *grad_p, float *grad_q, float *grad_gamma,
                              float *grad_beta, void *workspace, long long ws_bytes, void *stream);
/* The gradient's reverse index of idx (pairs grouped by target, ascending pair id) depends on the kNN graph alone:
 * geot_edgeconv_rix_build writes it into `rix` (geot_edgeconv_rix_ints ints) wherever the caller has the graph early;
 * geot_edgeconv_gn_max_grad_rix = geot_edgeconv_gn_max_grad with that index instead of idx (7 launches fewer on the
 * gradient's stream). */
long long geot_edgeconv_rix_ints(int b, int nq, int nk, int k);
int geot_edgeconv_rix_build(int b, int nq, int nk, int k, const int *idx, int *rix, long long rix_ints, void *stream);
int geot_edgeconv_gn_max_grad_rix(int b, int c, int nq, int nk, int k, int groups, float slope, const float *P,
                                  const float *Q, const int *rix, const float *gamma, const float *beta,
                                  const float *ysel, const float *ysum, const unsigned char *jsel, const float *stats,
                                  const float *grad_out, float *grad_p, float *grad_q, float *grad_gamma,
                                  float *grad_beta, void *workspace, long long ws_bytes, void *stream);

/* EdgeConv graph feature = DGCNN_Propagation.get_graph_feature
 * (openpoints/models/backbone/transformer.py:343-364: transpose + fancy-index gather + permute +
 * expand + cat), in one pass:  x_q (b,c,nq), x_k (b,c,nk), idx (b,nq,k) int32 neighbours in x_k ->
 * out (b,2c,nq,k) = cat(x_k[idx] - x_q, x_q).  _grad accumulates into grad_xq (b,c,nq) and grad_xk
 * (b,c,nk); workspace = b*nk*c zero-filled floats. */
int geot_graph_feature(int b, int c, int nq, int nk, int k, const float *x_q, const float *x_k,
                       const int *idx, float *out, void *stream);
int geot_graph_feature_grad(int b, int c, int nq, int nk, int k, const float *grad_out, const int *idx,
                            float *grad_xq, float *grad_xk, float *workspace, void *stream);

/* ---- three_nn / three_interpolate ------------------------------------------
 * pointnet2/_ext_src/src/interpolate_gpu.cu:64-71, 106-115, 148-157
 * openpoints/cpp/pointnet2_batch/src/interpolate_gpu.cu (…_launcher_fast)
 * dist2 holds SQUARED distances (callers take sqrt). */
int geot_three_nn(int b, int n, int m, const float *unknown, const float *known, float *dist2,
                  int *idx, void *stream);
int geot_three_interpolate(int b, int c, int m, int n, const float *points, const int *idx,
                           const float *weight, float *out, void *stream);
int geot_three_interpolate_grad(int b, int c, int n, int m, const float *grad_out, const int *idx,
                                const float *weight, float *grad_points, void *stream);

/* ---- kNN --------------------------------------------------------------------
 * Heap-ordered, offset-batched: pointops/src/knnquery/knnquery_cuda_kernel.cu:111-116
 * knnquery_cuda_launcher (extern "C" in knnquery_cuda_kernel.h:9-17).
 * idx (m,nsample) global indices, dist2 (m,nsample) squared.  0 <= nsample <= GEOT_KNN_KMAX_HEAP (1024; the reference
 * allows 1000), anything else is hipErrorInvalidValue before any launch.  The reference's literal max-heap, one list per
 * lane in LDS: 64 lanes per workgroup up to nsample 128, 32 up to 256, 16 up to 1024 (128 KB). */
int geot_knnquery_heap(int b, int m, int nsample, const float *xyz, const float *new_xyz,
                       const int *offset, const int *new_offset, int *idx, float *dist2,
                       void *stream);
/* Sorted kNN in d <= 32 dimensions (feature_space_loss's neighbours among the 17-dim soft-max vectors,
 * utils/insT_loss.py:19: knn_point = cdist + topk there): query (b,nq,d), ref (b,nr,d), k <= 64; ascending
 * (d2, index); d2 accumulated over the dimensions in order, un-contracted. */
int geot_knn_sorted_nd(int b, int nq, int nr, int d, int k, const float *query, const float *ref, int *idx,
                       float *dist2, void *stream);
/* geot_knnquery_heap for uniform batches (every segment n_per support points, m_per queries, as
 * pointops.knn builds them): sorted (nsample+1)-NN -- from the grid search for nsample <= 63, from the
 * long-list selection kernel of geot_knn_sorted for 64 <= nsample <= GEOT_KNN_KMAX_HEAP, which certifies
 * in its epilogue; queries whose first nsample+1 distances are strictly increasing (and below the heap's
 * 1e10 sentinel) have a unique answer and are written, the rest (ties, too few candidates) go through the
 * literal heap.  Identical output.  workspace: geot_knnquery_heap_ws_bytes, 16-byte aligned; (ABI 11) from nsample
 * 64 on it is 4 * (b * m_per + 4) bytes rounded up to 16, independent of nsample.  Without a (large
 * enough) workspace, or under GEOT_NN_IMPL=basic, the literal heap serves every query. */
long long geot_knnquery_heap_ws_bytes(int b, int n_per, int m_per, int nsample);
int geot_knnquery_heap_ws(int b, int n_per, int m_per, int nsample, const float *xyz, const float *new_xyz,
                          const int *offset, const int *new_offset, int *idx, float *dist2, void *workspace,
                          long long ws_bytes, void *stream);
/* Sorted brute-force kNN: the contract of the un-vendored knn_cuda.KNN
 * (openpoints/models/backbone/transformer.py:280,293,313,353) and of
 * knn_point = cdist + topk (openpoints/models/layers/knn.py:7-20).
 * query (b,nq,3), ref (b,nr,3) -> idx (b,nq,k) int32, dist2 (b,nq,k) squared,
 * ascending by (dist2, index); missing neighbours are (inf, 0).  0 <= k <= GEOT_KNN_KMAX_SORTED (4096),
 * anything else is hipErrorInvalidValue before any launch.  k <= 64: one wave per 4 queries (or the grid
 * search of geot_knn_sorted_ws); 65 <= k <= 4096: one workgroup per query, radix select of the k-th
 * (d2, index) over the distance bits + an LDS bitonic sort, no workspace (GEOT_NN_IMPL=basic keeps the
 * one-lane insertion kernel for k <= 256, for A/B runs). */
int geot_knn_sorted(int b, int nq, int nr, int k, const float *query, const float *ref, int *idx,
                    float *dist2, void *stream);

/* ---- openpoints pointops, channels-last -----
 * openpoints/cpp/pointops/src/{grouping,interpolation,subtraction,aggregation}/…_cuda_kernel.cu */
int geot_grouping_cl(int m, int nsample, int c, const float *input, const int *idx, float *out,
                     void *stream);
int geot_grouping_cl_grad(int m, int nsample, int c, const float *grad_out, const int *idx,
                          float *grad_in, void *stream);
int geot_interpolation_cl(int n, int c, int k, const float *input, const int *idx,
                          const float *weight, float *out, void *stream);
int geot_interpolation_cl_grad(int n, int c, int k, const float *grad_out, const int *idx,
                               const float *weight, float *grad_in, void *stream);
int geot_subtraction_cl(int n, int nsample, int c, const float *in1, const float *in2,
                        const int *idx, float *out, void *stream);
int geot_subtraction_cl_grad(int n, int nsample, int c, const int *idx, const float *grad_out,
                             float *grad_in1, float *grad_in2, void *stream);
int geot_aggregation_cl(int n, int nsample, int c, int w_c, const float *input,
                        const float *position, const float *weight, const int *idx, float *out,
                        void *stream);
int geot_aggregation_cl_grad(int n, int nsample, int c, int w_c, const float *input,
                             const float *position, const float *weight, const int *idx,
                             const float *grad_out, float *grad_in, float *grad_position,
                             float *grad_weight, void *stream);

/* ---- fused SetAbstraction body ---------------
 * Replaces the chain QueryAndGroup (pointnet2/pointnet2_utils.py:343-358: two
 * grouping_operation + centre subtraction + cat) -> SharedMLP
 * (pointnet2/pytorch_utils.py:8-33: 1x1 Conv2d + BatchNorm + ReLU stack) ->
 * max_pool2d over nsample (pointnet2/pointnet2_modules.py:360-363), for inference
 * (BatchNorm folded into the conv by the caller).  fp32 MFMA.
 * xyz (b,n,3), new_xyz (b,npoint,3), features (b,c_feat,n) or NULL when c_feat==0,
 * idx (b,npoint,nsample) from ball_query, out (b, widths[nlayers-1], npoint).
 * widths = host array of the nlayers output widths (each <= 256, nlayers <= 4);
 * relu_mask bit l = ReLU after layer l.  params = device block, per layer
 * W^T zero-padded to [kp][cp] then bias [cp], with kp_0 = 3+c_feat rounded up to even,
 * kp_l = cp_{l-1}, cp = width rounded up to 32/64/128/256;
 * geot_sa_param_floats returns its length (or -1 for unsupported shapes).
 * nsample must be 8, 16 or a multiple of 32.  ReLU and the max propagate NaN (as torch.relu and torch.max do), and
 * the padding columns of an activation are 0 even where a real column is +-inf.  b == 0 or npoint == 0 launches
 * nothing.  Refused (hipErrorInvalidValue): b, n, npoint or c_feat < 0, nlayers outside 1..4, a width outside
 * 1..256, another nsample, c_feat > 0 with NULL features, or weights + activation tiles over 160 KiB of LDS at the
 * smallest launch (geot_sa_plan returns 0 for these). */
int geot_sa_param_floats(int c_feat, int nlayers, const int *widths);
/* Host-only (ABI 10): the launch plan of geot_sa_group_mlp_max for these sizes, from the function the launcher
 * uses; cus = the device's CU count, out_aligned16 = 1 when out is 16-byte aligned.  Returns 1 and fills the first
 * n_out (up to 27) of: wide variant (1: some padded width is 256, 8 waves at most; 0: 12 at most), waves per
 * workgroup (12, 8 or 4: the most that fit), LDS bytes, workgroups (min(units / waves rounded up, cus): persistent,
 * each takes a contiguous share; 0 when b * npoint == 0), groups per 32-row tile (gpt: 4, 2, 1 for nsample 8, 16,
 * >= 32), tiles per group (nsample / 32, or 1), fast_np (the register-pooled path with padded last width / 64
 * stores per group, 0 = the LDS-pooled path; needs nsample 32, c_feat <= 8, an unpadded last width >= 64 and
 * b * npoint < 2^31), run_len (8: the fast path stores runs of 8 groups, needs npoint % 8 == 0, out_aligned16 and
 * >= 16 units per wave of the grid; else 1), units (b * npoint / gpt rounded up), parameter floats, activation row
 * stride, then per layer 0..3 the padded input width kp, the padded output width cp, the float offsets of W^T and
 * of the bias (0 past nlayers) -- when the kernel takes the shape; returns 0 and leaves out alone otherwise.
 * The launcher's GEOT_SA_FAST / GEOT_SA_RUN overrides are not part of the plan.  out is a HOST array. */
int geot_sa_plan(int b, int npoint, int nsample, int c_feat, int nlayers, const int *widths, int cus, int out_aligned16,
                 long long *out, int n_out);
int geot_sa_group_mlp_max(int b, int n, int npoint, int nsample, int c_feat, const float *xyz,
                          const float *new_xyz, const float *features, const int *idx,
                          float xyz_scale, int nlayers, const int *widths, int relu_mask,
                          const float *params, float *out, void *stream);

/* ---- NTM: per-point instance-dependent transition matrix ------
 * c = class count, 1 <= c <= GEOT_NTM_MAX_C (32).  c == 17 (the reference's num_classes,
 * cfgs/tooth_semi/default.yaml:29) runs the kernels specialised for it (MFMA / LDS tiles of 17 x 17 rows); every
 * other count -- the reference builds its heads and losses for any nclasses (transformer.py:1104-1110,
 * insT_loss.py:62-67) -- runs run-time-C kernels with the same arithmetic.  Three entry points exist for c == 17
 * only and return hipErrorInvalidValue otherwise, each with a generic counterpart: geot_ntm_sig_t_mean_grad_w
 * (use _grad_raw + one GEMM), geot_ntm_threed_loss_fwd_graph / _grad_graph (use geot_ntm_threed_loss[_ord] +
 * geot_ntm_threed_loss_grad).
 *
 * sig_t_mean.forward (openpoints/models/backbone/transformer.py:1120-1131), fused:
 *   p (b,c,n) softmax probs, W (c,c,2c) = the c Linear(2c->c, bias=False) weights stacked
 *   [kk][out][in], cm (c,c) class means -> ins_T (b*n,c,c): row kk = clamp([p_i, cm[kk]] @ W[kk]^T,
 *   1e-5, 1-1e-5), L1-normalised.
 * _grad_raw: d loss / d (pre-clamp row) for a given d loss / d ins_T (the caller finishes the tiny
 *   weight-gradient GEMM, as nn.Linear's backward does in the reference). */
int geot_ntm_sig_t_mean(int b, int n, int c, const float *p, const float *W, const float *cm,
                        float *ins_T, void *stream);
int geot_ntm_sig_t_mean_grad_raw(int b, int n, int c, const float *p, const float *W, const float *cm,
                                 const float *grad_ins_T, float *grad_raw, void *stream);
/* Weight gradient of sig_t_mean without materialising d raw: grad_W (c,c,2c) += d loss / d W given
 * grad_ins_T (b*n,c,c); workspace = geot_ntm_sig_t_mean_ws_floats(b, n) floats of scratch. */
long long geot_ntm_sig_t_mean_ws_floats(int b, int n);
int geot_ntm_sig_t_mean_grad_w(int b, int n, int c, const float *p, const float *W, const float *cm,
                               const float *grad_ins_T, float *grad_W, float *workspace, void *stream);
/* Logit correction (examples/segmentation/train.py:549-552), fused:
 *   newT_i = L1-normalise(lam * ema_t + (1-lam) * ins_T_i); out[:, i] = logits[:, i]^T @ newT_i.
 *   logits/out (b,c,n), ins_T (b*n,c,c), ema_t (c,c).  _grad: grad_logits (b,c,n) and grad_ins_T are
 *   written in full, grad_ema_t (c,c) is accumulated into (pre-zero it). */
int geot_ntm_correct(int b, int n, int c, float lam, const float *logits, const float *ins_T,
                     const float *ema_t, float *out, void *stream);
int geot_ntm_correct_grad(int b, int n, int c, float lam, const float *logits, const float *ins_T,
                          const float *ema_t, const float *grad_out, float *grad_logits,
                          float *grad_ins_T, float *grad_ema_t, void *stream);
/* Host-only (ABI 29): what the four entry points above launch for (b, n, c) on a device of `cus` compute units (<= 0: the
 * current device's), under GEOT_NTM_GENERIC as the launch reads it.  Returns the form of sig_t_mean -- 0 nothing to launch
 * (b * n == 0 or arguments out of range), 1 a wave per point, 2 a lane per point, 3 the matrix-core form, 4 the specialised
 * c == 17 kernels, -1 a launch that would be refused -- and fills out[0 .. min(n_out, 7)) with: form, CP (form 2) or CPAD
 * (form 3), tails (form 3: c % 4 != 0), ksplit (ranges of row tiles, form 3), workgroups, dynamic LDS bytes, and the
 * workgroups of geot_ntm_correct[_grad] for c != 17.  `backward` selects _grad_raw (both launch the same geometry). */
int geot_ntm_generic_plan(int b, int n, int c, int backward, int cus, long long *out, int n_out);
/* Class anchors, train.py:505-526: class_T (c,c) row cc = eta[b*, :, n*] of the point with the largest
 * eta[b, cc, n] (eta (b,c,n) fp32: the weak view's soft-max), the first maximum in flattened (b, n) order as
 * torch.argmax picks it; v_star (c, nullable) receives the maxima (the multi-rank exchange compares them). */
int geot_ntm_class_anchors(int b, int n, int c, const float *eta, float *class_T, float *v_star, void *stream);
/* The same anchors behind cfg.filter_outlier, train.py:510-526 (ABI 26; csrc/ntm_outlier.hip): before the arg-max of class cc
 * every probability of that class at or above its q-quantile over the batch counts as 0.  1 <= c <= 32, 1 <= b*n <= 2^24,
 * 0 <= q <= 1; anything else is hipErrorInvalidValue before any launch.  Two launches, no workspace: thresh (c) is a result
 * and the only scratch; v_star (c) may be NULL.  Exactly:
 *   thresh[cc] = torch.quantile(eta[:, cc, :].flatten(), q), linear interpolation, in fp32 as torch computes it: with M = b*n
 *     and s the ascending order of the class's values, rank = fl32(q) * fl32(M-1) (one fp32 product), lo = floor(rank),
 *     hi = ceil(rank), w = rank - lo, d = s[hi] - s[lo]; s[lo] + w*d when w < 0.5, else s[hi] - d*(1 - w), un-contracted
 *     (a numpy float32 restatement reproduces the bits; torch's own lerp may be contracted: one ulp in the last step).
 *     s[lo] and s[hi] come from an exact radix select on order-preserving keys of the bit patterns, so any finite float
 *     orders correctly, negatives included (-0 and +0 in either order).
 *   f(b, cc, n) = eta >= thresh[cc] ? 0 : eta    (0, not skipped: a class filtered everywhere has anchor 0, v_star 0)
 *   anchor of cc = the first maximum of f(., cc, .) in flattened (b, n) order; v_star[cc] = that filtered maximum
 *   class_T[cc][k] = f(b*, k, n*) for k <= cc, eta[b*, k, n*] for k > cc: the reference filters eta IN PLACE class after
 *     class (robust_eta is a view, :511-513), so the row read at :526 sees columns 0..cc filtered and the later ones not.
 * NaN is outside the contract, as for geot_ntm_class_anchors: results are then unspecified, accesses stay in bounds. */
int geot_ntm_filtered_anchors(int b, int n, int c, double q, const float *eta, float *class_T, float *v_star, float *thresh,
                              void *stream);
/* Class-level transition block, train.py:505-557 once the anchor rows class_T (c,c) are gathered: Gaussian
 * tooth-adjacency prior from sigma (c) over the label projection proj (c) (train.py:48), blend, the three
 * `X / X.sum(1)` normalisations exactly as written there (column k divided by row-sum k), EMA.  c <= 32.
 * Writes ema_t_corr, ema_t_next, prior_T (c,c) and, when ema_t_keep is not NULL, a copy of ema_t there (a caller
 * that keeps ema_t in one persistent buffer overwrites it with ema_t_next, train.py:556-557, before backward).
 * _grad writes d/d sigma (c) given d/d ema_t_corr and d/d prior_T (either may be NULL); sigma is the only
 * learnable input.  geo_lambda / ema_decay are DOUBLES (ABI 6): the reference multiplies fp32 tensors by the Python
 * floats cfg.geo_lambma and (1 - cfg.geo_lambma) (train.py:533-534, 540-545), i.e. by fl32(0.999) and fl32(1 - 0.999);
 * from a float argument the complement could only be formed as 1.f - fl32(0.999), 4.7e-5 off -- which is the whole
 * sigma gradient's relative error, since that gradient is proportional to (1 - geo)(1 - decay). */
int geot_ntm_class_transition(int c, double geo_lambda, double ema_decay, const float *class_T, const float *sigma,
                              const float *ema_t, const float *proj, float *ema_t_corr, float *ema_t_next,
                              float *prior_T, float *ema_t_keep, void *stream);
int geot_ntm_class_transition_grad(int c, double geo_lambda, double ema_decay, const float *class_T,
                                   const float *sigma, const float *ema_t, const float *proj,
                                   const float *grad_ema_t_corr, const float *grad_prior_T, float *grad_sigma,
                                   void *stream);
/* _grad_ws: as _grad, with grad_ema_t reduced through geot_ntm_correct_ws_floats(b, n) floats of scratch. */
long long geot_ntm_correct_ws_floats(int b, int n);
int geot_ntm_correct_grad_ws(int b, int n, int c, float lam, const float *logits, const float *ins_T,
                             const float *ema_t, const float *grad_out, float *grad_logits,
                             float *grad_ins_T, float *grad_ema_t, float *workspace, void *stream);
/* threeD_space_loss (utils/insT_loss.py:68-110) over a given kNN graph:
 *   positions (b,n,3), labels (b,n) int32, ins_T (b*n,c,c), nbr (b,n,k) int32 local neighbour ids
 *   (the reference uses knn_point(k+1)[..., 1:]); per_point (b*n) = sum_j w_ij |T_i-T_j|^2 /
 *   (sum_j w_ij + 1e-3), w_ij = [label_i==label_j] exp(-|p_i-p_j|^2/(2 sigma^2)); loss = mean.
 *   _grad accumulates grad_scale * d(sum per_point)/d ins_T into grad_ins_T (pre-zero it);
 *   pass grad_scale = upstream_grad / (b*n).  k <= 64. */
int geot_ntm_threed_loss(int b, int n, int c, int k, float sigma, const float *positions,
                         const int *labels, const float *ins_T, const int *nbr, float *per_point,
                         void *stream);
int geot_ntm_threed_loss_grad(int b, int n, int c, int k, float sigma, float grad_scale,
                              const float *positions, const int *labels, const float *ins_T,
                              const int *nbr, float *grad_ins_T, void *stream);
/* _grad_ws: the same gradient through an atomic-free gather over the kNN graph and its reverse (built in
 * the workspace, geot_ntm_threed_loss_ws_bytes(b, n, k) bytes); 3x faster when labels are spatially
 * coherent, i.e. on real scans, where most edges are live.  Falls back to _grad without a workspace. */
long long geot_ntm_threed_loss_ws_bytes(int b, int n, int k);
int geot_ntm_threed_loss_grad_ws(int b, int n, int c, int k, float sigma, float grad_scale,
                                 const float *positions, const int *labels, const float *ins_T,
                                 const int *nbr, const int *order, float *grad_ins_T, void *workspace,
                                 long long ws_bytes, void *stream);
/* `order` (b*n int32 global point ids, or NULL) = the order in which points are PROCESSED; results do not
 * depend on it.  With geot_spatial_order's output consecutive waves work on spatial neighbours and the
 * gathered (1156-byte) rows of a point's graph neighbours are found in L2: 1.5x on randomly ordered scans. */
int geot_ntm_threed_loss_ord(int b, int n, int c, int k, float sigma, const float *positions,
                             const int *labels, const float *ins_T, const int *nbr, const int *order,
                             float *per_point, void *stream);
/* Forward that leaves the graph (reverse adjacency with fixed 64-slot lists + overflow list, edge weights,
 * normalisers) in `graph` (geot_ntm_threed_graph_bytes(b, n, k) bytes), and the backward that consumes it:
 * the backward is then the gather alone.  Same results as the entry points above, except that
 * _grad_graph WRITES grad_ins_T in full (it need not be zero-filled). */
long long geot_ntm_threed_graph_bytes(int b, int n, int k);
int geot_ntm_threed_loss_fwd_graph(int b, int n, int c, int k, float sigma, const float *positions,
                                   const int *labels, const float *ins_T, const int *nbr, const int *order,
                                   float *per_point, void *graph, long long graph_bytes, void *stream);
int geot_ntm_threed_loss_grad_graph(int b, int n, int c, int k, float grad_scale, const float *upstream,
                                    const float *ins_T, const int *nbr, const int *order, const void *graph,
                                    long long graph_bytes, float *grad_ins_T, void *stream);
/* upstream: optional DEVICE scalar multiplied into grad_scale (autograd's incoming gradient), so the host
 * does not have to read it back; NULL = 1. */
int geot_spatial_order(int b, int n, const float *xyz, int *order, void *workspace, long long ws_bytes,
                       void *stream); /* workspace: geot_knn_grid_ws_bytes(b, n) bytes, 16-byte aligned */
/* feature_space_loss (utils/insT_loss.py:9-58; disabled in the shipped cfg, use_feat_loss): same graph
 * kernel over feat_dim-dimensional features (b,n,feat_dim) with SIGNED weights
 * w_ij = (label_i == label_j ? +1 : -1) exp(-|f_i-f_j|^2/(2 sigma^2)) and no per-point normalisation:
 * per_point (b*n) = sum_j w_ij |T_i-T_j|^2; the reference's loss is sum(per_point) / (b*n*k).
 * _grad: pass grad_scale = upstream_grad / (b*n*k). */
int geot_ntm_feature_loss(int b, int n, int c, int k, int feat_dim, float sigma, const float *feats,
                          const int *labels, const float *ins_T, const int *nbr, float *per_point,
                          void *stream);
int geot_ntm_feature_loss_grad(int b, int n, int c, int k, int feat_dim, float sigma, float grad_scale,
                               const float *feats, const int *labels, const float *ins_T, const int *nbr,
                               float *grad_ins_T, void *stream);
/* (ABI 17) the same gradient with the same bits on every run, for a step that is compared or replayed bit for bit: the
 * terms 2 w_ij (T_i - T_j) are summed as 2^-40 fixed-point integers (64-bit integer atomics: any order, one sum; exact
 * while |sum| < 2^23 per element -- row-stochastic T), then grad_ins_T = upstream[0] * grad_scale * sum is written in
 * full.  acc: b*n*c*c int64 of device scratch, ZERO on entry; upstream: device scalar or NULL (= 1);
 * grad_scale = 1 / (b*n*k). */
int geot_ntm_feature_loss_grad_det(int b, int n, int c, int k, int feat_dim, float sigma, float grad_scale,
                                   const float *feats, const int *labels, const float *ins_T, const int *nbr,
                                   long long *acc, const float *upstream, float *grad_ins_T, void *stream);

/* ---- dataloader-side ops ---------------------------------------------------------------
 * geot_grid_subsampling replaces cpp_subsampling.compute (openpoints/cpp/subsampling/wrapper.cpp:58-285 ->
 * grid_subsampling/grid_subsampling.cpp:4-106): voxel size sample_dl, points (n,3), optional features
 * (n,fdim) and integer labels (n,ldim).  Outputs have room for n rows; *out_count (device int) receives the
 * number of voxels M; rows 0..M-1 are the voxel barycentres (fp32 sums in input order, bit-identical to the
 * reference), mean features and majority labels, by ascending voxel key (the reference emits the same rows in
 * its hash map's iteration order; on a label tie it takes the first maximum in that order, here the smallest
 * tied label).  Cell indices follow the reference's x86-64 build, wrap included: (size_t)floor(x) goes through a signed
 * 64-bit integer there, and the fp32 origin floor(min / dl) * dl can land above the minimum corner, so the minimum point
 * can get an index of -1 = 2^64 - 1; its key ix + NX iy + NX NY iz is then, modulo 2^64, that of cell (NX - 1, iy - 1, iz),
 * and the point is merged into that cell when it is occupied.  NaN and infinite coordinates are outside the contract.
 * ws: geot_grid_subsampling_ws_bytes(n) bytes of device scratch (sized for the current device: -1 when the process has
 * no GPU). */
long long geot_grid_subsampling_ws_bytes(int n);
int geot_grid_subsampling(int n, int fdim, int ldim, float sample_dl, const float *points, const float *features,
                          const int *labels, float *out_points, float *out_features, int *out_labels,
                          int *out_count, void *ws, long long ws_bytes, void *stream);
/* pc_norm of openpoints/dataset/tooth_semi/tooth_dataset.py:108-114: stats (4 floats, device) = centroid xyz
 * and scale = max row norm of the centred cloud.  ws: geot_pc_norm_ws_bytes() bytes. */
long long geot_pc_norm_ws_bytes(void);
int geot_pc_norm_stats(int n, const float *points, float *stats, void *ws, long long ws_bytes, void *stream);
/* tooth_dataset.py:132-147: out_points[i] = (points[selected[i]] - centroid) / scale (m,3); with labels (n)
 * also out_labels (m) int64 and class_weights (num_classes) = histogram of the gathered labels over [0, num_classes) /
 * its total (inf -> 0).  A label outside [0, num_classes) is DROPPED from the histogram and carried in out_labels as it is
 * (the reference's torch.histogram closes its last bin on the right, so a label of exactly num_classes would count as
 * num_classes - 1 there; its label map never produces one); with no label in range every weight is 0 / 0 = NaN, as the
 * reference's expression gives.  selected NULL = identity (m == n).  m == 0: nothing is gathered, class_weights is still
 * written (NaN, the same 0 / 0), and selected, out_points and out_labels may be NULL.  hist_ws: num_classes + 1 ints; the
 * last one is set non-zero when an entry of selected was out of range (numpy raises IndexError there; the row is then
 * read from point 0). */
int geot_cloud_sample(int n, int m, int num_classes, const float *points, const int *labels,
                      const long long *selected, const float *stats, float *out_points, long long *out_labels,
                      float *class_weights, int *hist_ws, void *stream);

/* ---- FixMatch epoch meters (ABI 12) ----------------------------------------------------------------------------------
 * The per-iteration statistics of examples/segmentation/train.py:599-644 and their AverageMeters (:672-699), on the device
 * (geot_amd/csrc/meters.hip): no host synchronisation, capturable.  b * n < 2^24 unlabelled points, 1 <= c <= GEOT_NTM_MAX_C.
 * geot_fixmatch_meters_count adds into counts (8 + 4 c ints, zero on entry -- the finalize leaves them so):
 *   pseudo t (b,n) int64, conf (b,n) fp32 -> mask m = conf >= threshold; gt g (b,n) int64; prob (b,c,n) fp32, the student's
 *   strong-view soft-max -> s = its first maximum over c (a NaN counts as the maximum, as torch.max picks it).
 *   [0] sum m  [1] sum [t=g]  [2] sum [s=g]  [3] sum m[t=g]  [4] sum [t>0]  [5] sum m[t>0]  [6] sum m[t>0][t=g]
 *   [7] labels t or g outside [0, c)  [8 + k c + cls], k = 0..3: sum m[t=cls], sum m[t=cls][g=cls], sum [t=cls], sum [g=cls]
 * geot_fixmatch_meters_finalize (one workgroup) forms the iteration's values from counts with the reference's arithmetic,
 * updates the meters with n = n_u (n_l + n_u for the total loss, n_l for the supervised loss) and zeroes counts.
 *   meters_f32 (18): value[6], sum[6], avg[6] of th_percentage, mean_pseudo_label_acc, teacher_acc, student_acc,
 *                    over_th_wobg, over_acc_wobg (fp32 tensors in the reference)
 *   meters_f64 (18 + 9 c): value[6], sum[6], avg[6] of the loss meters loss, loss_l, loss_u, feat (0), identity (0), 3d;
 *                    then value[3c], sum[3c], avg[3c] of the per-class lists pseudo_label_acc, th_meter_u, th_meter_u_recall
 *   meters_i64 (5):  count of n_l + n_u, of n_l, of n_u; labels outside [0, c) so far; iterations
 *   loss / sup / unsup / threed: device fp32 scalars; ema_corr (c,c) is copied to ema_corr_out (both may be NULL). */
int geot_fixmatch_meters_count(int b, int n, int c, float threshold, const long long *pseudo, const float *conf,
                               const long long *gt, const float *prob, int *counts, void *stream);
int geot_fixmatch_meters_finalize(int b, int n, int c, int n_l, int n_u, const float *loss, const float *sup,
                                  const float *unsup, const float *threed, const float *ema_corr, int *counts,
                                  float *meters_f32, double *meters_f64, long long *meters_i64, float *ema_corr_out,
                                  void *stream);
/* (ABI 17) the same with the two switched losses of train.py:560-568 metered too (:678-679, n = n_u, in double): feat /
 * identity are device fp32 scalars, NULL = the switch is off and 0.0 is metered, as geot_fixmatch_meters_finalize does. */
int geot_fixmatch_meters_finalize6(int b, int n, int c, int n_l, int n_u, const float *loss, const float *sup,
                                   const float *unsup, const float *threed, const float *feat, const float *identity,
                                   const float *ema_corr, int *counts, float *meters_f32, double *meters_f64,
                                   long long *meters_i64, float *ema_corr_out, void *stream);

/* ---- validation metrics (ABI 13) ---------------------------------------------------------------------------------------
 * The counts behind examples/segmentation/train.py:802-832 get_seg_metrics (per-scan accuracy, IoU and DSC of the classes
 * present) and :757-763 (jaw and whole means), on the device (geot_amd/csrc/seg_metrics.hip): no host synchronisation.
 * b >= 0 scans in one launch (b == 0: nothing to do, success), 1 <= c <= GEOT_NTM_MAX_C; anything else is
 * hipErrorInvalidValue before any launch.  offsets (b + 1) int64 on the device: scan s owns vertices
 * [offsets[s], offsets[s + 1]) of the concatenated per-vertex arrays, at most 2^31 - 1 of them.
 * counts: b slots of c (c + 1) + 1 int64 each; the caller zeroes them, the launch ADDS into them (batches accumulate):
 *   [label * (c + 1) + pred]  vertices with that label and prediction, both in [0, c)
 *   [label * (c + 1) + c]     vertices with that label in [0, c) and a prediction outside [0, c)
 *   [c (c + 1)]               vertices whose label is outside [0, c)
 * Integer atomics only: the counts do not depend on the schedule.
 * geot_seg_confusion: pred / label int64 per vertex.
 * geot_seg_confusion_interp: the prediction is get_pred_whole's (train.py:781-800), made per vertex in registers:
 *   prob (b, c, n) fp32 = the soft-max of the n sampled points; idx (M, 3) int32 / dist2 (M, 3) fp32 = three_nn of every
 *   vertex among its scan's sampled points (squared distances); weights 1.0 / (sqrt(d2) + 1e-8) over their torch.sum
 *   ((r0 + r2) + r1), the interpolation p0 w0 + p1 w1 + p2 w2 un-contracted, torch.argmax's rule (first maximum, a NaN
 *   wins).  n >= 1. */
int geot_seg_confusion(int b, int c, const long long *offsets, const long long *pred, const long long *label,
                       long long *counts, void *stream);
int geot_seg_confusion_interp(int b, int c, int n, const long long *offsets, const float *prob, const int *idx,
                              const float *dist2, const long long *label, long long *counts, void *stream);

/* ---- FixMatch training batches from device-resident scans (ABI 14) -------------------------------------------------------
 * What the reference's two training loaders do per item on CPU workers (openpoints/dataset/tooth_semi/tooth_dataset.py:
 * 116-206, 308-415, openpoints/transforms/point_transformer_gpu.py, default collation), for a whole batch, in a number of
 * launches that does not depend on the batch; no host synchronisation.
 *
 * geot_cloud_sample_batch = geot_pc_norm_stats + geot_cloud_sample for s scans at once (5 launches).  The scans of a set lie
 * concatenated: points (total, 3), labels (total); offsets (n_scans + 1) int64 ON THE DEVICE, set scan i owns vertices
 * [offsets[i], offsets[i + 1]), 1 .. 2^31 - 1 of them.  scan_ids (s) int64 on the device names the set scan of every batch
 * slot (NULL: slot i is set scan i; then n_scans must be >= s).  sel (s, m) int64: vertex indices LOCAL to the slot's scan.
 * Per slot: raw (m, 3) = (points[sel] - centroid) / scale, y (m) int64, class_weights (num_classes), center (3), scale (1)
 * -- each bit-identical to the single-scan calls on that scan alone (the same fp64 partial-sum tree per scan, the same
 * (x^2 + y^2) + z^2 norm, IEEE divide; the maximum and the histogram do not depend on arrival order; no float atomics).
 * bad (s) int32: set to 1 for a slot with an entry of sel outside its scan (the row is then read from vertex 0, as
 * geot_cloud_sample does) and to 2 for a slot whose scan_ids / offsets entry is unusable -- a scan id outside [0, n_scans),
 * an empty scan, offsets[i] < 0 or offsets[i + 1] > total -- (nothing of that slot is read; its raw, y, class_weights, center
 * and scale are zero-filled: no 0 / 0 there), 0 otherwise.  ws: geot_cloud_sample_batch_ws_bytes(s, num_classes) bytes.
 * 1 <= s <= 65535, m >= 1, 1 <= num_classes <= 4096, n_scans >= 1, total >= 1, no NULL pointer but scan_ids; anything else
 * is hipErrorInvalidValue. */
long long geot_cloud_sample_batch_ws_bytes(int s, int num_classes);
int geot_cloud_sample_batch(int s, int m, int num_classes, int n_scans, long long total, const float *points,
                            const int *labels, const long long *offsets, const long long *scan_ids, const long long *sel,
                            float *raw, long long *y, float *class_weights, float *center, float *scale, int *bad, void *ws,
                            long long ws_bytes, void *stream);

/* geot_fixmatch_views: j view jobs in ONE launch (one workgroup per job).  jobs: j records of GEOT_VIEW_JOB_WORDS 32-bit
 * words on the device:
 *   [0] int  row of raw (n_rows, m, 3) the view is made of      [1] int  output row in pos / x / heights (n_out rows each)
 *   [2] int  flags: bit 0 rotate, bit 1 translate               [3] reserved (0)
 *   [4..6] float s    [7..15] float R, row-major    [16..18] float t    [19] reserved
 * With q = r * s (one rounding per element):
 *   x       (n_out, 3, m) channel-first = q                (PointCloudScaling* scales data['pos'] in place and data['x'] IS
 *                                                           that tensor: x is the scaled, un-centred cloud)
 *   heights (n_out, m, 1) = q[:, g] - min(q[:, g]),  g = gravity_dim in 0..2
 *   pos     (n_out, m, 3) = (q - mean(q)) / mx,  mx = max_i sqrtf((cx^2 + cy^2) + cz^2); with bit 0:
 *           pos_k = ((p0 R[k][0] + p1 R[k][1]) + p2 R[k][2]), with bit 1: + t[k]  (un-contracted, left to right)
 *   view_center (j, 3) = mean(q), view_scale (j) = mx         (per JOB, not per output row)
 * Every statement is a single fp32 operation except the mean: fp64 sums in a fixed tree, rounded once.  min / max
 * propagate NaN as torch does; m = 1 gives mx = 0 and pos = 0 / 0 = NaN, as the reference.  Results are bit-reproducible.
 * Up to GEOT_VIEW_REG_POINTS points a job's cloud is read once and held in registers; beyond, the same workgroup streams it
 * from memory three times (same tree, same results).  Two jobs must not name the same output row.  A job whose rows are
 * out of range writes nothing but NaN to its view_center / view_scale.
 * j >= 1, 1 <= m <= 357 913 941 (a row stays below 4 GB), n_rows >= 1, n_out >= 1, gravity_dim in 0..2, no NULL pointer;
 * anything else is hipErrorInvalidValue. */
#define GEOT_VIEW_JOB_WORDS 20
#define GEOT_VIEW_REG_POINTS 24576
int geot_fixmatch_views(int j, int m, int n_rows, int n_out, int gravity_dim, const float *raw, const void *jobs, float *pos,
                        float *x, float *heights, float *view_center, float *view_scale, void *stream);

/* ---- whole-scan prediction and validation counts from device-resident scans (ABI 15) --------------------------------------
 * geot_scan_predict: get_pred_whole (train.py:781-800) and, optionally, get_seg_metrics' counts for b batch slots in a
 * number of launches that does not depend on b or on the scans' sizes (six with the grid, one without); no host
 * synchronisation; neither neighbour indices, distances nor a (c, M) probability table are written.
 * The scans lie concatenated as for geot_cloud_sample_batch: points (total, 3) fp32, labels (total) int32, offsets
 * (n_scans + 1) int64 on the device; scan_ids (b) int64 on the device names the set scan of every slot (a scan may occur
 * in several slots, in any order).  known (b, n, 3): the slot's n sampled points in the scan's coordinates; prob (b, c, n):
 * their soft-max.  For every vertex v of slot s's scan, read in place:
 *   the three points of known[s] smallest by (d2, index), d2 = ((dx dx) + (dy dy)) + (dz dz) un-contracted -- geot_three_nn's
 *   contract: with n < 3 the missing entries are (+inf, index 0), and a NaN vertex gets three of those;
 *   geot_seg_confusion_interp's weights, interpolation and arg-max (first maximum, a NaN wins) on them;
 *   pred (optional): pred[out_offsets[s] + v] = class, out_offsets (b) int64 on the device;
 *   counts (optional; needs labels): row s of b rows of c (c + 1) + 1 int64, laid out and ADDED to as geot_seg_confusion's.
 * Bit for bit what geot_three_nn_ws per scan followed by geot_seg_confusion_interp yields.  Integer atomics only.
 * work: n_work records of four int32 on the device, 16-byte aligned -- (slot, first vertex, vertex count, 0) -- one
 * workgroup each; together they must cover every vertex of every slot once (geot_amd/validation.py scan_work_table
 * makes them from the scans' sizes).  A record whose slot, first vertex or count is out of range, and a slot whose scan_ids
 * entry lies outside [0, n_scans) or whose offsets pair is not 0 <= lo < hi <= total with hi - lo <= 2^31 - 1, is skipped:
 * nothing of it is read, written or counted (callers validate scan ids on the host, as for geot_cloud_sample_batch).
 * ws: geot_scan_predict_ws_bytes(b, n) bytes, 16-byte aligned, contents irrelevant (the grid over every slot's sampled
 * points; with n < 2048 or GEOT_NN_IMPL=basic|wave the n points are scanned instead and ws is not touched).
 * 0 <= b <= 65535 (0: nothing to do), 1 <= c <= GEOT_NTM_MAX_C, n >= 1, n_scans >= 1, total >= 1, n_work >= 0 (0: nothing
 * to do), pred or counts (or both) given; anything else is hipErrorInvalidValue before any launch. */
long long geot_scan_predict_ws_bytes(int b, int n);
int geot_scan_predict(int b, int c, int n, int n_scans, long long total, const float *points, const int *labels,
                      const long long *offsets, const long long *scan_ids, const float *known, const float *prob,
                      int n_work, const int *work, const long long *out_offsets, long long *pred, long long *counts,
                      void *ws, long long ws_bytes, void *stream);

/* ---- whole-scan predictions voted over several samples of the same scans (ABI 21) ------------------------------------------
 * geot_scan_vote: geot_scan_predict with one difference -- a vertex's c interpolated class values are not arg-maxed on the
 * spot but stored in, or added to, a caller-owned accumulator; after the last vote the arg-max is taken of the sum.  Every
 * other argument, the work table, the search, the skip rules and the workspace (geot_scan_predict_ws_bytes(b, n)) are
 * geot_scan_predict's; so is the number of launches.
 * acc: fp32, vertex-major, (sum of the slots' vertex counts, c); vertex v of slot s owns row out_offsets[s] + v (out_offsets
 * (b) int64 on the device).  Both are always required.  A skipped slot or work record leaves its rows untouched.
 * mode: GEOT_VOTE_SET -- this is the first vote: the values are stored (acc may arrive uninitialised); without it they are
 * added to what is there, value = acc + this vote's, one fp32 addition.  GEOT_VOTE_FINISH -- once this vote's values are in,
 * pred and / or counts are written from the sums as geot_scan_predict writes them from one vote's values (first maximum, a NaN
 * wins; counts ADDED to; counts needs labels).  pred and counts are legal only with GEOT_VOTE_FINISH.
 * The per-class value is geot_scan_predict's statement for statement, so one call with GEOT_VOTE_SET | GEOT_VOTE_FINISH writes
 * geot_scan_predict's pred and counts bit for bit and leaves the interpolated probabilities in acc.
 * One writer per accumulator element and no float atomics: the votes are added in call order, and the same calls give the
 * same bits.  GEOT_VOTE_IMPL=row|tile (read at every call) picks how acc is reached -- per vertex by the lanes that hold
 * its values, or 64 vertices at a time through an LDS tile -- with the same results.
 * geot_scan_predict's refusals, and: acc or out_offsets NULL, a mode bit other than the two, pred or counts without
 * GEOT_VOTE_FINISH; all hipErrorInvalidValue before any launch. */
#define GEOT_VOTE_SET 1
#define GEOT_VOTE_FINISH 2
int geot_scan_vote(int b, int c, int n, int n_scans, long long total, const float *points, const int *labels,
                   const long long *offsets, const long long *scan_ids, const float *known, const float *prob,
                   int n_work, const int *work, const long long *out_offsets, float *acc, int mode, long long *pred,
                   long long *counts, void *ws, long long ws_bytes, void *stream);

/* ---- whole-scan predictions from covering passes: every vertex predicted directly (ABI 30) ---------------------------------
 * Independent samples cover a scan badly: with M = 100 000 vertices and n = 16 000 samples one pass misses a vertex with
 * probability 1 - n / M = 0.84, so after 10 voted passes 0.84^10 = 17.5 % of the vertices were never seen by the model and
 * every label is interpolated.  P = ceil(M / n) = 7 passes whose samples PARTITION the scan show the model every vertex once.
 * geot_sample_draw_cover (below, with geot_sample_draw) draws such passes; geot_scan_cover takes a pass's soft-max to the
 * vertices it names: no neighbour search, no interpolation, no workspace, no float atomics.
 * Arguments as geot_scan_vote's, with sel (b, n) int64 -- the pass's vertex indices, local to each slot's scan, as
 * geot_sample_draw_cover wrote them -- and pass (>= 0) in place of points, known and the workspace.  prob (b, c, n)
 * channel-first, acc / out_offsets / mode / pred / counts / work as there.  With n_s the size of slot s's scan:
 *   scatter (one launch, grid (ceil(n / 256), b)): sample j of slot s OWNS its vertex iff q = pass * n + j < n_s (64-bit) and
 *   0 <= sel[s][j] < n_s; a position with q >= n_s is wrap-around fill and owns nothing.  An owner writes row r =
 *   out_offsets[s] + sel[s][j] of acc: acc[r][k] = prob[s][k][j] with GEOT_VOTE_SET, acc[r][k] = acc[r][k] + prob[s][k][j]
 *   (one fp32 addition) without.  Non-owners write nothing.  Over passes 0 .. ceil(n_s / n) - 1 of one cover every row has
 *   exactly one writer; GEOT_VOTE_SET marks the first ROUND and is passed to every pass of it.  The owners of one call must
 *   name distinct vertices per slot (geot_sample_draw_cover's do): rows are written without atomics.
 *   finish (GEOT_VOTE_FINISH with pred and / or counts; a second launch over the work table): pred and / or counts from the
 *   sums, by geot_scan_vote's rule -- first maximum, a NaN wins, counts laid out and ADDED to as geot_seg_confusion's (integer
 *   atomics only; counts needs labels).  It reads every row the work table names, so the last pass of a cover carries it.
 * Skip rules: geot_scan_vote's (an unusable slot or work record is neither read, written nor counted).  Refusals:
 * geot_scan_vote's (b, c, n, n_scans, total, n_work ranges; offsets, scan_ids, prob, acc, out_offsets NULL; counts without
 * labels; an unknown mode bit; pred or counts without GEOT_VOTE_FINISH; work NULL or not 16-byte aligned), sel NULL, and
 * pass < 0; all hipErrorInvalidValue before any launch.  b = 0 or n_work = 0: nothing to do. */
int geot_scan_cover(int b, int c, int n, int n_scans, long long total, const int *labels, const long long *offsets,
                    const long long *scan_ids, const long long *sel, const float *prob, int pass, int n_work, const int *work,
                    const long long *out_offsets, float *acc, int mode, long long *pred, long long *counts, void *stream);

/* ---- whole scans decoded at full resolution from one backbone pass (ABI 31) ---------------------------------------------------
 * PointTransformer_seg_T's last decoder stage (propogation_0, seg_head) is a pure function of a query's position once the
 * backbone has produced the features of its m centres (m = 8192 as configured): three_nn against the centres, the
 * inverse-distance interpolation, the skip channels [one_hot(cls), xyz], two 1x1 convolutions with BatchNorm, the head.  In eval
 * mode nothing ties the query set to the sampled set, so one forward pass plus this stage at every vertex predicts every vertex
 * directly -- where geot_scan_cover pays ceil(M / n) forward passes.  What this establishes is that the values are the model's
 * own decoder applied to those positions; the accuracy of decoded against interpolated or covered labels on real scans has
 * not been measured (there are no trained weights here).
 * The scans lie concatenated as for geot_scan_predict (points, offsets, scan_ids, the skip rules of slots and work records); no
 * workspace, no host synchronisation, one launch per call, no atomics in front, integer atomics only in finish.
 * work: n_work records of four int32 on the device, 16-byte aligned -- (slot, first vertex, vertex count, first output row):
 * geot_scan_predict's record with its fourth word in use.  Vertex first + i of the record owns row [3] + i of the call's
 * row-indexed arrays (z, q, idx, weight; the columns of logits), rows of them in all: the caller bounds z by decoding a batch in
 * chunks of vertices, a chunk boundary may fall inside a scan, and both entry points of a chunk take the same records.  A
 * record whose rows do not lie in [0, rows) is skipped like one whose slot, first vertex or count is out of range: nothing of
 * it is read, written or counted.  Records must not share rows.
 *
 * geot_scan_decode_front, for every vertex p of every record, slot s:
 *   query position  r = (p - center[s]) / scale[s]  (pc_norm: center (b, 3), scale (b), geot_cloud_sample_batch's statements),
 *   then  q = (r - view_center[s]) / view_scale[s]  (the `val` view's centre-and-normalise: view_center (b, 3), view_scale (b)
 *   as geot_fixmatch_views / geot_view_program write them): per coordinate the same four single fp32 operations the batcher
 *   applies to a sampled vertex, so a vertex that is sample j of the batch gets the bits of pos[s][j];
 *   the three of the slot's m centres known (b, m, 3) smallest by (d2, index), d2 = ((dx dx) + (dy dy)) + (dz dz) un-contracted
 *   -- geot_three_nn's contract (a NaN vertex gets three entries (+inf, index 0)) -- and geot_fp_weights' weights statement for
 *   statement: r_t = 1 / (sqrt(d2_t) + 1e-8), w_t = r_t / ((r_0 + r_1) + r_2);
 *   one point-major row of c_out channels, channel k:
 *     z[row][k] = act(ch_scale[k] * (((w_0 a[i_0][k] + w_1 a[i_1][k]) + w_2 a[i_2][k]) + skip_const[s][k]
 *                                    + ((W_xyz[k][0] q_x + W_xyz[k][1] q_y) + W_xyz[k][2] q_z)) + ch_shift[k])
 *   every operation rounded, left to right; act = torch.relu (a NaN stays NaN) with relu = 1, the identity with relu = 0.
 *   a (b, m, c_out): the stage's first convolution already applied to the centres' features, point-major; skip_const
 *   (b, c_out): the one-hot columns' contribution for the slot's jaw; W_xyz (c_out, 3): the xyz columns; ch_scale / ch_shift
 *   (c_out): the folded eval BatchNorm.  Any c_out >= 1: rows are stored four channels per lane where c_out is a multiple of 4
 *   and a, z, skip_const, W_xyz, ch_scale and ch_shift are 16-byte aligned, one channel per lane otherwise -- the same values.
 *   q (rows, 3) fp32, idx (rows, 3) int32, weight (rows, 3) fp32: optional (NULL) copies of the search, for tests.
 *   One writer per element: the same call gives the same bits.
 *   0 <= b <= 65535, m >= 3, c_out >= 1, relu 0 or 1, n_scans >= 1, total >= 1, n_work >= 0, 0 <= rows <= 2^31 - 1, no NULL among
 *   points .. ch_shift and z, work not NULL and 16-byte aligned; anything else is hipErrorInvalidValue before any launch.
 *   b = 0, n_work = 0 or rows = 0: nothing to do.  (No class count: the stage in front of the head does not know one.)
 *
 * geot_scan_decode_finish: logits (c, rows) channel-first -- the head's output for the chunk as a (1, rows) cloud -- over the
 * same records: the arg-max of every column by geot_scan_vote's rule (first maximum, a NaN wins);
 *   pred (optional): pred[out_offsets[s] + v] = class for vertex v of slot s, out_offsets (b) int64 on the device;
 *   counts (optional; needs labels): row s of b rows of c (c + 1) + 1 int64, laid out and ADDED to as geot_seg_confusion's.
 *   0 <= b <= 65535, 1 <= c <= GEOT_NTM_MAX_C, n_scans >= 1, total >= 1, n_work >= 0, 0 <= rows <= 2^31 - 1, offsets, scan_ids
 *   and logits not NULL, pred or counts (or both) given, out_offsets with pred, labels with counts, work not NULL and 16-byte
 *   aligned; anything else is hipErrorInvalidValue before any launch.  b = 0, n_work = 0 or rows = 0: nothing to do. */
int geot_scan_decode_front(int b, int m, int c_out, int relu, int n_scans, long long total, const float *points,
                           const long long *offsets, const long long *scan_ids, const float *center, const float *scale,
                           const float *view_center, const float *view_scale, const float *known, const float *a,
                           const float *skip_const, const float *w_xyz, const float *ch_scale, const float *ch_shift, int n_work,
                           const int *work, long long rows, float *z, float *q, int *idx, float *weight, void *stream);
int geot_scan_decode_finish(int b, int c, int n_scans, long long total, const int *labels, const long long *offsets,
                            const long long *scan_ids, int n_work, const int *work, long long rows, const float *logits,
                            const long long *out_offsets, long long *pred, long long *counts, void *stream);

/* ---- whole-scan predictions refined by their neighbours' majority (ABI 22) ---------------------------------------------------
 * geot_scan_refine: part_seg_refinement (train.py:57-73) for b batch slots, on per-vertex labels as geot_scan_predict /
 * geot_scan_vote write them, in a number of launches (six) that depends neither on b, nor on the scans' sizes, nor on what the
 * labels hold; no host synchronisation.  points, offsets, scan_ids, out_offsets: as for geot_scan_predict.  pred is refined
 * in place: vertex v of slot s is pred[out_offsets[s] + v]; the slots' ranges must not overlap.  Per slot, with snap the
 * slot's labels as they arrive:
 *   count[i], first[i]: the members of class i in snap and the lowest vertex index among them.  With fewer than two classes
 *   present the slot is left alone.  Otherwise every present class i with count[i] < n, or whose bit i of allowed[s] is clear
 *   (allowed (b) 32-bit masks on the device; NULL: every class is allowed), is refined, the classes in ascending first[i]:
 *     the queries are the vertices with snap == i (never a vertex that an earlier step relabelled to i);
 *     each takes its n + 1 nearest vertices of the same scan, itself included, by (d2, vertex index), d2 = ((dx dx) +
 *     (dy dy)) + (dz dz) as geot_three_nn forms it; an entry that was never filled (fewer than n + 1 finite distances) does
 *     not vote;
 *     it counts their CURRENT labels -- earlier steps' changes are seen, this step's are not: all queries of a step are
 *     computed before one is written -- sets the count of class i to zero and takes the first maximum (the lowest class among
 *     equals; all zero: class 0).
 * A label outside [0, c) is never a query, never votes and is never written.  Integer atomics only, and no result depends
 * on their order: the same call gives the same bits.
 * stats (optional): (b, 4) int32, WRITTEN (a skipped slot: zeros) -- steps taken, queries, vertices whose label changed,
 * labels outside [0, c).
 * ws: geot_scan_refine_ws_bytes(b, total_out, n) bytes, 16-byte aligned, contents irrelevant; total_out = the length of pred
 * (every out_offsets[s] + size of slot s <= total_out).  It holds the census, the plan, a query list of total_out ints and
 * the neighbour table of total_out (n + 1) ints: the worst case, since the query count stays on the device.
 * A slot whose scan_ids entry lies outside [0, n_scans), whose offsets pair is not 0 <= lo < hi <= total with hi - lo <=
 * 2^31 - 1, or whose out_offsets entry does not leave room for it in a ws_bytes-sized workspace, is skipped: nothing of it is
 * read or written.  That room is (ws_bytes - geot_scan_refine_ws_bytes(b, 0, n)) / (4 (n + 2)) vertices -- total_out exactly for a
 * workspace of the size asked for, more for a larger one: the check guards the workspace, the length of pred is the caller's.  0 <= b <= 65535 (0: nothing to do), 1 <= c <= GEOT_NTM_MAX_C, 1 <= n <= 63 (the wave's best-k list holds
 * one entry per lane: n + 1 <= 64), n_scans >= 1, total >= 1, no NULL among points, offsets, scan_ids, out_offsets, pred and ws,
 * ws_bytes >= geot_scan_refine_ws_bytes(b, 0, n); anything else is hipErrorInvalidValue before any launch.
 * geot_scan_refine_ws_bytes: -1 for arguments outside these ranges or total_out < 0. */
long long geot_scan_refine_ws_bytes(int b, long long total_out, int n);
int geot_scan_refine(int b, int c, int n, int n_scans, long long total, const float *points, const long long *offsets,
                     const long long *scan_ids, const long long *out_offsets, const unsigned *allowed, long long *pred,
                     int *stats, void *ws, long long ws_bytes, void *stream);

/* ---- per-tooth moments of whole-scan labels: what the 3DTeethSeg challenge scores are made of (ABI 32) ------------------------
 * geot_tooth_moments: for b batch slots, per class the vertex count, the position sum and the axis-aligned extent of the
 * LABELLED and of the PREDICTED vertices, and their overlap -- everything TSA, TLA and TIR need (geot_amd/validation.py
 * tooth_scores_from_moments) -- in one launch whatever the batch holds, no host synchronisation, integer atomics only.
 * The scans lie concatenated as for geot_scan_predict (points (total, 3) fp32, labels (total) int32, offsets, scan_ids, the
 * work records (slot, first vertex, vertex count, ignored) of scan_work_table, one workgroup each, and their skip rules: an
 * unusable slot or record is neither read nor counted); pred: int64 per vertex, vertex v of slot s at out_offsets[s] + v, as
 * geot_scan_predict / geot_scan_vote / geot_scan_cover / geot_scan_decode_finish / geot_scan_refine leave it; center (b, 3)
 * fp32: the batch's `center`, the origin the slot's positions are quantised around.
 * Per vertex v of slot s: d = points[v] - center[s], one fp32 subtraction per axis; the position is USABLE iff all three d are
 * finite and |d| < 16384; q = rint(d * 65536.0f), ties to even, a 64-bit integer per axis (|q| < 2^30; the resolution is
 * 2^-16 of a coordinate unit).  An unusable vertex adds 1 to the slot's last counter and nothing else.  A usable one joins the
 * label side of class k iff labels[v] == k, the prediction side of class k iff pred[v] == k, k in [0, c); a value outside
 * [0, c) on one side leaves the other side untouched.
 * moments: b rows of 21 c + 2 int64, zeroed by the caller; counts and sums are ADDED to and extents MAX-combined, so calls
 * over parts of a work table give the bits of one call over the whole.  Per class k, entries 21 k + ...
 *   [0] label-side vertex count   [1..3] sum of q per axis   [4..6] max(q + 2^30) per axis   [7..9] max(2^30 - q) per axis
 *   [10..19] the same ten entries of the prediction side      [20] vertices with label == pred == k
 * (both extent entries are positive wherever the count is: a zero row is the empty state, min = 2^30 - entry); the row ends
 * with [21 c] the vertices with label in [1, c) and pred in [1, c), and [21 c + 1] the unusable positions.
 * Everything is an integer: no result depends on the order of arrival, and a numpy restatement gives the same bits.
 * GEOT_TOOTH_MOMENTS_IMPL=basic (read at every call) takes the straightforward form -- one LDS atomic per lane and entry --
 * in place of the one that combines equal classes inside a wave first; the same bits.
 * 0 <= b <= 65535 (0: nothing to do), 1 <= c <= GEOT_NTM_MAX_C, n_scans >= 1, total >= 1, n_work >= 0 (0: nothing to do), no
 * NULL among points, labels, offsets, scan_ids, center, out_offsets, pred and moments, work not NULL and 16-byte aligned;
 * anything else is hipErrorInvalidValue before any launch. */
int geot_tooth_moments(int b, int c, int n_scans, long long total, const float *points, const int *labels,
                       const long long *offsets, const long long *scan_ids, const float *center, int n_work, const int *work,
                       const long long *out_offsets, const long long *pred, long long *moments, void *stream);

/* ---- whole-scan labels split into connected pieces, stray islands relabelled (ABI 34) ------------------------------------------
 * geot_scan_islands: the connected components of equal-label vertices over a neighbour table of each whole scan, and the
 * clean-up built on them -- a piece that is too small, of a class the jaw does not allow, or not the largest of a class that is
 * kept to one piece takes the majority label of what surrounds it -- for b batch slots in a number of launches (six; four in
 * the components-only form below) that depends neither on b, nor on the scans' sizes, nor on what the labels hold; no host
 * synchronisation, nothing read back, kernels only (no memset node: the call captures as kernel nodes).
 * offsets, scan_ids, out_offsets and the slots: as for geot_scan_refine; M_s is the vertex count of slot s's scan.  pred:
 * int64, vertex v of slot s at pred[out_offsets[s] + v]; the slots' ranges must not overlap.  nbr: (total_out, k) int32, row
 * out_offsets[s] + v lists neighbours of v as vertex indices local to the slot's scan; an entry that is negative, >= M_s or
 * equal to v DOES NOT EXIST; duplicates are harmless for the components and count once each in a vote.  keep, allowed: (b)
 * 32-bit class masks on the device, either may be NULL (keep NULL: no class is kept to its largest piece; allowed NULL: every
 * class is allowed).  Per usable slot, with L the slot's labels as they arrive (a snapshot):
 *   edges       {v, u} is an edge iff u is an existing entry of nbr[v] and 0 <= L[v] == L[u] < c.  The table is directed, the
 *               edge is not: one entry in either row joins the two.
 *   components  comp[v] (optional, (total_out) int32 laid out like pred; NULL: not written) = the lowest vertex index in v's
 *               connected component.  A vertex whose label is outside [0, c) is its own component; it never becomes an
 *               island, never votes and is never written.  comp describes the labels as they ARRIVED.
 *   size        the vertices of a component; the LARGEST component of class i in the slot is the one of greatest size, the one
 *               with the lowest root (= comp) among equals.
 *   islands     a component of class i is an island iff size < min_size, or bit i of allowed[s] is clear, or bit i of keep[s]
 *               is set and it is not the largest of its class.
 *   votes       an island's vote is a count per class j over all v in the island and all existing entries u of nbr[v]
 *               (forward entries only: rows of other vertices that name v do not count) with 0 <= L[u] < c, L[u] != i and u's
 *               component not an island.  The island's new label is the class with the most votes, the lowest class among
 *               equals; an island with no vote at all is STRANDED and keeps its label.  Counts are 32-bit: M_s k < 2^32.
 *   write       every vertex of an island that is not stranded gets the new label.  All decisions are taken from the snapshot
 *               before any label is written: one pass, not a fixed point.
 * With min_size <= 1, keep NULL and allowed NULL nothing can be an island: pred is not written and the vote and write
 * launches are left out -- the components-only form.  (keep given and all zero: six launches, nothing written either.)
 * stats (optional): (b, 4) int32, WRITTEN (a skipped slot: zeros) -- components among the labels in [0, c), islands, vertices
 * whose label changed, vertices in stranded islands.
 * Integer atomics only and no result depends on their order -- canonical roots (the component minimum), packed (size, ~root)
 * maxima, vote counts added per class -- so the same call gives the same bits and a numpy restatement gives them too.  The
 * components come from a lock-free union-find by hooking: a root is only ever linked under a smaller vertex, by
 * compare-and-swap on its own parent word, read with relaxed agent-scope atomics; hooking and flattening are separate
 * launches; every loop ends by the decrease of a vertex index and no workgroup ever waits for another.
 * GEOT_SCAN_ISLANDS_IMPL=basic (read at every call) counts the sizes with one atomic per vertex in place of the form that
 * combines equal roots inside a wave first; the same bits.
 * ws: geot_scan_islands_ws_bytes(b, total_out, c) bytes, 16-byte aligned, contents irrelevant; total_out = the length of pred
 * (every out_offsets[s] + M_s <= total_out).  It holds per slot and class the largest piece, and per vertex a parent, a size
 * and c vote counts.  A slot whose scan_ids entry lies outside [0, n_scans), whose offsets pair is not 0 <= lo < hi <= total
 * with hi - lo <= 2^31 - 1, or whose out_offsets entry does not leave room for it in a ws_bytes-sized workspace -- (ws_bytes -
 * geot_scan_islands_ws_bytes(b, 0, c)) / (4 (c + 2)) vertices -- is skipped: nothing of it is read or written.
 * 0 <= b <= 65535 (0: nothing to do), 1 <= c <= GEOT_NTM_MAX_C, 1 <= k <= 32, min_size >= 0, n_scans >= 1, total >= 1, no NULL
 * among offsets, scan_ids, out_offsets, nbr, pred and ws, ws 16-byte aligned, ws_bytes >= geot_scan_islands_ws_bytes(b, 0, c);
 * anything else is hipErrorInvalidValue before any launch.  geot_scan_islands_ws_bytes: -1 for arguments outside these ranges
 * or total_out < 0. */
long long geot_scan_islands_ws_bytes(int b, long long total_out, int c);
int geot_scan_islands(int b, int c, int k, int min_size, int n_scans, long long total, const long long *offsets,
                      const long long *scan_ids, const long long *out_offsets, const int *nbr, const unsigned *keep,
                      const unsigned *allowed, long long *pred, int *comp, int *stats, void *ws, long long ws_bytes, void *stream);

/* ---- one-ring neighbour tables of whole-scan triangle meshes (ABI 36) -----------------------------------------------------------
 * geot_mesh_neighbours: for b batch slots the table geot_scan_islands reads, built from the scans' triangles and not from a
 * spatial search -- seven launches whatever the slots, their sizes and their faces; no host synchronisation, nothing read back,
 * kernels only (no memset node: the call captures as kernel nodes).
 * offsets, scan_ids, out_offsets and the slots: as for geot_scan_islands; M_s is the vertex count of slot s's scan.  faces:
 * (total_faces, 3) int32 vertex indices local to their scan, the scans' faces concatenated; face_offsets (n_scans + 1): scan i's
 * faces are rows face_offsets[i] .. face_offsets[i + 1] of faces.  face_out_offsets (b + 1, device): the prefix of the slots'
 * face counts within this batch (slot s has face_out_offsets[s + 1] - face_out_offsets[s] faces); batch_faces: the same total
 * as a host value -- every usable slot's pair lies in [0, batch_faces].  nbr: (total_out, k) int32, WRITTEN, laid out exactly
 * as geot_scan_islands reads it.  Per usable slot:
 *   usable face  a face is usable iff all three of its indices lie in [0, M_s).  Any other face is IGNORED as a whole and counted;
 *                an index outside that range is never used as an address.
 *   row          row out_offsets[s] + v holds the DISTINCT vertices u != v that share a usable face with v, in ASCENDING index
 *                order; more than k of them: the k lowest (v is TRUNCATED).  Every unused entry is -1; a vertex in no usable
 *                face has a row of -1.  A usable face with a repeated index contributes its remaining distinct pair (none when
 *                all three are equal); v itself is never stored.  Duplicate faces and either winding change nothing.
 * stats (optional): (b, 4) int32, WRITTEN (a skipped slot: zeros) -- usable faces, ignored faces, truncated vertices, the longest
 * row written (the most entries other than -1 in a row of the slot: at most k).
 * Every output is an integer and depends on the SET of the slot's faces only -- not on their order, on the order of a face's
 * corners or on the schedule -- so the same call gives the same bits and a numpy restatement gives them too.  Integer atomics
 * only (raw degrees, fill cursors, the stats).  The form: per face 2 is added to the raw degree of each corner; an exclusive
 * scan of the raw degrees over all vertex rows (block-local scan, scan of the block sums, add: no look-back, no workgroup ever
 * waits for another); per face each corner reserves two entries of its raw row on a cursor and stores the two other corners;
 * per vertex the k lowest distinct values of its raw row are extracted by repeated "smallest value greater than the last one
 * written", with one round more to detect truncation.  A raw row of at most GEOT_MESH_NEIGHBOURS_LANE_ROW entries (that many / 2
 * faces at the vertex) is walked by one lane, a longer one by a whole wave.  Every loop is bounded by a count known at its start.
 * GEOT_MESH_NEIGHBOURS_IMPL=basic (read at every call): a lane per vertex whatever the row, one stats atomic per lane in place
 * of the form combined inside the wave; the same bits.
 * ws: geot_mesh_neighbours_ws_bytes(b, total_out, batch_faces) bytes, 16-byte aligned, contents irrelevant; total_out = the
 * rows of nbr (every out_offsets[s] + M_s <= total_out).  It holds the 6 batch_faces raw entries (24 batch_faces bytes, rounded up
 * to 16) and total_out + total_out / 4096 + 2 units of 16 bytes: per vertex row its row start and its cursor, per started 4096
 * rows a block sum, and the grand total (a whole unit per row, so that the size names total_out exactly: the call is not told
 * total_out and takes its vertex capacity from ws_bytes).  A slot whose scan_ids entry lies outside [0, n_scans), whose offsets
 * pair is not 0 <= lo < hi <= total with hi - lo <= 2^31 - 1, whose out_offsets entry does not leave room for it in a
 * ws_bytes-sized workspace -- the total_out that geot_mesh_neighbours_ws_bytes(b, total_out, batch_faces) = ws_bytes names --,
 * whose face_offsets pair is not 0 <= lo <= hi <= total_faces, or whose face_out_offsets pair is not 0 <= a <= z <= batch_faces
 * with z - a = hi - lo is skipped: nothing of it is read or written.  The usable slots' ranges of rows must not overlap
 * (overlapping ranges give wrong rows, never an access outside nbr or ws).
 * 0 <= b <= 65535 (0: nothing to do), 1 <= k <= 32, n_scans >= 1, total >= 1, total_faces >= 0, 0 <= batch_faces,
 * 6 batch_faces <= 2^31 - 1, no NULL among offsets, face_offsets, scan_ids, out_offsets, face_out_offsets, nbr and ws (faces may
 * be NULL only when total_faces == 0), ws 16-byte aligned, ws_bytes >= geot_mesh_neighbours_ws_bytes(b, 0, batch_faces);
 * anything else is hipErrorInvalidValue before any launch.  geot_mesh_neighbours_ws_bytes: -1 for arguments outside these
 * ranges, total_out < 0 or total_out > 2^30. */
long long geot_mesh_neighbours_ws_bytes(int b, long long total_out, long long batch_faces);
int geot_mesh_neighbours(int b, int k, int n_scans, long long total, long long total_faces, const int *faces,
                         const long long *offsets, const long long *face_offsets, const long long *scan_ids,
                         const long long *out_offsets, const long long *face_out_offsets, long long batch_faces, int *nbr,
                         int *stats, void *ws, long long ws_bytes, void *stream);

/* ---- per-vertex discrete Gaussian curvature of whole-scan triangle meshes (ABI 37) ----------------------------------------------
 * What the reference reads from files made offline with trimesh.curvature.discrete_gaussian_curvature_measure(mesh,
 * mesh.vertices, radius) (openpoints/dataset/io.py:51-57), here from the device-resident scans.  The semantics are restated from
 * trimesh's documentation; agreement with trimesh itself is NOT tested (it is not available where this was written).
 *   angle      of a face (a, b, c) at corner a: atan2(|e1 x e2|, e1 . e2), e1 = b - a, e2 = c - a
 *   defect(v)  2 pi - (the sum of the angles at v over all faces at v): boundary vertices too; a vertex in no face has 2 pi
 *   curvature(v) = the sum of defect(u) over all vertices u of the same scan with |u - v| <= radius, v included; radius in the
 *              scan's raw units
 *   batch form (|cur[sel]| - min_s) / (max_s - min_s), min / max of |cur| over the WHOLE scan; 0 everywhere when max == min
 *              (the reference's commented code would give NaN there)
 * Rules of this library, where trimesh's behaviour cannot be looked up:
 *   - a face with an index outside [0, M_s) or with a repeated index is IGNORED as a whole and counted; an index outside the
 *     range is never used as an address
 *   - every other face is USABLE; a usable face with a zero-length edge (two corners with equal coordinates) or a non-finite
 *     coordinate is DEGENERATE: it contributes three zero angles and is counted (among the usable ones too)
 *   - duplicate faces count twice: the result depends on the MULTISET of faces, not on their order, their winding or the order
 *     of a face's corners
 *   - a vertex with a non-finite coordinate is in nobody's ball, its own included (d2 <= r2 is false)
 * All three entry points launch kernels only on the given stream: no memset node, no host synchronisation, no float atomic,
 * nothing read back.
 *
 * geot_mesh_angle_defects: three launches.  The slot, offset and skip conventions are geot_mesh_neighbours' (offsets, scan_ids,
 * out_offsets, face_offsets, face_out_offsets, batch_faces; ragged scans read in place); points: (total, 3) float32, the set's
 * vertices.  total_out: the rows of defect_q, told (every usable slot has out_offsets[s] + M_s <= total_out).  defect_q:
 * (total_out) long long, WRITTEN for the rows of the usable slots: llrint(2 pi 2^32) - sum of llrint((double)angle 2^32) over
 * the usable faces' corners at the vertex, 2 pi taken from the double constant.  The three angles of a face are computed
 * independently in un-contracted fp32, each from (corner, the two others) in the symmetric form above (the cross product's
 * components only change sign and the dot product's products commute when the two others are swapped), with an atan2 of +, -,
 * *, correctly rounded / and sqrtf alone (range reduction to |t| <= tan(pi / 8) and a ten-term Taylor polynomial: truncation
 * below 4.5e-10; see csrc/mesh_curvature.hip) -- a numpy float32 restatement gives the same bits.  An angle whose |e1 x e2| or
 * e1 . e2 overflows is 0.  The quantised angles are added with 64-bit INTEGER atomics into defect_q itself, zeroed by the first
 * kernel: every word is independent of the schedule.
 * stats (optional): (b, 4) int32, WRITTEN (a skipped slot: zeros) -- usable faces, ignored faces, degenerate faces, vertices in
 * no usable face.
 * Overflow: a vertex's sum is at most valence * pi * 2^32 < 2^63 for every valence a call can hold (batch_faces < 2^29).  The
 * ball sum below adds at most M values: M * max |defect_q| must stay below 2^63 (2^24 vertices: |defect_q| < 2^39, a valence
 * of 40 flat angles); it wraps modulo 2^64 beyond.
 * ws: geot_mesh_angle_defects_ws_bytes(total_out) bytes (4 per row, rounded up to 16, plus 16: the valence counters), 16-byte
 * aligned, contents irrelevant.  A slot is skipped -- nothing of it is read or written -- under geot_mesh_neighbours' rules,
 * with total_out in place of the workspace's capacity, and when its scan has more than GEOT_CURVATURE_MAX_SCAN vertices.
 * 0 <= b <= 65535 (0: nothing to do), n_scans >= 1, total >= 1, total_faces >= 0, 0 <= batch_faces, 6 batch_faces <= 2^31 - 1,
 * 0 <= total_out <= 2^30, no NULL among points, offsets, face_offsets, scan_ids, out_offsets, face_out_offsets, defect_q and ws
 * (faces may be NULL only when total_faces == 0), ws 16-byte aligned and large enough; anything else is hipErrorInvalidValue
 * before any launch.  geot_mesh_angle_defects_ws_bytes: -1 for total_out outside [0, 2^30].
 *
 * geot_scan_ball_sum: for the M vertices of ONE scan, out[v] = (float)((double)S * 2^-32), S = the 64-bit integer sum of
 * value[u] over all u with sqdist3(u, v) <= radius * radius, both sides in un-contracted fp32 (geot_distance_mode's
 * expression), v itself included.  points: (M, 3) float32; value: (M) long long; out: (M) float32, WRITTEN; absminmax: two
 * unsigned words, WRITTEN: the minimum and the maximum of |out| over the scan as order-preserving keys (a non-negative float's
 * bits with the top bit set), by integer atomicMin / atomicMax.  It knows nothing about curvature.  Seven launches: the grid
 * build of geot_ball_query_ws (cell edge >= 1.0001 radius, at most 32 cells per axis), a two-word init, and one query kernel
 * that walks the 3 x 3 x 3 block of every vertex's cell, the vertices taken in the grid's record order: a lane per vertex (the
 * lanes of a wave mostly share their block, so their loads coincide); GEOT_BALL_SUM_IMPL=basic (read at every call): a wave per
 * vertex with a lane per candidate, the slower form on scan-sized meshes.  Integer sums: the same bits either way and on every
 * call.  At most 32 cells per axis: on a scan of 60 mm and a radius of 0.1 a block holds on the order of a thousand candidates
 * for a handful of members; a finer hashed grid is the open end.
 * ws: geot_scan_ball_sum_ws_bytes(M) bytes (= geot_knn_grid_ws_bytes(1, M)), 16-byte aligned, contents irrelevant.
 * 1 <= M <= GEOT_CURVATURE_MAX_SCAN, radius finite and > 0, no NULL, ws aligned and large enough; anything else is
 * hipErrorInvalidValue before any launch.  geot_scan_ball_sum_ws_bytes: -1 for M outside that range.
 *
 * geot_curvature_sample: ONE launch.  curvature: (total) float32, the set's flat curvature; absminmax: (n_scans, 2) unsigned, the
 * scans' key pairs as geot_scan_ball_sum wrote them; offsets / scan_ids (s): as for geot_cloud_sample_batch; sel: (s, m) int64
 * vertex indices local to each slot's scan.  out: (s, m) float32, WRITTEN: (|curvature| - min) / (max - min) of the slot's
 * scan in fp32, 0 everywhere unless max > min.  bad: (s) int32, WRITTEN: 0, 1 when an index lies outside the slot's scan (that
 * entry is 0 and the index is never used as an address), 2 for an unusable slot (scan id or offsets pair, as
 * geot_cloud_sample_batch: a row of zeros, nothing read).
 * 0 <= s <= 65535 (0: nothing to do), m >= 1, n_scans >= 1, total >= 1, no NULL; anything else is hipErrorInvalidValue before any
 * launch. */
long long geot_mesh_angle_defects_ws_bytes(long long total_out);
int geot_mesh_angle_defects(int b, int n_scans, long long total, long long total_faces, const float *points, const int *faces,
                            const long long *offsets, const long long *face_offsets, const long long *scan_ids,
                            const long long *out_offsets, const long long *face_out_offsets, long long batch_faces,
                            long long total_out, long long *defect_q, int *stats, void *ws, long long ws_bytes, void *stream);
long long geot_scan_ball_sum_ws_bytes(int m);
int geot_scan_ball_sum(int m, float radius, const float *points, const long long *value, float *out, unsigned *absminmax,
                       void *ws, long long ws_bytes, void *stream);
int geot_curvature_sample(int s, int m, int n_scans, long long total, const float *curvature, const unsigned *absminmax,
                          const long long *offsets, const long long *scan_ids, const long long *sel, float *out, int *bad,
                          void *stream);

/* ---- transform lists as per-view programs (ABI 16) ---------------------------------------------------------------------------
 * geot_view_program: geot_fixmatch_views for ANY list of the reference's point transforms that keeps the point count
 * (openpoints/transforms/point_transformer_gpu.py).  The host compiles the list, with one item's random draws, into ops
 * (geot_amd/openpoints/dataset/view_program.py); j jobs run in ONE launch, one workgroup per job, no host synchronisation.
 * jobs: j records of GEOT_VIEW_PROGRAM_JOB_WORDS 32-bit words, once on the device (what the kernel reads) and once on the
 * host (jobs_host, the same bytes: what this entry point checks before it launches):
 *   [0] int row of raw (n_rows, m, 3)    [1] int output row in pos / x / heights (n_out rows each)    [2] int op count, 0 ..
 *   GEOT_VIEW_MAX_OPS    [3] int first row of the job in noise (n_noise, m, 3)    [4] int first row of the job in mask
 *   (n_mask, m)    [5..7] reserved    then GEOT_VIEW_MAX_OPS ops of 14 words: int kind, int arg, float f[12].
 * With p the job's cloud (initially its row of raw), per op, every statement one fp32 operation, left to right:
 *    1 SCALE            p *= f[0..2]
 *    2 CENTER_NORM      arg bit 0 centring, bit 1 normalising, bits 2-3 the gravity column g:
 *                       heights (n_out, m, 1) = p[:, g] - min(p[:, g]); p -= mean(p) if centring; p /= mx if normalising,
 *                       mx = max_i sqrtf((p0^2 + p1^2) + p2^2) of the (centred) cloud
 *    3 XYZ_ALIGN        arg = g:  p -= mean(p); p[:, g] -= min(p[:, g])
 *    4 TRANSLATE        p += f[0..2]
 *    5 SCALE_TRANSLATE  p = p * f[0..2] + f[3..5]                        (two roundings)
 *    6 JITTER           p += noise[row [3] + arg]                         (the host finishes the noise: scaled, clamped)
 *    7 SCALE_JITTER     p = p * f[0..2] + noise[row [3] + arg]
 *    8 ROTATE           p_k = ((p0 f[3k] + p1 f[3k+1]) + p2 f[3k+2])      (f = R, row-major)
 *    9 FLIP             arg = axis:  p[:, axis] = max(ALL coordinates of p) - p[:, axis]
 *   10 ZERO             p = 0
 *   11 MASK             p *= mask[row [4] + arg]                          (per point)
 *   12 STORE_X          x (n_out, 3, m) channel-first = p (arg mode 0), 0 (mode 1) or p * mask[row [4] + (arg >> 2)] (mode 2);
 *                       mode = arg & 3
 * pos (n_out, m, 3) = p after the last op.  view_center (j, 3) / view_scale (j): the mean and mx of the job's last op 2 or 3
 * (0 / 1 for the part it does not compute, and for a job without such an op).  The mean is fp64 sums in geot_fixmatch_views'
 * fixed tree, rounded once; min / max propagate NaN as torch does; results are bit-reproducible, and the program SCALE,
 * STORE_X, CENTER_NORM (centring, normalising), ROTATE, TRANSLATE produces the bits of geot_fixmatch_views.  Up to
 * GEOT_VIEW_REG_POINTS points a job's cloud stays in registers across all ops; beyond, every op streams it through the job's
 * pos row.  heights is written by CENTER_NORM ops alone and may be NULL when no job has one; noise / mask may be NULL when
 * n_noise / n_mask is 0.
 * 1 <= j <= 65535, 1 <= m <= 357 913 941, n_rows >= 1, n_out >= 1, n_noise >= 0, n_mask >= 0, no other NULL pointer, every
 * row in range, every op count <= GEOT_VIEW_MAX_OPS, every kind and arg known, no output row named twice; anything else is
 * hipErrorInvalidValue before any launch.  (The kernel repeats the per-job test on the device copy: a job that fails it
 * there writes nothing but NaN to its view_center / view_scale.) */
#define GEOT_VIEW_MAX_OPS 16
#define GEOT_VIEW_PROGRAM_JOB_WORDS (8 + 14 * GEOT_VIEW_MAX_OPS)
int geot_view_program(int j, int m, int n_rows, int n_out, int n_noise, int n_mask, const float *raw, const void *jobs_host,
                      const void *jobs, const float *noise, const float *mask, float *pos, float *x, float *heights,
                      float *view_center, float *view_scale, void *stream);

/* ---- the batchers' vertex sample drawn on the device (ABI 19) --------------------------------------------------------------------
 * geot_sample_draw: what the reference draws per item on the host, np.random.choice(N, m, replace=N < m)
 * (openpoints/dataset/tooth_semi/tooth_dataset.py:134-135, 340-341), for the s slots of a batch in ONE launch -- grid
 * (ceil(m / 256), s), one thread per output element, no workspace, no host synchronisation.  NOT numpy's stream: a
 * counter-based generator, so sel depends on (seed, draw id, position) alone and is the same in every process.
 * The scans are those of geot_cloud_sample_batch: offsets (n_scans + 1) int64 on the device, scan_ids (s) int64 on the device
 * or NULL (slot i is set scan i); slot i works on n = the size of its scan, read on the device and checked as there
 * (scan id in [0, n_scans), 0 <= lo < hi <= total, hi - lo <= 2^31 - 1).  sel (s, m) int64, indices LOCAL to the slot's scan:
 * what geot_cloud_sample_batch takes as sel.  bad (s) int32: 2 for a slot whose table entry is unusable (its row of sel is
 * zeros), 0 otherwise.  Slot i draws with the draw id d = draw_base + i (mod 2^64); a caller that never hands out an id
 * twice never repeats a row.
 * Generator: Philox4x32-10 -- multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds,
 * the key bumped between rounds -- with the key (seed lo, seed hi); counter words are written (c0, c1, c2, c3) below.
 *   n >= m  (replace=False): sel[i][j] = pi_d(j), pi_d a keyed bijection on [0, 2^b) walked back into [0, n): while the
 *           value is >= n, pi_d is applied again.  b = max(10, bit length of n - 1), lb = b / 2 (floor), rb = b - lb,
 *           x = (L << rb) | R; eight rounds r = 0..7: even r  L ^= F(R, r) & (2^lb - 1), odd r  R ^= F(L, r) & (2^rb - 1),
 *           F(v, r) = word 0 of Philox on (v, r, d lo, d hi).  A row is m distinct indices; from n = 512 on fewer than two
 *           applications are expected per element, below the 10-bit floor costs up to 1024 / n (it is there for the
 *           quality of the small permutations, which the natural width does not mix).
 *   n <  m  (replace=True): sel[i][j] = the high 64 bits of (w0 | w1 << 32) * n, (w0, w1) = words 0 and 1 of Philox on
 *           (j, 0xFFFFFFFF, d lo, d hi).
 * Integer arithmetic only, no atomics, no dependence on arrival order: bit-reproducible (tests/_sample_draw_ref.py restates
 * it in numpy).
 * 1 <= s <= 65535, m >= 1, n_scans >= 1, total >= 1, offsets, sel and bad not NULL; anything else is hipErrorInvalidValue
 * before any launch. */
int geot_sample_draw(int s, int m, int n_scans, long long total, const long long *offsets, const long long *scan_ids,
                     unsigned long long seed, unsigned long long draw_base, long long *sel, int *bad, void *stream);
/* (ABI 30) geot_sample_draw_cover: the same arguments, slot / bad / scan-table rules, launch shape and integer arithmetic,
 * plus pass, 0 <= pass <= 2^31 - 1.  With sigma_d the walked bijection above (b = max(10, bit length of n - 1), the eight
 * Feistel rounds, applied again while the value is >= n) used for EVERY n >= 1 -- the multiply-high draw of n < m is not:
 *   q = pass * m + j (64-bit),   sel[i][j] = sigma_d(q mod n).
 * So for n >= m pass 0 is geot_sample_draw's row for the same id; passes 0 .. ceil(n / m) - 1 together name every vertex of
 * [0, n) (consecutive windows of one permutation); positions with q >= n are wrap-around fill that keeps the cloud at m
 * points and re-uses the start of the permutation.  pass < 0 is refused like the other arguments. */
int geot_sample_draw_cover(int s, int m, int n_scans, long long total, const long long *offsets, const long long *scan_ids,
                           unsigned long long seed, unsigned long long draw_base, int pass, long long *sel, int *bad,
                           void *stream);

/* ---- the batchers' view parameters, jitter noise and colour masks drawn on the device (ABI 20) -----------------------------------
 * geot_view_draw: what ViewProgram.draw draws per item on the host (a handful of scalars per view; an (m, 3) normal row per
 * jittering transform and an (m,) uniform row per ChromaticPerDropGPU) for the j jobs of a batch in ONE launch in front of
 * geot_view_program -- grid (ceil(m / 256), j), no workspace, no atomics, no host synchronisation.  It writes jobs (j
 * records of GEOT_VIEW_PROGRAM_JOB_WORDS words), noise (n_noise, m, 3) and mask (n_mask, m), all on the device and all in
 * geot_view_program's layout, from two tables the host compiles once per (list, batch layout), with nothing random in them,
 * each once on the device (tmpl, plans: what the kernel reads) and once on the host (tmpl_host, plans_host, the same bytes:
 * what this entry point checks):
 *   tmpl   j geot_view_program job records whose op lists are the lists' WORST case -- every RandomHorizontalFlip is two
 *          FLIP ops, every ChromaticDropGPU acting on pos a ZERO op, STORE_X in mode 2 when a per-point mask can reach x --
 *          with every drawn float at its neutral value.  Hand the same table to geot_view_program as jobs_host.
 *   plans  j records of GEOT_VIEW_DRAW_PLAN_WORDS words: [0] int view of the slot (0 only / labelled, 1 weak, 2 strong)
 *          [1] int slot: the job draws with the draw id d = draw_base + slot (mod 2^64)    [2] int step count, 0 ..
 *          GEOT_VIEW_DRAW_MAX_STEPS    [3] int index of the template's STORE_X op the x-side colour drops act on, or -1
 *          [4..7] reserved    then GEOT_VIEW_DRAW_MAX_STEPS steps of 12 words: int kind, int op (index into the template's
 *          ops, -1: the STORE_X op of [3]), int pos (place of the transform in its list, < 4096), int flags, float c[8].
 * A job's record is its template with the drawn fields overwritten.  Step kinds, u = a uniform, every statement ONE correctly
 * rounded fp32 operation, left to right:
 *   1 SCALE    op: SCALE / SCALE_TRANSLATE / SCALE_JITTER, f[0..2].  flags bit 0 anisotropic (unset: ONE draw serves the
 *              three), bits 1-3 scale_xyz, bits 4-5 mirror form.  v_k = u_k * c[1] + c[0] (c[0] = lo, c[1] = hi - lo);
 *              form 1: v_k *= (u'_k > c[2+k] ? 1 : -1); form 2: v_k *= (u'_k > 0.5 ? 1 : -1) * c[2+k] + (1 - c[2+k]);
 *              scale_xyz bit k unset: v_k = 1 (without anisotropy bit 0 decides for all three, as scale[0] = 1 does)
 *   2 SHIFT    op: TRANSLATE f[0..2] or SCALE_TRANSLATE f[3..5].  u_k * c[k], or with flags bit 0 ((u_k - 0.5) * 2) * c[k]
 *   3 NOISE    op: JITTER / SCALE_JITTER; fills that op's noise row.  Per point ONE generator call (w0..w3): r = sqrt(-2 ln
 *              u1), u1 = ((w >> 8) + 1) 2^-24; z = (r(w0) cos(w1), r(w0) sin(w1), r(w2) cos(w3)) with the angle u(w) turns;
 *              noise = min(max(z * c[0], -c[1]), c[1])  (c[0] = sigma, c[1] = clip)
 *   4 ROTATE   op: ROTATE f[0..8].  Per axis k: t = (c[k] * (u_k * 2 - 1)) * 0.5 turns (c = the angle bound in units of pi,
 *              |c[k]| <= 1024), the axis rotation by t; the three in the order number ((w3 >> 8) * 6) >> 24 of the six
 *              lexicographic orders; R = (A B) C, every entry (a0 b0 + a1 b1) + a2 b2; -sin is 0 - sin
 *   5 FLIP     ops op and op + 1, both FLIP.  any = u0 < c[0]; FLIP op stays when any and u1 < 0.5, FLIP op + 1 when any
 *              and u2 < 0.5; otherwise the op becomes SCALE by (1, 1, 1)
 *   6 DROP     u < c[0].  op a ZERO op: it becomes SCALE by (1, 1, 1) when NOT drawn; op -1: STORE_X's arg becomes 1 when drawn
 *   7 PERMASK  per point u > c[0] ? 1 : 0 into the mask row of op (a MASK op) or, op -1, of the STORE_X op (mode 2).  Steps
 *              that name one row write their product.
 * ln is the exponent of the 24-bit integer times fp32 ln 2 plus 2 atanh((f - 1) / (f + 1)) to the 11th power on the mantissa
 * f in [sqrt(1/2), sqrt 2); cos / sin reduce 4 t to the nearest integer exactly and use Taylor polynomials of degree 9 / 10
 * on [-pi/4, pi/4]: fp32 add, multiply, divide and square root only, NO math-library call, so the results do not change
 * with the toolchain and tests/_view_draw_ref.py reproduces every bit in numpy float32.  t = 0 gives cos 1, sin +0
 * exactly: an angle bound of 0 is R = I.
 * Generator: Philox4x32-10 as in geot_sample_draw, key (seed lo, seed hi), counter (element, tag, d lo, d hi); element = the
 * point for kinds 3 and 7, 0 otherwise; tag = 0x40000000 | view << 24 | pos << 8 | quantity with quantity 0 scale, 1 mirror,
 * 2 shift, 3 rotate, 4 flip, 5 drop, 6 noise, 7 per-point mask.  Bit 30 set and bit 31 clear: no tag equals a second counter
 * word of geot_sample_draw (0..7, 0xFFFFFFFF), so a slot's views share the slot's draw id with its vertex sample.
 * 1 <= j <= 65535, 1 <= m <= 357 913 941, n_noise >= 0, n_mask >= 0, no NULL pointer (noise / mask may be NULL when their
 * count is 0); every plan is checked against its template -- view, step count, kinds, pos, every op index in range and of a
 * kind the step may write, every noise and mask row inside the buffers, angle bounds finite -- anything else is
 * hipErrorInvalidValue before any launch.  The kernel repeats the test on the device copies; a job that fails it there
 * writes nothing. */
#define GEOT_VIEW_DRAW_MAX_STEPS 24
#define GEOT_VIEW_DRAW_PLAN_WORDS (8 + 12 * GEOT_VIEW_DRAW_MAX_STEPS)
int geot_view_draw(int j, int m, int n_noise, int n_mask, const void *tmpl_host, const void *plans_host, const void *tmpl,
                   const void *plans, unsigned long long seed, unsigned long long draw_base, void *jobs, float *noise,
                   float *mask, void *stream);

/* ---- FixMatch pseudo-label masks refined by the neighbours' probabilities (ABI 23) -------------------------------------------
 * geot_pseudo_refine: utils/pseudo_mask.py's pseudo_label_refine (mode GEOT_PSEUDO_MAX, :38-53), pseudo_label_refine_margin
 * (GEOT_PSEUDO_MARGIN, :55-90) and pseudo_label_refine_margin_v1 (GEOT_PSEUDO_MARGIN_V1, :92-170) behind their neighbour
 * search, for the b * npts points of a batch in ONE launch: no workspace, no atomics, no host synchronisation, safe to
 * capture.  prob (b, c, npts) fp32, the reference's channel-first layout; nbr (b, npts, n) int32 ids LOCAL to the point's
 * cloud -- slots 1 .. n of pointops.knn(pos, pos, n + 1): slot 0 is dropped as pseudo_mask.py:19-21 drops it, whatever it
 * holds; n the neighbourhood size, k the reference's n_neigbors.  Per point i and class cl, every statement ONE correctly
 * rounded fp32 operation in the order written (the library is built with -ffp-contract=off):
 *   1. of the n values prob[cl][nbr[i][j]] the k largest, in descending order (equal values are equal: their order cannot
 *      matter); a NaN ranks above every number, as in torch.topk;
 *   2. p = prob[cl][i], then once per taken value v, largest first:
 *        GEOT_PSEUDO_MAX, GEOT_PSEUDO_MARGIN   p = (p + beta * v) - ((p * v) * beta)                      (:48, :82)
 *        GEOT_PSEUDO_MARGIN_V1                 ub = (e_joint[cl] * p) / v;  p = (p + v) - (p * ub)         (:156-160)
 *   3. over the classes: value = the largest p (GEOT_PSEUDO_MAX), or the largest minus the second largest (the margin
 *      modes; two equal largest values give 0); NaN above every number again, as in torch.max / torch.topk;
 *   4. keep = value >= th ? 1 : 0 (a NaN value: 0).
 * beta: the reference's torch.exp(torch.tensor(-1/2)), computed by the caller in fp32.  e_joint: c fp32 entries on the
 * device (E_joint, :93-98), read in GEOT_PSEUDO_MARGIN_V1 only.  keep (b, npts) uint8, what the fused criteria take as
 * their hard mask; value (b, npts) fp32, optional (NULL: not written).  The result is the reference's bit for bit given the
 * same neighbour ids.
 * A neighbour id outside [0, npts) is never followed -- nothing is read through it: the point's keep is 0 and its value a
 * quiet NaN, every other point is unaffected; there is no flag output, and the id is not clamped into a neighbour.
 * GEOT_PSEUDO_REFINE_IMPL=point|split (read at every call) picks how a workgroup of 64 points shares the classes out -- a
 * lane per point over all classes, or four waves that take every fourth class each and merge their top two through LDS --
 * with the same bits.
 * 1 <= b <= 65535, 1 <= c <= GEOT_NTM_MAX_C (c >= 2 for the margin modes), 1 <= k <= n <= GEOT_PSEUDO_REFINE_MAX_N,
 * npts >= n + 1, a mode of the three, no NULL among prob, nbr and keep (nor e_joint in GEOT_PSEUDO_MARGIN_V1); anything else
 * is hipErrorInvalidValue before the launch. */
#define GEOT_PSEUDO_MAX 0
#define GEOT_PSEUDO_MARGIN 1
#define GEOT_PSEUDO_MARGIN_V1 2
#define GEOT_PSEUDO_REFINE_MAX_N 32
int geot_pseudo_refine(int b, int c, int npts, int n, int k, int mode, float th, float beta, const float *prob, const int *nbr,
                       const float *e_joint, unsigned char *keep, float *value, void *stream);

/* ---- the teacher-student point contrastive loss (ABI 24) ------------------------------------------------------------------------
 * utils/cluster_contrastloss.py's nativeContrastLoss_t (:1188-1408) with fixed shapes, counts kept on the device and no host
 * round trip: kernel launches only, no workspace cleared by memset, no float atomics, no dependence on arrival order --
 * bit-identical from run to run and safe to capture.  b clouds of p points, d channels, s = sample_nums; cap = b * s anchor
 * slots, of which the first A (read on the device) are in use; grids are sized by cap and slots beyond A idle: what they
 * would write stays as it arrived.  Features are read in place, point-major (b, p, d) or channel-first (b, d, p)
 * (channels_first != 0); point ids are global, cloud * p + point.
 *
 * geot_contrast_select (:1233-1264 and the draw of :1210): per cloud the candidates are the points with score >= th in
 * ascending order (a NaN score is none), K of them, m = min(K, s) anchors cand[perm[j]], j < m, packed cloud after cloud.
 *   score (b, p) fp32.  perm (b, s) int64: row c holds the first m entries of a permutation of [0, K_c); perm_q (s) int64: the
 *   first min(A, s) entries of a permutation of [0, A); both given (the host mode) or both NULL.  An entry outside its range
 *   is never followed: the anchor id / the bank row is -1, which the entry points below read as a row of zeros / skip.
 *   Both NULL: the keyed bijection of geot_sample_draw in its n >= m construction (Philox4x32-10, key = seed), n = K_c read
 *   on the device: entry j of cloud c is pi_d(j) walked back into [0, K_c) with the draw id d = *counter + c, the bank rows
 *   use n = A and d = *counter + b; the second kernel stores *counter + b + 1 to counter (every block draws from a copy the
 *   first kernel took).  counter: one unsigned long long on the device, required in this mode, not read with perm given.
 *   ws: geot_contrast_select_ws_ints(b, p) = b * p + b + 2 int32 of scratch.  anchors (cap) int32: ids of slots 0 .. A - 1,
 *   -1 beyond; count (b + 1) int32: m per cloud, then A; enqueue_rows (s) int32: anchor slots, -1 from min(A, s) on;
 *   inv (b * p) int32: the slot of a point that is an anchor, -1 otherwise.  Two launches.
 *
 * geot_contrast_loss (:1385-1388, _ppc_contrastive_andbank :1337-1377): slot a < A holds x = the row of feat_s and t = the
 * row of feat_t at anchors[a]; x^ = x / max(|x|, 1e-12), |x| = sqrt of the sum of squares (fma, channels lane, lane + 64,
 * .. per lane, then a butterfly over the wave), t^ likewise; only these A rows are normalised.  u_aj = (x^_a . t^_j) / tau
 * over the A slots, v_aq = (x^_a . bank_q) / tau over the 4 s bank rows, dot products by fma in ascending channel order, the
 * quotient a division; mu_a = max_j u_aj, nu_a = max_q v_aq, Z_a = sum_j exp(u_aj - mu_a) + sum_q exp(v_aq - nu_a),
 * W_a = sum_j exp(u_aj - mu_a) t^_j + sum_q exp(v_aq - nu_a) bank_q -- ONE streaming pass: keys in chunks of 1024, each
 * chunk in tiles of at least 16 keys with a running maximum (sum and W rescaled by exp(old - new)), the chunks merged in
 * ascending order; expf /
 * logf of the device library.  ell[a] = -(tau / tau_b) ((u_aa - mu_a) - log Z_a), u_aa by its own wave-wide dot product;
 * grad_dir[a] = t^_a - W_a / Z_a; loss = (sum of ell in a fixed tree) / A, exactly 0 when A = 0.
 *   bank (4 s, d) fp32.  Outputs xhat, that (cap, d), norm (cap) = |x|, ell (cap), grad_dir (cap, d), loss (1);
 *   ws: geot_contrast_ws_floats(b, s, d) fp32 of scratch.  Four launches.
 *
 * geot_contrast_loss_grad: upstream (1) fp32 on the device, g.  dy_a = -(g / (A tau_b)) grad_dir[a]; through the
 * normalisation as autograd of F.normalize does: |x| >= 1e-12: (dy - x^ (dy . x^)) / |x|, otherwise dy / 1e-12 (a row of norm
 * 0 included).  rows (cap, d) scratch; grad: the dense gradient in the layout of feat_s, EVERY element written (zero where
 * inv is -1) by a kernel.  Two launches.
 *
 * geot_contrast_enqueue (_queue_operations :1207-1220): cnt = min(A, s); row r < cnt of the block is
 * t^[enqueue_rows[r]] normalised once more; the block is rows [4 s - cnt, 4 s) and *ptr becomes 0 when *ptr + cnt > 4 s,
 * otherwise rows [*ptr, *ptr + cnt) and *ptr becomes (*ptr + cnt) mod 4 s.  ptr: one int64 on the device; a value outside
 * [0, 4 s) writes nothing.  A = 0 leaves bank and ptr untouched.  Call it after geot_contrast_loss has read the bank.
 * Two launches.
 *
 * 1 <= b <= GEOT_CONTRAST_MAX_B, 1 <= d <= GEOT_CONTRAST_MAX_D, 1 <= s <= GEOT_CONTRAST_MAX_S, p >= 1, b * p <= 2^31 - 1,
 * tau > 0, tau_b > 0, no NULL pointer but perm / perm_q (and counter with them); anything else is hipErrorInvalidValue before
 * any launch. */
#define GEOT_CONTRAST_MAX_B 64
#define GEOT_CONTRAST_MAX_D 256
#define GEOT_CONTRAST_MAX_S 1024
long long geot_contrast_select_ws_ints(int b, int p);
long long geot_contrast_ws_floats(int b, int s, int d);
int geot_contrast_select(int b, int p, int s, float th, const float *score, const long long *perm, const long long *perm_q,
                         unsigned long long seed, unsigned long long *counter, int *ws, int *anchors, int *count,
                         int *enqueue_rows, int *inv, void *stream);
int geot_contrast_loss(int b, int p, int d, int s, int channels_first, const float *feat_s, const float *feat_t,
                       const int *anchors, const int *count, const float *bank, float tau, float tau_b, float *xhat, float *that,
                       float *norm, float *ws, float *ell, float *grad_dir, float *loss, void *stream);
int geot_contrast_loss_grad(int b, int p, int d, int s, int channels_first, const int *count, const int *inv, const float *xhat,
                            const float *norm, const float *grad_dir, const float *upstream, float tau_b, float *rows,
                            float *grad, void *stream);
int geot_contrast_enqueue(int b, int d, int s, const int *count, const int *enqueue_rows, const float *that, float *bank,
                          long long *ptr, void *stream);

/* ---- the fused tail of an iteration: gradient clip + AdamW + the teacher's EMA (ABI 25) -------------------------------------
 * torch.nn.utils.clip_grad_norm_(norm_type=2, error_if_nonfinite=False), torch.optim.AdamW's step (decoupled weight decay,
 * both bias corrections; no amsgrad, no maximize) and t = d t + (1 - d) p for a mean teacher, over a list of T tensor
 * records, in two sweeps that read every parameter once.  The reference clips and steps in torch ops (examples/segmentation/
 * train.py:656-660, cfgs/tooth_semi/default.yaml:83) and names an ema_decay it never applies (cfgs/tooth_semi/
 * transformer_finetune_fixmatch_ntm.yaml:66).
 *
 * A record is GEOT_OPTIM_TAIL_REC_WORDS 32-bit words in a HOST array: five 64-bit device addresses p, g, exp_avg,
 * exp_avg_sq, t (t = 0: no teacher), the element count (int64), then four int32: first block (ignored on input: the
 * launcher's), group id, flags, index of the record's step counter.  Flags: GEOT_OPTIM_TAIL_CLIPPED (g is part of the norm and
 * is scaled by coef), GEOT_OPTIM_TAIL_VECTOR (ignored on input: set by the launcher when EVERY address of the record is 16-byte
 * aligned -- dwordx4 accesses; otherwise one element per access), GEOT_OPTIM_TAIL_EMA_ONLY (a buffer, or a parameter without a
 * gradient: only p and t are read, t = d t + (1 - d) p), GEOT_OPTIM_TAIL_INT64 (count int64 elements are copied from p to t).
 * A group is GEOT_OPTIM_TAIL_GROUP_WORDS words: beta1, beta2 (double), eps, weight_decay, lr (float), one word of padding and
 * a 64-bit device address of a float32 learning rate (0: use lr); at most GEOT_OPTIM_TAIL_MAX_GROUPS groups.
 *
 * The records reach the kernels BY VALUE in the kernel arguments, GEOT_OPTIM_TAIL_CAP per launch: nothing is uploaded, so the
 * calls capture into kernel nodes alone although gradient addresses change every iteration.  A workgroup of 256 threads owns
 * GEOT_OPTIM_TAIL_BLOCK_ELEMS consecutive elements of one record.
 *
 * geot_optim_tail_plan (host only): for T records with these counts, alignments (1: every address 16-byte aligned) and flags
 *   -> out[0] launches of the update sweep, out[1] launches of the norm sweep, out[2] workgroups of the update sweep, out[3]
 *   partial slots, out[4 + i] workgroups of record i, out[4 + T + i] its path (1 vector, 0 scalar).  Launch l of a sweep
 *   holds the sweep's records [l CAP, (l + 1) CAP) and is not issued when they hold no element; the norm sweep's records are
 *   the clipped ones that are neither EMA-only nor integer.  Returns 1, or 0 (n_out < 4 + 2 T, a negative count).  The
 *   launchers below call the same function.
 * geot_optim_tail_norm: slot k (fp32) = the sum of the squares of the k-th workgroup's gradient elements, workgroups counted
 *   through the clipped records in table order.  Every one of the plan's slots is written; no atomics.  n_slots: the room.
 * geot_optim_tail_finish: ONE workgroup.  clip != 0: the first n_slots slots are summed in a fixed order in double;
 *   scalars[0] = total_norm = (float)sqrt(sum), scalars[1] = coef = min(1, max_norm / (total_norm + 1e-6)) in fp32 (a NaN
 *   stays a NaN, an infinite norm gives 0, as torch.clamp does).  clip == 0: scalars = (0, 1).  Then steps[k] += 1 for the
 *   step index k of every record that is neither EMA-only nor integer (they must differ).  More than
 *   GEOT_OPTIM_TAIL_STEP_CAP such records take further launches of the same kernel.
 * geot_optim_tail_update: per element in fp32, un-contracted, in this order:
 *     g' = coef g (clipped records);  p1 = p - (lr wd) p;  m' = m + (1 - b1)(g' - m);  v' = b2 v + ((1 - b2) g') g';
 *     p' = p1 - ((lr / bc1) m') / (sqrt(v') / sqrt(bc2) + eps);  t' = d t + (1 - d) p'   (t given)
 *   with bc1 = 1 - b1^step, bc2 = 1 - b2^step from the counter geot_optim_tail_finish has just raised, formed in double.
 *   g is NOT written back (a caller drops its gradients right after: zero_grad(set_to_none=True)).  0 <= ema_decay < 1.
 * A malformed record, group or size is hipErrorInvalidValue before any launch. */
#define GEOT_OPTIM_TAIL_CAP 48             /* records per launch */
#define GEOT_OPTIM_TAIL_BLOCK_ELEMS 4096   /* elements per workgroup */
#define GEOT_OPTIM_TAIL_STEP_CAP 896       /* step counters per geot_optim_tail_finish launch */
#define GEOT_OPTIM_TAIL_REC_WORDS 16
#define GEOT_OPTIM_TAIL_GROUP_WORDS 10
#define GEOT_OPTIM_TAIL_MAX_GROUPS 4
#define GEOT_OPTIM_TAIL_CLIPPED 1
#define GEOT_OPTIM_TAIL_VECTOR 2
#define GEOT_OPTIM_TAIL_EMA_ONLY 4
#define GEOT_OPTIM_TAIL_INT64 8
int geot_optim_tail_plan(int t, const long long *counts, const int *aligned, const int *flags, long long *out, int n_out);
int geot_optim_tail_norm(int t, const void *records_host, float *slots, long long n_slots, void *stream);
int geot_optim_tail_finish(int t, const void *records_host, int clip, long long n_slots, const float *slots, float max_norm,
                           float *steps, int n_steps, float *scalars, void *stream);
int geot_optim_tail_update(int t, const void *records_host, int n_groups, const void *groups_host, const float *scalars,
                           const float *steps, int n_steps, double ema_decay, void *stream);

/* ---- the same tail with the gradients of k calls summed before one update (ABI 27; cfg step_per_update) ------------------------
 * The reference updates its optimizers every cfg.step_per_update-th iteration only (examples/segmentation/train.py:435, 440,
 * 463, 657-669): every backward adds into .grad, and clip_grad_norm_, both step() and both zero_grad() run when the count
 * reaches step_per_update.  Here the sum lives in ONE flat float32 accumulator per tail, the count in device memory, and every
 * call issues the same launches with the same arguments -- a captured graph of kernel nodes serves every call of a window.
 * The record and the group are the ones above, unchanged; g may be 0 (the parameter got no gradient in this call).
 *
 * acc / acc_offsets / n_acc: the accumulator (16-byte aligned, n_acc floats) and a DEVICE table of n_steps int64 offsets into
 *   it, indexed by a record's step-counter index; every offset a multiple of 4, offset + count <= n_acc (a record whose
 *   offset breaks that is passed over by the kernels).  Written once by the caller; nothing is uploaded per call.
 * gate: two DEVICE int32 -- gate[0] the calls of the open window (0 .. k-1 between calls), gate[1] whether the last
 *   geot_optim_tail_acc_finish was an update.
 * geot_optim_tail_acc_plan (host only): -> out[0] launches of the accumulate sweep, out[1] of the finish stage, out[2] of the
 *   update sweep, out[3] workgroups of the accumulate sweep, out[4] of the update sweep, out[5] partial slots.  The
 *   accumulate sweep holds the records that are neither EMA-only nor integer, GEOT_OPTIM_TAIL_CAP per launch in table order;
 *   the update sweep is geot_optim_tail_plan's; paths and workgroups per record are geot_optim_tail_plan's too.  Returns 1,
 *   or 0 (n_out < 6, a negative count).  The launchers below call the same function.
 * geot_optim_tail_accumulate: acc[e] = acc[e] + g[e] in fp32 for every such record with g != 0, one writer per element, and
 *   slot k (fp32) = the sum of the squares of the NEW accumulator values of the k-th workgroup of the clipped records, in
 *   geot_optim_tail_norm's partition and order: the slots are what geot_optim_tail_norm gives for the summed gradient.
 * geot_optim_tail_acc_finish: ONE workgroup.  gate[0] + 1 < k: gate = (gate[0] + 1, 0) and nothing else is written.
 *   Otherwise gate = (0, 1) and the stage is geot_optim_tail_finish: total_norm and coef from the slots, the step counters.
 * geot_optim_tail_acc_update: gate[1] == 0: every workgroup returns.  Otherwise geot_optim_tail_update with the accumulated
 *   value in the place of g; the accumulator's elements are zeroed as they are read.  EMA-only and integer records are
 *   applied under the same gate.
 * A malformed record, group or size is hipErrorInvalidValue before any launch. */
int geot_optim_tail_acc_plan(int t, const long long *counts, const int *aligned, const int *flags, long long *out, int n_out);
int geot_optim_tail_accumulate(int t, const void *records_host, float *acc, const long long *acc_offsets, long long n_acc,
                               int n_steps, float *slots, long long n_slots, void *stream);
int geot_optim_tail_acc_finish(int t, const void *records_host, int clip, long long n_slots, const float *slots, float max_norm,
                               float *steps, int n_steps, float *scalars, int *gate, int k, void *stream);
int geot_optim_tail_acc_update(int t, const void *records_host, int n_groups, const void *groups_host, const float *scalars,
                               const float *steps, int n_steps, double ema_decay, float *acc, const long long *acc_offsets,
                               long long n_acc, const int *gate, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GEOT_HIP_H */
