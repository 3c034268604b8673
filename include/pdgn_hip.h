/*
 * pdgn_hip.h -- C ABI of libpdgn_hip.so: the MI355X (gfx950) drop-in for the native
 * side of PDGN's hot path.
 *
 * Every entry point takes plain device pointers + sizes + a hipStream_t (passed as
 * void*), launches asynchronously on that stream, never allocates, never synchronises,
 * and returns 0 on success, a hipError_t value (>0) on a launch failure, or
 * PDGN_ERR_INVALID (-1) when an argument is out of the supported range.  The pointops /
 * structural-loss / BatchNorm / gather entry points keep no state.  The dense contractions
 * (pdgn_gemm_*) have state, all of it listed at pdgn_gemm_set_mode below: process-wide
 * switches (arithmetic mode, forced tile, matrix instruction: set once from the
 * environment, changed only by tests / tools), a process-wide arena for the two-part
 * mode's own scans (pdgn_gemm_set_scale_slots), and THREAD-LOCAL hand-overs (operand
 * maxima, tail workspace) that belong to the calling thread's next contraction call.
 * One process per GPU, contraction calls from one thread at a time per hand-over.
 *
 * All tensors are contiguous, batch-major; float = fp32, idx = int32 -- exactly the
 * layouts of the reference launchers cited per function (paths relative to the
 * reference repository root).
 */
#ifndef PDGN_HIP_H
#define PDGN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDGN_ERR_INVALID (-1)
#define PDGN_KNN_MAX_NSAMPLE 200 /* lib/pointops/src/knnquery/knnquery_cuda_kernel.cu:21-22 */

typedef void *pdgn_stream_t; /* hipStream_t */

/* ABI version of this header: bump it on any signature change, here and nowhere else.  The library returns it
 * (csrc/abi.hip) and pdgn_amd/_lib.py reads it, together with the ctypes signature of every prototype below, from this
 * file: keep the prototypes to `int` / `long long` results and `int`, `long long`, `unsigned [int]`,
 * `unsigned long long`, `float`, `double`, pointer and pdgn_stream_t parameters, each with a name. */
#define PDGN_ABI_VERSION 51
int pdgn_abi_version(void);

/* ------------------------------------------------------------------ pointops
 * Replaces knnquery_cuda_launcher (lib/pointops/src/knnquery/knnquery_cuda_kernel.h:14,
 * kernel knnquery_cuda_kernel.cu:6-50).  xyz (b,n,3), new_xyz (b,m,3) ->
 * idx (b,m,nsample) int32, dist2 (b,m,nsample) f32 (dist2 may be NULL).
 * Ascending (squared distance, index); for n < nsample the tail is idx 0 / +inf.
 * nsample <= PDGN_KNN_MAX_NSAMPLE. */
int pdgn_knnquery(int b, int n, int m, int nsample, const float *xyz, const float *new_xyz,
                  int32_t *idx, float *dist2, pdgn_stream_t stream);

/* Replaces grouping_forward_cuda_launcher_fast (grouping/grouping_cuda_kernel.h:19,
 * kernel grouping_cuda_kernel.cu:60-74).  points (b,c,n), idx (b,m,nsample) ->
 * out (b,c,m,nsample). */
int pdgn_grouping_forward(int b, int c, int n, int m, int nsample, const float *points,
                          const int32_t *idx, float *out, pdgn_stream_t stream);

/* Replaces grouping_backward_cuda_launcher (grouping/grouping_cuda_kernel.h:17,
 * kernel :28-46).  grad_out (b,c,m,nsample), idx -> grad_points (b,c,n), ACCUMULATED
 * into the caller's buffer (the caller zero-fills it, pointops.py:146). */
int pdgn_grouping_backward(int b, int c, int n, int m, int nsample, const float *grad_out,
                           const int32_t *idx, float *grad_points, pdgn_stream_t stream);

/* Replaces nearestneighbor_cuda_launcher_fast (interpolation/interpolation_cuda_kernel.h:22,
 * kernel interpolation_cuda_kernel.cu:134-176).  unknown (b,n,3), known (b,m,3) ->
 * dist2 (b,n,3) squared distances, idx (b,n,3). */
int pdgn_nearestneighbor(int b, int n, int m, const float *unknown, const float *known,
                         float *dist2, int32_t *idx, pdgn_stream_t stream);

/* Replaces interpolation_forward_cuda_launcher_fast (interpolation_cuda_kernel.h:23,
 * kernel :181-195).  points (b,c,m), idx/weight (b,n,3) -> out (b,c,n). */
int pdgn_interpolation_forward(int b, int c, int m, int n, const float *points,
                               const int32_t *idx, const float *weight, float *out,
                               pdgn_stream_t stream);

/* Replaces interpolation_backward_cuda_launcher (interpolation_cuda_kernel.h:20,
 * kernel :90-114).  grad_out (b,c,n) -> grad_points (b,c,m), ACCUMULATED. */
int pdgn_interpolation_backward(int b, int c, int n, int m, const float *grad_out,
                                const int32_t *idx, const float *weight, float *grad_points,
                                pdgn_stream_t stream);

/* ------------------------------------------------------------------ structural losses
 * Replaces nndistance (evaluation/pytorch_structural_losses/src/nndistance.cuh:1,
 * nndistance.cu:2-128).  xyz (b,n,3), xyz2 (b,m,3) -> result/result_i (b,n),
 * result2/result2_i (b,m): min squared distance and its argmin (lowest index on ties). */
int pdgn_nndistance(int b, int n, const float *xyz, int m, const float *xyz2, float *result,
                    int32_t *result_i, float *result2, int32_t *result2_i, pdgn_stream_t stream);

/* Replaces nndistancegrad (nndistance.cuh:2, nndistance.cu:129-154).  Zero-fills
 * grad_xyz1 (b,n,3) / grad_xyz2 (b,m,3) itself (on `stream`), then accumulates. */
int pdgn_nndistance_grad(int b, int n, const float *xyz1, int m, const float *xyz2,
                         const float *grad_dist1, const int32_t *idx1, const float *grad_dist2,
                         const int32_t *idx2, float *grad_xyz1, float *grad_xyz2,
                         pdgn_stream_t stream);

/* Replaces approxmatch (src/approxmatch.cuh:6, approxmatch.cu:3-182,299-307).
 * xyz1 (b,n,3), xyz2 (b,m,3) -> match (b,m,n); temp (b, 2*(n+m)) is scratch. */
int pdgn_approxmatch(int b, int n, int m, const float *xyz1, const float *xyz2, float *match,
                     float *temp, pdgn_stream_t stream);

/* Replaces matchcost (approxmatch.cuh:7, approxmatch.cu:184-224,309-316) -> out (b). */
int pdgn_matchcost(int b, int n, int m, const float *xyz1, const float *xyz2,
                   const float *match, float *out, pdgn_stream_t stream);

/* Replaces matchcostgrad (approxmatch.cuh:8, approxmatch.cu:229-291,318-326) ->
 * grad1 (b,n,3), grad2 (b,m,3). */
int pdgn_matchcost_grad(int b, int n, int m, const float *xyz1, const float *xyz2,
                        const float *match, float *grad1, float *grad2, pdgn_stream_t stream);

/* Fused forward-only EMD cost for the eval path (evaluation_metrics.py:26-31 calls
 * ApproxMatch then MatchCost and drops `match`): same arithmetic as
 * pdgn_approxmatch + pdgn_matchcost but `match` is never written to HBM.
 * temp: pdgn_emd_cost_temp_floats(b, n, m) floats of scratch (per pair the reference's remain / ratio vectors and the two
 * clouds as x-sorted float4 rows: the sweeps skip the runs of a tile whose exponentials are exactly zero), out (b). */
long long pdgn_emd_cost_temp_floats(long long pairs, int n, int m);
int pdgn_emd_cost(int b, int n, int m, const float *xyz1, const float *xyz2, float *temp,
                  float *out, pdgn_stream_t stream);

/* ------------------------------------------------------------------ point-deconvolution stack
 * Feature-space kNN graph of models/PDGNet_v2.py:447-458 / :488-502 (get_edge_features[_xyz]):
 * x (b,f,n) channels-first -> idx (b,n,k) int32 = ranks 1..k of the row-wise ascending order of
 * (-2<x_i,x_j> + |x_i|^2) + |x_j|^2 (rank 0 dropped; ties by index).  sqnorm (b,n) is scratch.
 * f <= 256, k <= 31.  n <= k (no reference counterpart: its slice [1 : k+1] of n sorted entries comes back short and the gather
 * fails): ranks 1 .. n-1 fill the leading slots and the remaining k - (n - 1) slots repeat rank 0, the point itself wherever it is
 * its own nearest -- an edge of length zero; this is what lets a generator start from fewer base points than it has neighbours. */
int pdgn_feature_knn(int b, int f, int n, int k, const float *x, float *sqnorm, int32_t *idx,
                     pdgn_stream_t stream);

/* Gather half of the re-associated edge convolutions (inte_conv_hk / conv2 / conv_fea / conv_xyz,
 * models/PDGNet_v2.py:559-625 applied to the edge tensors of :462-477, :505-525):
 *   out[b,n,p,c] = bias[b*bias_bstride + c] + Y[b,n,offc+c] + sum_{t<T} Y[b, idx[b,n,p+t], off + t*C + c]
 * Y (b,n,ldy) point-major, idx (b,n,k) with k >= T+P-1, out (b,n,P,C); bias may be NULL, is shared
 * (bias_bstride = 0) or per batch (bias_bstride = C: the contribution of input channels that are
 * constant over the points of a sample -- the broadcast global vector of :704-708 -- never enters
 * the per-point GEMM); offc < 0 drops the centre term. */
int pdgn_window_gather_sum(int b, int n, int k, int ldy, int T, int P, int C, int off, int offc,
                           const float *Y, const int32_t *idx, const float *bias, int bias_bstride,
                           float *out, pdgn_stream_t stream);
/* The same, also emitting the BatchNorm partial statistics of out viewed as (b*n*P, C) rows into `scratch`
 * (>= pdgn_bn_scratch_floats(b*n*P, C) floats; finish with pdgn_bn_stats_from_partials): the BatchNorm that follows
 * the gather-sum needs no statistics pass.  float4 path only (C, ldy, off, offc, bias_bstride multiples of 4). */
int pdgn_window_gather_sum_stats(int b, int n, int k, int ldy, int T, int P, int C, int off, int offc,
                                 const float *Y, const int32_t *idx, const float *bias, int bias_bstride,
                                 float *out, float *scratch, pdgn_stream_t stream);

/* Its adjoint: dY[b, idx[b,n,p+t], off+t*C+c] += dout[b,n,p,c] (atomic), and
 * dY[b,n,offc+c] = sum_p dout[b,n,p,c].  dY must be zero-filled by the caller. */
int pdgn_window_gather_sum_backward(int b, int n, int k, int ldy, int T, int P, int C, int off,
                                    int offc, const float *dout, const int32_t *idx, float *dY,
                                    pdgn_stream_t stream);

/* Transposed kNN graph (CSR over source points) of idx (b,n,k): rowptr (b,n+1), edges (b,n*k) with
 * edge records n*32 + s (k <= 31); scratch: 2*b*n ints. */
int pdgn_knn_graph_transpose(int b, int n, int k, const int32_t *idx, int32_t *rowptr, int32_t *edges,
                             int32_t *scratch, pdgn_stream_t stream);
/* Atomic-free form of pdgn_window_gather_sum_backward over the transposed graph: every element of
 * dY's column blocks [off, off+T*C) and [offc, offc+C) is WRITTEN exactly once (no zero-fill). */
int pdgn_window_gather_sum_backward_csr(int b, int n, int k, int ldy, int T, int P, int C, int off,
                                        int offc, const float *dout, const int32_t *rowptr,
                                        const int32_t *edges, float *dY, unsigned *max_out, int max_init, pdgn_stream_t stream);
/* (max_out, may be NULL: uint32[b n], the maximum of |dY| (bit pattern) over every row (b, j) of dY, collected over the calls that
 * fill one dY -- the first of them passes max_init = 1 and the array is zero-filled; atomic max, order-independent -- for
 * pdgn_gemm_set_operand_scales: the per-point product's input gradient takes dY as its first operand and scales it row by row.) */

/* Fused BatchNorm + activation over channels-last (rows x c) activations -- the
 * nn.BatchNorm2d + LeakyReLU/ReLU pairs of models/PDGNet_v2.py:537-545, 561-565, 603-625 in the
 * point-major layout.  act: 0 none, 1 ReLU, 2 LeakyReLU(0.01).  c % 4 == 0.
 *
 * pdgn_bn_scratch_floats(rows, c): number of floats of `scratch` the two reductions below need.
 * pdgn_bn_stats: batch statistics (training mode), two-stage reduction through `scratch`; stats out:
 * [scale | shift | mean | invstd] (4c floats), scale = gamma*invstd, shift = beta - mean*scale;
 * running_mean/var (may be NULL) are updated with `momentum` and the unbiased variance.
 * pdgn_bn_eval_stats: the same `stats` from the running statistics (eval mode).
 * pre_bias (may be NULL, c floats): the bias of the conv / linear layer that produced x when the caller left it
 * OUT of x (BatchNorm(x + b) == BatchNorm(x), so the GEMM needs no bias epilogue); it only enters the running mean
 * (training) and the effective mean (eval), which keeps nn.BatchNorm's buffers identical to the reference's.
 *
 * What each entry point writes of its scratch (tests/test_gpu_bn.py holds them to it; a call that returns -1 writes nothing at all).
 * pdgn_bn_scratch_floats(rows, c) = gy*2c + 2c, gy the row blocks of the launch geometry; the region has two tenants:
 *   pdgn_bn_stats                     writes the gy partial rows [sum (x - x[0]) | sum (x - x[0])^2] of 2c floats each and leaves
 *                                     the 2c floats behind them untouched
 *   pdgn_bn_stats_from_partials       reads gy rows [sum x | sum x^2] of 2c floats (no pivot) and writes nothing to scratch
 *   pdgn_bn_act_backward              writes the gy partial rows [sum dz | sum dz*xhat] AND, behind them, the 2c coefficients [ca | cb]
 *                                     of dx = scale*dz - ca - cb*x (both zero when training == 0): every float of the region
 *   pdgn_bn_stats_from_gemm_partials  reads the first ceil(rows / block_rows) partial rows only -- the rows beyond them (nparts may be
 *                                     larger) are never read -- the last of which covers rows - (that many - 1)*block_rows rows; in its
 *                                     two-launch forms it writes all pdgn_bn_blocks_scratch_doubles(c, nparts) doubles of its fp64
 *                                     scratch (slices that hold no partial row write zeros), in the one-launch form, or with
 *                                     scratch == NULL, none; the two give the same statistics
 *   pdgn_bn_eval_stats                has no scratch; running_mean / running_var are inputs */
long long pdgn_bn_scratch_floats(long long rows, int c);
int pdgn_bn_stats(long long rows, int c, float eps, float momentum, const float *x, const float *gamma,
                  const float *beta, const float *pre_bias, float *running_mean, float *running_var,
                  float *scratch, float *stats, pdgn_stream_t stream);
int pdgn_bn_eval_stats(int c, float eps, const float *gamma, const float *beta, const float *pre_bias,
                       const float *running_mean, const float *running_var, float *stats,
                       pdgn_stream_t stream);
/* Statistics whose first stage was done by a producer: `scratch` holds the per-row-block partial sums of x in the
 * layout of pdgn_bn_stats (pdgn_window_gather_sum_stats writes them while producing x). */
int pdgn_bn_stats_from_partials(long long rows, int c, float eps, float momentum, const float *gamma,
                                const float *beta, const float *pre_bias, float *running_mean, float *running_var,
                                const float *scratch, float *stats, pdgn_stream_t stream);
/* The second stage over the BLOCK-SHIFTED partials pdgn_gemm_nt / pdgn_gemm_nn / pdgn_thin_nt write from their epilogue:
 * nparts rows of [3c] floats, row b = per-column  sum (x - pv_b) | sum (x - pv_b)^2 | pv_b  over rows b*block_rows .. of x,
 * pv_b = the block's own first row (no cancellation when |mean| >> std); combined per block in fp64. */
int pdgn_bn_stats_from_gemm_partials(long long rows, int c, long long nparts, int block_rows, float eps, float momentum,
                                     const float *gamma, const float *beta, const float *pre_bias,
                                     float *running_mean, float *running_var, const float *partials,
                                     float *stats, double *scratch, pdgn_stream_t stream);
/* scratch: pdgn_bn_blocks_scratch_doubles(c, nparts) fp64 elements (may be NULL, and is unused for short lists): long
 * lists are summed by several workgroups per channel group in a first launch and joined, in order, by a second. */
long long pdgn_bn_blocks_scratch_doubles(int c, long long nparts);
/* y = act(x*scale + shift) [* mul]   (mul may be NULL; same shape as x) */
int pdgn_bn_act_forward(long long rows, int c, int act, const float *x, const float *stats,
                        const float *mul, float *y, int interleave_n, pdgn_stream_t stream);
/* dz = dy [* mul] * act'(z);  bsums (2c floats out): [0:c] = sum dz (= dbeta), [c:2c] = sum dz*xhat (= dgamma);
 * dx = scale*(dz - mean(dz) - xhat*mean(dz*xhat)) if training else scale*dz;
 * dmul (may be NULL) = dy * act(z). */
int pdgn_bn_act_backward(long long rows, int c, int act, int training, const float *x,
                         const float *dy, const float *mul, const float *stats, float *scratch,
                         float *bsums, float *dx, float *dmul, int interleave_n, pdgn_stream_t stream);
/* interleave_n = N > 0 (c even... a multiple of 4, mul NULL, rows % N == 0): y / dy are stored INTERLEAVED -- x row b*N + n, channel
 * 2c + j  <->  y row b*2N + j*N + n, channel c ((rows * 2) x (c / 2)): the (B,2Fout,N,1) -> (B,Fout,2N) regrouping of a
 * deconvolution block's result (models/PDGNet_v2.py:645-647) in point-major form, without a separate permute copy. */

/* BatchNorm + activation + max-pool over the n rows of each sample (the tail of the PointNet-style
 * discriminators, models/PDGNet_v2.py:886-911): x (b*n, c) -> ymax / yarg (b, c); the activated tensor
 * is never written.  stats from pdgn_bn_stats / pdgn_bn_eval_stats over all b*n rows.
 * scratch: pdgn_bn_maxpool_scratch_floats(b, c) floats (per sample and split: c maxima, then, behind all of them, c int32 rows).
 *
 * Ties.  Both forms return the same ymax bits for the same stats; they may name different rows where several rows attain it:
 *   pdgn_bn_act_maxpool        yarg = the LOWEST row whose activated value act(fma(x, scale, shift)) equals ymax
 *   pdgn_bn_stats_act_maxpool  yarg = the lowest row attaining the largest x of the sample where scale >= 0 (a scale of exactly 0
 *                              included), the lowest row attaining the smallest x where scale < 0; ymax is that row's activated value
 * The two differ where different x give the same activated bits: under ReLU's plateau (every z <= 0: the first form names row 0 of
 * the sample), at scale == 0, and where fma(x, scale, shift) rounds two x to one value.  Where one row alone attains ymax both name it.
 * Either yarg is a valid input of the adjoint below: the gradient flows to the row it names. */
long long pdgn_bn_maxpool_scratch_floats(int b, int c);
int pdgn_bn_act_maxpool(int b, int n, int c, int act, const float *x, const float *stats, float *scratch,
                        float *ymax, int32_t *yarg, pdgn_stream_t stream);
/* Training mode without statistics from the producer: batch statistics (stats (4c) out; running statistics updated as by pdgn_bn_stats)
 * AND the pooled output in one pass over x -- the pass keeps per (sample, split, channel) the largest and the smallest x and picks by
 * the sign of the channel's scale afterwards (act(scale x + shift) is monotone in x).  scratch: pdgn_bn_stats_maxpool_scratch_floats
 * (b*16 partial rows of 2c floats, pivot x[0], then maxima, their rows, minima, their rows: b*16*c each). */
long long pdgn_bn_stats_maxpool_scratch_floats(int b, int c);
int pdgn_bn_stats_act_maxpool(int b, int n, int c, int act, float eps, float momentum, const float *x, const float *gamma,
                              const float *beta, const float *pre_bias, float *running_mean, float *running_var, float *scratch,
                              float *stats, float *ymax, int32_t *yarg, pdgn_stream_t stream);
/* Its adjoint in one streaming pass: dx (b*n, c) from dout (b, c); bsums (2c) = [dbeta | dgamma];
 * scratch: b*c + 2c floats, all written: dz (b, c) = dout*act'(z at row yarg), then the coefficients [ca | cb] of
 * dx = (n == yarg ? scale*dz : 0) - ca - cb*x.  act' is decided by z > 0 here and in pdgn_bn_act_backward: at z == 0 it is the
 * negative side's (0 for ReLU, 0.01 for LeakyReLU). */
int pdgn_bn_act_maxpool_backward(int b, int n, int c, int act, int training, const float *x,
                                 const float *dout, const int32_t *yarg, const float *stats,
                                 float *scratch, float *bsums, float *dx, pdgn_stream_t stream);
/* The same adjoint carried through the dense layer in front of it (PointDiscriminator_k.fc1's last Conv1d + BatchNorm1d + LeakyReLU +
 * MaxPool1d, models/PDGNet_v2.py:886-911; training statistics): with x = h W^T and dx = S - 1 ca^T - x diag(cb) (S non-zero at the
 * b*c arg-max entries only)
 *     dh = S W - 1 (ca^T W) - h (W^T diag(cb) W)        one (b*n, k, k) product, a k x k Gram matrix, a scatter of b*c rows of W
 *     dW = S^T h - ca (1^T h) - diag(cb) W (h^T h)      one k x k Gram matrix of h, one (c, k, k) product, a gather of b*c rows of h
 * -- the dense (b*n, c) gradient is never formed and neither (b*n, c, k) product is computed.
 * x (b*n, c) the layer's raw output, yarg / stats as saved by pdgn_bn_act_maxpool, dout (b, c), h (b*n, k) pitch ldh, W (c, k) pitch
 * ldw (16-byte aligned rows); k % 4 == 0, k <= 256, n <= 65535.  Outputs, each may be NULL: dh (b*n, k) contiguous; dW (c, k) pitch
 * lddw (needs k a power of two >= 16); bsums (2c) = [dbeta | dgamma].  scratch: pdgn_dense_bn_maxpool_backward_scratch floats. */
long long pdgn_dense_bn_maxpool_backward_scratch(int b, int c, int k);
int pdgn_dense_bn_maxpool_backward(int b, int n, int c, int k, int act, const float *x, const float *dout, const int32_t *yarg,
                                   const float *stats, const float *h, int ldh, const float *W, int ldw, float *scratch,
                                   float *dh, float *dW, int lddw, float *bsums, pdgn_stream_t stream);
/* The input gradient alone (frozen parameters: the generator's update through a discriminator, models/PDGNet_v2.py:330-352). */
long long pdgn_dense_bn_maxpool_input_grad_scratch(int b, int c, int k);
int pdgn_dense_bn_maxpool_input_grad(int b, int n, int c, int k, int act, const float *x, const float *dout,
                                     const int32_t *yarg, const float *stats, const float *h, int ldh,
                                     const float *W, int ldw, float *scratch, float *dh, pdgn_stream_t stream);

/* Column sums per group of rows: out[g, c] = sum over rows g*group_rows .. (g+1)*group_rows - 1 of x[r, c]; x (groups*group_rows, c)
 * pitch ldx (16-byte aligned rows), c a power of two in 16 .. 1024, out (groups, c) contiguous and ZERO on entry.  The bias
 * gradients torch's autograd takes with sum(dim=...) behind nn.Conv1d / nn.Conv2d layers that no BatchNorm follows
 * (models/PDGNet_v2.py:835-862 heads, :604-618 per-sample terms of the edge convolutions). */
int pdgn_group_colsum(long long groups, long long group_rows, int c, const float *x, long long ldx, float *out,
                      pdgn_stream_t stream);

/* Softmax over the k neighbour slots fused with the slot/channel interleave of
 * models/PDGNet_v2.py:634-641: h (m,k,c) -> w (m, k/2, 2c) with w[m,p,2c'+j] = softmax_s(h[m,:,c'])[s=(k/2)j+p].
 * k even, k <= 32. */
int pdgn_softmax_slots_permute(long long m, int k, int c, const float *h, float *w, pdgn_stream_t stream);
/* Same with the preceding BatchNorm + activation folded in (conv_all.4 + LeakyReLU, models/PDGNet_v2.py:623-625):
 * x (m,k,c) is the raw conv output, stats the [scale|shift|mean|invstd] row of pdgn_bn_stats / pdgn_bn_eval_stats,
 * act as in pdgn_bn_act_forward; the activated logits are never written.  c even. */
int pdgn_bn_softmax_slots_permute(long long m, int k, int c, int act, const float *x, const float *stats,
                                  float *w, pdgn_stream_t stream);
/* The whole bilateral weighting (models/PDGNet_v2.py:623-642) in one pass: w as above and
 * y = act_u(u*scale_u + shift_u) * w for u (m, k/2, 2c) the raw inte_conv_hk output (stats_u: its 4*(2c) statistics
 * row); w may be NULL (not needed when no backward pass follows). */
int pdgn_bn_softmax_slots_permute_mul(long long m, int k, int c, int act, const float *x, const float *stats,
                                      int act_u, const float *u, const float *stats_u, float *w, float *y,
                                      unsigned *max_out, const float *gamma_u, const float *beta_u, float bound_scale,
                                      unsigned *cmax_out, pdgn_stream_t stream);
/* (max_out, may be NULL: uint32[m], the maximum of |y| (bit pattern) over each point's k c outputs = the row maxima of y as the
 * (m, k c) first operand of conv2's dense half -- what pdgn_absmax_rows_cols would compute by a pass over y; zero-filled by the
 * call, atomic max.
 * cmax_out, may be NULL: uint32[k c], an upper BOUND of that operand's column maxima (its weight gradient scales it column by column):
 * |beta_u[j]| + |gamma_u[j]| * bound_scale for column (p, j) -- with bound_scale = sqrt(n - 1) for batch statistics over n = m k / 2
 * samples, since |xhat| <= sqrt(n - 1) and the softmax weights are <= 1; gamma_u / beta_u: the 2c BatchNorm parameters of u.) */
/* Adjoint of pdgn_bn_softmax_slots_permute_mul in two passes over (x, u, w, dy): BatchNorm_u backward, slot-softmax
 * backward and BatchNorm_x backward with dW / dh kept in registers.  scratch: pdgn_bilateral_scratch_floats(m,k,c)
 * floats; bsums_x (2c) = [sum dz_x | sum dz_x*xhat] (= dbeta, dgamma of BN_x), bsums_u (4c) likewise for BN_u;
 * training = 0: running-statistics BatchNorms (no batch terms in dx / du).  c % 4 == 0, k even, k <= 16 (all k slots of a
 * channel pair live in registers; wider neighbourhoods: pdgn_bn_softmax_slots_permute + pdgn_bn_act_backward). */
long long pdgn_bilateral_scratch_floats(long long m, int k, int c);
int pdgn_bilateral_weighting_backward(long long m, int k, int c, int act, int training, const float *x,
                                      const float *stats_x, const float *u, const float *stats_u, const float *w,
                                      const float *dy, float *scratch, float *bsums_x, float *bsums_u, float *dx,
                                      float *du, pdgn_stream_t stream);
/* dh[m,s,c'] = w_s (dw_s - sum_s' w_s' dw_s'), w / dw in the permuted layout. */
int pdgn_softmax_slots_permute_backward(long long m, int k, int c, const float *w, const float *dw,
                                        float *dh, pdgn_stream_t stream);

/* Dense contraction of a point-major layer on the matrix cores, fp32 in and out:
 *   C (m x n, row pitch ldc) = A (m x k, pitch lda) W (n x k, pitch ldw)^T (+ bias[n]) (+ addend (m x n, pitch ldadd)),
 * all row-major; n, k and every pitch are multiples of 4 floats, base pointers 16-byte aligned.
 * Arithmetic (pdgn_gemm_nt / _nn / _nt_ex / _tn_big): every fp32 operand value is split into three bf16 parts
 * (x = h + m + l to 2^-25 |x|) and a product is six bf16 MFMA products accumulated in fp32 (csrc/gemm_x3.hip) -- per product
 * an error of <= 2^-23 |a w|, measured against fp64 below that of the fp32 matrix instructions; no scaling, the fp32
 * exponent range is kept; an infinite operand value yields NaN (inf - inf in the split), where fp32 arithmetic may yield inf.
 * In the default mode the large products run on TWO scaled fp16 parts and three fp16 MFMA products instead (mode 2 below: same
 * operands and results, half the matrix-core work, against fp64 below both other forms); PDGN_GEMM=x3 keeps three parts everywhere.
 * PDGN_GEMM=fp32 in the environment at first use, or pdgn_gemm_set_mode(0), selects the fp32 matrix instructions instead
 * (csrc/gemm_nt.hip; 0.6-0.9x the rate).
 * (The reference's Conv2d/Conv1d/Linear forward at models/PDGNet_v2.py:559-625, 835-862, 886-1014 in
 * point-major form; with the transposed weight it is their input gradient dX = dY W.)  stat_part (may be
 * NULL): pdgn_gemm_nt_stat_rows(m, n, k) rows of [3n] floats = per-column sum (x - pv) | sum (x - pv)^2 | pv of blocks of
 * pdgn_gemm_nt_stat_block_rows(m, n, k) rows of C (pv: the block's first row), the partials
 * pdgn_bn_stats_from_gemm_partials turns into BatchNorm statistics.  Without
 * stat_part and with ldc == n the launch may add partial tiles with fp32 atomics (C is zero-filled by the
 * call itself where needed). */
/* Products with a per-sample operand of R <= 64 rows (csrc/skinny.hip; the 35-row layers of models/PDGNet_v2.py:704-707,
 * 825-828, 835-862 and the constant-channel contribution of DESIGN.md section 2), fp32 matrix instructions, one pass over the large
 * operand:
 *   pdgn_skinny_nt: C (R x N) = A (R x K) B (N x K)^T (+ bias[N])      K % 4 == 0, rows of A / B 16-byte aligned
 *   pdgn_skinny_nn: C (R x N) += A (R x K) B (K x N)                    C ZERO-FILLED by the caller (K slices add with fp32 atomics); N % 4 == 0
 *   pdgn_skinny_tn: C (N x K) = A (R x N)^T B (R x K)
 * every operand with its own row pitch (a column slice of a wider weight needs no copy). */
int pdgn_skinny_nt(int R, int N, int K, const float *A, int lda, const float *B, int ldb, const float *bias, float *C, int ldc,
                   pdgn_stream_t stream);
int pdgn_skinny_nn(int R, int N, int K, const float *A, int lda, const float *B, int ldb, float *C, int ldc, pdgn_stream_t stream);
/* pdgn_skinny_nt with an activation after the bias (act 0 none, 1 ReLU, 2 LeakyReLU(0.01)): a discriminator head's nn.Linear +
 * nn.LeakyReLU on the batch's pooled rows (models/PDGNet_v2.py:896-911) in one launch. */
int pdgn_skinny_nt_act(int R, int N, int K, const float *A, int lda, const float *B, int ldb, const float *bias, float *C, int ldc,
                       int act, pdgn_stream_t stream);
/* pdgn_skinny_nn with A[r][k] scaled by act'(P[r][k]) on load (act 1 = ReLU, 2 = LeakyReLU(0.01); P (R x K) the pre-activation a
 * Linear + activation saved): that layer's input gradient dx = (dy * act'(pre)) W in one launch when its parameters are frozen
 * (the discriminators' nn.Linear heads during the generator's update, models/PDGNet_v2.py:330-352, :896-911). */
int pdgn_skinny_nn_masked(int R, int N, int K, const float *A, int lda, const float *P, int ldp, int act, const float *B,
                          int ldb, float *C, int ldc, pdgn_stream_t stream);
int pdgn_skinny_tn(int R, int N, int K, const float *A, int lda, const float *B, int ldb, float *C, int ldc, pdgn_stream_t stream);
/* A weight matrix split ONCE into the three bf16 parts the contractions multiply (x = h + m + l, csrc/split.hip) instead of by
 * every workgroup's loader: src (rows x cols fp32, pitch ld_src) -> planes (3 x [rows][ld_planes] bf16, plane_stride elements
 * apart; may be NULL) and / or planes_t, the same for the TRANSPOSE (3 x [cols][ld_planes_t]; may be NULL).  The pad columns
 * of EVERY row, the last row's too, are zero-filled up to cols rounded up to 32 (ld_planes beyond that stays unwritten; the
 * contraction's 16-byte loads reach at most cols rounded up to 8): plane_stride >= rows * ld_planes (plane_stride_t >= cols *
 * ld_planes_t, its pads filled up to rows rounded up to 32), else PDGN_ERR_INVALID.
 * pdgn_gemm_nt_ps = pdgn_gemm_nt_ex with such planes as the second operand (n x k, pitch ldw, wplane elements between planes;
 * ldw and wplane multiples of 8, the planes 16-byte aligned):
 * forward y = x W^T with W's planes, input gradient dX = dY W with the planes of W^T.  parts = 3 (these planes) or 2 (the two
 * fp16 planes of pdgn_split_f16x2, below).  Bit-identical to the unsplit call that runs on the same number of parts; matrix-core
 * modes only (PDGN_ERR_INVALID under pdgn_gemm_set_mode(0)).  No reference counterpart. */
int pdgn_split_bf16x3(int rows, int cols, const float *src, int ld_src, unsigned short *planes, int ld_planes,
                      long long plane_stride, unsigned short *planes_t, int ld_planes_t, long long plane_stride_t,
                      pdgn_stream_t stream);
int pdgn_gemm_nt_ps(long long m, int n, int k, const float *A, int lda, const unsigned short *Wplanes, int ldw, long long wplane,
                    int parts, const float *bias, const float *addend, int ldadd, float *C, int ldc, float *stat_part,
                    const float *row_bias, int ld_rb, int rows_per_group, int act, const float *gate, int ldgate,
                    pdgn_stream_t stream);
/* Stream-K tails without atomics (matrix-core mode).  A launch whose tiles do not fill the last round of workgroups finishes with a
 * tail that splits the leftover tiles' k range over the CUs.  With a workspace of pdgn_gemm_tail_workspace_floats(m, n, k, with_stats)
 * floats handed over by pdgn_gemm_set_tail_workspace -- to the NEXT pdgn_gemm_nt / _nn / _nt_ps call of the calling thread, which
 * consumes it -- the tail stores partial tiles there and a small kernel adds them into C (deterministic, no zero-fill); without one
 * it adds them with fp32 atomics.  The buffer must stay valid until that call's launches have run.  No reference counterpart. */
long long pdgn_gemm_tail_workspace_floats(long long m, int n, int k, int with_stats);
/* The same for pdgn_gemm_tn_big (dW = dY^T X: few output tiles, the reduction over the m rows split in k slices): with a workspace of
 * this many floats handed over the same way the slices' partial tiles are summed in a fixed order (no atomics, no zero-fill of dW,
 * bit-identical from run to run); 0: the call does not split. */
long long pdgn_gemm_tn_big_workspace_floats(long long m, int n, int k);
int pdgn_gemm_set_tail_workspace(float *ws, long long floats);
/* The kernel instance (host symbol; NULL for the 16x16x32 arm) and grid of the plain data-parallel launch of pdgn_gemm_nt_ps(m, n, k)
 * under the switches in force: for measurements that look that launch up in a recorded iteration.  Host-side only. */
int pdgn_gemm_nt_ps_launch_info(long long m, int n, int k, int parts, const void **sym, int *grid);
/* Host symbols of the small kernels a contraction call may launch around its matrix-core kernels: the reduce of a stream-K tail's
 * partial tiles, the scan of an operand's maxima (mode 2). */
int pdgn_gemm_aux_symbols(const void **reduce, const void **scan);
/* Process-wide switches of the dense contractions (read from PDGN_GEMM / PDGN_NT_CFG once, at first use).
 * pdgn_gemm_set_mode: 2 = matrix cores, two scaled fp16 parts where that pays and three bf16 parts elsewhere (default; below),
 * 1 = three bf16 parts everywhere, 0 = fp32 matrix instructions, < 0 = query; returns the previous mode.
 * pdgn_gemm_set_config: -1 = the launch model's pick (default), 0 .. 3 = force a tile configuration (measurement / tests),
 * < -1 = query; returns the previous value.
 * pdgn_gemm_set_shape: the bf16 matrix instruction of the matrix-core mode: 32 = v_mfma_f32_32x32x16_bf16 for every launch, 16 =
 * v_mfma_f32_16x16x32_bf16 for every launch (same tiles, same operands; results differ in the last bits), -1 = the built-in choice
 * per instance class, 0x1000 | mask = a per-class mask (bit 4 * tile + class; gemm_x3.hip), anything else = query; returns the
 * previous mask.  PDGN_X3_SHAPE / PDGN_X3_SHAPE16_MASK set the process default. */
int pdgn_gemm_set_mode(int mode);
/* Mode 2 (round 5; the default, PDGN_GEMM=x2): the contractions whose time is their matrix-core work run on the fp16 matrix
 * cores with TWO parts per value; the others stay on three bf16 parts (mode 1's arithmetic).  pdgn_gemm_two_part(m, n, k,
 * scan_bytes) says which a call (m, n, k) is when scan_bytes of its operands would still have to be scanned for their maxima: the
 * 256 x 128 tile, k >= 128, >= 20 GFLOP and at most 4.5 bytes to scan per kflop (measured: tools/x2_shapes.py).
 * Two parts (round 6: scaled PER ROW; one scale per operand until then): every ROW of each operand as the kernel sees it -- row m
 * of A, row n of W; for an operand given transposed the COLUMNS of the matrix in memory: pdgn_gemm_nn's Wt, both operands of
 * pdgn_gemm_tn_big -- is multiplied by a power of two 2^e_r, e_r = 14 - floor(log2 max |x| over that row) (so that nothing leaves
 * fp16's range), split as x 2^e = h + l (round-to-nearest fp16 of the value and of the exact remainder: |err| <= 2^-23 |x| for
 * values within 2^-16 of THEIR ROW's largest, an absolute 2^-39 of the row's maximum below; mode 1 needs no scale and keeps every
 * value's own 24 bits), a product is the three fp16 MFMA products al wh + ah wl + ah wh accumulated in fp32, and C[m, n] is
 * multiplied by 2^-e_A[m] 2^-e_W[n] (exact).  An output row therefore depends on its own input row's scale only: the input gradient
 * of a point with a small output gradient is as accurate, relative to that row, as any other's (tests/test_gpu_deconv.py::
 * test_two_part_rows_spanning_thirty_binades).  Per product |err| <= ~2^-21 |a w| in the worst case; in sums the fp32 accumulation
 * all modes share dominates, of which this form does half as much: measured against fp64 BELOW the other two modes (bench.py
 * gemm_accuracy, tools/x2_check.py: all three operand layouts, 1e-20 .. 1e15).  Half the matrix-core work of mode 1.
 * The maxima are arrays of bit patterns of |x| (uint32; unsigned order = magnitude order: producers combine them with integer /
 * atomic max in any order).  They come from a scan in front of the launch (x2_maxima_kernel: one pass, row and / or column
 * maxima) into an arena the caller provides once -- pdgn_gemm_set_scale_slots(device memory, bytes; handed out round-robin in 1-KB
 * units, 4 bytes per kernel-side row: it must hold the arrays of every launch that can be in flight; the library never
 * allocates); without one a two-part call that has to scan returns PDGN_ERR_INVALID -- or from the caller: pdgn_absmax_rows_cols
 * (rowmax[rows] and / or colmax[cols] of a matrix in one pass), or the kernel that WRITES the operand
 * (pdgn_bn_softmax_slots_permute_mul's and pdgn_window_gather_sum_backward_csr's max_out: row maxima), handed over for the operands of
 * the calling thread's NEXT contraction call (pdgn_gemm_set_operand_scales(max_a, max_w): the kernel-side rows of the first /
 * second operand as that entry point takes them -- _nt / _nt_ps: rows of A, rows of W; _nn: rows of A, columns of Wt; _tn_big:
 * columns of dY, columns of X; NULL = scanned by the call; consumed by that call; finite upper bounds serve as well): an
 * activation that feeds several products is scanned once, or never.
 * pdgn_split_f16x2 = pdgn_split_bf16x3 for a two-part product: two fp16 planes (h | l, every row scaled by its own power of two) and
 * the rows' maxima as uint32[rows] right behind them (element offset 2 * plane_stride: the buffer holds 2 * plane_stride + 2 * rows
 * elements; plane_stride >= rows * ld_planes, a multiple of 8); the transposed planes' rows are the matrix's columns.
 * pdgn_gemm_nt_ps takes either kind of planes and is told which (parts = 3 | 2).  No reference counterpart.
 * State: the mode / tile / instruction switches are process-wide; the arena is process-wide; the hand-overs (operand maxima, tail
 * workspace) are THREAD-LOCAL and belong to the calling thread's next contraction call only, whether it launches or is refused. */
int pdgn_gemm_set_scale_slots(void *slots, long long bytes);
int pdgn_absmax_rows_cols(long long rows, int cols, const float *src, int ld, unsigned *rowmax, unsigned *colmax,
                          pdgn_stream_t stream);
int pdgn_gemm_set_operand_scales(const unsigned *max_a, const unsigned *max_w);
int pdgn_gemm_two_part(long long m, int n, int k, long long scan_bytes);
/* The same question for a product against PRE-SPLIT planes (which kind to make: pdgn_split_f16x2 or _bf16x3): with nothing to
 * convert for the weight the two-part loop is ahead from ~2 GFLOP on, k >= 32; two-part planes run on the 256 x 128 tile whatever
 * pdgn_gemm_nt_config says for three parts (a launch with stat_part: only where that IS the pick, else PDGN_ERR_INVALID), and their
 * tail workspace is pdgn_gemm_nt_ps_workspace_floats(m, n, k, parts, with_stats). */
int pdgn_gemm_two_part_planes(long long m, int n, int k, long long scan_bytes);
/* Round 6: a product on two-part planes with a short reduction (k = 32, 64, 128), n >= 128, m >= 4096, m n >= 1.6e7 and neither
 * bias, addend nor epilogue extras runs on the ROW-PANEL kernel (csrc/gemm_rp.hip: a workgroup keeps 256 rows of A in registers as
 * matrix-instruction fragments and streams the weight's column tiles; same arithmetic as the tile kernel, bit for bit; no tail, no
 * workspace).  Its BatchNorm partials (stat_part) cover a 256-row panel each (the eight waves of a workgroup join their 32-row sums): pdgn_gemm_nt_ps_stat_rows / _stat_block_rows answer for the
 * call that will actually run (plain != 0: no bias / addend / extras). */
long long pdgn_gemm_nt_ps_stat_rows(long long m, int n, int k, int parts, int plain);
int pdgn_gemm_nt_ps_stat_block_rows(long long m, int n, int k, int parts, int plain);
/* 1 when that call runs on the row-panel kernel (the rule above under the switches in force), else 0: a caller skips the scan of
 * A's row maxima then -- the kernel takes them itself. */
int pdgn_gemm_nt_ps_row_panel(long long m, int n, int k, int parts, int plain);
long long pdgn_gemm_nt_ps_workspace_floats(long long m, int n, int k, int parts, int with_stats);
int pdgn_split_f16x2(int rows, int cols, const float *src, int ld_src, unsigned short *planes, int ld_planes,
                     long long plane_stride, unsigned short *planes_t, int ld_planes_t, long long plane_stride_t,
                     pdgn_stream_t stream);
int pdgn_gemm_set_config(int cfg);
int pdgn_gemm_set_shape(int shape);
int pdgn_gemm_nt(long long m, int n, int k, const float *A, int lda, const float *W, int ldw,
                 const float *bias, const float *addend, int ldadd, float *C, int ldc, float *stat_part,
                 pdgn_stream_t stream);
/* Dense layers with at most 4 channels on one side (the xyz-in / xyz-out layers: Conv1d(3, 64) of the discriminators
 * and conv_xyz, models/PDGNet_v2.py:559-566, 886-1014; Conv1d(64, 3) of the heads, :835-862) as streaming kernels, no padding:
 *   Y (m x n, pitch ldy) = X (m x k, pitch ldx) W'^T (+ bias[n]),   W'[j, kk] = W[j * wrs + kk * wcs]
 * with either k <= 4 and n % 4 == 0 (Y 16-byte aligned rows) or n <= 4 and k % 4 == 0 (X 16-byte aligned rows).  The strides
 * let one entry serve a weight and its transpose (forward: wrs = k, wcs = 1; input gradient dX = dY W: wrs = 1, wcs = C_in).
 * stat_part (k <= 4 form only, may be NULL): pdgn_thin_stat_rows(m) rows of [3n] floats (blocks of pdgn_thin_stat_block_rows()
 * rows), the BatchNorm partials of Y in the layout pdgn_bn_stats_from_gemm_partials reads.  Returns -3 for shapes outside
 * these two forms. */
long long pdgn_thin_stat_rows(long long m);
int pdgn_thin_stat_block_rows(void);
int pdgn_thin_nt(long long m, int n, int k, const float *X, int ldx, const float *W, int wrs, int wcs,
                 const float *bias, float *Y, int ldy, float *stat_part, pdgn_stream_t stream);
/* The same with a LeakyReLU-derivative factor (k <= 4 form): Y *= (gate > 0 ? 1 : 0.01), gate (m x n, pitch ldgate) a saved
 * activation -- Y is then the gradient wrt that activation's input (backward of the heads, models/PDGNet_v2.py:835-862). */
int pdgn_thin_nt_ex(long long m, int n, int k, const float *X, int ldx, const float *W, int wrs, int wcs,
                    const float *bias, float *Y, int ldy, float *stat_part, const float *gate, int ldgate, pdgn_stream_t stream);
/* Weight (+ bias) gradient of such a layer: O[i * osi + j * osj] += sum_r A[r, i] B[r, j] for A (m x ta <= 4, pitch lda),
 * B (m x wb, wb % 4 == 0, pitch ldb, 16-byte aligned rows); sum_a[ta] += column sums of A, sum_b[wb] += column sums of B
 * (either may be NULL).  O and the sums are accumulated with fp32 atomics: the caller passes them zero-filled. */
int pdgn_thin_tn(long long m, int ta, int wb, const float *A, int lda, const float *B, int ldb, float *O, int osi,
                 int osj, float *sum_a, float *sum_b, pdgn_stream_t stream);
/* The same product with the second operand given transposed, C = A Wt with Wt (k x n, row pitch ldw): the input
 * gradient dX = dY W of a dense layer straight from its (C_out x C_in) weight (models/PDGNet_v2.py conv / linear backward). */
int pdgn_gemm_nn(long long m, int n, int k, const float *A, int lda, const float *Wt, int ldw,
                 const float *bias, const float *addend, int ldadd, float *C, int ldc, float *stat_part,
                 pdgn_stream_t stream);
/* Weight gradient on the same kernel (both operands transposed, reduction over the m rows split over the workgroups):
 * dW (n x k) = dY (m x n, pitch ldy)^T X (m x k, pitch ldx); dW is zero-filled by the call.  Meant for outputs of at
 * least one 128 x 64 tile (pdgn_gemm_tn keeps the small ones). */
int pdgn_gemm_tn_big(long long m, int n, int k, const float *dY, int ldy, const float *X, int ldx, float *dW, int dw_is_zero,
                     pdgn_stream_t stream);
/* dw_is_zero != 0: the caller hands over an all-zero dW (e.g. a slice of one zero-filled arena per backward pass): the
 * split-K launch then adds into it without a zero-fill launch of its own. */
/* pdgn_gemm_nt / pdgn_gemm_nn (transposed_w != 0) with an extended epilogue, applied after bias / addend in this order:
 *   + row_bias[(row / rows_per_group) * ld_rb + col]   a bias per group of rows (the per-sample term of the generator's heads:
 *                                                      mlp1..4 on cat([g broadcast, x]), models/PDGNet_v2.py:835-862, 868-876)
 *   LeakyReLU(0.01) on the result (act = 2; 0 = none)
 *   * (gate[row, col] > 0 ? 1 : 0.01)                  the LeakyReLU derivative of a saved activation: C is then the gradient
 *                                                      wrt that layer's pre-activation
 * each replacing an elementwise pass over C.  Whole tiles only (no stream-K tail).  row_bias / gate may be NULL. */
int pdgn_gemm_nt_ex(long long m, int n, int k, const float *A, int lda, const float *W, int ldw, const float *bias,
                    const float *addend, int ldadd, float *C, int ldc, float *stat_part, const float *row_bias, int ld_rb,
                    int rows_per_group, int act, const float *gate, int ldgate, int transposed_w, pdgn_stream_t stream);
long long pdgn_gemm_nt_stat_rows(long long m, int n, int k);
int pdgn_gemm_nt_stat_block_rows(long long m, int n, int k);
/* Tile configuration the launch model picks (0: 256x128, 1: 128x128, 2: 160x64, 3: 128x64 workgroup tiles); host only. */
int pdgn_gemm_nt_config(long long m, int n, int k, int with_stats);

/* Weight gradient of a point-major dense layer on the fp32 matrix cores, reduction split over
 * workgroups:  dW (n x k) += dY (m x n)^T  X (m x k), all row-major, m >> n, k.
 * dW must be zero-filled by the caller; n % 4 == 0, k % 4 == 0. */
int pdgn_gemm_tn(long long m, int n, int k, const float *dY, const float *X, float *dW,
                 pdgn_stream_t stream);

/* ------------------------------------------------------------------ local-pair shape loss
 * Neighbourhood mean / covariance of models/PDGNet_v2.py:127-134 fused with the grouping of
 * :142-147: xyz (b,n,3), idx (b,m,k) (from pdgn_knnquery) -> mu (b,m,3), cov (b,m,9)
 * (cov = (1/k) sum_s (p_s - mu)(p_s - mu)^T). */
int pdgn_local_stats(int b, int n, int m, int k, const float *xyz, const int32_t *idx, float *mu,
                     float *cov, pdgn_stream_t stream);
/* Adjoint: dxyz (b,n,3) += scatter of dmu (b,m,3), dcov (b,m,9); dxyz zero-filled by the caller. */
int pdgn_local_stats_backward(int b, int n, int m, int k, const float *xyz, const int32_t *idx,
                              const float *dmu, const float *dcov, float *dxyz, pdgn_stream_t stream);

/* utils/chamfer_loss.py:13-38 without the (B,M,N) matrix: P[i,j] = (|x_i|^2 + |y_j|^2) - 2<x_i,y_j>
 * (Gram form, no clamp); x (b,m,d), y (b,n,d), d <= 16 -> minx/argx (b,m) = min/argmin over j,
 * miny/argy (b,n) = min/argmin over i (lowest index on ties). */
int pdgn_chamfer_gram(int b, int m, int n, int d, const float *x, const float *y, float *minx,
                      int32_t *argx, float *miny, int32_t *argy, pdgn_stream_t stream);
/* Gradient of sum(gminx*minx) + sum(gminy*miny) wrt x and y (zero-fills gx, gy itself). */
int pdgn_chamfer_gram_grad(int b, int m, int n, int d, const float *x, const float *y,
                           const float *gminx, const int32_t *argx, const float *gminy,
                           const int32_t *argy, float *gx, float *gy, pdgn_stream_t stream);
/* The same for the loss scale * (sum minx + sum miny) (utils/chamfer_loss.py:16-20) with upstream gradient g[0] (a device
 * scalar): every minimum's gradient is g[0] * scale, no expanded gradient tensor.  When gy == gx + b*m*d one fill zeroes both. */
int pdgn_chamfer_gram_grad_uniform(int b, int m, int n, int d, const float *x, const float *y, const float *g,
                                   float scale, const int32_t *argx, const int32_t *argy, float *gx, float *gy,
                                   pdgn_stream_t stream);
/* Scalar ends of the step's losses, one launch each way (csrc/loss_small.hip; fixed summation order):
 * pdgn_scaled_sum: out[0] = scale * sum_i x[i] (the Chamfer minima, chamfer_loss.py:16-20);
 * pdgn_mse_const: out[0] = scale * mean_i (x[i] - target)^2 -- nn.MSELoss against a constant, the adversarial terms
 * mse(D(x), 1) / mse(D(x), 0) of models/PDGNet_v2.py:186-190, 246-250 (scale: their 1/2);
 * pdgn_mse_const_backward: dx[i] = g[0] * scale * 2 (x[i] - target) / n. */
int pdgn_scaled_sum(long long n, const float *x, float scale, float *out, pdgn_stream_t stream);
int pdgn_mse_const(long long n, const float *x, float target, float scale, float *out, pdgn_stream_t stream);
/* pdgn_mse_const_count: pdgn_mse_const plus, in the same pass of the same single workgroup, three integer counts of x against a
 * decision boundary (the adaptive discriminator augmentation's statistic, below: pdgn_augment_tick_ada):
 *   count[0] = #{x[i] > boundary}, count[1] = #{x[i] < boundary}, count[2] = n
 * (a value equal to the boundary and a NaN count to neither).  The counts are STORED, not added: `count` is the caller's slot of
 * four 32-bit words (16 bytes, 4-byte aligned; word 3 is not touched), one slot per discriminator.  out[0] is bit for bit
 * pdgn_mse_const's: the float sum runs in the same order; the integer sums are block reductions (wave shuffles, then shared
 * memory), no atomics.  The backward is pdgn_mse_const_backward.  Replaces nothing in the reference.
 * PDGN_ERR_INVALID: n < 1 or n >= 2^31 (the counts are 32-bit), a null or misaligned x / out / count. */
int pdgn_mse_const_count(long long n, const float *x, float target, float scale, float boundary, float *out, int32_t *count,
                         pdgn_stream_t stream);
int pdgn_mse_const_backward(long long n, const float *x, float target, float scale, const float *g, float *dx,
                            pdgn_stream_t stream);
/* The hinge and the non-saturating logistic GAN objectives on a discriminator's raw scores (logits), siblings of the pdgn_mse_const
 * trio: the same launch shapes (one workgroup of 1024 forward; the backward's grid rule) and the same fixed summation order --
 * thread t adds its elements t, t + 1024, ... in that order with plain fp32 additions, then the xor butterfly 32 .. 1 over a wave and
 * the sixteen wave totals in index order.  Least squares has no kind here: it stays on pdgn_mse_const (0 is reserved for it).
 *   pdgn_gan_term: out[0] = scale * (s / (float)n), s = sum_i f(x[i]);
 *     hinge:    d_real f = max(0, 1 - x), d_fake f = max(0, 1 + x), g f = -x; with v = 1 -+ x: f = v > 0 ? v : (v == v ? 0 : v);
 *     logistic: f = softplus(t) = fmaxf(t, 0) + log1pf(expf(-fabsf(t))), t = -x for d_real and g, t = x for d_fake.
 *   pdgn_gan_term_backward: dx[i] = c * f'(x[i]), c = g[0] * scale / (float)n evaluated left to right (g: the upstream gradient, a
 *     device scalar); hinge: f' = -1 (d_real) / +1 (d_fake) where v > 0, else 0 -- the forward's own test, so the kink x = 1
 *     (x = -1) has f' = 0 --, g: f' = -1; logistic: f' = sigma(x) (d_fake), -sigma(-x) (d_real, g), sigma(t) from e = expf(-fabsf(t))
 *     as 1 / (1 + e) for t >= 0 and e / (1 + e) otherwise.
 *   pdgn_gan_term_count: pdgn_gan_term plus the three counts of pdgn_mse_const_count against `boundary` (0 for a logit), stored the
 *     same way into the caller's slot (word 3 not touched; integer block sums, no atomics); out[0] is bit for bit pdgn_gan_term's.
 * A NaN score gives a NaN out[0] and a NaN dx[i] in every kind and role (a hinge written fmaxf(0, v) would hide it from the
 * gradient guard); +-inf give the IEEE results of the expressions above.  Every operation is its own fp32 rounding.  Replaces
 * nothing in the reference (models/PDGNet_v2.py:186-190, 246-250 is least squares only).
 * PDGN_ERR_INVALID: n < 1, a kind or role not listed here, a null or 4-byte-misaligned pointer; pdgn_gan_term_count: n >= 2^31. */
#define PDGN_GAN_HINGE 1
#define PDGN_GAN_LOGISTIC 2
#define PDGN_GAN_D_REAL 0
#define PDGN_GAN_D_FAKE 1
#define PDGN_GAN_G 2
int pdgn_gan_term(long long n, const float *x, int kind, int role, float scale, float *out, pdgn_stream_t stream);
int pdgn_gan_term_count(long long n, const float *x, int kind, int role, float scale, float boundary, float *out, int32_t *count,
                        pdgn_stream_t stream);
int pdgn_gan_term_backward(long long n, const float *x, int kind, int role, float scale, const float *g, float *dx,
                           pdgn_stream_t stream);

/* All-pairs evaluation (evaluation/evaluation_metrics.py:85-121 expands every sample against every
 * reference batch): the same kernels over explicit pair lists, pair p = (cloud ia[p] of the first
 * tensor, cloud ib[p] of the second); outputs are indexed by p.  temp: npairs*2*(n+m) floats. */
int pdgn_emd_cost_indexed(int npairs, int n, int m, const float *xyz1, const int32_t *ia,
                          const float *xyz2, const int32_t *ib, float *temp, float *out,
                          pdgn_stream_t stream);
int pdgn_chamfer_gram_indexed(int npairs, int m, int n, int d, const float *x, const int32_t *ia,
                              const float *y, const int32_t *ib, float *minx, int32_t *argx,
                              float *miny, int32_t *argy, pdgn_stream_t stream);

/* Weight re-association of a point-deconvolution block and its adjoint, one launch each:
 * Wi = inte_conv_hk.0.weight (4F,2F,1,T), W2 = conv2.conv.weight (2Fo,2F,1,2k), Wf = conv_fea.0.weight (16,2F,1,1) or
 * NULL -> the per-point GEMM operand Wcat (Mw x F) split into its first fc columns (WcatC, NULL when fc == 0) and the
 * rest (WcatV), and conv2's dense operand Wb (2Fo, (k-T+1)*4F).  Mw = T*4F + 4F + k*2Fo + 2Fo (+ 32 with Wf).
 * Backward: any of the three upstream gradients may be NULL (= zero); dWf NULL for blocks without conv_fea. */
int pdgn_deconv_assemble(int F, int Fo, int k, int T, int fc, const float *Wi, const float *W2, const float *Wf,
                         float *WcatC, float *WcatV, float *Wb, pdgn_stream_t stream);
int pdgn_deconv_assemble_backward(int F, int Fo, int k, int T, int fc, const float *gWcatC, const float *gWcatV,
                                  const float *gWb, float *dWi, float *dW2, float *dWf, pdgn_stream_t stream);

/* Per-sample biases of a block's gather-sums under the constant-channel split: for spec i = (T_i, C_i, off_i, offc_i)
 *   bb[b, o_i + c] = bias_i[c] + Yc[b, offc_i + c] + sum_{t<T_i} Yc[b, off_i + t*C_i + c],   o_i = C_0 + .. + C_{i-1},
 * Yc (b, ldy); nspec <= 4; bias[i] may be NULL.  Adjoint: g (b, sum C_i) -> dYc (b, ldy), dbias[i] (C_i) or NULL. */
int pdgn_sample_bias(int b, int ldy, int nspec, const int *T, const int *C, const int *off, const int *offc,
                     const float *const *bias, const float *Yc, float *bb, pdgn_stream_t stream);
int pdgn_sample_bias_backward(int b, int ldy, int nspec, const int *T, const int *C, const int *off, const int *offc,
                              const float *g, float *dYc, float *const *dbias, pdgn_stream_t stream);

/* nn.Sequential(Linear, [BatchNorm1d,] [LeakyReLU | ReLU]) on r <= 64 rows in one launch (the generator's per-sample
 * global branches and first layer, models/PDGNet_v2.py:704-707, 825-828): x (r,k), W (n,k), y (r,n); k <= 1024.
 * bn_mode 0: no BatchNorm; 1: batch statistics (running_mean / running_var updated when given); 2: running statistics.
 * running_var takes the unbiased variance, var r / (r - 1); with r == 1 (where torch raises) the biased one, 0: y == act(beta).
 * pre (r,n) and stat (2n: mean | invstd) are written for the adjoint (may be NULL).  Backward: dpre (r,n) = gradient
 * wrt the linear output (the caller forms dx = dpre W), dgamma, dbeta, dbias (n), dW (n,k); any of those four may be NULL. */
int pdgn_small_mlp_forward(int r, int k, int n, int act, int bn_mode, float eps, float momentum, const float *x,
                           const float *W, const float *bias, const float *gamma, const float *beta,
                           float *running_mean, float *running_var, float *y, float *pre, float *stat,
                           pdgn_stream_t stream);
int pdgn_small_mlp_backward(int r, int k, int n, int act, int bn_mode, const float *x, const float *dy, const float *pre,
                            const float *stat, const float *gamma, const float *beta, float *dpre, float *dgamma,
                            float *dbeta, float *dbias, float *dW, pdgn_stream_t stream);

/* ---- pointops entry points PDGN itself never calls, same argument meaning as the
 * reference launchers; index outputs int32, label statistics int32, caller allocates (and zero-fills where the
 * reference's Python does). */
/* ballquery_cuda_launcher_fast (ballquery/ballquery_cuda_kernel.h:10): first <= nsample points with d2 < r^2 in
 * index order; the first hit fills every slot; an empty ball leaves idx untouched (caller zero-fills, pointops.py:190). */
int pdgn_ballquery(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz,
                   int32_t *idx, pdgn_stream_t stream);
/* furthestsampling_cuda_launcher (sampling/sampling_cuda_kernel.h:13): xyz (b,n,3), temp (b,n) pre-filled with 1e10
 * (pointops.py:24), idx (b,m); starts at point 0; exact ties go to the lowest index. */
int pdgn_furthestsampling(int b, int n, int m, const float *xyz, float *temp, int32_t *idx, pdgn_stream_t stream);
/* gathering_{forward,backward}_cuda_launcher (sampling_cuda_kernel.h:10-11), also featuregather
 * (featuredistribute_cuda_kernel.h:12-13): out[b,c,j] = points[b,c,idx[b,j]]; the adjoint accumulates (+=). */
int pdgn_gathering_forward(int b, int c, int n, int m, const float *points, const int32_t *idx, float *out,
                           pdgn_stream_t stream);
int pdgn_gathering_backward(int b, int c, int n, int m, const float *grad_out, const int32_t *idx,
                            float *grad_points, pdgn_stream_t stream);
/* grouping_int_forward_cuda_launcher_fast (grouping_int/grouping_int_cuda_kernel.h:10): int64 features. */
int pdgn_grouping_int_forward(int b, int c, int n, int m, int nsample, const long long *points, const int32_t *idx,
                              long long *out, pdgn_stream_t stream);
/* featuredistribute_cuda_launcher (featuredistribute_cuda_kernel.h:10): nearest max_xyz (b,n,3) point of every
 * xyz (b,m,3) point. */
int pdgn_featuredistribute(int b, int n, int m, const float *max_xyz, const float *xyz, int32_t *distribute_idx,
                           pdgn_stream_t stream);
/* labelstat_* launchers (labelstat/labelstat_cuda_kernel.h:10-17). */
int pdgn_labelstat_idx(int b, int n, int m, int nsample, int nclass, const int32_t *label_stat, const int32_t *idx,
                       int32_t *new_label_stat, pdgn_stream_t stream);
int pdgn_labelstat_ballrange(int b, int n, int m, float radius, int nclass, const float *new_xyz, const float *xyz,
                             const int32_t *label_stat, int32_t *new_label_stat, pdgn_stream_t stream);
int pdgn_labelstat_and_ballquery(int b, int n, int m, float radius, int nsample, int nclass, const float *new_xyz,
                                 const float *xyz, const int32_t *label_stat, int32_t *idx, int32_t *new_label_stat,
                                 pdgn_stream_t stream);

/* ------------------------------------------------------------------ max-pool over the points
 * nn.MaxPool2d((1, N)) at the head of every generator block (models/PDGNet_v2.py:675/:699, :716/:736, :754/:777,
 * :794/:810) on the point-major layout: x (b,n,c) -> out (b,c) and the point index of each maximum (lowest index on
 * ties), which is all the adjoint needs: grad_x[b,r,ch] = (r == arg[b,ch]) ? grad_out[b,ch] : 0 (c % 4 == 0).
 * scratch_val / scratch_arg hold pdgn_point_max_scratch(b,n,c) floats / int32 each. */
long long pdgn_point_max_scratch(int b, int n, int c);
int pdgn_point_max(int b, int n, int c, const float *x, float *scratch_val, int32_t *scratch_arg, float *out, int32_t *arg,
                   pdgn_stream_t stream);
int pdgn_point_max_backward(int b, int n, int c, const float *grad_out, const int32_t *arg, float *grad_x,
                            pdgn_stream_t stream);

/* ------------------------------------------------------------------ scheduling support
 * No reference counterpart (the reference runs on one CUDA stream).  One wavefront that occupies `stream` for
 * `microseconds` (<= 100000) of wall time: pdgn_amd/streams.py times pairs of these to learn which HIP streams share a
 * hardware queue -- streams on one queue serialise, and the stream-overlapped G+D schedule keeps the default stream's
 * queue to itself. */
int pdgn_spin(unsigned int microseconds, pdgn_stream_t stream);

/* ------------------------------------------------------------------ launch-list replay (csrc/replay.hip)
 * No reference counterpart (the reference issues its iteration op by op from Python, models/PDGNet_v2.py:171-256).
 * A captured hipGraph_t of the iteration is read back node by node and re-issued with plain launches on caller-chosen
 * streams: pdgn_replay_marker(id, stream) inside the capture tags a stream; pdgn_replay_build turns the graph into a plan
 * (kernel / memset / flat device-to-device memcpy / empty nodes only: anything else returns a negative code); chains =
 * runs of nodes that were captured on one stream (pdgn_replay_chains: marker id or -1, and length, per chain);
 * pdgn_replay_set_stream binds a chain to a hipStream_t; pdgn_replay_launch issues every node once, in capture order,
 * with event pairs for the dependencies that cross chains.  counts8 = nodes, kernels, memsets, memcpys, empty nodes,
 * chains, events, labelled chains.  The graph (and the memory its launches address) must outlive the plan. */
int pdgn_replay_marker(int id, pdgn_stream_t stream);
int pdgn_replay_build(void *hip_graph, void **plan_out);
int pdgn_replay_info(void *plan, int *counts8);
int pdgn_replay_chains(void *plan, int *labels, int *nodes_per_chain);
int pdgn_replay_set_stream(void *plan, int chain, pdgn_stream_t stream);
int pdgn_replay_launch(void *plan);
int pdgn_replay_launch_range(void *plan, int lo, int hi); /* nodes [lo, hi) of the list */
int pdgn_replay_position(void *plan, int chain, int nth); /* list position of a chain's n-th node, or -1 */
/* Markers with id >= 64 are HOST POINTS, not stream tags: places of the list at which the caller does what a capture cannot
 * record (the RCCL all-reduces of the data-parallel iteration).  Returns their number; ids / list positions / chains of the first
 * max_out in list order.  The caller issues [lo, pos + 1), makes its own call on that chain's stream, and goes on. */
int pdgn_replay_points(void *plan, int *ids, int *pos, int *chain, int max_out);
int pdgn_replay_joined(void *plan); /* 1: the chain of marker 0 ends behind every other chain's last node */
/* In-iteration timing: pdgn_replay_kernel_nodes finds the list positions of the nodes launched through a host symbol (a kernel
 * instance, e.g. from pdgn_gemm_nt_ps_launch_info) with a given grid.x (< 0: any); pdgn_replay_chain_neighbor steps along a node's
 * chain (the memset in front of a stream-K launch, the tail kernel behind it); pdgn_replay_time_spans brackets spans [first, last] of
 * one chain with two timing events on that chain's stream for the next `slots` passes; pdgn_replay_time_read waits for them and
 * returns ms_out[i * slots + j] for j < counts[i].  bench.py measures its roofline kernel this way, inside the timed steps. */
int pdgn_replay_kernel_nodes(void *plan, const void *sym, int gx, int *pos, int max_out);
int pdgn_replay_chain_neighbor(void *plan, int pos, int dir, int *kind_out, const void **sym_out);
int pdgn_replay_time_spans(void *plan, const int *first, const int *last, int n, int slots);
int pdgn_replay_time_read(void *plan, float *ms_out, int *counts);
int pdgn_replay_launch_timed(void *plan, double *us32); /* measurement: host microseconds per call kind / chain */
int pdgn_replay_probe_chain(void *plan, int chain, int stride, float *ms_out, int *pos_out, int max_out); /* measurement: device-time progress of one chain */
int pdgn_replay_destroy(void *plan);

/* ------------------------------------------------------------------ optimiser
 * One Adam step (lr, betas, eps; no weight decay / amsgrad / maximize -- the reference's five torch.optim.Adam, models/PDGNet_v2.py:
 * 121-125, 186-226, 256) of a whole list of fp32 tensors: replaces torch._fused_adam_ (five launches of 64 K-element chunks, 230 us
 * for the generator's 12.7 M parameters).  p, g, m, v: HOST arrays of ntensors device pointers (parameter, gradient, first and
 * second moment; 4-byte aligned, 16-byte aligned ones take the vector path), n: their element counts; the pointers travel in the
 * kernel arguments (72 tensors per launch, one workgroup per 4096 elements).  step (device): the count t >= 1 of THIS update as one
 * float.  torch's arithmetic, bit for bit: m <- beta1 m + (1 - beta1) g; v <- beta2 v + (1 - beta2) g g; p <- p - lr / (1 - beta1^t) * m /
 * (sqrt(v) / sqrt(1 - beta2^t) + eps), bias corrections and 1 - beta in fp64 (torch keeps lr and the betas as doubles). */
int pdgn_adam_multi(int ntensors, void *const *p, const void *const *g, void *const *m, void *const *v, const long long *n, double lr,
                    double beta1, double beta2, double eps, const float *step, pdgn_stream_t stream);
/* dst[i] (n[i] floats) <- src[i] for a list of fp32 tensors, the same way (128 tensors per launch): the pack of a network's fresh
 * gradients into the flat buffer of its one all-reduce (the gradient reduction of nn.DataParallel, models/PDGNet_v2.py:101-105);
 * replaces torch._foreach_copy_. */
int pdgn_copy_multi(int ntensors, void *const *dst, const void *const *src, const long long *n, pdgn_stream_t stream);
/* The averaged generator: an exponential moving average e of the parameters, kept by the optimizer's own launch.  No reference
 * counterpart (the reference evaluates the generator of the last iteration).  pdgn_adam_ema_multi is pdgn_adam_multi with one more
 * HOST array of device pointers, e (4-byte aligned; a tensor whose five pointers are 16-byte aligned takes the vector path, the
 * results are the same): p, m, v come out bit for bit as pdgn_adam_multi writes them, and in the same launch, on the same walk
 * (64 tensors per launch here: five pointer arrays in 3.4 KB of kernel arguments), with t = step[0], the count of THIS update,
 *   d_t = min(ema_decay, (1 + t) / (10 + t))    in fp64, evaluated on the device;    omd = (float)(1.0 - d_t)
 *   e   = fadd(e, fmul(omd, fsub(p_new, e)))     three separately rounded fp32 operations, never contracted into an FMA.
 * State touched: p, m, v, e; read: g, step.  Keeps none of its own, allocates nothing.
 * PDGN_ERR_INVALID: pdgn_adam_multi's cases, a null or misaligned e[i], ema_decay outside [0, 1); checked before any launch. */
int pdgn_adam_ema_multi(int ntensors, void *const *p, const void *const *g, void *const *m, void *const *v, void *const *e,
                        const long long *n, double lr, double beta1, double beta2, double eps, double ema_decay, const float *step,
                        pdgn_stream_t stream);
/* The average alone, by the same expressions (the same bits as the fused launch gives for the same p and e): for an optimizer
 * step that did not go through pdgn_adam_ema_multi.  e, p: HOST arrays of ntensors device pointers (128 tensors per launch), n:
 * element counts, step (device): the count t of the update that produced p.  State touched: e; read: p, step.  Allocates nothing.
 * No reference counterpart.  PDGN_ERR_INVALID: ntensors < 1, a null or misaligned pointer, n[i] < 1, ema_decay outside [0, 1). */
int pdgn_ema_multi(int ntensors, void *const *e, const void *const *p, const long long *n, double ema_decay, const float *step,
                   pdgn_stream_t stream);

/* ------------------------------------------------------------------ gradient guard
 * The 2-norm of a network's whole gradient list, known on the device before the optimizer's launch reads it: global-norm
 * clipping, a view of the gradient magnitudes, and an update that does not happen when a gradient is not finite -- also where no
 * host is in the loop (a replayed launch list).  No reference counterpart: the reference's five optimizer.step() calls
 * (models/PDGNet_v2.py:186-226, 256) apply whatever gradient they are given.
 *
 * The guard record, one per network, in device memory (32 bytes, 4-byte aligned; the caller zero-fills it once): */
typedef struct pdgn_guard_record {
    float norm;          /* (float) sqrt(total): the fp64 root of the fp64 sum of squares, rounded once (Inf / NaN when the total is) */
    float coef;          /* the clip factor: (float) min(1.0, max_norm / (sqrt(total) + 1e-6)) in fp64 for a finite total and a finite
                            max_norm > 0; exactly 1.0f for max_norm <= 0 or infinite ("no clipping") and for a non-finite total */
    float applied;       /* 1.0f: the total is finite; 0.0f: some element is NaN or +-Inf (fp64 squares of fp32 values cannot overflow) */
    float found_inf;     /* 1.0f - applied: the flag in the form torch's fused optimizer kernel takes as `found_inf` */
    unsigned n_applied;  /* calls so far with applied == 1 ...                                                                    */
    unsigned n_skipped;  /* ... and with applied == 0: written by the finalising workgroup alone, with ordinary vector stores      */
    unsigned reserved[2];
} pdgn_guard_record;
/* Doubles of workspace pdgn_gradnorm_multi needs for a list: one per 4096-element chunk of every tensor (sum of ceil(n[i] / 4096));
 * -1 for ntensors < 1, a null n, an n[i] < 1 or more than 2^30 - 1 chunks in one launch's 128 tensors. */
long long pdgn_gradnorm_workspace_doubles(int ntensors, const long long *n);
/* record <- the guard record of the list g (HOST array of ntensors device pointers to fp32 tensors, 4-byte aligned, n: element
 * counts), max_norm as above.  ceil(ntensors / 128) launches of one workgroup per 4096-element chunk -- every element squared and
 * added IN FP64 (per thread in element order, the wave by a shuffle tree, the waves from LDS in order), one partial per chunk
 * into workspace -- then ONE workgroup that adds the partials in index order and writes the record.  No float atomics, no
 * counter of finished workgroups: the same bytes at the same addresses give the same bits.  State touched: workspace (8-byte
 * aligned, workspace_doubles >= pdgn_gradnorm_workspace_doubles(ntensors, n) doubles), record (norm, coef, applied, found_inf
 * overwritten; n_applied or n_skipped incremented); read: g.  Allocates nothing.  PDGN_ERR_INVALID, checked before any launch:
 * an invalid list (the -1 cases above), a null or misaligned g[i], workspace or record, a workspace too small, max_norm NaN. */
int pdgn_gradnorm_multi(int ntensors, const void *const *g, const long long *n, double max_norm, double *workspace,
                        long long workspace_doubles, pdgn_guard_record *record, pdgn_stream_t stream);
/* pdgn_adam_multi / pdgn_adam_ema_multi / pdgn_ema_multi behind a guard: the same kernel text with one more switch.  Every
 * workgroup reads `coef` and `applied` from the record (complete before the launch: same stream, behind pdgn_gradnorm_multi).
 * applied == 0: it returns before touching p, m, v or e -- the caller advances `step` by the device value `applied`, so a skipped
 * update leaves every byte of the optimizer's state as it was.  Otherwise the gradient in the arithmetic is fmul(g, coef),
 * rounded on its own, never contracted into what follows; g itself is not written.  coef == 1 and applied == 1: the bits of the
 * unguarded entry points.  They replace those entry points where a guard is on; state touched: p, m, v (e); read: g, step, guard.
 * PDGN_ERR_INVALID: the unguarded entry point's cases, a null or misaligned guard; checked before any launch. */
int pdgn_adam_guard_multi(int ntensors, void *const *p, const void *const *g, void *const *m, void *const *v, const long long *n,
                          double lr, double beta1, double beta2, double eps, const float *step, const pdgn_guard_record *guard,
                          pdgn_stream_t stream);
int pdgn_adam_ema_guard_multi(int ntensors, void *const *p, const void *const *g, void *const *m, void *const *v, void *const *e,
                              const long long *n, double lr, double beta1, double beta2, double eps, double ema_decay, const float *step,
                              const pdgn_guard_record *guard, pdgn_stream_t stream);
int pdgn_ema_guard_multi(int ntensors, void *const *e, const void *const *p, const long long *n, double ema_decay, const float *step,
                         const pdgn_guard_record *guard, pdgn_stream_t stream);

/* ------------------------------------------------------------------ learning-rate schedule
 * The rate of an Adam launch as a function of Adam's own device-side step count: warm-up, decay and drops also where no host is in
 * the loop (a replayed launch list re-issues `lr` as the double it was captured with), and with no state of its own -- a resumed
 * run continues from the restored counter.  No reference counterpart: the reference's five optimizers keep lr 1e-4 throughout
 * (models/PDGNet_v2.py:121-125).
 *
 * A schedule is a table of PDGN_LR_TABLE_DOUBLES fp64 words in device memory (8-byte aligned), a piecewise-linear factor f(t):
 *   tab[0]                      n, the number of knots, 1 <= n <= PDGN_LR_MAX_KNOTS
 *   tab[1 + 2i], tab[2 + 2i]    t_i, f_i for i < n: t_i finite, >= 0, strictly increasing; f_i finite, >= 0; the rest is not read
 * With t the step count of THIS update (step[0] as the Adam kernels read it, after the increment; the t of the average's warm-up):
 *   f(t) = f_0                  for t <= t_0
 *   f(t) = f_{n-1}              for t >= t_{n-1}
 *   f(t) = dadd(f_i, dmul(dsub(f_{i+1}, f_i), ddiv(dsub(t, t_i), dsub(t_{i+1}, t_i))))   otherwise, for the i with t_i <= t < t_{i+1},
 *                               found by a scan from i = 0
 *   lr_eff = dmul(lr, f(t))     and step_size = (float)(lr_eff / (double)bc1), the expression lr was in
 * Every fp64 operation is rounded on its own (__dadd_rn and its kin), none contracted into an FMA, and there is no transcendental
 * function: a numpy fp64 restatement gives the same bits; at t = t_i the factor is exactly f_i.  A malformed table on the device
 * (n no integer in 1 .. 16; some t_{i+1} > t_i false for i + 1 < n, NaN included) gives f = f_0 = tab[2]; nothing past tab[2n] is
 * read, and nothing past tab[2] when n is out of range.  The values are the host's to validate before it uploads them. */
#define PDGN_LR_MAX_KNOTS 16
#define PDGN_LR_TABLE_DOUBLES 33
/* pdgn_adam_multi / _ema_multi / _guard_multi / _ema_guard_multi with a schedule: the same kernel text with one more switch, the
 * table read with uniform loads and evaluated once per workgroup where step_size is formed.  e null: no average (ema_decay is
 * not read); guard null: no guard -- the four combinations are four kernels, and with f == 1 their results are the bits of the
 * entry point without a schedule.  A skipped update (guard, applied == 0) returns before anything is touched; t advances by
 * `applied` only, so it does not advance the schedule either.  State touched: p, m, v (e); read: g, step, guard, sched.  Allocates
 * nothing.  PDGN_ERR_INVALID: that entry point's cases, a null or misaligned (8 bytes) sched; checked before any launch. */
int pdgn_adam_sched_multi(int ntensors, void *const *p, const void *const *g, void *const *m, void *const *v, void *const *e,
                          const long long *n, double lr, double beta1, double beta2, double eps, double ema_decay, const float *step,
                          const pdgn_guard_record *guard, const double *sched, pdgn_stream_t stream);
/* The schedule for the update that is ABOUT to happen, by one thread of one launch on `stream`: t = fadd(step[0], guard ?
 * guard->applied : 1.0f) -- the fp32 sum the counter update in front of the Adam launch forms -- out2[0] = f(t), out2[1] = lr_eff
 * (fp64, 8-byte aligned), out_lr32[0] = (float)lr_eff, written with ordinary vector stores.  For the optimizer routes that go
 * through torch's fused kernel (it takes the fp32 word as a tensor lr) and for tests.  State touched: out2, out_lr32; read: sched,
 * step, guard (nullable).  PDGN_ERR_INVALID: a null or misaligned pointer (guard excepted), lr negative or NaN. */
int pdgn_lr_eval(const double *sched, double lr, const float *step, const pdgn_guard_record *guard, double *out2, float *out_lr32,
                 pdgn_stream_t stream);

/* ------------------------------------------------------------------ deterministic mode
 * pdgn_set_deterministic: process-wide switch, like pdgn_gemm_set_mode.  -1 queries the current value; any other value
 * sets it (non-zero: on) and returns the previous one.  PDGN_DETERMINISTIC=1 in the environment at first use turns it on;
 * the default is off.  The _det entry points below are the fixed-order forms of the scatter-add adjoints above: bitwise
 * repeatable (each output sums its contributions in increasing index order, with no float atomics), same arguments plus
 * an integer workspace of the caller's.  The Python layer picks them while the mode is on (pdgn_amd._lib.deterministic). */
int pdgn_set_deterministic(int on);
/* Ints of workspace one CSR transpose of an index tensor takes: b * (2 * targets + 1 + edges). */
long long pdgn_det_workspace_ints(int b, int targets, long long edges);
/* pdgn_grouping_backward, fixed order: ws = pdgn_det_workspace_ints(b, n, m * nsample) ints; grad_points ACCUMULATED. */
int pdgn_grouping_backward_det(int b, int c, int n, int m, int nsample, const float *grad_out, const int32_t *idx,
                               int32_t *ws, float *grad_points, pdgn_stream_t stream);
/* pdgn_interpolation_backward, fixed order: ws = pdgn_det_workspace_ints(b, m, 3 * n) ints; grad_points ACCUMULATED. */
int pdgn_interpolation_backward_det(int b, int c, int n, int m, const float *grad_out, const int32_t *idx,
                                    const float *weight, int32_t *ws, float *grad_points, pdgn_stream_t stream);
/* pdgn_gathering_backward, fixed order: ws = pdgn_det_workspace_ints(b, n, m) ints; grad_points ACCUMULATED. */
int pdgn_gathering_backward_det(int b, int c, int n, int m, const float *grad_out, const int32_t *idx, int32_t *ws,
                                float *grad_points, pdgn_stream_t stream);
/* pdgn_nndistance_grad, fixed order (a point's own term first, then those of the other cloud's points whose nearest it
 * is, in their index order): ws = pdgn_det_workspace_ints(b, n, m) + pdgn_det_workspace_ints(b, m, n) ints. */
int pdgn_nndistance_grad_det(int b, int n, const float *xyz1, int m, const float *xyz2, const float *grad_dist1,
                             const int32_t *idx1, const float *grad_dist2, const int32_t *idx2, int32_t *ws,
                             float *grad_xyz1, float *grad_xyz2, pdgn_stream_t stream);

/* ------------------------------------------------------------------ batch feeder
 * One launch fills one training batch from a device-resident data set: replaces ShapeNetCore.__getitem__'s three
 * np.random.choice sub-samplings and the DataLoader's shuffled collate (datasets_4point.py:370-380), the unpacking, the four
 * transposes and the two np.random.normal(0, 0.2) draws of the training loop (models/PDGNet_v2.py:171-178, 184, 195, 206, 217,
 * 228).  data (S,N,3) normalised clouds; order (S) int32, the epoch's permutation of [0, S) (entries are clamped to that
 * range); local row b takes cloud c = order[first + b]:
 *   p4[b] (3,N)     = data[c] transposed;
 *   pk[b,:,j]       = data[c, i, :], i uniform in [0, N) drawn WITH replacement, independently per row, resolution, iteration;
 *   z1, z2 (B,128)  ~ N(0, sigma^2).
 * Randomness is Philox4x32-10 (Salmon et al., SC'11), counter-based and a pure function of the arguments -- no device state,
 * no dependence on grid shape or launch order:
 *   key     = (seed low 32, seed high 32)
 *   counter = (group j, global row = row0 + b, t low 32, tag | (t >> 32 & 0xffffff) << 8)
 *   tag     = 0, 1, 2: the index streams of p1, p2, p3;  3, 4: z1, z2  (5: the host's epoch permutation, pdgn_amd.data.epoch_order;
 *             6: the round keys of pdgn_feed_batch_resample, 7: the start index of pdgn_feed_fps_pyramid, 8 .. 11: the surface draws
 *             of pdgn_feed_batch_mesh, 12: pdgn_sample_surface, 13: the round keys of pdgn_sample_ragged, all below)
 * A group is the four output words of one counter.  Index streams: word e of group j is column 4j + e, i = (word * N) >> 32
 * (bias of a point's probability at most N / 2^32 relative: 4.8e-7 at N = 2048).  Noise: group j gives columns 4j .. 4j+3 as
 * two Box-Muller pairs (words 0,1 and 2,3): u1 = ((w >> 8) + 1) * 2^-24 in (0, 1], u2 = (w' >> 8) * 2^-24 in [0, 1),
 * (sigma * sqrt(-2 ln u1) * cos(2 pi u2), sigma * sqrt(-2 ln u1) * sin(2 pi u2)), evaluated in fp32 with the accurate logf /
 * sincosf.  With the GLOBAL row (row0 = rank * B) and the global iteration t, W ranks at local batch B draw exactly what one
 * rank draws at batch B * W.  The clouds are bit-exact copies; one thread writes four consecutive columns (16-byte stores
 * where the row length is a multiple of 4 and the base 16-byte aligned).
 * PDGN_ERR_INVALID: B <= 0 or > 65535, S, N or an r <= 0, first < 0, first + B > S, row0 < 0 or row0 + B > 2^32, a null
 * pointer, z1 / z2 not 16-byte aligned.  All of these are checked on the host before anything is launched. */
int pdgn_feed_batch(int B, int S, int N, int r1, int r2, int r3, const float *data, const int32_t *order, long long first,
                    unsigned long long seed, unsigned long long t, long long row0, float sigma, float *p1, float *p2, float *p3,
                    float *p4, float *z1, float *z2, pdgn_stream_t stream);

/* The same launch for clouds stored DENSER than they are trained on: data (S,M,3), of which the leading P points of a cloud (the
 * pool) may be drawn and N points make the finest output, N <= P <= M.  A fresh N-point subset per row and iteration (the training
 * protocol of the 15 000-point ShapeNetCore.v2.PC15k sets; no reference counterpart: the reference trains on a pre-cut file).
 * With c = order[first + b]:
 *   p4[b,:,j]       = data[c, pi(j), :],  j < N, pi a bijection of [0, P) chosen by (seed, t, global row): N DISTINCT points, drawn
 *                     without replacement;
 *   pk[b,:,j]       = data[c, i, :],  i = (word * P) >> 32: pdgn_feed_batch's counters and tags 0 1 2, WITH replacement from the pool,
 *                     independently of p4 (datasets_4point.py:374-379 draws them from the whole stored cloud);
 *   z1, z2          exactly what pdgn_feed_batch writes for the same (seed, t, row0, sigma) (tags 3 4).
 * pi is a keyed balanced Feistel network extended to [0, P) by cycle-walking, evaluated per output point (no sort, no state):
 *   bits = max(2, bit length of P - 1),  h = (bits + 1) / 2 (integer division),  the network permutes [0, 2^(2h)) >= [0, P);
 *   keys k0 .. k5 = words 0 1 2 3 of the counter (0, global row, t low 32, 6 | (t >> 32 & 0xffffff) << 8) and words 0 1 of the counter
 *                   (1, ...) with the key (seed low 32, seed high 32): one key set per row and iteration;
 *   E(x):  L = x >> h, R = x & (2^h - 1);  for i = 0 .. 5: (L, R) <- (R, L ^ F(R, k_i));  E = L << h | R
 *   F(r, k) = (((r ^ k) * 0x9E3779B1) mod 2^32) >> (32 - h)            (the top h bits of a multiplicative hash)
 *   pi(j):  x = E(j);  while x >= P: x = E(x).
 * Every Feistel round is invertible whatever F is, so E is a bijection of [0, 2^(2h)); following E from j < P until it is
 * back below P visits j's own cycle, so the walk ends (at j itself at the latest) and pi is a bijection of [0, P).  2^(2h) <= 4 P,
 * so a pass lands below P with probability >= 1/4.  Uniformity is a claim for pools of thousands of points only (chi^2
 * of the inclusion counts at P = 15000, N = 2048: tests/test_resample_host.py); at h <= 3 bits the round function is visibly
 * non-uniform and only bijectivity holds.  One thread owns four consecutive columns: four 12-byte gathers, a 16-byte store per
 * channel where aligned.  No LDS, no atomics.
 * PDGN_ERR_INVALID: pdgn_feed_batch's cases (with P or M <= 0 as well), N > P, P > M, 3 M beyond the int range; checked on the
 * host before anything is launched. */
int pdgn_feed_batch_resample(int B, int S, int M, int P, int N, int r1, int r2, int r3, const float *data, const int32_t *order,
                             long long first, unsigned long long seed, unsigned long long t, long long row0, float sigma, float *p1,
                             float *p2, float *p3, float *p4, float *z1, float *z2, pdgn_stream_t stream);

/* The same launch for shapes stored as TRIANGLE MESHES (the form ShapeNetCore is distributed in; no reference counterpart: the
 * reference trains on a pre-sampled file): every output column of every resolution is a fresh i.i.d. point of the surface of the
 * row's shape.  A mesh set is four device arrays:
 *   verts    (V,3) float     the vertices of all S shapes, concatenated
 *   faces    (F,3) int32     GLOBAL vertex indices
 *   face_off (S+1) int32     shape c owns the faces [face_off[c], face_off[c+1]), F_c of them, F_c >= 1
 *   alias    (F,2) uint32    per face the record (threshold, alias) of its shape's alias table (Walker 1977 / Vose 1991), alias a face
 *                            index LOCAL to the shape; 8-byte aligned: one 8-byte load serves a draw
 * Local row b takes shape c = order[first + b] (clamped as pdgn_feed_batch clamps).  Column j of resolution k (k = 0 .. 3: p1 .. p4)
 * uses the four words w0 .. w3 of ONE Philox4x32-10 call, key (seed low 32, seed high 32),
 *   counter = (j, global row = row0 + b, t low 32, tag | (t >> 32 & 0xffffff) << 8),  tag = 8 + k:
 *   face     s = (w0 * F_c) >> 32;  f = w1 < alias[face_off[c] + s].threshold ? s : alias[face_off[c] + s].alias        (local to c)
 *   inside   a = w2 >> 8, b = w3 >> 8;  if a + b > 2^24: a = 2^24 - a, b = 2^24 - b;  u = a * 2^-24, v = b * 2^-24
 *            (integers up to 2^24: every value is exact in fp32, the fold cannot round; u, v >= 0 and u + v <= 1 exactly)
 *   point    per coordinate, with (v0, v1, v2) the vertices of face f:  e1 = v1 - v0, e2 = v2 - v0,  p = (v0 + u * e1) + v * e2,
 *            every operation rounded to fp32 on its own (never contracted to a fused multiply-add).
 * A face is drawn with probability area / the shape's area up to the table's quantisation (thresholds are 32-bit: 2^-31 in total
 * variation) and the bias of the slot draw (F_c / 2^32 relative); a face of threshold 0 that is nobody's alias is never drawn.  The four
 * resolutions are independent draws (the mesh analogue of the reference's independent with-replacement sub-samplings).  z1, z2: exactly
 * what pdgn_feed_batch writes for the same (seed, t, row0, sigma) (tags 3 4).  face_rec (B, r1 + r2 + r3 + N) int32, nullable
 * (tests; NULL in production): the GLOBAL face index drawn for every output column, in the order p1 p2 p3 p4.  One thread owns four
 * consecutive columns of one resolution (16-byte stores per channel where the row length is a multiple of 4 and the base 16-byte
 * aligned); four dependent gathers per point (face_off, alias, faces, verts); no LDS, no atomics.  The kernel TRUSTS the table:
 * F_c >= 1, vertex indices inside [0, V), alias < F_c are the caller's to guarantee (pdgn_amd.meshes.MeshSet does).
 * PDGN_ERR_INVALID: pdgn_feed_batch's cases, a null verts / faces / face_off / alias, S < 1, V < 1, F < S, 3 F or 3 V beyond the int
 * range, alias not 8-byte aligned (the others, face_rec included: 4 bytes); checked on the host before anything is launched. */
int pdgn_feed_batch_mesh(int B, int S, int V, int F, int N, int r1, int r2, int r3, const float *verts, const int32_t *faces,
                         const int32_t *face_off, const uint32_t *alias, const int32_t *order, long long first, unsigned long long seed,
                         unsigned long long t, long long row0, float sigma, float *p1, float *p2, float *p3, float *p4, float *z1,
                         float *z2, int32_t *face_rec, pdgn_stream_t stream);

/* The same draw as an op (held-out and evaluation clouds): out (S,n,3) point-major, out[s, j] a point of the surface of shape s by
 * the construction above from the counter (j, s, draw low 32, 12 | (draw >> 32 & 0xffffff) << 8): tag 12 keeps these streams apart
 * from every training draw of the same seed.  face_rec (S,n) int32, nullable: the global face index of every point.
 * PDGN_ERR_INVALID: S < 1, n < 1, a null or misaligned mesh pointer (as above) or out (4 bytes). */
int pdgn_sample_surface(int S, int n, const float *verts, const int32_t *faces, const int32_t *face_off, const uint32_t *alias,
                        unsigned long long seed, unsigned long long draw, float *out, int32_t *face_rec, pdgn_stream_t stream);

/* The same launch for clouds that store DIFFERENT numbers of points (part-annotation sets, scans, the output of any surface sampler with
 * a density target; no reference counterpart for the device feed: PartDataset.__getitem__, datasets_4point.py:76-96, which draws
 * np.random.choice(len, n, replace = len <= n) per item on the host, is the nearest thing).  A ragged set is two device arrays:
 *   points   (T,3) float      the points of all S shapes, back to back
 *   off      (S+1) int64      shape c owns the points [off[c], off[c+1]), M_c = off[c+1] - off[c] of them, M_c >= 1; 8-byte aligned
 * All integer arithmetic is exact; the Philox layout, key and tags are pdgn_feed_batch's.  Local row b takes shape c = order[first + b]
 * (clamped as pdgn_feed_batch clamps); lo = off[c] clamped into [0, T], M_c = off[c+1] - lo clamped into [0, T - lo] -- a bad table reads
 * other points than it names, never outside points; a row with M_c = 0 (only reachable with a table pdgn_amd.clouds.CloudSet refuses)
 * writes zeros to its columns of p1 .. p4.
 *   p4[b,:,j]       = points[lo + pi_c(j mod M_c)],  j < N, pi_c the keyed Feistel permutation of pdgn_feed_batch_resample with P
 *                     replaced by M_c: h_c = (max(2, bit length of M_c - 1) + 1) / 2 computed per row, the six round keys from the
 *                     counters (0 | 1, global row, t low 32, 6 | (t >> 32 & 0xffffff) << 8), cycle-walked into [0, M_c).
 *                     M_c >= N: N DISTINCT points of the shape, a fresh subset per visit.  M_c < N: every stored point appears
 *                     floor(N / M_c) or ceil(N / M_c) times -- the whole short cloud, its duplicates spread evenly, no new random
 *                     stream.  (The reference draws such a cloud fully WITH replacement, which leaves about a fraction
 *                     (1 - 1/M_c)^N of its points out of the item: holes.  Here nothing stored is left out.)
 *   pk[b,:,j]       = points[lo + ((word * M_c) >> 32)]: pdgn_feed_batch's counters and tags 0 1 2, WITH replacement from the whole
 *                     shape, independently of p4;
 *   z1, z2          exactly what pdgn_feed_batch writes for the same (seed, t, row0, sigma) (tags 3 4).
 * On a set whose shapes all store M points every output byte equals pdgn_feed_batch_resample(M = P = M); W ranks at batch B draw what
 * one rank draws at B * W; a resumed epoch is fed what an uninterrupted one is.  Geometry is pdgn_feed_batch_resample's: one thread
 * owns four consecutive columns of one row (four 12-byte gathers, a 16-byte store per channel where the row length is a multiple of 4
 * and the base 16-byte aligned), blockIdx.y is the row, no LDS, no atomics; offsets into points are 64-bit.
 * PDGN_ERR_INVALID: pdgn_feed_batch's cases, a null points or off, off not 8-byte or points not 4-byte aligned, T < 1, T > 2^31 - 1
 * (a shape's count -- the domain of its permutation and the operand of the multiply-high -- is one 31-bit number; with 64-bit
 * offsets 3 T itself needs no smaller bound: 2^31 - 1 points are 24 GiB); checked on the host before anything is launched. */
int pdgn_feed_batch_ragged(int B, int S, int N, int r1, int r2, int r3, const float *points, const long long *off, long long T,
                           const int32_t *order, long long first, unsigned long long seed, unsigned long long t, long long row0,
                           float sigma, float *p1, float *p2, float *p3, float *p4, float *z1, float *z2, pdgn_stream_t stream);

/* The same draw as an op (the reference clouds of the test phase and the reports): out (S,n,3) point-major,
 *   out[s, j, :] = points[off[s] + pi_s(j mod M_s)],
 * pi_s as above with the round keys from the counters (0 | 1, s, draw low 32, 13 | (draw >> 32 & 0xffffff) << 8), key (seed low 32,
 * seed high 32): tag 13 keeps these streams apart from every training draw of the same seed; a pure function of (seed, draw).  The
 * range of a shape is clamped as above.
 * PDGN_ERR_INVALID: S < 1, n < 1, a null or misaligned points / off (as above) or out (4 bytes), T < 1, T > 2^31 - 1. */
int pdgn_sample_ragged(int S, int n, const float *points, const long long *off, long long T, unsigned long long seed,
                       unsigned long long draw, float *out /* (S,n,3) */, pdgn_stream_t stream);

/* ------------------------------------------------------------------ farthest-point sampling, register resident (csrc/fps.hip)
 * The iteration of furthestsampling_cuda_launcher (lib/pointops/src/sampling/sampling_cuda_kernel.cu:59-168; pdgn_furthestsampling
 * above keeps that launcher's signature) for a caller in front of every training iteration: one workgroup per cloud, the cloud
 * and the running minimum distance in registers for the whole call -- global memory is read once and written once per selected
 * index; there is no `temp` argument.  Same arithmetic as pdgn_furthestsampling: d = fma(dz,dz, fma(dy,dy, dx*dx)), the
 * running minimum is fminf and starts at 1e10 (pointops.py:24), a round takes the point of the largest minimum, exact ties go
 * to the LOWEST index -- so that from start 0 the output is index for index pdgn_furthestsampling's.  A point already taken
 * has minimum 0 and is taken again only when every point has (fewer distinct points than m: the lowest index repeats).
 * Supported n: 1 .. PDGN_FPS_MAX_N (what the registers of one workgroup hold); a larger n is PDGN_ERR_INVALID, not a slower path.
 *
 * pdgn_fps_order: xyz (b,n,3), start (b) int32 or NULL (= 0 for every cloud), order (b,m) int32:
 *   order[:,0] = start, then m - 1 rounds; 1 <= m <= n.  start[.] must be in [0, n): it lives on the device and is the caller's to
 *   validate (pdgn_amd.pointops.fps_order does, on the host); the kernel clamps what it finds into the range.
 * PDGN_ERR_INVALID: b < 0, n < 1 or > PDGN_FPS_MAX_N, m < 1 or > n, a null or misaligned (4 bytes) xyz / order; b = 0 returns 0
 * and launches nothing.  Checked on the host before anything is launched. */
#define PDGN_FPS_MAX_N 8192
int pdgn_fps_order(int b, int n, int m, const float *xyz, const int32_t *start, int32_t *order, pdgn_stream_t stream);

/* The feeder's farthest-point pyramid (no reference counterpart: datasets_4point.py:370-380 draws the three sub-resolutions
 * independently and with replacement, which is what pdgn_feed_batch does): the same kernel on the finest real batch the feed launch
 * has just written, p4 (B,3,N) channel-major, r3 - 1 rounds per row, and in the same launch
 *   pk[b,:,j] = p4[b,:, order[b,j]],  j < rk,  k = 1 2 3        (bit copies; p1, p2, p3 are (B,3,r1) (B,3,r2) (B,3,r3))
 * so that p1 is the leading r1 columns of p2, p2 the leading r2 of p3 and every level is a farthest-point subset of the level above.
 * order_out (B,r3) int32 may be NULL.  The start index of row b is word 0 of the Philox4x32-10 counter
 *   (0, global row = row0 + b, t low 32, PDGN_FEED_TAG_FPS | (t >> 32 & 0xffffff) << 8),  key (seed low 32, seed high 32)
 * (pdgn_feed_batch's layout; tag 7 is used by neither the feeder, 0 .. 6, nor the augmentation, PDGN_AUG_TAG_BASE ..), reduced to
 * [0, N) by (word * N) >> 32.  A pure function of its arguments: ranks compose through row0 and a resumed epoch repeats.
 * PDGN_ERR_INVALID: B < 1, N < 1 or > PDGN_FPS_MAX_N, not 1 <= r1 <= r2 <= r3 <= N, row0 < 0 or row0 + B > 2^32, a null or
 * misaligned (4 bytes) p4 / p1 / p2 / p3.  Checked on the host before anything is launched. */
#define PDGN_FEED_TAG_FPS 7
int pdgn_feed_fps_pyramid(int B, int N, int r1, int r2, int r3, const float *p4, unsigned long long seed, unsigned long long t,
                          long long row0, float *p1, float *p2, float *p3, int32_t *order_out, pdgn_stream_t stream);

/* ------------------------------------------------------------------ discriminator augmentation
 * A fresh random similarity transform plus jitter for every cloud in front of every discriminator call (DiffAugment, Zhao et al.
 * 2020 / ADA, Karras et al. 2020, for point clouds), differentiable, drawn on the device.  No reference counterpart
 * (utils/provider.py's augmentation is host code of another training loop and is not ported).
 *
 *   rows[b*N + n] = A_b x[b, :, n] + t_b + jitter,      A_b = s R F
 *   F       negates coordinate flip_axis;
 *   R       rotates about up_axis by theta = rot_max * v:  with (ia, ib) = (up + 1, up + 2) mod 3,
 *           R[ia][ia] = R[ib][ib] = cos, R[ia][ib] = -sin, R[ib][ia] = sin, R[up][up] = 1;
 *   s       = exp(log_scale_max * v): log-uniform in [1 / scale_max, scale_max);
 *   t_i     = trans_max * v_i;
 *   jitter  ~ N(0, sigma^2) per point and coordinate;
 *   v       = ((word >> 8) - 2^23) * 2^-23 in [-1, 1), exact in fp32.
 * Each of the five components is enabled per sample iff (its word >> 8) < its threshold, an integer in [0, 2^24]: 0 is never,
 * 2^24 always, round(p 2^24) probability p.  A disabled component is exactly the identity (cos = 1, sin = 0, s = 1, t = 0, no
 * jitter added).  Arithmetic, every operation rounded on its own:
 *   A[i][j]    = fmul(s, j == flip_axis && flipped ? -R[i][j] : R[i][j])
 *   rows[.][i] = fadd(fadd(fadd(fmul(A[i][0], x0), fmul(A[i][1], x1)), fmul(A[i][2], x2)), t_i)   (+ jitter_i by one more fadd when enabled)
 *   dx[b,j,n]  = fadd(fadd(fmul(A[0][j], d0), fmul(A[1][j], d1)), fmul(A[2][j], d2)),   d = d_rows[b*N + n]
 * so that an fp32 host evaluation from affine_out reproduces rows (sigma = 0) and dx bit for bit.
 *
 * The parameters are a table in device memory (64 bytes, 4-byte aligned) that the launches read: its address is what a captured
 * launch bakes in, its contents are the host's to overwrite in place (and to validate: the kernels take what they find). */
typedef struct pdgn_aug_table {
    unsigned thr_flip, thr_rot, thr_scale, thr_trans, thr_jitter; /* enable thresholds, each in [0, 2^24] */
    int flip_axis, up_axis;                                       /* 0 .. 2 */
    float rot_max;                                                /* radians */
    float log_scale_max;                                          /* ln(scale_max) >= 0 */
    float trans_max;
    float sigma;
    unsigned reserved[5];
} pdgn_aug_table;
/* Randomness: Philox4x32-10 with the feeder's layout (pdgn_feed_batch above: the same routine, csrc/philox.h):
 *   key     = (seed low 32, seed high 32)
 *   counter = (group, global row = row0 + b, t low 32, tag | (t >> 32 & 0xffffff) << 8),    t = clock[0] - 1
 *   tag     = PDGN_AUG_TAG_BASE + 3 * network + role: network 0 .. 3 = D1 .. D4; role 0 = real, 1 = fake (the generated cloud of the
 *             discriminator's update), 2 = gen (the generator's own pass through the discriminator): 16 .. 27, disjoint from the
 *             feeder's tags 0 .. 5 -- under one seed all twelve call sites of an iteration draw independently of each other and of the feed
 *   group 0      words 0 .. 3: flip, rotation, scale, translation enabled?
 *   group 1      word 0: jitter enabled?  word 1: v of theta, word 2: v of s
 *   group 2      words 0 .. 2: v of t_x, t_y, t_z
 *   group 4 + n  point n's jitter: Box-Muller pairs (words 0, 1) -> x, y and (words 2, 3) -> z, unused; pdgn_feed_batch's formula
 * The CLOCK is a 64-bit word in device memory (8-byte aligned) that the kernels read themselves -- it is not a launch argument, so
 * a replayed launch list draws afresh every time.  It counts the iterations BEGUN: pdgn_augment_tick opens an iteration, and every
 * launch of that iteration draws at t = clock - 1 (the first iteration after clock = c draws at t = c).  With the GLOBAL row
 * (row0 = rank * B), W ranks at batch B draw what one rank draws at batch B * W.
 *
 * pdgn_augment_rows_fwd: x (B,3,N) -> rows (B*N,3); replaces the copy kernel of PointDiscriminator.forward's
 * `x.transpose(1, 2).reshape(B * N, 3)` (torch; the reference's Conv1d reads (B,3,N) directly, models/PDGNet_v2.py:886-1014).
 * x_point_major != 0: x is stored (B,N,3) -- a (B,3,N) view of point-major rows, which is what the generator hands out
 * (torch's reshape is a view then, and this launch replaces nothing: it is one the feature adds).  dx_point_major likewise for dx.
 * affine_out (may be NULL): (B,12), per sample A row-major then t, exactly the values used.  One thread writes four points'
 * rows (16-byte loads and stores where N % 4 == 0 and both bases are 16-byte aligned, element-wise otherwise).
 * pdgn_augment_rows_bwd: d_rows (B*N,3) -> dx (B,3,N) = A^T d_rows; replaces that copy's adjoint (torch's copy kernel in the
 * backward pass).  It re-derives A from the same counter words: nothing but the clock word itself links the two launches, which
 * must therefore run in the same iteration (no tick between them).  Translation and jitter have zero / identity adjoints.
 * pdgn_augment_tick: clock[0] += 1 by one thread of one launch on `stream` (an ordinary vector store); replaces nothing -- the
 * one launch per iteration the feature adds.
 * State touched: rows / dx / affine_out / clock; read: x / d_rows, table, clock.  Allocates nothing.
 * PDGN_ERR_INVALID: B outside [1, 65535], N < 1 or 3 N >= 2^31, a null x / rows / table / clock, a pointer not 4-byte (clock:
 * 8-byte) aligned, row0 < 0 or row0 + B > 2^32, a tag outside [PDGN_AUG_TAG_BASE, PDGN_AUG_TAG_BASE + PDGN_AUG_SITES); all
 * checked on the host before anything is launched. */
#define PDGN_AUG_TAG_BASE 16
#define PDGN_AUG_SITES 12
int pdgn_augment_rows_fwd(int B, int N, const float *x, int x_point_major, float *rows, float *affine_out, const pdgn_aug_table *table,
                          const unsigned long long *clock, unsigned long long seed, long long row0, int tag, pdgn_stream_t stream);
int pdgn_augment_rows_bwd(int B, int N, const float *d_rows, float *dx, int dx_point_major, const pdgn_aug_table *table,
                          const unsigned long long *clock, unsigned long long seed, long long row0, int tag, pdgn_stream_t stream);
int pdgn_augment_tick(unsigned long long *clock, pdgn_stream_t stream);

/* ------------------------------------------------------------------ adaptive discriminator augmentation (ADA, Karras et al. 2020)
 * The probability p behind the table's thresholds, steered on the device from the discriminators' own outputs on the real batch.
 * The statistic is taken against the objective's decision boundary b: least squares (real -> 1, fake -> 0) has b = 0.5, the hinge
 * and the logistic objectives score with a logit and have b = 0, the paper's sign.  Per iteration and discriminator i the
 * real-batch loss term (pdgn_mse_const_count, pdgn_gan_term_count) stores pos_i = #{x > b}, neg_i = #{x < b}, n_i = n into slot i of
 * `slots`, a contiguous int32[16] of its own (4 words per discriminator, word 3 unused; separate from the state so that it can be
 * all-reduced (SUM) across ranks).  pdgn_augment_tick_ada, which opens every iteration in place of pdgn_augment_tick:
 *   clock[0] += 1
 *   fold: (P, G, N) = the sum of the four slots; the slots are zeroed.  If N > 0: pos += P, neg += G, n += N, the per-network
 *         accumulators net[3 i ..] += slot i, iters += 1  (an iteration that contributed nothing does not count)
 *   if iters >= interval, ONE update:
 *         r    = (double)(pos - neg) / (double)n                        IEEE fp64, the operands exact
 *         step = max(1, (n * 2^24) / (4 * span))                        unsigned 64-bit integer division; span: the number of real
 *                                                                       clouds over which p travels 0 -> 1 (4: four discriminators count each)
 *         r > target: thr += step;  r < target: thr -= step;  r == target: thr unchanged;  thr clamped to [thr_min, thr_max]
 *         table->thr_<component k> = thr for every k with bit k of `mask` set (flip, rot, scale, trans, jitter = bits 0 .. 4); a
 *         component outside the mask (its range is zero) keeps what it has, 0
 *         last_r = r, last_pos / last_neg / last_n = pos, neg, n, last_net = net; pos = neg = n = iters = 0, net = 0, updates += 1
 * thr = round(p 2^24) as in the table.  Integers throughout, and the step derived from n: W ranks at batch B whose slots are
 * summed take exactly the step one rank takes at B W.
 * No fence and no atomic: every writer of a slot (one pdgn_mse_const_count per discriminator and iteration, on that discriminator's
 * stream) is stream-ordered BEFORE the next tick, which runs on the issuing stream after all chains of the previous iteration
 * have joined it, and before any side stream of its own iteration forks; each slot has a single writer per iteration, the state
 * and the thresholds only the tick (and the host, between iterations, in stream order).  The argument of the clock, above.
 * The state is the host's to write (and to validate: the kernel takes what it finds); 8-byte aligned, 40 64-bit words. */
typedef struct pdgn_ada_state {
    double target;                                /* word 0: in (-1, 1) */
    unsigned long long interval;                  /* 1: contributing iterations per update, >= 1 */
    unsigned long long span;                      /* 2: real clouds for p to travel from 0 to 1, in [1, 2^40] */
    unsigned long long thr_min, thr_max;          /* 3, 4: thr_min <= thr_max <= 2^24 */
    unsigned long long mask;                      /* 5: bit k: the tick writes thr into component k's threshold */
    unsigned long long thr;                       /* 6: the current threshold, round(p 2^24) */
    unsigned long long pos, neg, n;               /* 7 .. 9: accumulators since the last update */
    unsigned long long iters;                     /* 10: contributing iterations since the last update */
    unsigned long long updates;                   /* 11: updates made */
    double last_r;                                /* 12: r of the last update */
    unsigned long long last_pos, last_neg, last_n; /* 13 .. 15: its totals */
    unsigned long long last_net[12];              /* 16 .. 27: its per-network (pos, neg, n), D1 .. D4 */
    unsigned long long net[12];                   /* 28 .. 39: per-network accumulators since the last update */
} pdgn_ada_state;
#define PDGN_ADA_STATE_WORDS 40
#define PDGN_ADA_SLOT_WORDS 16
/* pdgn_augment_tick_ada: one launch of a single wave on `stream`, plain loads and ordinary vector stores; replaces
 * pdgn_augment_tick in adaptive mode, so an adaptive iteration has exactly the launches of a fixed-p one.
 * State touched: clock, state, slots, table's five thresholds.  Allocates nothing.
 * PDGN_ERR_INVALID (host-side, from a copy the caller passes of the parameters it wrote -- the device record is not read on the
 * host): a null clock / state / slots / table, clock or state not 8-byte aligned, slots or table not 4-byte aligned,
 * interval < 1, span < 1 or > 2^40, thr_min > thr_max, thr_max > 2^24. */
int pdgn_augment_tick_ada(unsigned long long *clock, pdgn_ada_state *state, int32_t *slots, pdgn_aug_table *table, long long interval,
                          long long span, long long thr_min, long long thr_max, pdgn_stream_t stream);

/* ------------------------------------------------------------------ preview sheets
 * A contact sheet of point clouds as ONE 8-bit grey image (what pdgn_amd/report.py writes at a snapshot): `rows` samples down,
 * `cols` <= 8 cloud lists across, every cell `cell` x `cell` pixels; image (rows * cell, cols * cell) uint8, row-major.
 * clouds: HOST array of `cols` device pointers, npoints: HOST array of their point counts; cloud c is (rows, npoints[c], 3)
 * fp32, or (rows, 3, npoints[c]) where bit c of channel_major is set.  view: HOST, 3 x 4 row-major; for a point (x, y, z)
 *   u = fma(m02, z, fma(m01, y, fma(m00, x, m03)))   column inside the cell, pixel floor(u)
 *   v = fma(m12, z, fma(m11, y, fma(m10, x, m13)))   row inside the cell, pixel floor(v)
 *   d = fma(m22, z, fma(m21, y, fma(m20, x, m23)))   depth, clamped to [0, 1], 0 = nearest
 * in exactly this order.  q = min((uint32)(d * 2^24), 2^24 - 1); key = q << 8 | shade, shade = 255 - (q >> 17) (255 nearest ..
 * 128 farthest).  Every pixel of the disc dx^2 + dy^2 <= radius^2 around (floor(u), floor(v)) that lies INSIDE the point's own
 * cell takes the minimum of its key and this one (integer atomic minimum on a uint32: the result does not depend on the
 * order of arrival, so the image is bitwise repeatable); pixels outside the cell are dropped, never written to a
 * neighbour.  A pixel no point reached is 0, any other one the low byte of its smallest key.  Points with a NaN coordinate
 * are skipped.  workspace: pdgn_render_workspace_bytes(rows, cols, cell) bytes of the caller's (one uint32 key per pixel),
 * 16-byte aligned; image 4-byte aligned.  Three launches on `stream` (clear, splat, resolve): 46 us for 35 x 5 cells of 128 pixels.
 * PDGN_ERR_INVALID: rows outside [1, 65535], cols outside [1, 8], cell outside [1, 4096], more than 2^30 pixels, radius
 * outside [0, 16], a point count outside [1, 2^24], a null or misaligned pointer; all checked before anything is launched. */
long long pdgn_render_workspace_bytes(int rows, int cols, int cell);
int pdgn_render_sheet(int rows, int cols, const float *const *clouds, const int *npoints, int channel_major, const float *view,
                      int cell, int radius, void *workspace, uint8_t *image, pdgn_stream_t stream);
/* pdgn_render_sheet_lit: the same sheet, shaded by surface normals where a column has them.  Every argument of
 * pdgn_render_sheet means what it means there; two more:
 *   normals  HOST array of `cols` device pointers: normals[c] is (rows, npoints[c], 3) fp32, POINT-major whatever cloud c's layout is
 *            (what pdgn_estimate_normals writes), or NULL
 *   light    HOST, 3 floats: the direction of the light, unit length is the caller's to guarantee
 * A column whose entry is NULL is shaded exactly as pdgn_render_sheet shades it, byte for byte.  A column with normals gets two-sided
 * headlight shading:  c = |(nx lx + ny ly) + nz lz|, every operation rounded on its own; c = 0 where !(c >= 0) (a NaN normal: the darkest
 * shade); c = 1 where c > 1; shade = 48 + (uint32)(207 c), truncating: 48 (edge on) .. 255 (facing the light).  key = q << 8 | shade under
 * the same integer minimum and the same resolve, so the nearest point still wins the pixel and the image stays bitwise repeatable; being
 * two-sided, the shading needs no consistently oriented normals.  Three launches on `stream` (pdgn_render_sheet's clear and resolve
 * kernels, a splat kernel of its own).  PDGN_ERR_INVALID: whatever pdgn_render_sheet refuses, a null `normals` array or `light`, a
 * normals[c] that is not 4-byte aligned; all checked before anything is launched. */
int pdgn_render_sheet_lit(int rows, int cols, const float *const *clouds, const float *const *normals, const int *npoints, int channel_major,
                          const float *view, const float *light, int cell, int radius, void *workspace, uint8_t *image, pdgn_stream_t stream);
/* pdgn_render_sheet_mesh: a sheet whose columns are each a cloud list or a list of TRIANGLE MESHES (csrc/render_mesh.hip, DESIGN.md
 * section 7v; no reference counterpart).  Column c is a mesh column where mesh_verts[c] is not NULL; every other column is a cloud column
 * and clouds[c], normals[c], npoints[c], channel_major bit c and radius mean what they mean in pdgn_render_sheet_lit (of a mesh column
 * they are not read).  All the mesh_* arguments are HOST arrays of `cols` entries, per column:
 *   mesh_verts   device (mesh_nverts[c], 3) fp32
 *   mesh_faces   device (mesh_nfaces[c], 3) int32
 *   mesh_range   device (rows, 3) int32: (first face, face count, vertex base) of the row's mesh.  The faces first .. first + count - 1,
 *                clipped to [0, mesh_nfaces[c]), are drawn; the base is added to each of their indices (surface-nets output: indices
 *                local to their cloud, base = vert_off[row]; a packed mesh set: global indices, base 0).  A count <= 0 draws nothing.
 *   mesh_mask    device (mesh_nfaces[c]) int32 or NULL: a face whose word is 0 is skipped
 *   mesh_shade   0: flat-lit, one shade per face from its fp32 normal and `light`; 1: depth, 255 - (q >> 17) of the pixel's own depth
 * The triangles are rasterised exactly, in integers, after a snap to 4 sub-pixel bits (the definition: the head of csrc/render_mesh.hip;
 * tests/mesh_render_mirror.py spells it in numpy) into the same key buffer under the same key q << 8 | shade and the same integer minimum
 * as the points: a vertex and a point at the same place land on the same pixel with the same q, and the image is bitwise repeatable
 * and independent of the order of the faces.  Launches on `stream`: pdgn_render_sheet's clear, pdgn_render_sheet_lit's splat over the
 * cloud columns (skipped where there are none), the triangle kernel over the mesh columns, pdgn_render_sheet's resolve.  workspace and
 * image as in pdgn_render_sheet.  PDGN_ERR_INVALID: whatever pdgn_render_sheet_lit refuses of the sheet and of a cloud column, a null
 * mesh_* array other than mesh_mask, no mesh column at all, and of a mesh column a null range pointer, a null faces pointer beside a
 * face count above 0, a misaligned verts, faces, range or mask pointer, a vertex count outside [1, 2^28], a face count outside
 * [0, 2^28] or a shade that is not 0 or 1; all checked before anything is launched. */
int pdgn_render_sheet_mesh(int rows, int cols, const float *const *clouds, const float *const *normals, const int *npoints, int channel_major,
                           const float *const *mesh_verts, const int32_t *const *mesh_faces, const int32_t *const *mesh_range,
                           const int32_t *const *mesh_mask, const int *mesh_nverts, const int *mesh_nfaces, const int *mesh_shade,
                           const float *view, const float *light, int cell, int radius, void *workspace, uint8_t *image, pdgn_stream_t stream);

/* ------------------------------------------------------------------ exact EMD (csrc/auction.hip)
 * The assignment problem between two clouds of n points each, cost |a_i - b_j| (Euclidean, what pdgn_matchcost sums), solved in
 * integers by a forward auction with epsilon scaling: one workgroup per pair, all state in LDS, bids resolved by 64-bit integer
 * atomic maxima on packed keys, so the result is bitwise repeatable.  No reference counterpart.
 *   quantum  q = cmax * 2^-pdgn_auction_quantum_bits(), cmax the diagonal of the bounding box of both clouds; integer cost
 *            rint(|a_i - b_j| / q), recomputed from the coordinates at every look (no n x n matrix), times n + 1 so that the last
 *            phase (epsilon = 1) ends at an optimum of the integer problem: within n q of the true optimum.
 *   assign   (b,n) int32: assign[p][i] = j, point b_j of cloud p of xyz2 is matched to point a_i of xyz1; always a permutation
 *   cost     (b): the sum of the unquantised fp32 distances of that assignment, in a fixed order (NaN: see status 2)
 *   status   (b) int32: 0 the optimum of the integer problem; 1 a cap was reached (16 n + 64 rounds in a phase,
 *            pdgn_auction_max_bids(n) bids in all, or a bid of 2^51): what was assigned stays, the rest is completed in index order;
 *            2 decided before any loop: no finite positive quantum, q < 2^-126 (all points equal, or an extent so small that the
 *            fp32 diagonal -- whose squares are denormal below extents of 2^-63 and vanish near 2^-75 -- is under 2^-106: cost of
 *            the identity; a coordinate or the diagonal not finite: cost NaN), the identity permutation
 *   bids     (b) long long or NULL: bids made, <= pdgn_auction_max_bids(n) = 64 n phases(n) (no launch; -1 for an unsupported n)
 * Supported n: 1 .. PDGN_AUCTION_MAX_N (56 bytes of LDS per point: 112 KB); a larger n is PDGN_ERR_INVALID, not a slower path.
 * pdgn_auction_assign_indexed: pair p = (cloud ia[p] of xyz1, cloud ib[p] of xyz2), cost and status only -- the same kernel, the
 * same bits as the batched entry point on the same pairs.
 * pdgn_auction_cost_grad: the adjoint of `cost` at a fixed assignment, g (b) the upstream gradient:
 *   grad1[p][i] = g[p] (a_i - b_j) / sqrt(max(|a_i - b_j|^2, 1e-20)), j = assign[p][i];  grad2[p][j] = -grad1[p][i]
 * (pdgn_matchcost_grad's clamp).  Every row is stored once, nothing is added; an index outside [0, n) stores no row.
 * PDGN_ERR_INVALID: b / npairs < 0, n < 1 or > PDGN_AUCTION_MAX_N, a null pointer (bids excepted) or one not 4-byte (bids: 8-byte)
 * aligned; b = 0 returns 0 and launches nothing.  Allocates nothing, one launch on `stream`. */
#define PDGN_AUCTION_MAX_N 2048
int pdgn_auction_quantum_bits(void);
long long pdgn_auction_max_bids(int n);
int pdgn_auction_assign(int b, int n, const float *xyz1, const float *xyz2, int32_t *assign, float *cost, int32_t *status,
                        long long *bids, pdgn_stream_t stream);
int pdgn_auction_assign_indexed(int npairs, int n, const float *xyz1, const int32_t *ia, const float *xyz2, const int32_t *ib,
                                float *cost, int32_t *status, pdgn_stream_t stream);
int pdgn_auction_cost_grad(int b, int n, const float *xyz1, const float *xyz2, const int32_t *assign, const float *g, float *grad1,
                           float *grad2, pdgn_stream_t stream);

/* ------------------------------------------------------------------ visible faces of a mesh set (csrc/visible.hip)
 * Which faces of the shapes of a mesh set (verts, faces, face_off: as pdgn_feed_batch_mesh takes them) can be seen from NV
 * orthographic views: per (shape, view) a depth buffer of R x R pixels in LDS, filled by integer minima, and one depth test per face
 * against it.  The header block of csrc/visible.hip is the normative definition (snap to integers, pass 1, pass 2, the fallback of a
 * face that covers no pixel centre); tests/visible_mirror.py spells it in numpy.  No reference counterpart.
 *   frame  (S,4) float, device: per shape the centre (3) and the radius rho > 0 of a ball that holds its vertices
 *   views  (NV,3,3) float, device: per view the rows e_x, e_y (image axes) and e_z (depth: the view looks along +e_z, a smaller e_z . p
 *          is nearer the eye); orthonormal is the caller's to guarantee, 1 <= NV <= PDGN_VISIBLE_MAX_VIEWS
 *   R      PDGN_VISIBLE_MIN_RES .. PDGN_VISIBLE_MAX_RES; 4 R^2 bytes of LDS per workgroup
 *   mask   (F) uint32, cleared here on `stream`, then bit v of mask[f] is set when face f passes in view v.  A face of zero area in 3D,
 *          or one that names a vertex outside [0, V), keeps 0.
 * The two biases of the test, in depth quanta of rho 2^-20: PDGN_VISIBLE_BIAS_COVER (a face that covers pixel centres: two layers
 * closer than rho 2^-10 are one surface) and pdgn_mesh_visibility_bias_small(R) = floor(3 2^20 / R) (a face that covers none: the depth
 * a face at 45 degrees spans over 1.5 pixels; PDGN_ERR_INVALID for an unsupported R).
 * The result is a pure function of the arguments, bit for bit: integer minima and integer ORs only.  One memset and one launch of S NV
 * workgroups on `stream`; before them the radii are read back once (the call waits for `stream`: a once-per-run pass, not for capture).
 * PDGN_ERR_INVALID, with nothing launched and nothing written: S, V or F < 1, 3 V, 3 F or S NV beyond the int range, NV or R outside their
 * ranges, a null pointer or one not 4-byte aligned, a radius that is not finite or not positive. */
#define PDGN_VISIBLE_MAX_VIEWS 32
#define PDGN_VISIBLE_MIN_RES 16
#define PDGN_VISIBLE_MAX_RES 192
#define PDGN_VISIBLE_BIAS_COVER 1024
int pdgn_mesh_visibility_bias_cover(void);
int pdgn_mesh_visibility_bias_small(int R);
int pdgn_mesh_visibility(int S, int V, int F, const float *verts, const int32_t *faces, const int32_t *face_off, const float *frame,
                         const float *views, int NV, int R, uint32_t *mask, pdgn_stream_t stream);

/* ------------------------------------------------------------------ face orientation from visibility (csrc/visible.hip)
 * Which SIDE of every face the views see: pdgn_mesh_visibility's depth pass, then per (face, view) the count of the face's covered pixel
 * centres that pass the depth test, added to the face's front or back column by the sign of its snapped 2D area in the stored vertex
 * order.  A face with more back votes than front votes is stored the wrong way round (Takayama et al. 2014).  The second header block of
 * csrc/visible.hip is the normative definition; tests/face_orient_mirror.py spells it in numpy.  No reference counterpart.
 * The arguments are pdgn_mesh_visibility's, with the same ranges, and
 *   votes  (F,2) uint32, cleared here on `stream`: votes[f][0] the centres (or the one fallback test) that passed in views that see the
 *          front of f -- the side its stored vertices run counter-clockwise from --, votes[f][1] those in views that see its back.  A
 *          dead face, and a face edge-on in a view, have no vote.  At most NV R^2 per word.
 *   mask   (F) uint32 or NULL: where given, cleared and then set to exactly the bits pdgn_mesh_visibility gives on the same arguments
 * A pure function of the arguments, bit for bit: integer minima, integer sums and ORs only.  One or two memsets and one launch of S NV
 * workgroups on `stream`, after the same read-back of the radii.  PDGN_ERR_INVALID, with nothing launched and nothing written: as
 * pdgn_mesh_visibility, with votes in the place of mask as the pointer that must not be null. */
int pdgn_mesh_face_votes(int S, int V, int F, const float *verts, const int32_t *faces, const int32_t *face_off, const float *frame,
                         const float *views, int NV, int R, uint32_t *mask, uint32_t *votes, pdgn_stream_t stream);

/* ------------------------------------------------------------------ repulsion regulariser and spacing statistics (csrc/repulsion.hip)
 * Every point of a cloud against every other point of the SAME cloud, in one launch: the repulsion term of the point-upsampling
 * literature (PU-Net) in a polynomial form, its gradient, and the squared distance to the nearest other point.  The header block of
 * csrc/repulsion.hip is the normative statement of the operation order; tests/repulsion_mirror.py spells it in numpy.  No reference
 * counterpart.  xyz (b,n,3); inv_h2 = 1 / h^2 for the radius h > 0.  Per point i, over j = 0 .. n-1 ascending, j != i:
 *   d = x_i - x_j, d2 = (dx dx + dy dy) + dz dz, nn2_i = min(nn2_i, d2), t = 1 - d2 inv_h2, and where !(t <= 0): s_i += t t, g_i += t d
 * every fp32 operation rounded on its own.  A NaN coordinate makes s_i and g_i NaN (it fails `t <= 0`).
 *   s          (b,n) workspace, always written: s_i
 *   loss       (1): (float)(T / (double)(b n)), T = sum_c (double)P_c over the clouds c ascending; P_c = sum_i s_i of cloud c in the
 *              fixed fp32 order of one wave (csrc/repulsion.hip: 64 lane sums over i = lane, lane + 64, ..., then a butterfly)
 *   per_cloud  (b) or NULL: (float)((double)P_c / n)
 *   grad       (b,n,3) or NULL: coef * g_i, d loss / d x_i for coef = -8 inv_h2 / (b n) (each unordered pair is in the sum twice and
 *              the derivative is gathered per point: nothing is scattered, nothing is added atomically); the caller computes coef
 *              in fp64 and rounds it once
 *   nn2        (b,n) or NULL: +inf for n = 1
 * Results do not depend on the launch geometry (pdgn_repulsion_chunk() is the number of points staged in LDS at a time: tests put
 * n on either side of it).  Two launches on `stream` (all pairs, then the reduction), no atomics, nothing allocated.
 * pdgn_repulsion_backward: dxyz[k] = g[0] * grad[k] for k < count (the saved grad times the upstream device scalar), one launch.
 * PDGN_ERR_INVALID, with nothing launched and nothing written: b < 1, n < 1 or > PDGN_REPULSION_MAX_N, b n beyond 2^28, inv_h2 (or coef)
 * not finite or inv_h2 not positive, count < 1, a null pointer (per_cloud, grad, nn2 excepted) or one not 4-byte aligned. */
#define PDGN_REPULSION_MAX_N 8192
int pdgn_repulsion_chunk(void);
int pdgn_repulsion(int b, int n, const float *xyz, float inv_h2, float coef, float *s, float *loss, float *per_cloud, float *grad,
                   float *nn2, pdgn_stream_t stream);
int pdgn_repulsion_backward(long long count, const float *grad, const float *g, float *dxyz, pdgn_stream_t stream);

/* ------------------------------------------------------------------ surface normals (csrc/normals.hip)
 * Per point, the eigen-decomposition of the covariance of its k neighbours: the normal (the eigenvector of the smallest eigenvalue) and
 * the three eigenvalues, what the lit preview sheets, evaluation.surface_stats (surface variation, Pauly et al. 2002) and the PLY export
 * read.  The header block of csrc/normals.hip is the normative statement of the operation order (mean, covariance, PDGN_NORMALS_SWEEPS
 * cyclic Jacobi sweeps with no convergence test, selection, sign, poison); tests/normals_mirror.py spells it in numpy and the two agree bit
 * for bit.  No reference counterpart.
 *   xyz      (b,n,3)
 *   idx      (b,n,k) int32: for every point k indices into its own cloud, any (repeats allowed); what pdgn_knnquery(b, n, n, k, xyz, xyz)
 *            writes has the point itself first.  Taken in slot order.
 *   orient   0: the component of largest magnitude (lowest index on ties) is made non-negative; 1: n . o >= 0 (along the direction o);
 *            2: n . (o - x_i) >= 0 (towards the position o); 3: n . (x_i - o) >= 0 (away from it).  o = (ox, oy, oz), ignored under 0.
 *   normals  (b,n,3): V's column of the smallest eigenvalue as the iteration leaves it (unit length to a few ulp, not renormalised)
 *   eig      (b,n,3) or NULL: lambda0 <= lambda1 <= lambda2 as computed (a tiny negative lambda0 from rounding is not clamped; equal
 *            values keep the lower column first, so k = 1, or k equal points whose fp32 mean is exact, give the normal (1, 0, 0) and
 *            three zeros)
 * A point with an index outside [0, n) -- which is never dereferenced -- or with an eigenvalue that is not finite (a NaN or infinite
 * coordinate among its neighbours) gets six NaNs; no other point is affected.  Results do not depend on the launch geometry, nor on
 * whether the launch copies the clouds into LDS first (256-thread workgroups and n <= PDGN_NORMALS_STAGE_MAX_N: tests put n on either side).
 * One launch on `stream`, no atomics, nothing allocated: 11.1 us for 35 x 2048 points at k = 16 (pdgn_knnquery at that shape: 117 us; profiles/normals_cost.txt).
 * PDGN_ERR_INVALID, with nothing launched and nothing written: b < 1, n < 1, k outside [1, PDGN_NORMALS_MAX_K], b n beyond 2^28, orient
 * outside 0 .. 3, a non-finite ox / oy / oz where orient != 0, a null pointer (eig excepted) or one not 4-byte aligned. */
#define PDGN_NORMALS_MAX_K 64
#define PDGN_NORMALS_SWEEPS 5
#define PDGN_NORMALS_STAGE_MAX_N 4096
int pdgn_estimate_normals(int b, int n, int k, const float *xyz, const int32_t *idx, int orient, float ox, float oy, float oz,
                          float *normals, float *eig, pdgn_stream_t stream);

/* ------------------------------------------------------------------ flatness regulariser (csrc/flatness.hip)
 * The batch mean of Pauly's surface variation sigma_i = l0 / ((l0 + l1) + l2 + eps) of every point's k-neighbourhood, and its gradient with
 * respect to the points: the term that pulls a generated cloud ONTO its surface (the repulsion term spreads it ALONG the surface).  The
 * header block of csrc/flatness.hip is the normative definition; tests/flatness_mirror.py spells it in numpy and the two agree bit for
 * bit.  The eigenvalues are pdgn_estimate_normals' on the same lists, bit for bit (csrc/pca3.h is shared).  No reference counterpart.
 *   xyz         (b,n,3)
 *   idx         (b,n,k) int32: for every point k indices into its own cloud, any (repeats allowed), taken in slot order.  The lists are
 *               DATA: the neighbour choice is not differentiated.
 *   eps         >= 0: added to the trace in the denominator (a floor under the trace of a nearly coincident neighbourhood)
 *   coef        the factor of the gradient: 1 / (b n) for d loss / d xyz; the caller computes it in fp64 and rounds it once
 *   sigma       (b,n), always written: sigma_i; 0 for a DEGENERATE point (!(l0 > 0) or !(trace + eps > 0): coincident points, an exactly
 *               flat neighbourhood), NaN for a BAD one (an index outside [0, n) -- never dereferenced -- or an eigenvalue that is not finite)
 *   loss        (1): (float)(T / (double)(b n)), T = sum_c (double)P_c, P_c = sum_i sigma_i in pdgn_repulsion's fixed fp32 order of one wave
 *   per_cloud   (b) or NULL: (float)((double)P_c / n)
 *   degenerate  (b) int32 or NULL: the number of degenerate points of every cloud (zeroed by the call, integer atomics)
 *   grad        (b,n,3) or NULL: grad_j = coef * sum over the in-edges e = i k + s of j (idx[i][s] == j), in ASCENDING e, of H_i (x_j - mu_i)
 *               with H_i = (2 / (k q)) (v v^T - sigma_i I); zero rows for a degenerate source, NaN for every target on a bad point's list.
 *               Gathered over a CSR transpose of idx whose rows are in increasing edge id: no float atomics, bitwise repeatable.
 *   ws          pdgn_flatness_workspace_bytes(b, n, k, 1) bytes, 16-byte aligned, or NULL where grad is NULL (not read then): the 48-byte
 *               records (mu, H) and the transpose's integers
 * With grad == NULL no record is written and nothing is transposed; sigma, loss, per_cloud and degenerate are the same bits either way.
 * Results do not depend on the launch geometry, nor on whether the clouds pass through LDS (as pdgn_estimate_normals).  Kernel and memset
 * nodes only on `stream` (the per-point launch and the reduction; with grad the transpose -- one workgroup per cloud up to 4096 points, csrc/det.hip's
 * memset and two launches above -- and the gather), nothing
 * allocated, no host synchronisation.  The backward of the autograd node is pdgn_repulsion_backward (dxyz = up * grad).
 * pdgn_flatness_workspace_bytes: 0 for with_grad == 0; PDGN_ERR_INVALID for dimensions pdgn_flatness refuses.
 * PDGN_ERR_INVALID, with nothing launched and nothing written: b < 1, n < 1, k outside [1, PDGN_NORMALS_MAX_K], b n k >= 2^31, eps negative or
 * not finite, coef not finite, a null pointer (per_cloud, degenerate, grad and ws excepted), grad without ws, a pointer not 4-byte (ws:
 * 16-byte) aligned. */
long long pdgn_flatness_workspace_bytes(int b, int n, int k, int with_grad);
int pdgn_flatness(int b, int n, int k, const float *xyz, const int32_t *idx, float eps, float coef, float *sigma, float *loss,
                  float *per_cloud, int32_t *degenerate, float *grad, void *ws, pdgn_stream_t stream);

/* ------------------------------------------------------------------ consistent normal orientation (csrc/orient.hip)
 * pdgn_orient_normals gives the normals of every cloud one consistent sign: a minimum spanning tree of the symmetrised neighbour graph
 * under the weight 1 - |n_u . n_v| (Prim, Hoppe et al. 1992), grown from the highest point of each connected component, whose normal is
 * turned upwards; every other point takes the sign that agrees with its tree parent.  The header block of csrc/orient.hip is the
 * normative statement of the rules (live points, edges, weight, rounds, ties); tests/orient_mirror.py spells them in numpy and the two
 * agree bit for bit: every decision is a comparison of integers.  No reference counterpart.
 *   xyz         (b,n,3)
 *   idx         (b,n,k) int32: neighbour lists (pdgn_knnquery's, or any: slot order and repeats change nothing; an index outside
 *               [0, n) is never dereferenced, it and a self index are ignored)
 *   normals_in  (b,n,3): unoriented normals (pdgn_estimate_normals, orient 0)
 *   normals_out (b,n,3): normals_in with the sign bit of all three components flipped or kept; may be normals_in itself
 *   parent      (b,n) int32 or NULL: the tree parent, -1 for the root of a component, -2 for a dead point (a coordinate or a normal
 *               component that is not finite: it keeps its input bits and takes no part in the graph)
 *   stats       (b,4) int32 or NULL: components, normals flipped, weak tree edges (weight above 0.5: more than 60 degrees between the
 *               two lines, the sign across it is a guess), dead points
 *   workspace   pdgn_orient_workspace_ints(b, n, k) int32 of the caller's: the reverse adjacency; contents undefined on return
 * One workgroup per cloud, one launch on `stream`, integer LDS atomics only, nothing allocated; repeatable bit for bit.  n is at most
 * PDGN_ORIENT_MAX_N (what one workgroup's LDS holds); a larger n is PDGN_ERR_INVALID, not a slower path.  The rounds are sequential:
 * about n of them per cloud (profiles/orient_cost.txt).
 * PDGN_ERR_INVALID, with nothing launched and nothing written: b < 1, n < 1 or > PDGN_ORIENT_MAX_N, k outside [1, PDGN_NORMALS_MAX_K],
 * b n beyond 2^28, a null xyz / idx / normals_in / normals_out / workspace, any pointer not 4-byte aligned.
 * pdgn_orient_workspace_ints: host only; the number of int32 the workspace must hold, PDGN_ERR_INVALID for a shape the entry point refuses. */
#define PDGN_ORIENT_MAX_N 4096
long long pdgn_orient_workspace_ints(int b, int n, int k);
int pdgn_orient_normals(int b, int n, int k, const float *xyz, const int32_t *idx, const float *normals_in, float *normals_out,
                        int32_t *parent, int32_t *stats, int32_t *workspace, pdgn_stream_t stream);

/* ------------------------------------------------------------------ normal orientation from visibility (csrc/cloudvis.hip)
 * The sign of a cloud's normals from which side of every point a ring of orthographic views sees (hidden point removal by a splatted
 * depth buffer, Katz et al. 2007; the votes of Takayama et al. 2014, as pdgn_mesh_face_votes casts them for faces), then a pooling of
 * the votes over each point's neighbours in its tangent plane.  Thin sheets, whose two sides fall into one neighbourhood, and clouds of
 * any size: nothing here is sequential.  The header block of csrc/cloudvis.hip is the normative statement of both sets of rules;
 * tests/cloudvis_mirror.py spells them in numpy and the two agree bit for bit.  No reference counterpart.
 *
 * pdgn_cloud_normal_votes: per (cloud, view) a depth buffer of R x R pixels in LDS (4 R^2 bytes), every live point's depth written by
 * integer minima into the pixel that holds it and into every pixel whose centre lies within `splat` of it; then a point passes where its
 * depth is at most its own pixel's minimum plus `bias`, and a point that passes adds w = (uint32)(min(|s|, 1) 256), s = g . e_z, to its
 * front (s < 0) or back (s > 0) count.
 *   xyz, normals  (b,n,3); a point with a value that is not finite among its six is dead: it splats nothing and gets no votes
 *   frame   (b,4) float, device: per cloud the centre and the radius rho of a ball that holds it (pdgn_mesh_visibility's frame; a rho
 *           that is not positive and finite snaps every point to a corner or the middle of the image: defined, and useless)
 *   views   (NV,3,3) float, device: pdgn_mesh_visibility's table, 1 <= NV <= PDGN_VISIBLE_MAX_VIEWS
 *   R       PDGN_CLOUDVIS_MIN_RES .. PDGN_VISIBLE_MAX_RES
 *   splat   >= 0, in pixel units with 8 sub-pixel bits (256 = one pixel): the radius of a point's disc; 0 writes the own pixel only
 *   bias    >= 0, in depth quanta of rho 2^-20
 *   votes   (b,n,2) uint32, cleared here on `stream`: front, back; at most NV 256 per word
 * One memset and one launch of b NV workgroups on `stream`, no host synchronisation, nothing allocated; integer minima and integer sums
 * only: a pure function of the arguments bit for bit, and a permutation of a cloud's points permutes its rows.
 *
 * pdgn_orient_pool: v_i = front_i - back_i, then `rounds` Jacobi rounds v'_i = 2 v_i + sum over the slots of c_ij v_j, c_ij in {-1, 0, 1}
 * the sign of g_i . g_j where j lies in the tangent planes of both points and the two normal lines are within 60 degrees, and
 * o_i = -g_i iff the final v_i < 0.
 *   idx         (b,n,k) int32 as pdgn_orient_normals takes them: out of range (never dereferenced), self and dead entries are ignored,
 *               a repeated entry counts as often as it occurs
 *   normals_in  (b,n,3); normals_out (b,n,3): normals_in with the sign bit of all three components flipped or kept; may be normals_in
 *   votes       (b,n,2) uint32: pdgn_cloud_normal_votes'
 *   rounds      0 .. PDGN_CLOUDVIS_MAX_ROUNDS
 *   pooled      (b,n) int64 or NULL: the final v_i (0 for a dead point)
 *   stats       (b,4) int32 or NULL, cleared here on `stream`: normals flipped, live points undecided (final v_i == 0: they keep their
 *               bits), live points unseen (front + back == 0 before any pooling), dead points
 *   workspace   2 b n int64 of the caller's (16 b n bytes, 8-byte aligned; the rounds ping-pong through it); contents undefined on return
 * rounds + 1 launches (and the memset of stats) on `stream`, one thread per point, integer atomics on stats only, nothing allocated;
 * repeatable bit for bit.
 * PDGN_ERR_INVALID, with nothing launched and nothing written: b < 1, n < 1, b n beyond 2^28, NV, R, k (1 .. PDGN_NORMALS_MAX_K) or rounds
 * outside their ranges, a negative splat or bias, a null pointer (pooled and stats excepted), a pointer not 4-byte (pooled, workspace:
 * 8-byte) aligned. */
#define PDGN_CLOUDVIS_MIN_RES 1
#define PDGN_CLOUDVIS_MAX_ROUNDS 4
int pdgn_cloud_normal_votes(int b, int n, const float *xyz, const float *normals, const float *frame, const float *views, int NV, int R,
                            int splat, int bias, uint32_t *votes, pdgn_stream_t stream);
int pdgn_orient_pool(int b, int n, int k, const float *xyz, const int32_t *idx, const float *normals_in, const uint32_t *votes, int rounds,
                     float *normals_out, long long *pooled, int32_t *stats, long long *workspace, pdgn_stream_t stream);

/* ------------------------------------------------------------------ surface reconstruction (csrc/reconstruct.hip)
 * From oriented points to a triangle mesh: a signed-distance field on a regular grid by implicit moving least squares with the compact
 * weight (1 - d^2 / h^2)^2, then its iso-surface by surface nets.  The header block of csrc/reconstruct.hip is the normative statement of
 * the operation order and of the mesh's rules (live points, nodes, active cells, vertices, quads, winding, output order);
 * tests/reconstruct_mirror.py spells them in numpy and the two agree bit for bit.  No reference counterpart.  R nodes per axis, node
 * (i,j,k) at (i R + j) R + k; a cloud's grid is origin (3), voxel, and for the field inv = 1 / h^2.
 *
 * pdgn_imls_grid: field (b, R^3) from xyz (b,n,3) and oriented normals (b,n,3).
 *   grid       (b,5) on the device: origin x y z, voxel, inv per cloud
 *   grid_host  the caller's HOST copy of the same (b,5) values: what is checked here (the device record is not read on the host)
 *   field      (b, R^3): negative inside; NaN (0x7FC00000) at a node with no live point within h.  A point with a non-finite coordinate
 *              or normal component is skipped.
 *   cull       1: per brick of 4 x 4 x 4 nodes the points that provably cannot reach it are left out, which changes no bit; 0: every
 *              point is visited at every node (measurement and tests)
 * One launch on `stream` per 2^22 workgroups (one for every cube of 8 x 8 x 8 nodes, R rounded up: a single launch for anything but
 * huge batches), no atomics, nothing allocated.  pdgn_imls_chunk(): the points staged in LDS at a time (tests put n on either side).
 * Results do not depend on the launch geometry.
 * PDGN_ERR_INVALID, with nothing launched and nothing written: b < 1, n < 1, R outside [PDGN_RECON_MIN_R, PDGN_RECON_MAX_R], b R^3 >= 2^31,
 * cull outside 0 .. 1, a null pointer or one not 4-byte aligned, a value of grid_host that is not finite, a voxel or inv that is not positive.
 *
 * pdgn_surface_nets_count: field (b, R^3) -> vflag (b, R^3) int32, 1 at the node that is the lowest corner of an active cell (ascending
 * node id is ascending cell id), qcnt (b, R^3) int32, the quads (0 .. 3) of the node's three edges, and stats (b,4) int32: vertices, faces,
 * open edges, invalid nodes.  Launches on `stream`: one that clears stats, then per 65535 clouds the cells and the quads; integer atomics
 * for the counters only.  PDGN_ERR_INVALID as above (shape, pointers), nothing launched, nothing written.
 *
 * pdgn_surface_nets_emit: the vertices and faces at their ranks.  vscan / qscan (b, R^3) int32: the INCLUSIVE prefix sums of vflag / qcnt
 * within each cloud (torch.cumsum along the node axis); vert_off / face_off (b+1) int32 on the device: exclusive prefix sums of the clouds'
 * vertex / face counts; total_verts / total_faces: their last entries as the caller read them from stats; vert_capacity / face_capacity:
 * the rows verts (.,3) fp32 / faces (.,3) int32 hold.  grid (b,4) on the device: origin, voxel; grid_host: the host copy, checked here.
 * Face entries are indices into the cloud's own vertices.  Nothing is written past the totals whatever the scans hold.  One launch per
 * 65535 clouds, no atomics.  PDGN_ERR_INVALID, nothing launched, nothing written: the shape cases above, a null or misaligned pointer
 * (verts / faces may be null where their total is 0), a total below 0 or above (2^31 - 1) / 3, a capacity below its total, a value of
 * grid_host that is not finite or a voxel that is not positive. */
#define PDGN_RECON_MIN_R 2
#define PDGN_RECON_MAX_R 256
int pdgn_imls_chunk(void);
int pdgn_imls_grid(int b, int n, int R, const float *xyz, const float *normals, const float *grid, const float *grid_host, int cull,
                   float *field, pdgn_stream_t stream);
int pdgn_surface_nets_count(int b, int R, const float *field, int32_t *vflag, int32_t *qcnt, int32_t *stats, pdgn_stream_t stream);
int pdgn_surface_nets_emit(int b, int R, const float *field, const float *grid, const float *grid_host, const int32_t *vflag,
                           const int32_t *vscan, const int32_t *qcnt, const int32_t *qscan, const int32_t *vert_off,
                           const int32_t *face_off, long long total_verts, long long total_faces, long long vert_capacity,
                           long long face_capacity, float *verts, int32_t *faces, pdgn_stream_t stream);

/* ------------------------------------------------------------------ point-to-surface distance (csrc/meshdist.hip)
 * The closest point of a triangle set: for every point of xyz (b,n,3) the live faces of shape shape[c] of a mesh set are searched.  Per
 * point the result is the lexicographic minimum of (d2_f, f) over those faces -- one unsigned 64-bit compare on bits(d2_f) << 32 | f, d2_f
 * being non-negative -- where d2_f is the per-face value whose fp32 operation order the header block of csrc/meshdist.hip states
 * (tests/p2m_mirror.py spells it in numpy; the two agree bit for bit) and f the face's index in the caller's face array.  A NaN d2_f never
 * wins.  The order in which faces are visited, the record order, the launch geometry and `cull` change no bit.  Unsigned distances; not
 * differentiable in the mesh.  No reference counterpart.
 *
 * pdgn_mesh_dist_prepare: once per mesh set (and per set of live faces): the face records and the boxes of their groups.
 *   verts (V,3), faces (F,3) int32 global vertex indices, face_off (S+1) int32: the mesh set's arrays
 *   group_off  (S+1) int32: exclusive prefix sums of ceil(F_s / pdgn_mesh_dist_group()) over the shapes; G = group_off[S], at most
 *              F / group + S
 *   live       (F) int32: 0 = the face is never visited (area zero, hidden, ...), indexed by the face's own index
 *   order      (F) int32 or NULL: slot -> face, a permutation that keeps every shape's faces inside the shape's own range
 *              [face_off[s], face_off[s+1]) (any order gives the same bits; DESIGN.md section 7t has what each costs); NULL: slot i holds face i
 *   records    (F,12) fp32, 16-byte aligned: per slot (a.x a.y a.z bits(f) | b.x b.y b.z 0 | c.x c.y c.z 0), f = -1 for a dead slot (a
 *              face that is not live, or one that names a vertex outside [0, V))
 *   groups     (G,8) fp32, 16-byte aligned: per group of slots (lo.x lo.y lo.z 0 | hi.x hi.y hi.z 0), the box of its live faces
 *              (+inf / -inf where it has none)
 * pdgn_mesh_dist_workspace_floats(S, F): host only; 12 F + 8 (F / group + S), what records and groups take together at most;
 * PDGN_ERR_INVALID for a shape the entry points refuse.  One launch on `stream`, no atomics, nothing allocated.
 *
 * pdgn_point_mesh_distance:
 *   shape      (b) int32: the shape of each cloud; repeats and any order are fine; an index outside [0, S) counts as a shape with no
 *              live face
 *   d2         (b,n): the least squared distance;  face (b,n) int32: the face that attains it;  closest (b,n,3) or NULL: the closest
 *              point.  NaN (0x7FC00000), -1, NaN for a point with a non-finite coordinate and where no live face gave a value
 *   cull       1: faces and groups of faces whose box provably lies farther than the best so far are left out, which changes no bit;
 *              0: every live face is visited at every point (measurement and tests)
 * One launch on `stream`, one thread per point, a workgroup per run of pdgn_mesh_dist_chunk() points of a cloud, the shape's records
 * through LDS that many at a time; no atomics, nothing allocated.
 * PDGN_ERR_INVALID, with nothing launched and nothing written: S, V, F, G, b or n < 1, 3 V or 3 F or b n >= 2^31, b ceil(n / chunk) > 2^23, G > F / group + S, cull
 * outside 0 .. 1, a null pointer other than order / closest, a pointer not 4-byte aligned (records, groups: 16-byte). */
int pdgn_mesh_dist_group(void);
int pdgn_mesh_dist_chunk(void);
long long pdgn_mesh_dist_workspace_floats(int S, int F);
int pdgn_mesh_dist_prepare(int S, int V, int F, int G, const float *verts, const int32_t *faces, const int32_t *face_off,
                           const int32_t *group_off, const int32_t *live, const int32_t *order, float *records, float *groups,
                           pdgn_stream_t stream);
int pdgn_point_mesh_distance(int b, int n, int S, int F, int G, const float *xyz, const int32_t *shape, const int32_t *face_off,
                             const int32_t *group_off, const float *records, const float *groups, int cull, float *d2, int32_t *face,
                             float *closest, pdgn_stream_t stream);

/* ------------------------------------------------------------------ generalized winding numbers (csrc/winding.hip)
 * Inside / outside of a triangle set (Jacobson et al. 2013): for every point of xyz (b,n,3) the solid angles that the live faces of shape
 * shape[c] subtend at it are summed.  Per face, h_f is half the signed solid angle by the van Oosterom-Strackee formula in the fp32
 * operation order that the header block of csrc/winding.hip states (tests/winding_mirror.py spells it in numpy; the two agree bit for
 * bit), t_f = llrint((double)h_f 2^32), and per point
 *   T       (b,n) int64: the sum of t_f;  INT64_MIN for a point with a non-finite coordinate and where any face gave a non-finite h_f;
 *           0 for a shape with no live face
 *   w       (b,n) fp32: (float)((double)T K), K the double nearest 1 / (2^33 pi): the winding number;  NaN (0x7FC00000) where T is INT64_MIN
 *   inside  (b,n) int32 or NULL: T >= pdgn_winding_half_turn() = llrint(pi 2^32), which is w >= 1/2
 * A sum of integers: the record order, the split over workgroups, the point order and the launch geometry change no bit.  No reference
 * counterpart.
 *   records    what pdgn_mesh_dist_prepare wrote for the same S, F and face_off (the group boxes are not used); 16-byte aligned
 *   shape      (b) int32 as for pdgn_point_mesh_distance: an index outside [0, S) counts as a shape with no live face
 *   splits     k >= 1: the chunks of pdgn_mesh_dist_chunk() record slots of each shape are divided over exactly k workgroups per run of
 *              points;  0: the library takes pdgn_winding_splits(b, n, F) -- F is the bound on a shape's face count that this call has; a
 *              caller that knows the largest face count of the shapes it names asks pdgn_winding_splits with it and passes the answer
 *   workspace  pdgn_winding_workspace_bytes(b, n, F, splits) bytes, 8-byte aligned: one int64 per point and part, each written before it is
 *              read (nothing to zero); may be NULL where that is 0 (one part)
 * One thread per point, a workgroup per run of 256 points of a cloud and part; one launch on `stream` for one part, a second small one
 * that adds the parts otherwise.  No atomics, nothing allocated.
 * pdgn_winding_splits(b, n, faces): host only; ceil(2048 / (b ceil(n / 256))) -- eight workgroups for each of 256 CUs -- at most
 * ceil(faces / 256) / 2 and 4096, at least 1.  pdgn_winding_workspace_bytes: host only; 8 parts b n, 0 for one part.  Both PDGN_ERR_INVALID
 * for sizes the entry point refuses.
 * PDGN_ERR_INVALID, with nothing launched and nothing written: S, F, b or n < 1, F > 2^28, b n >= 2^31, splits outside 0 .. 4096,
 * b ceil(n / 256) parts > 2^23, a null pointer other than inside (and workspace for one part), a pointer not 4-byte aligned (records:
 * 16-byte; workspace, T: 8-byte). */
long long pdgn_winding_half_turn(void);
int pdgn_winding_splits(int b, int n, int faces);
long long pdgn_winding_workspace_bytes(int b, int n, int F, int splits);
int pdgn_winding_number(int b, int n, int S, int F, const float *xyz, const int32_t *shape, const int32_t *face_off, const float *records,
                        int splits, long long *workspace, long long *T, float *w, int32_t *inside, pdgn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PDGN_HIP_H */
