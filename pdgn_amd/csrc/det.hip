// det.hip -- deterministic mode: the process-wide switch (pdgn_set_deterministic) and fixed-order adjoints of the
// reference-compatible scatter-adds (grouping, interpolation, gathering, nndistance gradient).
//
// The default adjoints scatter with float atomics, so the order in which contributions meet an output depends on the
// schedule and the last bits of a sum change from run to run.  Here the scatter becomes a gather over a CSR transpose
// of the index tensor whose rows list their edges in INCREASING edge id:
//   1. det_count_kernel       edges per target (integer atomics: the counts do not depend on the order);
//   2. det_scan_fill_kernel   one wave per batch: exclusive scan of the counts into row pointers, then a stable fill --
//                             64 edges at a time in edge order, each lane's slot = its row's cursor + its rank among the
//                             lanes of the same target (shuffles), one integer atomic per (target, 64 edges) moves the
//                             cursor; the row's edge list therefore comes out sorted;
//   3. a gather kernel        one thread per output element sums its row's contributions in that order.
// Integer workspace (the caller's): b * (2 * targets + 1 + edges) ints per transpose (det_ints below).
#include "common.h"

#include <atomic>
#include <stdlib.h>

static std::atomic<int> &det_flag() {
    static std::atomic<int> v{[] { const char *e = getenv("PDGN_DETERMINISTIC"); return (e && e[0] && e[0] != '0') ? 1 : 0; }()};
    return v;
}

extern "C" int pdgn_set_deterministic(int on) {
    if (on == -1) return det_flag().load();
    return det_flag().exchange(on ? 1 : 0);
}

#define DET_THREADS 256

__global__ __launch_bounds__(DET_THREADS) void det_count_kernel(int E, int nt, const int32_t *__restrict__ idx,
                                                                int *__restrict__ cnt) {
    const int bs = blockIdx.y, e = blockIdx.x * DET_THREADS + threadIdx.x;
    if (e >= E) return;
    const int t = idx[(size_t)bs * E + e];
    if ((unsigned)t < (unsigned)nt) atomicAdd(cnt + (size_t)bs * nt + t, 1);    // (out-of-range indices contribute nothing)
}

__global__ __launch_bounds__(PDGN_WAVE) void det_scan_fill_kernel(int E, int nt, const int32_t *__restrict__ idx,
                                                                  int *__restrict__ cnt, int *__restrict__ rowptr,
                                                                  int *__restrict__ edges) {
    const int bs = blockIdx.x, lane = threadIdx.x;
    int *C = cnt + (size_t)bs * nt, *R = rowptr + (size_t)bs * (nt + 1), *Ed = edges + (size_t)bs * E;
    const int32_t *I = idx + (size_t)bs * E;
    int base = 0;
    for (int i0 = 0; i0 < nt; i0 += PDGN_WAVE) {
        const int i = i0 + lane, v = i < nt ? C[i] : 0;
        int x = v;
        for (int d = 1; d < PDGN_WAVE; d <<= 1) {
            const int y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (i < nt) R[i] = C[i] = base + x - v;                  // row start; C becomes the row's cursor
        base += __shfl(x, PDGN_WAVE - 1);
    }
    if (lane == 0) R[nt] = base;
    __threadfence();                                            // the cursors are in place before the atomics below read them
    __syncthreads();
    for (int e0 = 0; e0 < E; e0 += PDGN_WAVE) {
        const int e = e0 + lane;
        int t = e < E ? I[e] : -1;
        if ((unsigned)t >= (unsigned)nt) t = -1;
        int rank = 0, same = 0, leader = lane;
        for (int l = PDGN_WAVE - 1; l >= 0; --l) {
            const int tl = __shfl(t, l);
            if (tl == t) {
                ++same;
                if (l < lane) { ++rank; leader = l; }
            }
        }
        int b0 = 0;
        if (t >= 0 && rank == 0) b0 = atomicAdd(C + t, same);   // the lowest lane of each target moves the cursor
        b0 = __shfl(b0, leader);
        if (t >= 0) Ed[b0 + rank] = e;
    }
}

// out[bs, ch, i] (+)= sum over row i's edges e, in increasing e, of G[bs, ch, e / DIV] (* W[bs, e]).
template <int DIV, bool WEIGHTED>
__global__ __launch_bounds__(DET_THREADS) void det_gather_kernel(int c, int nt, int E, int gs, const int *__restrict__ rowptr,
                                                                 const int *__restrict__ edges, const float *__restrict__ G,
                                                                 const float *__restrict__ W, float *__restrict__ out) {
    const int bs = blockIdx.z, i = blockIdx.x * DET_THREADS + threadIdx.x;
    if (i >= nt) return;
    const int *R = rowptr + (size_t)bs * (nt + 1), *Ed = edges + (size_t)bs * E;
    const int p0 = R[i], p1 = R[i + 1];
    for (int ch = blockIdx.y; ch < c; ch += gridDim.y) {
        const float *g = G + ((size_t)bs * c + ch) * gs;
        float *o = out + ((size_t)bs * c + ch) * nt + i;
        float acc = *o;
        for (int p = p0; p < p1; ++p) {
            const int e = Ed[p];
            float v = g[e / DIV];
            if (WEIGHTED) v = __fmul_rn(v, W[(size_t)bs * E + e]);
            acc = __fadd_rn(acc, v);
        }
        *o = acc;
    }
}

// nndistance.cu:129-148 in a fixed order: grad of point j of one cloud = its own term g*(a_j - b_idx[j]), then minus the
// terms of the other cloud's points whose nearest neighbour is j, in their index order.  z = 0: cloud 1, z = 1: cloud 2.
__global__ __launch_bounds__(DET_THREADS) void det_nndist_grad_kernel(
    int n, int m, const float *__restrict__ xyz1, const float *__restrict__ xyz2, const float *__restrict__ gd1,
    const int32_t *__restrict__ idx1, const float *__restrict__ gd2, const int32_t *__restrict__ idx2,
    const int *__restrict__ rowptr1, const int *__restrict__ edges1, const int *__restrict__ rowptr2,
    const int *__restrict__ edges2, float *__restrict__ g1, float *__restrict__ g2) {
    const int bs = blockIdx.y;
    const bool rev = blockIdx.z != 0;
    const int na = rev ? m : n, nb = rev ? n : m;
    const int j = blockIdx.x * DET_THREADS + threadIdx.x;
    if (j >= na) return;
    const float *A = (rev ? xyz2 : xyz1) + (size_t)bs * na * 3;
    const float *B = (rev ? xyz1 : xyz2) + (size_t)bs * nb * 3;
    const float *gda = (rev ? gd2 : gd1) + (size_t)bs * na, *gdb = (rev ? gd1 : gd2) + (size_t)bs * nb;
    const int32_t *id = (rev ? idx2 : idx1) + (size_t)bs * na;
    const int *R = (rev ? rowptr2 : rowptr1) + (size_t)bs * (na + 1), *Ed = (rev ? edges2 : edges1) + (size_t)bs * nb;
    float *ga = (rev ? g2 : g1) + (size_t)bs * na * 3;
    const int j2 = id[j];
    const float g = gda[j] * 2;
    const int p0 = R[j], p1 = R[j + 1];
    for (int c = 0; c < 3; ++c) {
        float acc = 0.f;
        acc = __fadd_rn(acc, g * (A[j * 3 + c] - B[j2 * 3 + c]));
        for (int p = p0; p < p1; ++p) {
            const int i = Ed[p];
            acc = __fadd_rn(acc, -((gdb[i] * 2) * (B[i * 3 + c] - A[j * 3 + c])));
        }
        ga[j * 3 + c] = acc;
    }
}

long long det_ints(long long b, long long nt, long long E) { return b * (2 * nt + 1 + E); }

// CSR transpose of idx (b, E) over nt targets in ws: [cnt b*nt][rowptr b*(nt+1)][edges b*E].
int det_transpose(int b, int nt, long long E, const int32_t *idx, int *ws, int **rowptr, int **edges, hipStream_t s) {
    int *cnt = ws;
    *rowptr = ws + (size_t)b * nt;
    *edges = *rowptr + (size_t)b * (nt + 1);
    hipError_t err = hipMemsetAsync(cnt, 0, (size_t)b * nt * sizeof(int), s);
    if (err != hipSuccess) return (int)err;
    if (E > 0) hipLaunchKernelGGL(det_count_kernel, dim3(cdiv(E, DET_THREADS), b), dim3(DET_THREADS), 0, s, (int)E, nt, idx, cnt);
    hipLaunchKernelGGL(det_scan_fill_kernel, dim3(b), dim3(PDGN_WAVE), 0, s, (int)E, nt, idx, cnt, *rowptr, *edges);
    return pdgn_launch_status();
}

static bool det_dims_ok(int b, int c, long long nt, long long E) {
    return b >= 0 && b <= 65535 && c >= 0 && nt >= 0 && E >= 0 && nt < 0x7fffffffLL && E < 0x7fffffffLL &&
           det_ints(b, nt, E) < 0x7fffffffLL;
}

template <int DIV, bool WEIGHTED>
static int det_scatter(int b, int c, int nt, long long E, int gs, const float *grad_out, const int32_t *idx, const float *w,
                       int32_t *ws, float *out, hipStream_t s) {
    int *rowptr, *edges;
    const int rc = det_transpose(b, nt, E, idx, ws, &rowptr, &edges, s);
    if (rc) return rc;
    hipLaunchKernelGGL((det_gather_kernel<DIV, WEIGHTED>), dim3(cdiv(nt, DET_THREADS), c < 65535 ? c : 65535, b),
                       dim3(DET_THREADS), 0, s, c, nt, (int)E, gs, rowptr, edges, grad_out, w, out);
    return pdgn_launch_status();
}

extern "C" long long pdgn_det_workspace_ints(int b, int targets, long long edges) {
    return det_ints(b, targets, edges);
}

extern "C" int pdgn_grouping_backward_det(int b, int c, int n, int m, int nsample, const float *grad_out, const int32_t *idx,
                                          int32_t *ws, float *grad_points, pdgn_stream_t stream) {
    const long long ms = (long long)m * nsample;
    if (m < 0 || nsample < 0 || !det_dims_ok(b, c, n, ms)) return PDGN_ERR_INVALID;
    if (b == 0 || c == 0 || n == 0 || ms == 0) return 0;
    return det_scatter<1, false>(b, c, n, ms, (int)ms, grad_out, idx, nullptr, ws, grad_points, (hipStream_t)stream);
}

extern "C" int pdgn_interpolation_backward_det(int b, int c, int n, int m, const float *grad_out, const int32_t *idx,
                                               const float *weight, int32_t *ws, float *grad_points, pdgn_stream_t stream) {
    if (n < 0 || !det_dims_ok(b, c, m, 3LL * n)) return PDGN_ERR_INVALID;
    if (b == 0 || c == 0 || n == 0 || m == 0) return 0;
    return det_scatter<3, true>(b, c, m, 3LL * n, n, grad_out, idx, weight, ws, grad_points, (hipStream_t)stream);
}

extern "C" int pdgn_gathering_backward_det(int b, int c, int n, int m, const float *grad_out, const int32_t *idx, int32_t *ws,
                                           float *grad_points, pdgn_stream_t stream) {
    if (b < 0 || c < 1 || n < 1 || m < 1 || c > 65535 || !det_dims_ok(b, c, n, m)) return PDGN_ERR_INVALID;
    if (b == 0) return 0;
    return det_scatter<1, false>(b, c, n, m, m, grad_out, idx, nullptr, ws, grad_points, (hipStream_t)stream);
}

extern "C" int pdgn_nndistance_grad_det(int b, int n, const float *xyz1, int m, const float *xyz2, const float *grad_dist1,
                                        const int32_t *idx1, const float *grad_dist2, const int32_t *idx2, int32_t *ws,
                                        float *grad_xyz1, float *grad_xyz2, pdgn_stream_t stream) {
    if (!det_dims_ok(b, 0, n, m) || !det_dims_ok(b, 0, m, n) || det_ints(b, n, m) + det_ints(b, m, n) >= 0x7fffffffLL)
        return PDGN_ERR_INVALID;
    if (b == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    if (n == 0 || m == 0) {                                     // (no pairs: zero gradients, as pdgn_nndistance_grad)
        if (n && (e = hipMemsetAsync(grad_xyz1, 0, (size_t)b * n * 3 * sizeof(float), s)) != hipSuccess) return (int)e;
        if (m && (e = hipMemsetAsync(grad_xyz2, 0, (size_t)b * m * 3 * sizeof(float), s)) != hipSuccess) return (int)e;
        return 0;
    }
    int *r1, *e1, *r2, *e2;
    int rc = det_transpose(b, n, m, idx2, ws, &r1, &e1, s);    // cloud 1's rows: the cloud-2 points whose nearest is there
    if (rc) return rc;
    rc = det_transpose(b, m, n, idx1, ws + det_ints(b, n, m), &r2, &e2, s);
    if (rc) return rc;
    hipLaunchKernelGGL(det_nndist_grad_kernel, dim3(cdiv(n > m ? n : m, DET_THREADS), b, 2), dim3(DET_THREADS), 0, s, n, m, xyz1,
                       xyz2, grad_dist1, idx1, grad_dist2, idx2, r1, e1, r2, e2, grad_xyz1, grad_xyz2);
    return pdgn_launch_status();
}
