// flatness.hip -- the flatness regulariser of the generator's loss: the batch mean of Pauly's surface variation sigma = l0 / (l0 + l1 + l2)
// of every point's k-neighbourhood, and its gradient with respect to the points (include/pdgn_hip.h: pdgn_flatness).
// The neighbour lists are the caller's and are DATA: the neighbour choice is not differentiated.  No BLAS, no float atomics.
//
// NORMATIVE DEFINITION (tests/flatness_mirror.py restates it in numpy; every operation below is one fp32 rounding: __fadd_rn / __fsub_rn /
// __fmul_rn / __fdiv_rn and sqrtf, nothing contracted; dot3 is common.h's dot3_rn).  One cloud x of n points, lists idx (n, k),
// inv = 1 / (float)k, eps >= 0, coef.
//
//   per point i   steps 1 to 4 of normals.hip exactly (pca3.h: the same statements): mean mu, covariance, PDGN_NORMALS_SWEEPS Jacobi
//                 sweeps, selection -- l0 <= l1 <= l2 and v, the column of the smallest, are the bits pdgn_estimate_normals writes, up to the
//                 sign of v, which does not matter here.   tr = (l0 + l1) + l2,   q = tr + eps.
//       bad         an index outside [0, n) (never dereferenced, as in normals) or an eigenvalue that is not finite:
//                   sigma_i = NaN, all six h NaN -- the cloud's per_cloud, the loss and the gradient of every target on the list are NaN
//       degenerate  not bad, and !(l0 > 0) or !(q > 0):  sigma_i = 0, h = 0, counted in degenerate[cloud]
//                   (coincident points and an exactly flat neighbourhood land here)
//       live        sigma_i = l0 / q,   w = (2 * inv) / q,
//                   h_ab = w * (v_a * v_b - sigma_i) for a == b,   h_ab = w * (v_a * v_b) for a != b        (the symmetric H_i, six entries)
//       record      (mu as step 1 rounds it, h00, h01, h02, h11, h12, h22): 48 bytes
//   gradient      with sum_s (x_(j_s) - mu) = 0 the mean's own derivative cancels:  d sigma_i / d x_j = sum over {s: idx[i][s] = j} of
//                 H_i (x_j - mu_i), repeated entries included.  For target j, over its in-edges e = i * k + s in ASCENDING e, from acc = 0:
//                     d = x_j - mu_i
//                     acc.x = acc.x + dot3(h00, h01, h02, d);   acc.y = acc.y + dot3(h01, h11, h12, d);   acc.z = acc.z + dot3(h02, h12, h22, d)
//                 then grad_j = coef * acc  (each component).
//   loss          repulsion.hip's reduction of its s array applied to sigma: one wave per cloud, the xor tree, fp64 across clouds;
//                 per_cloud[c] = (float)(P_c / n),  loss = (float)(T / (b n)).  Degenerate points count as zeros in the mean.
//
// SHAPE.  flat_point_kernel: one thread per point with the geometry and the LDS staging rule of normals_kernel (256 / 128 / 64 threads, the
// cloud through LDS at 256 threads and n <= PDGN_NORMALS_STAGE_MAX_N); the order over the slots is each thread's own, so the launch geometry
// changes no bit.  The degenerate points are counted per wave with a ballot and one integer atomic.  The scatter over the kNN edges is a
// gather over a CSR transpose of idx whose rows list their edges in INCREASING edge id -- the row order is the property, not the mechanism:
//   n <= FLAT_TR_MAX_N   flat_transpose_kernel, one workgroup of 16 waves per cloud, counts and cursors in LDS: count (LDS integer atomics),
//                        a workgroup-wide exclusive scan, then the stable fill of det.hip's one-wave kernel with the waves side by side --
//                        1024 edges a turn, wave w the 64 edges w * 64 .. of the turn; every lane's rank among the lanes of the same target
//                        by shuffles, all waves at once; then the waves move the cursors one after the other, in edge order.  det.hip's fill
//                        spends two global round trips per 64 edges (1170 us at 35 x 2048 x 16; profiles/flatness_cost.txt)
//   larger clouds        det.hip's transpose (memset, count, one-wave scan and fill), 65535 clouds at a time
// flat_gather_kernel: one thread per target, FG_ROWS records' loads (three 16-byte loads each, wave-divergent) issued before the first is
// used, the additions in row order.
#include "pca3.h"

#define FG_THREADS 256
#define FG_ROWS 4
#define FLAT_REC 12                                                // floats per record: mu (3), h (6), 3 unused
#define FT_THREADS 1024
#define FT_WAVES (FT_THREADS / PDGN_WAVE)
#define FLAT_TR_MAX_N 4096                                         // targets whose cursors one workgroup keeps in LDS (16 KB)
#define FT_PER (FLAT_TR_MAX_N / FT_THREADS)                        // consecutive targets a thread owns in the scan

template <int BLOCK, bool STAGE>
__global__ __launch_bounds__(BLOCK) void flat_point_kernel(int n, int k, int per, const float *__restrict__ xyz,
                                                           const int32_t *__restrict__ idx, float eps, float *__restrict__ sigma,
                                                           int *__restrict__ degenerate, float4 *__restrict__ rec) {
    const int cl = blockIdx.x / per;                               // `per` workgroups per cloud
    const int i = (blockIdx.x - cl * per) * BLOCK + threadIdx.x;
    const float *cloud = xyz + (size_t)cl * n * 3;
    extern __shared__ float staged[];
    if constexpr (STAGE) {
        for (int e = threadIdx.x; e < 3 * n; e += BLOCK) staged[e] = cloud[e];
        __syncthreads();
    }
    if (i >= n) return;
    auto at3 = [&](int e) -> float {
        if constexpr (STAGE) return staged[e];
        else return cloud[e];
    };
    const size_t at = (size_t)cl * n + i;
    const float inv = __fdiv_rn(1.0f, (float)k);
    const Pca3 e = pca3(n, k, idx + at * k, inv, at3);
    const float q = __fadd_rn(__fadd_rn(__fadd_rn(e.l0, e.l1), e.l2), eps);
    const bool bad = e.outside || !(isfinite(e.l0) && isfinite(e.l1) && isfinite(e.l2));
    const bool deg = !bad && (!(e.l0 > 0.f) || !(q > 0.f));
    float sg = 0.f, h00 = 0.f, h01 = 0.f, h02 = 0.f, h11 = 0.f, h12 = 0.f, h22 = 0.f;
    if (bad) {
        sg = h00 = h01 = h02 = h11 = h12 = h22 = __builtin_nanf("");
    } else if (!deg) {
        sg = __fdiv_rn(e.l0, q);
        const float w = __fdiv_rn(__fmul_rn(2.0f, inv), q);
        h00 = __fmul_rn(w, __fsub_rn(__fmul_rn(e.nx, e.nx), sg));
        h01 = __fmul_rn(w, __fmul_rn(e.nx, e.ny));
        h02 = __fmul_rn(w, __fmul_rn(e.nx, e.nz));
        h11 = __fmul_rn(w, __fsub_rn(__fmul_rn(e.ny, e.ny), sg));
        h12 = __fmul_rn(w, __fmul_rn(e.ny, e.nz));
        h22 = __fmul_rn(w, __fsub_rn(__fmul_rn(e.nz, e.nz), sg));
    }
    sigma[at] = sg;
    if (degenerate) {                                              // a wave's points are one cloud's: one integer atomic per wave
        const unsigned long long m = __ballot(deg);
        if (deg && lane_id() == __ffsll(m) - 1) atomicAdd(degenerate + cl, __popcll(m));
    }
    if (rec) {
        float4 *r = rec + at * 3;
        r[0] = make_float4(e.mx, e.my, e.mz, h00);
        r[1] = make_float4(h01, h02, h11, h12);
        r[2] = make_float4(h22, 0.f, 0.f, 0.f);
    }
}

// The CSR transpose of one cloud's idx (E = n k edges) over nt <= FLAT_TR_MAX_N targets by one workgroup: rowptr (nt + 1), edges (E), every
// row in increasing edge id; an index outside [0, nt) is in no row.
__global__ __launch_bounds__(FT_THREADS) void flat_transpose_kernel(int E, int nt, const int32_t *__restrict__ idx, int *__restrict__ rowptr,
                                                                    int *__restrict__ edges) {
    __shared__ int cur[FLAT_TR_MAX_N];                             // counts, then the rows' cursors
    __shared__ int wsum[FT_WAVES];
    const int tid = threadIdx.x, lane = lane_id(), wave = tid / PDGN_WAVE;
    const int32_t *I = idx + (size_t)blockIdx.x * E;
    int *R = rowptr + (size_t)blockIdx.x * (nt + 1), *Ed = edges + (size_t)blockIdx.x * E;
    for (int t = tid; t < nt; t += FT_THREADS) cur[t] = 0;
    __syncthreads();
    for (int e = tid; e < E; e += FT_THREADS) {
        const int t = I[e];
        if ((unsigned)t < (unsigned)nt) atomicAdd(&cur[t], 1);     // (LDS, integer: the counts do not depend on the order)
    }
    __syncthreads();
    // exclusive scan: a thread's FT_PER targets, the threads of a wave by shuffles, the waves through wsum
    int c[FT_PER], sum = 0;
#pragma unroll
    for (int u = 0; u < FT_PER; ++u) {
        const int t = tid * FT_PER + u;
        c[u] = t < nt ? cur[t] : 0;
        sum += c[u];
    }
    int x = sum;
    for (int d = 1; d < PDGN_WAVE; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == PDGN_WAVE - 1) wsum[wave] = x;
    __syncthreads();
    int run = x - sum;
    for (int w = 0; w < wave; ++w) run += wsum[w];
#pragma unroll
    for (int u = 0; u < FT_PER; ++u) {
        const int t = tid * FT_PER + u;
        if (t < nt) cur[t] = R[t] = run;
        run += c[u];
    }
    if (tid == FT_THREADS - 1) R[nt] = run;
    __syncthreads();
    // the stable fill: FT_THREADS edges a turn
    for (int e0 = 0; e0 < E; e0 += FT_THREADS) {
        const int e = e0 + tid;
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
        for (int w = 0; w < FT_WAVES; ++w) {                       // the waves one after the other: the lowest lane of each target moves the cursor
            if (w == wave && t >= 0 && rank == 0) b0 = atomicAdd(&cur[t], same);
            __syncthreads();
        }
        b0 = __shfl(b0, leader);
        if (t >= 0) Ed[b0 + rank] = e;
    }
}

// One thread per target j: its row of the transpose lists the in-edges e = i * k + s in increasing e.
__global__ __launch_bounds__(FG_THREADS) void flat_gather_kernel(int n, int k, int per, const float *__restrict__ xyz,
                                                                 const int *__restrict__ rowptr, const int *__restrict__ edges,
                                                                 const float4 *__restrict__ rec, float coef, float *__restrict__ grad) {
    const int cl = blockIdx.x / per;
    const int j = (blockIdx.x - cl * per) * FG_THREADS + threadIdx.x;
    if (j >= n) return;
    const size_t at = (size_t)cl * n + j;
    const int *R = rowptr + (size_t)cl * (n + 1), *Ed = edges + (size_t)cl * n * k;
    const float4 *rc = rec + (size_t)cl * n * 3;
    const float xj = xyz[3 * at], yj = xyz[3 * at + 1], zj = xyz[3 * at + 2];
    float ax = 0.f, ay = 0.f, az = 0.f;
    auto add = [&](const float4 &r0, const float4 &r1, const float4 &r2) {
        const float dx = __fsub_rn(xj, r0.x), dy = __fsub_rn(yj, r0.y), dz = __fsub_rn(zj, r0.z);
        ax = __fadd_rn(ax, dot3_rn(r0.w, r1.x, r1.y, dx, dy, dz));
        ay = __fadd_rn(ay, dot3_rn(r1.x, r1.z, r1.w, dx, dy, dz));
        az = __fadd_rn(az, dot3_rn(r1.y, r1.w, r2.x, dx, dy, dz));
    };
    int p = R[j];
    const int p1 = R[j + 1];
    for (; p + FG_ROWS <= p1; p += FG_ROWS) {
        float4 r[FG_ROWS][3];
#pragma unroll
        for (int u = 0; u < FG_ROWS; ++u) {
            const float4 *src = rc + (size_t)(Ed[p + u] / k) * 3;
            r[u][0] = src[0], r[u][1] = src[1], r[u][2] = src[2];
        }
#pragma unroll
        for (int u = 0; u < FG_ROWS; ++u) add(r[u][0], r[u][1], r[u][2]);
    }
    for (; p < p1; ++p) {
        const float4 *src = rc + (size_t)(Ed[p] / k) * 3;
        add(src[0], src[1], src[2]);
    }
    grad[3 * at] = __fmul_rn(coef, ax), grad[3 * at + 1] = __fmul_rn(coef, ay), grad[3 * at + 2] = __fmul_rn(coef, az);
}


static bool flat_dims_ok(int b, int n, int k) {
    return b >= 1 && n >= 1 && k >= 1 && k <= PDGN_NORMALS_MAX_K && (long long)b * n * k < (1LL << 31);
}

// ws = [records: b n 48 bytes][the transpose's integers, cloud chunk after cloud chunk]
extern "C" long long pdgn_flatness_workspace_bytes(int b, int n, int k, int with_grad) {
    if (!flat_dims_ok(b, n, k)) return PDGN_ERR_INVALID;
    if (!with_grad) return 0;
    return (long long)b * n * FLAT_REC * 4 + det_ints(b, n, (long long)n * k) * 4;
}

extern "C" int pdgn_flatness(int b, int n, int k, const float *xyz, const int32_t *idx, float eps, float coef, float *sigma, float *loss,
                             float *per_cloud, int32_t *degenerate, float *grad, void *ws, pdgn_stream_t stream) {
    if (!flat_dims_ok(b, n, k)) return PDGN_ERR_INVALID;
    if (!isfinite(eps) || eps < 0.f || !isfinite(coef)) return PDGN_ERR_INVALID;
    if (!xyz || !idx || !sigma || !loss || (grad && !ws)) return PDGN_ERR_INVALID;
    if (!pdgn_aligned(xyz, 4) || !pdgn_aligned(idx, 4) || !pdgn_aligned(sigma, 4) || !pdgn_aligned(loss, 4) || !pdgn_aligned(per_cloud, 4) ||
        !pdgn_aligned(degenerate, 4) || !pdgn_aligned(grad, 4) || (grad && !pdgn_aligned(ws, 16)))
        return PDGN_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    float4 *rec = grad ? (float4 *)ws : nullptr;
    if (degenerate) {
        const hipError_t err = hipMemsetAsync(degenerate, 0, (size_t)b * sizeof(int32_t), st);
        if (err != hipSuccess) return (int)err;
    }
    // normals.hip's geometry: the largest workgroup that still leaves one per CU (256 of them), 64 where even that does not; one launch
    // whatever b is; the cloud through LDS where the workgroups are the large ones and it fits
    const int block = (long long)b * cdiv(n, 256) >= 256 ? 256 : (long long)b * cdiv(n, 128) >= 256 ? 128 : 64;
    const int per = cdiv(n, block);
    const dim3 grid((unsigned)((long long)b * per));
    const bool stage = block == 256 && n <= PDGN_NORMALS_STAGE_MAX_N;
    if (stage)
        hipLaunchKernelGGL((flat_point_kernel<256, true>), grid, dim3(256), 12u * n, st, n, k, per, xyz, idx, eps, sigma, degenerate, rec);
    else if (block == 256)
        hipLaunchKernelGGL((flat_point_kernel<256, false>), grid, dim3(256), 0, st, n, k, per, xyz, idx, eps, sigma, degenerate, rec);
    else if (block == 128)
        hipLaunchKernelGGL((flat_point_kernel<128, false>), grid, dim3(128), 0, st, n, k, per, xyz, idx, eps, sigma, degenerate, rec);
    else
        hipLaunchKernelGGL((flat_point_kernel<64, false>), grid, dim3(64), 0, st, n, k, per, xyz, idx, eps, sigma, degenerate, rec);
    rp_reduce_launch(b, n, sigma, loss, per_cloud, st);
    if (!grad) return pdgn_launch_status();
    // the transpose of idx (b, n k) over n targets (the header block: SHAPE), then the gather; ws keeps det.hip's layout either way
    const long long E = (long long)n * k;
    int *ints = (int *)(rec + (size_t)b * n * 3);
    const int gper = cdiv(n, FG_THREADS);
    auto gather = [&](int c0, int cb, const int *rowptr, const int *edges) {
        hipLaunchKernelGGL(flat_gather_kernel, dim3((unsigned)((long long)cb * gper)), dim3(FG_THREADS), 0, st, n, k, gper,
                           xyz + (size_t)c0 * n * 3, rowptr, edges, rec + (size_t)c0 * n * 3, coef, grad + (size_t)c0 * n * 3);
    };
    if (n <= FLAT_TR_MAX_N) {
        int *rowptr = ints + (size_t)b * n, *edges = rowptr + (size_t)b * (n + 1);
        hipLaunchKernelGGL(flat_transpose_kernel, dim3(b), dim3(FT_THREADS), 0, st, (int)E, n, idx, rowptr, edges);
        gather(0, b, rowptr, edges);
        return pdgn_launch_status();
    }
    for (int c0 = 0; c0 < b; c0 += 65535) {                        // (det.hip's grid.y carries the cloud)
        const int cb = b - c0 < 65535 ? b - c0 : 65535;
        int *rowptr, *edges;
        const int rc = det_transpose(cb, n, E, idx + (size_t)c0 * E, ints + det_ints(c0, n, E), &rowptr, &edges, st);
        if (rc) return rc;
        gather(c0, cb, rowptr, edges);
    }
    return pdgn_launch_status();
}
