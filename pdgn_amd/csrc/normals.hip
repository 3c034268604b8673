// normals.hip -- per-point surface normals and neighbourhood eigenvalues from the covariance of each point's k nearest neighbours
// (include/pdgn_hip.h: pdgn_estimate_normals).  The neighbour lists are the caller's (pdgn_knnquery).  One launch,
// no BLAS, no atomics, nothing allocated.
//
// NORMATIVE OPERATION ORDER (tests/normals_mirror.py restates it in numpy; every operation below is one fp32 rounding: __fadd_rn /
// __fsub_rn / __fmul_rn / __fdiv_rn and sqrtf -- the correctly rounded root, never __fsqrt_rn, see csrc/auction.hip -- nothing
// contracted; steps 1 to 4 are the statements of csrc/pca3.h, which flatness.hip runs too).  One cloud x of n points; for point i with neighbours j_s = idx[i][s], s = 0 .. k-1 ascending:
//
//   1  mean         inv = 1 / (float)k;   m = 0;  m = m + x_(j_s)  for every s;   mu = m * inv                  (each component on its own)
//   2  covariance   cxx = cxy = cxz = cyy = cyz = czz = 0;  for every s:  d = x_(j_s) - mu,  cxx = cxx + dx*dx,  cxy = cxy + dx*dy,
//                   cxz = cxz + dx*dz,  cyy = cyy + dy*dy,  cyz = cyz + dy*dz,  czz = czz + dz*dz;   then a = c * inv for each of the six.
//                   (the neighbours are gathered a second time: 2 k gathers per point, not 3 k registers)
//   3  Jacobi       V = identity; PDGN_NORMALS_SWEEPS times over the pairs (p, q) = (0,1), (0,2), (1,2), r the remaining index:
//                       if a_pq == 0: nothing
//                       theta = (a_qq - a_pp) / (2 * a_pq)
//                       t = 1 / (|theta| + sqrtf(theta*theta + 1));   t = -t where theta < 0
//                       c = 1 / sqrtf(t*t + 1);   s = t * c
//                       a_pp = a_pp - t*a_pq;   a_qq = a_qq + t*a_pq;   a_pq = 0          (t*a_pq is rounded once and used twice)
//                       a_rp' = c*a_rp - s*a_rq;   a_rq' = s*a_rp + c*a_rq
//                       v_kp' = c*v_kp - s*v_kq;   v_kq' = s*v_kp + c*v_kq   for the rows k = 0, 1, 2 of V
//                   The trip count is fixed, there is no convergence test: a NaN cannot hang the kernel (NaN == 0 is false: it rotates).
//   4  selection    the diagonal (a_00, a_11, a_22) with its column numbers through three compare-and-swaps on `<`, positions (0,1), (1,2),
//                   (0,1): ascending, equal values keep the lower column first.  eig = the sorted diagonal as computed (a tiny negative value
//                   is not clamped); normal = the column of V that belongs to the smallest, as it stands (not renormalised).
//   5  sign         orient 0: m = 0;  m = 1 where |n_1| > |n_0|;  m = 2 where |n_2| > |n_m|;  the normal is negated where n_m < 0
//                   orient 1: negated where dot(n, o) < 0;   2: where dot(n, o - x_i) < 0;   3: where dot(n, x_i - o) < 0
//                   dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z
//   6  poison       an index outside [0, n) is never dereferenced (the thread reads point 0 in its place) and makes all six outputs of the
//                   point NaN; so does an eigenvalue that is not finite.  No other point is affected.
//
// SHAPE.  One thread per point.  Its 2 k gathers of 12 bytes go to L2 in the small launches and to LDS in the large ones: where the
// workgroups have 256 threads and the cloud is at most PDGN_NORMALS_STAGE_MAX_N points (48 KB), each workgroup first copies its cloud
// into LDS with coalesced loads.  Measured at 35 clouds, k = 16 (kernel trace, median of 30 launches), L2 / LDS:
// 256 points 7.7 / 8.5 us, 512: 7.5 / 8.4, 1024: 10.1 / 9.7, 2048: 12.5 / 10.6, 4096: 23.5 / 15.0 -- the workgroups of 64 and 128 threads
// of the small launches would each copy a whole cloud for few points of their own, and lose.  The order over the slots is each thread's
// own, so block size, grid size and where the gathers go change no bit.  Block size: the largest of 256 / 128 / 64 that still gives the
// chip a workgroup per CU (35 x 256 points: 140 one-wave workgroups, not 35 of four waves).  50 VGPRs, nothing spilled, no scratch.
#include "pca3.h"

template <int BLOCK, bool STAGE>
__global__ __launch_bounds__(BLOCK) void normals_kernel(int n, int k, int per, const float *__restrict__ xyz,
                                                        const int32_t *__restrict__ idx, int orient, float ox, float oy, float oz,
                                                        float *__restrict__ normals, float *__restrict__ eig) {
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
    // 1 to 4: mean, covariance, Jacobi, selection (pca3.h)
    const Pca3 e = pca3(n, k, idx + at * k, __fdiv_rn(1.0f, (float)k), at3);
    const bool outside = e.outside;
    float nx = e.nx, ny = e.ny, nz = e.nz, l0 = e.l0, l1 = e.l1, l2 = e.l2;
    // 5: sign
    bool flip;
    if (orient == 0) {
        float lead = nx;
        if (fabsf(ny) > fabsf(lead)) lead = ny;
        if (fabsf(nz) > fabsf(lead)) lead = nz;
        flip = lead < 0.f;
    } else {
        const float xi = at3(3 * i), yi = at3(3 * i + 1), zi = at3(3 * i + 2);
        const float wx = orient == 1 ? ox : orient == 2 ? __fsub_rn(ox, xi) : __fsub_rn(xi, ox);
        const float wy = orient == 1 ? oy : orient == 2 ? __fsub_rn(oy, yi) : __fsub_rn(yi, oy);
        const float wz = orient == 1 ? oz : orient == 2 ? __fsub_rn(oz, zi) : __fsub_rn(zi, oz);
        flip = dot3_rn(nx, ny, nz, wx, wy, wz) < 0.f;
    }
    if (flip) nx = -nx, ny = -ny, nz = -nz;
    // 6: poison
    if (outside || !(isfinite(l0) && isfinite(l1) && isfinite(l2))) nx = ny = nz = l0 = l1 = l2 = __builtin_nanf("");
    normals[3 * at] = nx, normals[3 * at + 1] = ny, normals[3 * at + 2] = nz;
    if (eig) eig[3 * at] = l0, eig[3 * at + 1] = l1, eig[3 * at + 2] = l2;
}


extern "C" int pdgn_estimate_normals(int b, int n, int k, const float *xyz, const int32_t *idx, int orient, float ox, float oy, float oz,
                                     float *normals, float *eig, pdgn_stream_t stream) {
    if (b < 1 || n < 1 || k < 1 || k > PDGN_NORMALS_MAX_K || (long long)b * n > (1LL << 28)) return PDGN_ERR_INVALID;
    if (orient < 0 || orient > 3 || (orient != 0 && !(isfinite(ox) && isfinite(oy) && isfinite(oz)))) return PDGN_ERR_INVALID;
    if (!xyz || !idx || !normals) return PDGN_ERR_INVALID;
    if (!pdgn_aligned(xyz, 4) || !pdgn_aligned(idx, 4) || !pdgn_aligned(normals, 4) || !pdgn_aligned(eig, 4)) return PDGN_ERR_INVALID;
    // the largest workgroup that still leaves one per CU (256 of them); 64 where even that does not
    const int block = (long long)b * cdiv(n, 256) >= 256 ? 256 : (long long)b * cdiv(n, 128) >= 256 ? 128 : 64;
    // one launch whatever b is: grid.x carries (cloud, workgroup of the cloud), at most 2^28 of them (grid.y would end at 65535 clouds)
    const int per = cdiv(n, block);
    const dim3 grid((unsigned)((long long)b * per));
    // the cloud through LDS where the workgroups are the large ones and it fits (the header block: SHAPE)
    const bool stage = block == 256 && n <= PDGN_NORMALS_STAGE_MAX_N;
    hipStream_t st = (hipStream_t)stream;
    if (stage)
        hipLaunchKernelGGL((normals_kernel<256, true>), grid, dim3(256), 12u * n, st, n, k, per, xyz, idx, orient, ox, oy, oz, normals, eig);
    else if (block == 256)
        hipLaunchKernelGGL((normals_kernel<256, false>), grid, dim3(256), 0, st, n, k, per, xyz, idx, orient, ox, oy, oz, normals, eig);
    else if (block == 128)
        hipLaunchKernelGGL((normals_kernel<128, false>), grid, dim3(128), 0, st, n, k, per, xyz, idx, orient, ox, oy, oz, normals, eig);
    else
        hipLaunchKernelGGL((normals_kernel<64, false>), grid, dim3(64), 0, st, n, k, per, xyz, idx, orient, ox, oy, oz, normals, eig);
    return pdgn_launch_status();
}
