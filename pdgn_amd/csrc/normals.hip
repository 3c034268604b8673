// normals.hip -- per-point surface normals and neighbourhood eigenvalues from the covariance of each point's k nearest neighbours
// (include/pdgn_hip.h: pdgn_estimate_normals).  The neighbour lists are the caller's (pdgn_knnquery).  One launch,
// no BLAS, no atomics, nothing allocated.
//
// NORMATIVE OPERATION ORDER (tests/normals_mirror.py restates it in numpy; every operation below is one fp32 rounding: __fadd_rn /
// __fsub_rn / __fmul_rn / __fdiv_rn and sqrtf -- the correctly rounded root, never __fsqrt_rn, see csrc/auction.hip -- nothing
// contracted).  One cloud x of n points; for point i with neighbours j_s = idx[i][s], s = 0 .. k-1 ascending:
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
#include "common.h"

#include <math.h>

// One Jacobi rotation of the header block on the pair (p, q): r is the remaining index, (v0p, v0q) .. (v2p, v2q) the two columns of V.
__device__ __forceinline__ void nrm_rotate(float &app, float &aqq, float &apq, float &arp, float &arq, float &v0p, float &v0q,
                                           float &v1p, float &v1q, float &v2p, float &v2q) {
    if (apq == 0.f) return;
    const float theta = __fdiv_rn(__fsub_rn(aqq, app), __fmul_rn(2.0f, apq));
    float t = __fdiv_rn(1.0f, __fadd_rn(fabsf(theta), sqrtf(__fadd_rn(__fmul_rn(theta, theta), 1.0f))));
    t = theta < 0.f ? -t : t;
    const float c = __fdiv_rn(1.0f, sqrtf(__fadd_rn(__fmul_rn(t, t), 1.0f)));
    const float s = __fmul_rn(t, c);
    const float tap = __fmul_rn(t, apq);
    app = __fsub_rn(app, tap);
    aqq = __fadd_rn(aqq, tap);
    apq = 0.f;
    const float rp = arp, rq = arq;
    arp = __fsub_rn(__fmul_rn(c, rp), __fmul_rn(s, rq));
    arq = __fadd_rn(__fmul_rn(s, rp), __fmul_rn(c, rq));
    const float a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
    v0p = __fsub_rn(__fmul_rn(c, a0), __fmul_rn(s, b0)), v0q = __fadd_rn(__fmul_rn(s, a0), __fmul_rn(c, b0));
    v1p = __fsub_rn(__fmul_rn(c, a1), __fmul_rn(s, b1)), v1q = __fadd_rn(__fmul_rn(s, a1), __fmul_rn(c, b1));
    v2p = __fsub_rn(__fmul_rn(c, a2), __fmul_rn(s, b2)), v2q = __fadd_rn(__fmul_rn(s, a2), __fmul_rn(c, b2));
}

// compare-and-swap of the selection: (la, ca) <-> (lb, cb) where lb < la
__device__ __forceinline__ void nrm_cas(float &la, int &ca, float &lb, int &cb) {
    const bool sw = lb < la;
    const float l = la;
    const int c = ca;
    la = sw ? lb : la, ca = sw ? cb : ca;
    lb = sw ? l : lb, cb = sw ? c : cb;
}

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
    const int32_t *mine = idx + at * k;
    const float inv = __fdiv_rn(1.0f, (float)k);
    // 1: the mean (and whether every index is inside the cloud)
    bool outside = false;
    float mx = 0.f, my = 0.f, mz = 0.f;
#pragma unroll 4
    for (int s = 0; s < k; ++s) {
        int j = mine[s];
        const bool ok = (unsigned)j < (unsigned)n;
        outside |= !ok;
        j = ok ? j : 0;
        mx = __fadd_rn(mx, at3(3 * j)), my = __fadd_rn(my, at3(3 * j + 1)), mz = __fadd_rn(mz, at3(3 * j + 2));
    }
    mx = __fmul_rn(mx, inv), my = __fmul_rn(my, inv), mz = __fmul_rn(mz, inv);
    // 2: the covariance
    float a00 = 0.f, a01 = 0.f, a02 = 0.f, a11 = 0.f, a12 = 0.f, a22 = 0.f;
#pragma unroll 4
    for (int s = 0; s < k; ++s) {
        int j = mine[s];
        j = (unsigned)j < (unsigned)n ? j : 0;
        const float dx = __fsub_rn(at3(3 * j), mx), dy = __fsub_rn(at3(3 * j + 1), my), dz = __fsub_rn(at3(3 * j + 2), mz);
        a00 = __fadd_rn(a00, __fmul_rn(dx, dx)), a01 = __fadd_rn(a01, __fmul_rn(dx, dy)), a02 = __fadd_rn(a02, __fmul_rn(dx, dz));
        a11 = __fadd_rn(a11, __fmul_rn(dy, dy)), a12 = __fadd_rn(a12, __fmul_rn(dy, dz)), a22 = __fadd_rn(a22, __fmul_rn(dz, dz));
    }
    a00 = __fmul_rn(a00, inv), a01 = __fmul_rn(a01, inv), a02 = __fmul_rn(a02, inv);
    a11 = __fmul_rn(a11, inv), a12 = __fmul_rn(a12, inv), a22 = __fmul_rn(a22, inv);
    // 3: cyclic Jacobi, V[row][column] = v<row><column>
    float v00 = 1.f, v01 = 0.f, v02 = 0.f, v10 = 0.f, v11 = 1.f, v12 = 0.f, v20 = 0.f, v21 = 0.f, v22 = 1.f;
#pragma unroll 1
    for (int sweep = 0; sweep < PDGN_NORMALS_SWEEPS; ++sweep) {
        nrm_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);         // (0,1), r = 2
        nrm_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);         // (0,2), r = 1
        nrm_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);         // (1,2), r = 0
    }
    // 4: selection
    float l0 = a00, l1 = a11, l2 = a22;
    int c0 = 0, c1 = 1, c2 = 2;
    nrm_cas(l0, c0, l1, c1);
    nrm_cas(l1, c1, l2, c2);
    nrm_cas(l0, c0, l1, c1);
    float nx = c0 == 0 ? v00 : c0 == 1 ? v01 : v02;
    float ny = c0 == 0 ? v10 : c0 == 1 ? v11 : v12;
    float nz = c0 == 0 ? v20 : c0 == 1 ? v21 : v22;
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
