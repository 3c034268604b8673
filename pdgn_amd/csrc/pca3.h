// pca3.h -- steps 1 to 4 of the per-point neighbourhood eigen-decomposition whose operation order the header block of normals.hip states
// (mean, covariance, PDGN_NORMALS_SWEEPS cyclic Jacobi sweeps, selection): the statements normals.hip had, moved here so that
// flatness.hip runs the same ones and gets the same bits (DESIGN.md sections 7q and 7x).  Everything is inlined into its one caller per
// kernel; the resource remarks of normals_kernel are what they were.
#pragma once
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

// What steps 1 to 4 leave for one point: the mean as step 1 rounds it, the eigenvalues ascending, V's column of the smallest, and whether
// an index of the list lay outside [0, n).
struct Pca3 {
    float mx, my, mz;
    float l0, l1, l2;
    float nx, ny, nz;
    bool outside;
};

// Steps 1 to 4 for the list mine[0 .. k) of one point of a cloud of n points; at3(e) reads float e of the cloud (global memory or LDS).
template <class At3>
__device__ __forceinline__ Pca3 pca3(int n, int k, const int32_t *__restrict__ mine, float inv, At3 at3) {
    Pca3 r;
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
    r.nx = c0 == 0 ? v00 : c0 == 1 ? v01 : v02;
    r.ny = c0 == 0 ? v10 : c0 == 1 ? v11 : v12;
    r.nz = c0 == 0 ? v20 : c0 == 1 ? v21 : v22;
    r.mx = mx, r.my = my, r.mz = mz;
    r.l0 = l0, r.l1 = l1, r.l2 = l2;
    r.outside = outside;
    return r;
}
