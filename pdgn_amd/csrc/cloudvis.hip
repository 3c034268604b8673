// cloudvis.hip -- pdgn_cloud_normal_votes and pdgn_orient_pool: the sign of a cloud's normals from which side of every point a ring of
// orthographic views sees (include/pdgn_hip.h).  A point that a view sees with its normal turned towards the eye
// votes FRONT, one seen with its normal turned away votes BACK (Takayama et al. 2014, as csrc/visible.hip does for faces); whether a view
// sees a point is a depth test against a buffer into which every point was splatted as a small disc (hidden point removal, Katz et al.
// 2007, in its depth-buffer form).  The votes are then pooled over each point's neighbours in its tangent plane, and a negative total
// turns the normal round.  Unlike the propagation of csrc/orient.hip nothing is sequential and nothing crosses a thin sheet: the two
// sides of a slab are seen from opposite views, and a neighbour across the slab lies along the normal, where the pooling ignores it.
//
// NORMATIVE RULES (tests/cloudvis_mirror.py restates them in numpy; every fp32 operation below is one rounding, nothing contracted;
// dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z as in csrc/normals.hip).  One cloud: x (n,3), g (n,3); its frame (centre ctr, radius rho);
// view v has the rows e_x, e_y, e_z; the image is R x R pixels.
//
// THE VOTES (pdgn_cloud_normal_votes).
//   Live.   Point i is live iff x_i and g_i are six finite numbers.  A dead point splats nothing and gets no votes.
//   Snap.   csrc/visible.hip's, word for word.  For a point p:  d = p - ctr;  x = ((e_x0 d0 + e_x1 d1) + e_x2 d2), y and z likewise with e_y
//           and e_z; every fp32 subtraction, product and sum is rounded on its own.  With s = R 2^7 (exact in fp32):
//             X = (int) clamp(rint((x / rho) s), -s, s) + s         in [0, 2^8 R]: pixel units with 8 sub-pixel bits
//             Y likewise;   Z = (int) clamp(rint((z / rho) 2^20), -2^20, 2^20) + 2^20      in [0, 2^21]; a smaller Z is nearer the eye
//           (x / rho is the correctly rounded fp32 quotient, rint rounds halves to even, a NaN clamps to the lower end.)  After the snap
//           nothing is floating point but the vote's weight.
//   Pass 1. Every pixel starts at 0xffffffff.  A live point takes buf[p] = min(buf[p], Z) at
//             its OWN pixel (min(X >> 8, R - 1), min(Y >> 8, R - 1)), and at
//             every pixel (px, py), 0 <= px, py < R, whose centre C = ((2 px + 1) 2^7, (2 py + 1) 2^7) has
//             (C.x - X)^2 + (C.y - Y)^2 <= splat^2  in int64 (the disc of radius `splat` sub-pixel units, clipped to the image).
//   Pass 2. After one barrier.  A live point PASSES in this view iff Z <= buf[own pixel] + bias (its own pixel holds at most its own Z).
//   Vote.   For a point that passes: s = dot3(g, e_z) (the view looks along +e_z).  s < 0: the normal faces the eye, FRONT; s > 0: BACK;
//           s == 0 or NaN: no vote.  w = (uint32)(fminf(|s|, 1) * 256.f), truncated (a view that sees the point edge-on counts little).
//           votes[i][s > 0] += w.
// Everything the result depends on is an integer minimum or an integer sum: two runs agree bit for bit and a permutation of a cloud's
// points permutes its rows.  A count is at most NV 256 <= 2^13.
//
// THE POOLING (pdgn_orient_pool).  idx (n,k); votes as above.
//   Start.  v_i = (int64)front_i - (int64)back_i for a live i; v_i = 0, now and after every round, for a dead one.
//   Slots.  For a live i and a slot s, j = idx[i][s]: ignored where j is outside [0, n) (never dereferenced), j == i, or j is dead (rule 2
//           of csrc/orient.hip).  A j that fills several slots counts as often as it occurs.
//   Coefficient.  d = x_j - x_i (three subtractions), d2 = dot3(d, d), a = dot3(d, g_i), a' = dot3(d, g_j), t = dot3(g_i, g_j).
//           c_ij = sign(t) (+1 or -1) where  a*a <= 0.25f*d2  and  a'*a' <= 0.25f*d2  and  |t| > 0.5f  all hold, else 0: j lies within 30
//           degrees of the tangent planes of both points and the two normal lines are within 60 degrees.  The neighbour across a thin
//           sheet lies along the normal and is left out; a coincident neighbour (d2 = 0) passes the first two.
//   Round.  v'_i = 2 v_i + sum over the slots of c_ij v_j, from the v of the round before (Jacobi).  `rounds` of them, 0 .. 4:
//           |v| <= 2^13 66^4 < 2^38.
//   Output. o_i = -g_i (three sign bits) iff the final v_i < 0; otherwise o_i = g_i bit for bit.  pooled_i = the final v_i.
//   Stats.  Per cloud: flipped (v_i < 0), undecided (live and v_i == 0), unseen (live and front_i + back_i == 0), dead.
//
// THE KERNELS.  Votes: one workgroup of 256 threads per (cloud, view), view fastest in the grid, so that the NV workgroups that read the
// same cloud run next to each other and hit in L2; a thread per point in both passes (the snap is computed twice: 30 flops against a
// register array of unknown length).  The depth buffer is dynamic LDS, 4 R^2 bytes: 16 KB at R = 64, where a CU holds eight workgroups
// (its 32 waves), 144 KB at R = 192, where it holds one.  Pass 1 is ds_min_u32 without return: about nine per point at the default disc
// of 1.5 pixels, and neighbouring points meet on the same words, which the LDS serialises per word -- a few dozen cycles against the
// point's 24 bytes from L2.  A thread walks its own disc, so a disc far wider than a few pixels (a splat beyond the image: R^2 minima
// per point) is correct and slow.  Pass 2 reads one word per point and adds one word with global_atomic_add_u32 without return.
// Pooling: one thread per point per round, 256-thread workgroups that never straddle a cloud; a slot costs 32 gathered bytes.  The
// last launch writes the normals and nothing before it does, so normals_out may be normals_in.
#include "common.h"

#include <math.h>

#define CV_THREADS 256
#define CV_EMPTY 0xffffffffu

struct CvArgs {
    const float *xyz, *nrm, *frame, *views;
    uint32_t *votes;
    int n, NV, R, splat, bias;
};

struct CvView {
    float ex[3], ey[3], ez[3], c[3], rho;
    int R;
};

// ---- the snap of csrc/visible.hip (a local copy: visible.hip stays as it is)
__device__ __forceinline__ float cv_dot(const float *e, float d0, float d1, float d2) {
    return __fadd_rn(__fadd_rn(__fmul_rn(e[0], d0), __fmul_rn(e[1], d1)), __fmul_rn(e[2], d2));
}

__device__ __forceinline__ int cv_quant(float t, float rho, float s) {
    const float q = rintf(__fmul_rn(t / rho, s));
    return (int)fminf(fmaxf(q, -s), s) + (int)s;                 // (fmaxf drops a NaN: the lower end)
}

__device__ __forceinline__ void cv_snap(const CvView &w, const float *p, int &X, int &Y, int &Z) {
    const float d0 = __fsub_rn(p[0], w.c[0]), d1 = __fsub_rn(p[1], w.c[1]), d2 = __fsub_rn(p[2], w.c[2]);
    const float s = (float)(w.R << 7);
    X = cv_quant(cv_dot(w.ex, d0, d1, d2), w.rho, s);
    Y = cv_quant(cv_dot(w.ey, d0, d1, d2), w.rho, s);
    Z = cv_quant(cv_dot(w.ez, d0, d1, d2), w.rho, 1048576.f);
}

__device__ __forceinline__ bool cv_finite3(const float *p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

extern __shared__ unsigned cv_buf[];

__global__ __launch_bounds__(CV_THREADS) void cloudvis_votes_kernel(CvArgs a) {
    const int tid = threadIdx.x, R = a.R;
    const int cloud = blockIdx.x / a.NV, view = blockIdx.x - cloud * a.NV;
    CvView w;
    const float *e = a.views + 9 * view, *fr = a.frame + 4 * (size_t)cloud;
#pragma unroll
    for (int i = 0; i < 3; ++i) w.ex[i] = e[i], w.ey[i] = e[3 + i], w.ez[i] = e[6 + i], w.c[i] = fr[i];
    w.rho = fr[3], w.R = R;
    const float *x = a.xyz + (size_t)cloud * a.n * 3, *g = a.nrm + (size_t)cloud * a.n * 3;
    for (int i = tid; i < R * R; i += CV_THREADS) cv_buf[i] = CV_EMPTY;
    __syncthreads();

    // ---- pass 1: the own pixel and the disc
    const long long s2 = (long long)a.splat * a.splat;
    for (int i = tid; i < a.n; i += CV_THREADS) {
        const float p[3] = {x[3 * (size_t)i], x[3 * (size_t)i + 1], x[3 * (size_t)i + 2]};
        if (!(cv_finite3(p) && cv_finite3(g + 3 * (size_t)i))) continue;
        int X, Y, Z;
        cv_snap(w, p, X, Y, Z);
        atomicMin(cv_buf + min(Y >> 8, R - 1) * R + min(X >> 8, R - 1), (unsigned)Z);
        // the pixels whose centres lie in [X - splat, X + splat] x [Y - splat, Y + splat]: centre 256 px + 128 (floor and ceiling by shifts)
        const int px0 = (int)max(((long long)X - a.splat - 128 + 255) >> 8, 0LL), px1 = (int)min(((long long)X + a.splat - 128) >> 8, (long long)R - 1);
        const int py0 = (int)max(((long long)Y - a.splat - 128 + 255) >> 8, 0LL), py1 = (int)min(((long long)Y + a.splat - 128) >> 8, (long long)R - 1);
        for (int py = py0; py <= py1; ++py) {
            const long long dy = (long long)(256 * py + 128 - Y), rem = s2 - dy * dy;
            for (int px = px0; px <= px1; ++px) {
                const long long dx = (long long)(256 * px + 128 - X);
                if (dx * dx <= rem) atomicMin(cv_buf + py * R + px, (unsigned)Z);
            }
        }
    }
    __syncthreads();

    // ---- pass 2: the depth test and the vote
    for (int i = tid; i < a.n; i += CV_THREADS) {
        const float p[3] = {x[3 * (size_t)i], x[3 * (size_t)i + 1], x[3 * (size_t)i + 2]};
        const float q[3] = {g[3 * (size_t)i], g[3 * (size_t)i + 1], g[3 * (size_t)i + 2]};
        if (!(cv_finite3(p) && cv_finite3(q))) continue;
        int X, Y, Z;
        cv_snap(w, p, X, Y, Z);
        if ((long long)Z > (long long)cv_buf[min(Y >> 8, R - 1) * R + min(X >> 8, R - 1)] + a.bias) continue;
        const float s = cv_dot(q, w.ez[0], w.ez[1], w.ez[2]);    // dot3(g, e_z)
        if (!(s < 0.f || s > 0.f)) continue;
        const unsigned wt = (unsigned)__fmul_rn(fminf(fabsf(s), 1.0f), 256.0f);
        if (wt) atomicAdd(a.votes + 2 * ((size_t)cloud * a.n + i) + (s > 0.f), wt);
    }
}

// ---------------------------------------------------------------------------- the pooling
struct PoolArgs {
    int n, k, bpc;                                               // bpc: workgroups per cloud
    const float *xyz, *gin;
    const int32_t *idx;
    const uint32_t *votes;
    const long long *vin;                                        // the round before; null: the start (front - back)
    long long *vout;
    float *out;
    long long *pooled;
    int32_t *stats;
};

__device__ __forceinline__ long long pool_value(const PoolArgs &a, size_t at) {
    return a.vin ? a.vin[at] : (long long)a.votes[2 * at] - (long long)a.votes[2 * at + 1];
}

__global__ __launch_bounds__(CV_THREADS) void cloudvis_pool_round_kernel(PoolArgs a) {
    const int cloud = blockIdx.x / a.bpc, i = (blockIdx.x - cloud * a.bpc) * CV_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const size_t base = (size_t)cloud * a.n, at = base + i;
    const float *xi = a.xyz + 3 * at, *gi = a.gin + 3 * at;
    const float x0 = xi[0], x1 = xi[1], x2 = xi[2], g0 = gi[0], g1 = gi[1], g2 = gi[2];
    if (!(isfinite(x0) && isfinite(x1) && isfinite(x2) && isfinite(g0) && isfinite(g1) && isfinite(g2))) {
        a.vout[at] = 0;
        return;
    }
    long long acc = 2 * pool_value(a, at);
    const int32_t *row = a.idx + at * a.k;
    for (int s = 0; s < a.k; ++s) {
        const int j = row[s];
        if ((unsigned)j >= (unsigned)a.n || j == i) continue;
        const float *xj = a.xyz + 3 * (base + j), *gj = a.gin + 3 * (base + j);
        const float h0 = gj[0], h1 = gj[1], h2 = gj[2];
        if (!(cv_finite3(xj) && isfinite(h0) && isfinite(h1) && isfinite(h2))) continue;
        const float d0 = __fsub_rn(xj[0], x0), d1 = __fsub_rn(xj[1], x1), d2c = __fsub_rn(xj[2], x2);
        const float lim = __fmul_rn(0.25f, dot3_rn(d0, d1, d2c, d0, d1, d2c));
        const float ai = dot3_rn(d0, d1, d2c, g0, g1, g2), aj = dot3_rn(d0, d1, d2c, h0, h1, h2), t = dot3_rn(g0, g1, g2, h0, h1, h2);
        if (__fmul_rn(ai, ai) <= lim && __fmul_rn(aj, aj) <= lim && fabsf(t) > 0.5f) {
            const long long vj = pool_value(a, base + j);
            acc += t > 0.f ? vj : -vj;
        }
    }
    a.vout[at] = acc;
}

// The last launch: the signs, pooled and the counters.  vin null: rounds == 0.
__global__ __launch_bounds__(CV_THREADS) void cloudvis_pool_apply_kernel(PoolArgs a) {
    const int cloud = blockIdx.x / a.bpc, i = (blockIdx.x - cloud * a.bpc) * CV_THREADS + threadIdx.x;
    bool flip = false, undecided = false, unseen = false, dead = false;
    if (i < a.n) {
        const size_t at = (size_t)cloud * a.n + i;
        const float *xi = a.xyz + 3 * at;
        const unsigned b0 = __float_as_uint(a.gin[3 * at]), b1 = __float_as_uint(a.gin[3 * at + 1]), b2 = __float_as_uint(a.gin[3 * at + 2]);
        dead = !(cv_finite3(xi) && isfinite(__uint_as_float(b0)) && isfinite(__uint_as_float(b1)) && isfinite(__uint_as_float(b2)));
        const long long v = dead ? 0 : pool_value(a, at);
        flip = v < 0, undecided = !dead && v == 0;
        unseen = !dead && a.votes[2 * at] + a.votes[2 * at + 1] == 0u;
        const unsigned sg = flip ? 0x80000000u : 0u;
        float *o = a.out + 3 * at;
        o[0] = __uint_as_float(b0 ^ sg), o[1] = __uint_as_float(b1 ^ sg), o[2] = __uint_as_float(b2 ^ sg);
        if (a.pooled) a.pooled[at] = v;
    }
    if (a.stats) {                                               // (a workgroup is inside one cloud: one integer add per wave and counter)
        const int c0 = __popcll(__ballot(flip)), c1 = __popcll(__ballot(undecided)), c2 = __popcll(__ballot(unseen)), c3 = __popcll(__ballot(dead));
        if (lane_id() == 0) {
            int32_t *st = a.stats + 4 * (size_t)cloud;
            if (c0) atomicAdd(st, c0);
            if (c1) atomicAdd(st + 1, c1);
            if (c2) atomicAdd(st + 2, c2);
            if (c3) atomicAdd(st + 3, c3);
        }
    }
}

static bool cv_shape_ok(int b, int n) { return b >= 1 && n >= 1 && (long long)b * n <= (1LL << 28); }

extern "C" int pdgn_cloud_normal_votes(int b, int n, const float *xyz, const float *normals, const float *frame, const float *views, int NV,
                                       int R, int splat, int bias, uint32_t *votes, pdgn_stream_t stream) {
    // host-side checks only: nothing is launched and nothing written before all of them have passed
    if (!cv_shape_ok(b, n) || NV < 1 || NV > PDGN_VISIBLE_MAX_VIEWS || R < PDGN_CLOUDVIS_MIN_RES || R > PDGN_VISIBLE_MAX_RES) return PDGN_ERR_INVALID;
    if (splat < 0 || bias < 0 || (long long)b * NV > 0x7fffffffLL) return PDGN_ERR_INVALID;
    if (!xyz || !normals || !frame || !views || !votes) return PDGN_ERR_INVALID;
    if (((uintptr_t)xyz | (uintptr_t)normals | (uintptr_t)frame | (uintptr_t)views | (uintptr_t)votes) & 3) return PDGN_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    CvArgs a;
    a.xyz = xyz, a.nrm = normals, a.frame = frame, a.views = views, a.votes = votes;
    a.n = n, a.NV = NV, a.R = R, a.splat = splat, a.bias = bias;
    const size_t lds = (size_t)R * R * 4;
    if (lds > 48 * 1024) {                                       // beyond what a launch gets unasked: opt in, as csrc/visible.hip
        hipError_t e = hipFuncSetAttribute((const void *)cloudvis_votes_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipError_t e = hipMemsetAsync(votes, 0, sizeof(uint32_t) * 2 * (size_t)b * n, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(cloudvis_votes_kernel, dim3(b * NV), dim3(CV_THREADS), lds, s, a);
    return pdgn_launch_status();
}

extern "C" int pdgn_orient_pool(int b, int n, int k, const float *xyz, const int32_t *idx, const float *normals_in, const uint32_t *votes,
                                int rounds, float *normals_out, long long *pooled, int32_t *stats, long long *workspace, pdgn_stream_t stream) {
    if (!cv_shape_ok(b, n) || k < 1 || k > PDGN_NORMALS_MAX_K || rounds < 0 || rounds > PDGN_CLOUDVIS_MAX_ROUNDS) return PDGN_ERR_INVALID;
    if (!xyz || !idx || !normals_in || !votes || !normals_out || !workspace) return PDGN_ERR_INVALID;
    if (((uintptr_t)xyz | (uintptr_t)idx | (uintptr_t)normals_in | (uintptr_t)votes | (uintptr_t)normals_out | (uintptr_t)stats) & 3)
        return PDGN_ERR_INVALID;
    if (((uintptr_t)pooled | (uintptr_t)workspace) & 7) return PDGN_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    PoolArgs a = {};
    a.n = n, a.k = k, a.bpc = cdiv(n, CV_THREADS);
    a.xyz = xyz, a.gin = normals_in, a.idx = idx, a.votes = votes, a.out = normals_out, a.pooled = pooled, a.stats = stats;
    const long long blocks = (long long)b * a.bpc;               // (at most 2^28 + 2^20)
    if (stats) {
        hipError_t e = hipMemsetAsync(stats, 0, sizeof(int32_t) * 4 * (size_t)b, s);
        if (e != hipSuccess) return (int)e;
    }
    long long *bufs[2] = {workspace, workspace + (size_t)b * n};
    for (int r = 0; r < rounds; ++r) {
        a.vout = bufs[r & 1];
        hipLaunchKernelGGL(cloudvis_pool_round_kernel, dim3((unsigned)blocks), dim3(CV_THREADS), 0, s, a);
        const int rc = pdgn_launch_status();
        if (rc) return rc;
        a.vin = a.vout;
    }
    a.vout = nullptr;
    hipLaunchKernelGGL(cloudvis_pool_apply_kernel, dim3((unsigned)blocks), dim3(CV_THREADS), 0, s, a);
    return pdgn_launch_status();
}
