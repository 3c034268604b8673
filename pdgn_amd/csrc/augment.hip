// augment.hip -- differentiable augmentation of what the discriminators see: a fresh random similarity transform (flip, rotation
// about the up axis, isotropic scale, translation) plus per-point jitter for every cloud in front of every discriminator call.
// pdgn_augment_rows_fwd writes the transformed cloud straight into the (B*N, 3) row layout PointDiscriminator.forward starts
// from: for a real batch, stored (B,3,N), it takes the place of that forward's `x.transpose(1, 2).reshape(B * N, 3)` copy kernel;
// for a generated cloud -- a (B,3,N) view of point-major rows, for which torch's reshape is a view -- it is one launch more, and
// pdgn_augment_rows_bwd another in the generator's backward.  No reference counterpart (utils/provider.py's host-side augmentation
// is not ported).
// Randomness: Philox4x32-10, a pure function of (seed, clock, global row, tag) with the clock READ FROM DEVICE MEMORY, so a replayed
// launch list draws afresh every iteration; layout in include/pdgn_hip.h, host mirror in tests/augment_mirror.py.
//
// One thread = four consecutive points of one sample: three 16-byte loads along N (one per channel, a wave reads 1 KiB contiguous
// per channel) and 48 contiguous bytes of rows (three 16-byte stores), or the other way round in the adjoint.  A point-major cloud
// is read (and its gradient written) as it lies, 48 contiguous bytes a thread, with no copy in front.  Every thread derives
// its sample's matrix itself (three Philox groups, one sincosf, one expf: uniform over the workgroup, which sees one sample).
// No LDS, no atomics.
#include "common.h"
#include "philox.h"

#define AUG_THREADS 256
#define AUG_GROUP_ENABLE 0u                                      // words: flip, rotate, scale, translate enabled?
#define AUG_GROUP_SHAPE 1u                                       // words: jitter enabled?, angle, log-scale, (unused)
#define AUG_GROUP_SHIFT 2u                                       // words: translation x, y, z, (unused)
#define AUG_GROUP_POINT0 4u                                      // group 4 + n: the three normals of point n (words 0,1 -> x, y; 2,3 -> z, unused)

struct AugArgs {
    int N, groups, vec;
    int pm;                                                      // the cloud-side tensor (x / dx) is point-major, (B,N,3): a (B,3,N) VIEW of rows -- what the generator hands out
    unsigned k0, k1, row0, tag;
    const pdgn_aug_table *tab;
    const unsigned long long *clock;
    const float *in;
    float *out;
    float *affine;
};

struct AugAffine {
    float a[9], t[3];                                            // rows = a x + t, a row-major
    float sigma;
    bool jitter;
    unsigned t_lo, c3;                                           // the counter words every group of this sample shares
};

// a word's upper 24 bits as a number in [-1, 1): ((w >> 8) - 2^23) 2^-23, exact in fp32
__device__ __forceinline__ float aug_unit(unsigned w) { return (float)((int)(w >> 8) - 8388608) * 1.1920928955078125e-7f; }

__device__ __forceinline__ void aug_affine(const AugArgs &g, unsigned row, AugAffine &o) {
    const pdgn_aug_table *tab = g.tab;
    const unsigned long long t = g.clock[0] - 1ull;              // the clock counts the iterations BEGUN: the one in flight is clock - 1
    o.t_lo = (unsigned)t;
    o.c3 = g.tag | (((unsigned)(t >> 32) & 0xffffffu) << 8);
    unsigned e[4], d[4], w[4];
    philox4x32_10(AUG_GROUP_ENABLE, row, o.t_lo, o.c3, g.k0, g.k1, e);
    philox4x32_10(AUG_GROUP_SHAPE, row, o.t_lo, o.c3, g.k0, g.k1, d);
    philox4x32_10(AUG_GROUP_SHIFT, row, o.t_lo, o.c3, g.k0, g.k1, w);
    const bool flip = (e[0] >> 8) < tab->thr_flip, rot = (e[1] >> 8) < tab->thr_rot;
    const bool scale = (e[2] >> 8) < tab->thr_scale, shift = (e[3] >> 8) < tab->thr_trans;
    o.jitter = (d[0] >> 8) < tab->thr_jitter;
    o.sigma = tab->sigma;
    float c = 1.0f, s = 0.0f;
    if (rot) sincosf(__fmul_rn(tab->rot_max, aug_unit(d[1])), &s, &c);
    const float sc = scale ? expf(__fmul_rn(tab->log_scale_max, aug_unit(d[2]))) : 1.0f;
    const int u = tab->up_axis, fa = tab->flip_axis;
    const int ia = u == 2 ? 0 : u + 1;                           // the rotation's plane: axes (ia, ib) = (u + 1, u + 2) mod 3
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float r = (i == u && j == u) ? 1.0f : (i == u || j == u) ? 0.0f : (i == j) ? c : (i == ia) ? -s : s;
            o.a[3 * i + j] = __fmul_rn(sc, (flip && j == fa) ? -r : r);
        }
        o.t[i] = shift ? __fmul_rn(tab->trans_max, aug_unit(w[i])) : 0.0f;
    }
}

__global__ __launch_bounds__(AUG_THREADS) void augment_rows_fwd_kernel(AugArgs g) {
    const int q = blockIdx.x * AUG_THREADS + threadIdx.x;        // points 4q .. 4q+3 of sample b
    const int b = blockIdx.y;
    if (q >= g.groups) return;
    const unsigned row = g.row0 + (unsigned)b;
    AugAffine m;
    aug_affine(g, row, m);
    if (g.affine && q == 0) {
        float *dst = g.affine + (size_t)b * 12;
#pragma unroll
        for (int i = 0; i < 9; ++i) dst[i] = m.a[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) dst[9 + i] = m.t[i];
    }
    const int n0 = 4 * q;
    const int cols = min(4, g.N - n0);
    const float *src = g.in + (g.pm ? ((size_t)b * g.N + n0) * 3 : (size_t)b * 3 * g.N + n0);
    float x[3][4];
    if (g.pm) {                                                  // 48 contiguous bytes in, 48 out
        float v[12];
        if (g.vec) {
            const float4 *s4 = reinterpret_cast<const float4 *>(src);
            float4 a = s4[0], c = s4[1], e = s4[2];
            v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = c.x, v[5] = c.y, v[6] = c.z, v[7] = c.w;
            v[8] = e.x, v[9] = e.y, v[10] = e.z, v[11] = e.w;
        } else {
#pragma unroll
            for (int i = 0; i < 12; ++i) v[i] = i < 3 * cols ? src[i] : 0.0f;
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
            for (int p = 0; p < 4; ++p) x[ch][p] = v[3 * p + ch];
    } else if (g.vec) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float4 v = *reinterpret_cast<const float4 *>(src + (size_t)ch * g.N);
            x[ch][0] = v.x, x[ch][1] = v.y, x[ch][2] = v.z, x[ch][3] = v.w;
        }
    } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
            for (int p = 0; p < 4; ++p) x[ch][p] = p < cols ? src[(size_t)ch * g.N + p] : 0.0f;
    }
    float o[12];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int i = 0; i < 3; ++i)                              // ((a_i0 x0 + a_i1 x1) + a_i2 x2) + t_i: four products and sums, each rounded on its own
            o[3 * p + i] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m.a[3 * i], x[0][p]), __fmul_rn(m.a[3 * i + 1], x[1][p])),
                                               __fmul_rn(m.a[3 * i + 2], x[2][p])), m.t[i]);
    if (m.jitter) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (p < cols) {
                unsigned w[4];
                philox4x32_10(AUG_GROUP_POINT0 + (unsigned)(n0 + p), row, m.t_lo, m.c3, g.k0, g.k1, w);
                float j0, j1, j2, unused;
                box_muller(w[0], w[1], m.sigma, j0, j1);
                box_muller(w[2], w[3], m.sigma, j2, unused);
                o[3 * p] = __fadd_rn(o[3 * p], j0), o[3 * p + 1] = __fadd_rn(o[3 * p + 1], j1), o[3 * p + 2] = __fadd_rn(o[3 * p + 2], j2);
            }
        }
    }
    float *dst = g.out + ((size_t)b * g.N + n0) * 3;
    if (g.vec) {
        float4 *d4 = reinterpret_cast<float4 *>(dst);
        d4[0] = make_float4(o[0], o[1], o[2], o[3]);
        d4[1] = make_float4(o[4], o[5], o[6], o[7]);
        d4[2] = make_float4(o[8], o[9], o[10], o[11]);
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i)
            if (i < 3 * cols) dst[i] = o[i];
    }
}

__global__ __launch_bounds__(AUG_THREADS) void augment_rows_bwd_kernel(AugArgs g) {
    const int q = blockIdx.x * AUG_THREADS + threadIdx.x;
    const int b = blockIdx.y;
    if (q >= g.groups) return;
    AugAffine m;
    aug_affine(g, g.row0 + (unsigned)b, m);
    const int n0 = 4 * q;
    const int cols = min(4, g.N - n0);
    const float *src = g.in + ((size_t)b * g.N + n0) * 3;
    float d[12];
    if (g.vec) {
        const float4 *s4 = reinterpret_cast<const float4 *>(src);
        float4 u = s4[0], v = s4[1], w = s4[2];
        d[0] = u.x, d[1] = u.y, d[2] = u.z, d[3] = u.w, d[4] = v.x, d[5] = v.y, d[6] = v.z, d[7] = v.w;
        d[8] = w.x, d[9] = w.y, d[10] = w.z, d[11] = w.w;
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) d[i] = i < 3 * cols ? src[i] : 0.0f;
    }
    float o[3][4];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int p = 0; p < 4; ++p)                              // (a_0j d0 + a_1j d1) + a_2j d2: the transpose's column j, each operation rounded on its own
            o[j][p] = __fadd_rn(__fadd_rn(__fmul_rn(m.a[j], d[3 * p]), __fmul_rn(m.a[3 + j], d[3 * p + 1])), __fmul_rn(m.a[6 + j], d[3 * p + 2]));
    if (g.pm) {
        float *dst = g.out + ((size_t)b * g.N + n0) * 3;
        if (g.vec) {
            float4 *d4 = reinterpret_cast<float4 *>(dst);
            d4[0] = make_float4(o[0][0], o[1][0], o[2][0], o[0][1]);
            d4[1] = make_float4(o[1][1], o[2][1], o[0][2], o[1][2]);
            d4[2] = make_float4(o[2][2], o[0][3], o[1][3], o[2][3]);
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if (p < cols) dst[3 * p + j] = o[j][p];
        }
        return;
    }
    float *dst = g.out + (size_t)b * 3 * g.N + n0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float *dj = dst + (size_t)j * g.N;
        if (g.vec) {
            *reinterpret_cast<float4 *>(dj) = make_float4(o[j][0], o[j][1], o[j][2], o[j][3]);
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (p < cols) dj[p] = o[j][p];
        }
    }
}

__global__ void augment_tick_kernel(unsigned long long *clock) {
    if (blockIdx.x == 0 && threadIdx.x == 0) clock[0] = clock[0] + 1ull;
}

// The adaptive tick (include/pdgn_hip.h: pdgn_ada_state): clock += 1, the four discriminators' slots folded into the accumulators and
// zeroed, and -- once `interval` contributing iterations have accumulated -- one integer step of the threshold towards the target.
// One thread: ~50 independent loads and as many stores, once per iteration.  No fence, no atomic: every writer of a slot is
// stream-ordered before this launch and this launch before every reader of the table (the argument of the clock).
__global__ void augment_tick_ada_kernel(unsigned long long *clock, pdgn_ada_state *st, int *slots, pdgn_aug_table *tab) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    clock[0] = clock[0] + 1ull;
    unsigned long long c[12], P = 0, G = 0, N = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = (unsigned long long)(unsigned)slots[4 * i + j];
        P += c[3 * i], G += c[3 * i + 1], N += c[3 * i + 2];
    }
#pragma unroll
    for (int i = 0; i < PDGN_ADA_SLOT_WORDS; ++i) slots[i] = 0;
    if (N == 0) return;                                          // an iteration that contributed nothing does not count
    unsigned long long pos = st->pos + P, neg = st->neg + G, n = st->n + N, iters = st->iters + 1ull;
    unsigned long long net[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) net[i] = st->net[i] + c[i];
    if (iters < st->interval) {
        st->pos = pos, st->neg = neg, st->n = n, st->iters = iters;
#pragma unroll
        for (int i = 0; i < 12; ++i) st->net[i] = net[i];
        return;
    }
    const double r = (double)((long long)pos - (long long)neg) / (double)n;
    const unsigned long long q = (n << 24) / (4ull * st->span);
    const long long step = (long long)(q < 1ull ? 1ull : q);
    const double target = st->target;
    long long thr = (long long)st->thr;
    if (r > target) thr += step;
    else if (r < target) thr -= step;
    const long long lo = (long long)st->thr_min, hi = (long long)st->thr_max;
    thr = thr < lo ? lo : thr > hi ? hi : thr;
    st->thr = (unsigned long long)thr;
    const unsigned long long mask = st->mask;
    if (mask & 1ull) tab->thr_flip = (unsigned)thr;
    if (mask & 2ull) tab->thr_rot = (unsigned)thr;
    if (mask & 4ull) tab->thr_scale = (unsigned)thr;
    if (mask & 8ull) tab->thr_trans = (unsigned)thr;
    if (mask & 16ull) tab->thr_jitter = (unsigned)thr;
    st->last_r = r, st->last_pos = pos, st->last_neg = neg, st->last_n = n;
#pragma unroll
    for (int i = 0; i < 12; ++i) st->last_net[i] = net[i], st->net[i] = 0ull;
    st->pos = st->neg = st->n = st->iters = 0ull;
    st->updates = st->updates + 1ull;
}

// host-side checks only: nothing here touches the device
static int aug_args(int B, int N, const float *in, float *out, float *affine, const pdgn_aug_table *table, const unsigned long long *clock,
                    unsigned long long seed, long long row0, int tag, int point_major, AugArgs &a) {
    if (B <= 0 || B > 65535 || N <= 0 || (long long)N > 0x7fffffffLL / 3 - 4) return PDGN_ERR_INVALID;
    if (!in || !out || !table || !clock) return PDGN_ERR_INVALID;
    if ((((uintptr_t)in | (uintptr_t)out | (uintptr_t)affine | (uintptr_t)table) & 3) || ((uintptr_t)clock & 7)) return PDGN_ERR_INVALID;
    if (row0 < 0 || row0 + B > 0x100000000LL) return PDGN_ERR_INVALID;                       // the global row is one 32-bit counter word
    if (tag < PDGN_AUG_TAG_BASE || tag >= PDGN_AUG_TAG_BASE + PDGN_AUG_SITES) return PDGN_ERR_INVALID;
    a.N = N, a.groups = (N + 3) / 4, a.pm = point_major != 0;
    a.vec = N % 4 == 0 && !(((uintptr_t)in | (uintptr_t)out) & 15);
    a.k0 = (unsigned)seed, a.k1 = (unsigned)(seed >> 32);
    a.row0 = (unsigned)row0, a.tag = (unsigned)tag;
    a.tab = table, a.clock = clock, a.in = in, a.out = out, a.affine = affine;
    return 0;
}

extern "C" int pdgn_augment_rows_fwd(int B, int N, const float *x, int x_point_major, float *rows, float *affine_out,
                                     const pdgn_aug_table *table, const unsigned long long *clock, unsigned long long seed, long long row0,
                                     int tag, pdgn_stream_t stream) {
    AugArgs a;
    if (aug_args(B, N, x, rows, affine_out, table, clock, seed, row0, tag, x_point_major, a)) return PDGN_ERR_INVALID;
    hipLaunchKernelGGL(augment_rows_fwd_kernel, dim3(cdiv(a.groups, AUG_THREADS), B), dim3(AUG_THREADS), 0, (hipStream_t)stream, a);
    return pdgn_launch_status();
}

extern "C" int pdgn_augment_rows_bwd(int B, int N, const float *d_rows, float *dx, int dx_point_major, const pdgn_aug_table *table,
                                     const unsigned long long *clock, unsigned long long seed, long long row0, int tag,
                                     pdgn_stream_t stream) {
    AugArgs a;
    if (aug_args(B, N, d_rows, dx, nullptr, table, clock, seed, row0, tag, dx_point_major, a)) return PDGN_ERR_INVALID;
    hipLaunchKernelGGL(augment_rows_bwd_kernel, dim3(cdiv(a.groups, AUG_THREADS), B), dim3(AUG_THREADS), 0, (hipStream_t)stream, a);
    return pdgn_launch_status();
}

extern "C" int pdgn_augment_tick(unsigned long long *clock, pdgn_stream_t stream) {
    if (!clock || ((uintptr_t)clock & 7)) return PDGN_ERR_INVALID;
    hipLaunchKernelGGL(augment_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, clock);
    return pdgn_launch_status();
}

extern "C" int pdgn_augment_tick_ada(unsigned long long *clock, pdgn_ada_state *state, int32_t *slots, pdgn_aug_table *table, long long interval,
                                     long long span, long long thr_min, long long thr_max, pdgn_stream_t stream) {
    if (!clock || !state || !slots || !table) return PDGN_ERR_INVALID;
    if ((((uintptr_t)clock | (uintptr_t)state) & 7) || (((uintptr_t)slots | (uintptr_t)table) & 3)) return PDGN_ERR_INVALID;
    if (interval < 1 || span < 1 || span > (1LL << 40) || thr_min < 0 || thr_min > thr_max || thr_max > (1LL << 24)) return PDGN_ERR_INVALID;
    static_assert(sizeof(pdgn_ada_state) == 8 * PDGN_ADA_STATE_WORDS, "pdgn_ada_state: 40 64-bit words");
    hipLaunchKernelGGL(augment_tick_ada_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, clock, state, slots, table);
    return pdgn_launch_status();
}
