// feed.hip -- pdgn_feed_batch: one launch writes a whole training batch (the four real resolutions and the two noise
// tensors) from a device-resident data set into the buffers the training step reads.  Replaces, per iteration, the
// DataLoader's shuffle + collate, ShapeNetCore.__getitem__'s three np.random.choice sub-samplings
// (datasets_4point.py:370-380), the four transposes (models/PDGNet_v2.py:184,195,206,217) and the two np.random.normal
// draws (:178, :228).  Randomness: Philox4x32-10, counter-based, a pure function of the arguments (layout in
// include/pdgn_hip.h); the host mirror of the tests (tests/feed_mirror.py) spells the same function in numpy.
//
// One thread = one 4-word Philox group = four consecutive output columns of one row: four gathered points (12 floats
// in, one 16-byte store per channel), four points of the transposed full cloud (48 contiguous bytes in, one 16-byte
// store per channel) or four normals (one 16-byte store).  A wave therefore writes 1 KiB contiguous per channel.
// No LDS, no atomics.
//
// pdgn_feed_batch_resample: the same launch for clouds stored with M >= N points each.  p4 is a fresh N-point subset of the
// cloud's leading P points per row and iteration -- column j takes point pi(j), pi a keyed Feistel permutation of [0, P)
// (construction in include/pdgn_hip.h; mirror: tests/resample_mirror.py) -- four 12-byte gathers per thread instead of 48
// contiguous bytes; the sub-resolutions draw from the pool, the noise is pdgn_feed_batch's.
//
// pdgn_feed_batch_mesh / pdgn_sample_surface: the same launch for shapes stored as triangle meshes.  Every output column is a fresh
// point of the row's surface: ONE Philox call per column picks a face through the shape's alias table (one 8-byte load: area-
// proportional) and a point inside it (folded barycentric coordinates, exact in fp32); four dependent gathers per point (face_off,
// alias record, face, vertices) instead of one, no LDS, no atomics; the noise is pdgn_feed_batch's (construction in
// include/pdgn_hip.h; mirror: tests/mesh_mirror.py).
//
// pdgn_feed_batch_ragged / pdgn_sample_ragged: the same launch for clouds that store DIFFERENT numbers of points (one (T,3) array and an
// (S+1) int64 offset table).  A kernel of its own beside feed_batch_kernel<>, with that kernel's geometry and helpers: the row's range
// (two 8-byte loads, clamped into the array) replaces the row stride, the Feistel half width is computed per row from the row's own
// count, column j of p4 takes point pi(j mod M_c) -- N distinct points of a long cloud, the whole of a short one with its duplicates
// spread evenly -- and the sub-resolutions draw from the whole shape; 64-bit offsets into the points (construction in
// include/pdgn_hip.h; mirror: tests/ragged_mirror.py).
#include "common.h"
#include "philox.h"                                             // philox4x32_10, box_muller (shared with augment.hip)

#define FEED_THREADS 256
#define FEED_NOISE_DIM 128                                      // (B,128): models/PDGNet_v2.py:178 with main.py:23's default
#define FEED_TAG_Z1 3u
#define FEED_TAG_Z2 4u
#define FEED_TAG_PERM 6u                                        // the round keys of the resampling permutation
#define FEED_PERM_ROUNDS 6
#define FEED_TAG_MESH 8u                                        // 8 .. 11: the surface draws of p1 .. p4 (pdgn_feed_batch_mesh)
#define FEED_TAG_SURFACE 12u                                    // pdgn_sample_surface
#define FEED_TAG_RAGGED 13u                                     // the round keys of pdgn_sample_ragged

struct FeedArgs {
    int S, N, r[3];
    int M, P;                                                    // points stored per cloud (the row stride) and the pool drawn from; pdgn_feed_batch: M = P = N
    int h;                                                       // resample: bits of one Feistel half
    int g[6];                                                    // exclusive prefix of the groups of one row: p1 p2 p3 p4 z1 z2 (g[5] + 32 = all)
    int groups;
    int vec;                                                     // bit k: output k (p1 p2 p3 p4) takes 16-byte stores; bit 4: the cloud rows take 16-byte loads
    const float *data;
    const int *order;
    long long first;
    unsigned k0, k1, t_lo, t_hi24;
    unsigned row0;
    float sigma;
    float *p[4];
    float *z[2];
};

__device__ __forceinline__ void store4(float *dst, int cols, bool vec, float a, float b, float c, float d) {
    if (vec) {                                                   // (vec: the row length is a multiple of 4, so cols == 4 here)
        *reinterpret_cast<float4 *>(dst) = make_float4(a, b, c, d);
    } else {
        dst[0] = a;
        if (cols > 1) dst[1] = b;
        if (cols > 2) dst[2] = c;
        if (cols > 3) dst[3] = d;
    }
}

// group j of z1 (which = 0) / z2 (1) of local row b: columns 4j .. 4j+3, two Box-Muller pairs (every feed kernel's noise)
__device__ __forceinline__ void feed_noise_group(int j, int which, int b, unsigned row, unsigned t_lo, unsigned t_hi24, unsigned k0, unsigned k1,
                                                 float sigma, float *z) {
    unsigned w[4];
    philox4x32_10((unsigned)j, row, t_lo, (which ? FEED_TAG_Z2 : FEED_TAG_Z1) | (t_hi24 << 8), k0, k1, w);
    float n0, n1, n2, n3;
    box_muller(w[0], w[1], sigma, n0, n1);
    box_muller(w[2], w[3], sigma, n2, n3);
    *reinterpret_cast<float4 *>(z + (size_t)b * FEED_NOISE_DIM + 4 * j) = make_float4(n0, n1, n2, n3);   // (128 floats per row: 16-byte aligned whenever the base is; checked on the host)
}

// one pass of the Feistel network over [0, 2^(2h)): a bijection for any round function
__device__ __forceinline__ unsigned feistel_pass(unsigned x, int h, const unsigned key[FEED_PERM_ROUNDS]) {
    unsigned L = x >> h, R = x & ((1u << h) - 1u);
#pragma unroll
    for (int i = 0; i < FEED_PERM_ROUNDS; ++i) {
        const unsigned f = ((R ^ key[i]) * 0x9E3779B1u) >> (32 - h);
        const unsigned nr = L ^ f;
        L = R, R = nr;
    }
    return (L << h) | R;
}

// RESAMPLE = false is pdgn_feed_batch (M = P = N, p4 the transposed cloud), true pdgn_feed_batch_resample
template <bool RESAMPLE>
__global__ __launch_bounds__(FEED_THREADS) void feed_batch_kernel(FeedArgs a) {
    const int q = blockIdx.x * FEED_THREADS + threadIdx.x;       // the group of row b this thread owns
    const int b = blockIdx.y;
    if (q >= a.groups) return;
    const unsigned row = a.row0 + (unsigned)b;
    unsigned w[4];
    if (q >= a.g[4]) {                                           // ---- noise: group j of z1 / z2 -> columns 4j .. 4j+3
        const int which = q >= a.g[5];
        feed_noise_group(q - a.g[4 + which], which, b, row, a.t_lo, a.t_hi24, a.k0, a.k1, a.sigma, a.z[which]);
        return;
    }
    const int c = min(max(a.order[a.first + b], 0), a.S - 1);    // (a permutation of [0, S) by contract; clamped so that a bad one cannot read outside data)
    const float *cloud = a.data + (size_t)c * a.M * 3;
    if (RESAMPLE && q >= a.g[3]) {                               // ---- N distinct points of the pool: columns 4j .. 4j+3 take the points pi(4j) .. pi(4j+3)
        const int j = q - a.g[3];
        const int cols = min(4, a.N - 4 * j);
        unsigned key[8];
        philox4x32_10(0u, row, a.t_lo, FEED_TAG_PERM | (a.t_hi24 << 8), a.k0, a.k1, key);
        philox4x32_10(1u, row, a.t_lo, FEED_TAG_PERM | (a.t_hi24 << 8), a.k0, a.k1, key + 4);
        float v[12];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned x = i < cols ? (unsigned)(4 * j + i) : 0u;  // (< N <= P: inside the domain, and on a cycle that comes back below P)
            do x = feistel_pass(x, a.h, key); while (x >= (unsigned)a.P);
            const float *pt = cloud + (size_t)x * 3;             // x < P <= M
            v[3 * i] = pt[0], v[3 * i + 1] = pt[1], v[3 * i + 2] = pt[2];
        }
        float *dst = a.p[3] + (size_t)b * 3 * a.N + 4 * j;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            store4(dst + (size_t)ch * a.N, cols, a.vec & 8, v[ch], v[3 + ch], v[6 + ch], v[9 + ch]);
        return;
    }
    if (q >= a.g[3]) {                                           // ---- the full cloud, transposed: points 4j .. 4j+3
        const int j = q - a.g[3];
        const int cols = min(4, a.N - 4 * j);
        const float *src = cloud + (size_t)12 * j;
        float v[12];
        if (a.vec & 16) {
            const float4 *s4 = reinterpret_cast<const float4 *>(src);
            float4 x = s4[0], y = s4[1], z = s4[2];
            v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w, v[4] = y.x, v[5] = y.y, v[6] = y.z, v[7] = y.w;
            v[8] = z.x, v[9] = z.y, v[10] = z.z, v[11] = z.w;
        } else {
#pragma unroll
            for (int i = 0; i < 12; ++i) v[i] = i < 3 * cols ? src[i] : 0.f;
        }
        float *dst = a.p[3] + (size_t)b * 3 * a.N + 4 * j;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            store4(dst + (size_t)ch * a.N, cols, a.vec & 8, v[ch], v[3 + ch], v[6 + ch], v[9 + ch]);
        return;
    }
    // ---- a sub-resolution: columns 4j .. 4j+3 of p_k[b] are the points i = umulhi(word, P), drawn with replacement
    const int k = (q >= a.g[1]) + (q >= a.g[2]);
    const int j = q - a.g[k];
    const int r = a.r[k];
    const int cols = min(4, r - 4 * j);
    philox4x32_10((unsigned)j, row, a.t_lo, (unsigned)k | (a.t_hi24 << 8), a.k0, a.k1, w);
    float v[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float *pt = cloud + (size_t)__umulhi(w[i], (unsigned)a.P) * 3;
        v[3 * i] = pt[0], v[3 * i + 1] = pt[1], v[3 * i + 2] = pt[2];
    }
    float *dst = a.p[k] + (size_t)b * 3 * r + 4 * j;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        store4(dst + (size_t)ch * r, cols, (a.vec >> k) & 1, v[ch], v[3 + ch], v[6 + ch], v[9 + ch]);
}

// what every feed entry point refuses (host-side checks only: nothing here touches the device)
static bool feed_args_invalid(int B, int S, int N, int r1, int r2, int r3, const int32_t *order, long long first, long long row0,
                              const float *p1, const float *p2, const float *p3, const float *p4, const float *z1, const float *z2) {
    if (B <= 0 || B > 65535 || S <= 0 || N <= 0 || r1 <= 0 || r2 <= 0 || r3 <= 0) return true;
    if (first < 0 || first > (long long)S - B) return true;                                   // first + B > S
    if (row0 < 0 || row0 + B > 0x100000000LL) return true;                                    // the global row is one 32-bit counter word
    if (!order || !p1 || !p2 || !p3 || !p4 || !z1 || !z2) return true;
    if ((((uintptr_t)z1 | (uintptr_t)z2) & 15) || (((uintptr_t)p1 | (uintptr_t)p2 | (uintptr_t)p3 | (uintptr_t)p4) & 3)) return true;
    return (long long)r1 + r2 + r3 + N > 0x7fffff00LL;
}

static int feed_launch(bool resample, int B, int S, int M, int P, int N, int r1, int r2, int r3, const float *data, const int32_t *order,
                       long long first, unsigned long long seed, unsigned long long t, long long row0, float sigma, float *p1, float *p2,
                       float *p3, float *p4, float *z1, float *z2, pdgn_stream_t stream) {
    if (feed_args_invalid(B, S, N, r1, r2, r3, order, first, row0, p1, p2, p3, p4, z1, z2)) return PDGN_ERR_INVALID;
    if (N > P || P > M || !data || ((uintptr_t)data & 3)) return PDGN_ERR_INVALID;
    if ((long long)M > 0x7fffffffLL / 3) return PDGN_ERR_INVALID;
    FeedArgs a;
    a.S = S, a.N = N, a.r[0] = r1, a.r[1] = r2, a.r[2] = r3;
    a.M = M, a.P = P;
    int bits = 2;                                                // the Feistel network permutes [0, 2^(2h)) >= [0, P)
    while (bits < 31 && (1LL << bits) < (long long)P) ++bits;
    a.h = (bits + 1) / 2;
    const int len[4] = {r1, r2, r3, N};
    float *const out[4] = {p1, p2, p3, p4};
    int at = 0;
    a.vec = 0;
    for (int k = 0; k < 4; ++k) {
        a.g[k] = at;
        at += (len[k] + 3) / 4;
        a.p[k] = out[k];
        if (len[k] % 4 == 0 && !((uintptr_t)out[k] & 15)) a.vec |= 1 << k;
    }
    if (!resample && N % 4 == 0 && !((uintptr_t)data & 15)) a.vec |= 16;
    a.g[4] = at, a.g[5] = at + FEED_NOISE_DIM / 4;
    a.groups = at + 2 * (FEED_NOISE_DIM / 4);
    a.data = data, a.order = order, a.first = first;
    a.k0 = (unsigned)seed, a.k1 = (unsigned)(seed >> 32);
    a.t_lo = (unsigned)t, a.t_hi24 = (unsigned)(t >> 32) & 0xffffffu;
    a.row0 = (unsigned)row0;
    a.sigma = sigma;
    a.z[0] = z1, a.z[1] = z2;
    dim3 grid(cdiv(a.groups, FEED_THREADS), B);
    if (resample)
        hipLaunchKernelGGL(feed_batch_kernel<true>, grid, dim3(FEED_THREADS), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(feed_batch_kernel<false>, grid, dim3(FEED_THREADS), 0, (hipStream_t)stream, a);
    return pdgn_launch_status();
}

extern "C" int pdgn_feed_batch(int B, int S, int N, int r1, int r2, int r3, const float *data, const int32_t *order, long long first,
                               unsigned long long seed, unsigned long long t, long long row0, float sigma, float *p1, float *p2,
                               float *p3, float *p4, float *z1, float *z2, pdgn_stream_t stream) {
    return feed_launch(false, B, S, N, N, N, r1, r2, r3, data, order, first, seed, t, row0, sigma, p1, p2, p3, p4, z1, z2, stream);
}

extern "C" int pdgn_feed_batch_resample(int B, int S, int M, int P, int N, int r1, int r2, int r3, const float *data, const int32_t *order,
                                        long long first, unsigned long long seed, unsigned long long t, long long row0, float sigma,
                                        float *p1, float *p2, float *p3, float *p4, float *z1, float *z2, pdgn_stream_t stream) {
    return feed_launch(true, B, S, M, P, N, r1, r2, r3, data, order, first, seed, t, row0, sigma, p1, p2, p3, p4, z1, z2, stream);
}

// ---------------------------------------------------------------------------- triangle meshes
struct MeshRef {
    const float *verts;                                          // (V,3), every shape's vertices
    const int *faces;                                            // (F,3), global vertex indices
    const int *face_off;                                         // (S+1)
    const uint2 *alias;                                          // (F): (threshold, alias local to the shape)
};

// One point of the surface of the shape that owns the faces [base, base + Fc), from the four words of one Philox call: the face by
// the alias table (w0: the slot, w1: against its threshold), the point by folded barycentric coordinates (w2, w3).  Every float
// operation is rounded on its own (no contraction), so that plain fp32 numpy reproduces the bits.  Returns the global face index.
__device__ __forceinline__ int mesh_point(const MeshRef &m, int base, unsigned Fc, const unsigned w[4], float p[3]) {
    const unsigned s = __umulhi(w[0], Fc);
    const uint2 rec = m.alias[(size_t)base + s];
    const int f = base + (int)(w[1] < rec.x ? s : rec.y);
    const int *face = m.faces + (size_t)f * 3;
    const float *v0 = m.verts + (size_t)face[0] * 3, *v1 = m.verts + (size_t)face[1] * 3, *v2 = m.verts + (size_t)face[2] * 3;
    unsigned a = w[2] >> 8, b = w[3] >> 8;
    if (a + b > (1u << 24)) a = (1u << 24) - a, b = (1u << 24) - b;       // the other half of the parallelogram, mirrored back
    const float u = (float)a * 5.9604644775390625e-8f, v = (float)b * 5.9604644775390625e-8f;   // (a, b <= 2^24: exact)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float e1 = __fsub_rn(v1[ch], v0[ch]), e2 = __fsub_rn(v2[ch], v0[ch]);
        p[ch] = __fadd_rn(__fadd_rn(v0[ch], __fmul_rn(u, e1)), __fmul_rn(v, e2));
    }
    return f;
}

struct MeshFeedArgs {
    int S, len[4];                                               // r1 r2 r3 N
    int g[6];                                                    // as FeedArgs::g
    int groups;
    int vec;                                                     // bit k: output k takes 16-byte stores
    MeshRef mesh;
    const int *order;
    long long first;
    unsigned k0, k1, t_lo, t_hi24;
    unsigned row0;
    float sigma;
    float *p[4];
    float *z[2];
    int *face_rec;                                               // (B, rec_stride) or null
    int rec_at[4], rec_stride;                                   // where p_k's columns start in a row of face_rec
};

__global__ __launch_bounds__(FEED_THREADS) void feed_batch_mesh_kernel(MeshFeedArgs a) {
    const int q = blockIdx.x * FEED_THREADS + threadIdx.x;
    const int b = blockIdx.y;
    if (q >= a.groups) return;
    const unsigned row = a.row0 + (unsigned)b;
    if (q >= a.g[4]) {
        const int which = q >= a.g[5];
        feed_noise_group(q - a.g[4 + which], which, b, row, a.t_lo, a.t_hi24, a.k0, a.k1, a.sigma, a.z[which]);
        return;
    }
    const int c = min(max(a.order[a.first + b], 0), a.S - 1);
    const int base = a.mesh.face_off[c];
    const unsigned Fc = (unsigned)(a.mesh.face_off[c + 1] - base);
    const int k = (q >= a.g[1]) + (q >= a.g[2]) + (q >= a.g[3]);
    const int j = q - a.g[k];
    const int r = a.len[k];
    const int cols = min(4, r - 4 * j);
    float v[12];
    int f[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {                                // (a column past the row's end is drawn like any other and not stored)
        unsigned w[4];
        philox4x32_10((unsigned)(4 * j + i), row, a.t_lo, (FEED_TAG_MESH + (unsigned)k) | (a.t_hi24 << 8), a.k0, a.k1, w);
        f[i] = mesh_point(a.mesh, base, Fc, w, v + 3 * i);
    }
    float *dst = a.p[k] + (size_t)b * 3 * r + 4 * j;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        store4(dst + (size_t)ch * r, cols, (a.vec >> k) & 1, v[ch], v[3 + ch], v[6 + ch], v[9 + ch]);
    if (a.face_rec) {
        int *rec = a.face_rec + (size_t)b * a.rec_stride + a.rec_at[k] + 4 * j;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < cols) rec[i] = f[i];
    }
}

struct SurfaceArgs {
    int S, n, groups, vec;
    MeshRef mesh;
    unsigned k0, k1, d_lo, d_hi24;
    float *out;
    int *face_rec;
};

__global__ __launch_bounds__(FEED_THREADS) void sample_surface_kernel(SurfaceArgs a) {
    const int j = blockIdx.x * FEED_THREADS + threadIdx.x;       // columns 4j .. 4j+3
    if (j >= a.groups) return;
    const int cols = min(4, a.n - 4 * j);
    for (int s = blockIdx.y; s < a.S; s += gridDim.y) {
        const int base = a.mesh.face_off[s];
        const unsigned Fc = (unsigned)(a.mesh.face_off[s + 1] - base);
        float v[12];
        int f[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned w[4];
            philox4x32_10((unsigned)(4 * j + i), (unsigned)s, a.d_lo, FEED_TAG_SURFACE | (a.d_hi24 << 8), a.k0, a.k1, w);
            f[i] = mesh_point(a.mesh, base, Fc, w, v + 3 * i);
        }
        float *dst = a.out + ((size_t)s * a.n + (size_t)4 * j) * 3;                           // 48 contiguous bytes
        if (a.vec) {                                             // (n a multiple of 4 and the base 16-byte aligned: so is every group)
            float4 *d4 = reinterpret_cast<float4 *>(dst);
            d4[0] = make_float4(v[0], v[1], v[2], v[3]), d4[1] = make_float4(v[4], v[5], v[6], v[7]), d4[2] = make_float4(v[8], v[9], v[10], v[11]);
        } else {
#pragma unroll
            for (int i = 0; i < 12; ++i)
                if (i < 3 * cols) dst[i] = v[i];
        }
        if (a.face_rec) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < cols) a.face_rec[(size_t)s * a.n + 4 * j + i] = f[i];
        }
    }
}

// null or misaligned mesh pointers: what both mesh entry points refuse
static bool mesh_invalid(int S, const float *verts, const int32_t *faces, const int32_t *face_off, const uint32_t *alias, const int32_t *face_rec,
                         MeshRef &m) {
    if (S < 1 || !verts || !faces || !face_off || !alias) return true;
    if ((((uintptr_t)verts | (uintptr_t)faces | (uintptr_t)face_off | (uintptr_t)face_rec) & 3) || ((uintptr_t)alias & 7)) return true;
    m.verts = verts, m.faces = faces, m.face_off = face_off, m.alias = reinterpret_cast<const uint2 *>(alias);
    return false;
}

extern "C" int pdgn_feed_batch_mesh(int B, int S, int V, int F, int N, int r1, int r2, int r3, const float *verts, const int32_t *faces,
                                    const int32_t *face_off, const uint32_t *alias, const int32_t *order, long long first,
                                    unsigned long long seed, unsigned long long t, long long row0, float sigma, float *p1, float *p2,
                                    float *p3, float *p4, float *z1, float *z2, int32_t *face_rec, pdgn_stream_t stream) {
    MeshFeedArgs a;
    if (feed_args_invalid(B, S, N, r1, r2, r3, order, first, row0, p1, p2, p3, p4, z1, z2)) return PDGN_ERR_INVALID;
    if (mesh_invalid(S, verts, faces, face_off, alias, face_rec, a.mesh)) return PDGN_ERR_INVALID;
    if (V < 1 || F < S || V > 0x7fffffff / 3 || F > 0x7fffffff / 3) return PDGN_ERR_INVALID;          // (every shape owns a face)
    a.S = S;
    const int len[4] = {r1, r2, r3, N};
    float *const out[4] = {p1, p2, p3, p4};
    int at = 0, rec = 0;
    a.vec = 0;
    for (int k = 0; k < 4; ++k) {
        a.len[k] = len[k], a.g[k] = at, a.rec_at[k] = rec, a.p[k] = out[k];
        at += (len[k] + 3) / 4, rec += len[k];
        if (len[k] % 4 == 0 && !((uintptr_t)out[k] & 15)) a.vec |= 1 << k;
    }
    a.rec_stride = rec;
    a.g[4] = at, a.g[5] = at + FEED_NOISE_DIM / 4;
    a.groups = at + 2 * (FEED_NOISE_DIM / 4);
    a.order = order, a.first = first;
    a.k0 = (unsigned)seed, a.k1 = (unsigned)(seed >> 32);
    a.t_lo = (unsigned)t, a.t_hi24 = (unsigned)(t >> 32) & 0xffffffu;
    a.row0 = (unsigned)row0;
    a.sigma = sigma;
    a.z[0] = z1, a.z[1] = z2;
    a.face_rec = face_rec;
    hipLaunchKernelGGL(feed_batch_mesh_kernel, dim3(cdiv(a.groups, FEED_THREADS), B), dim3(FEED_THREADS), 0, (hipStream_t)stream, a);
    return pdgn_launch_status();
}

extern "C" int pdgn_sample_surface(int S, int n, const float *verts, const int32_t *faces, const int32_t *face_off,
                                   const uint32_t *alias, unsigned long long seed, unsigned long long draw, float *out, int32_t *face_rec,
                                   pdgn_stream_t stream) {
    SurfaceArgs a;
    if (mesh_invalid(S, verts, faces, face_off, alias, face_rec, a.mesh)) return PDGN_ERR_INVALID;
    if (n < 1 || n > 0x7fffff00 || !out || ((uintptr_t)out & 3)) return PDGN_ERR_INVALID;
    a.S = S, a.n = n, a.groups = (n + 3) / 4;
    a.vec = n % 4 == 0 && !((uintptr_t)out & 15);
    a.k0 = (unsigned)seed, a.k1 = (unsigned)(seed >> 32);
    a.d_lo = (unsigned)draw, a.d_hi24 = (unsigned)(draw >> 32) & 0xffffffu;
    a.out = out, a.face_rec = face_rec;
    hipLaunchKernelGGL(sample_surface_kernel, dim3(cdiv(a.groups, FEED_THREADS), min(S, 65535)), dim3(FEED_THREADS), 0, (hipStream_t)stream, a);
    return pdgn_launch_status();
}

// ---------------------------------------------------------------------------- ragged clouds
struct RaggedRef {
    const float *points;                                         // (T,3), every shape's points back to back
    const long long *off;                                        // (S+1): shape c owns the points [off[c], off[c+1])
    long long T;
};

// The points [lo, lo + M) of shape c.  lo is clamped into [0, T] and M into [0, T - lo]: a table that does not ascend inside [0, T] reads
// other points than it names, never outside the array (T <= 2^31 - 1, checked on the host: M is a 31-bit count).
__device__ __forceinline__ void ragged_range(const RaggedRef &r, int c, long long &lo, unsigned &M) {
    const long long a = r.off[c], e = r.off[c + 1];
    lo = min(max(a, 0LL), r.T);
    M = (unsigned)max(min(max(e, 0LL), r.T) - lo, 0LL);
}

// bits of one Feistel half for a domain of M >= 1 points: (max(2, bit length of M - 1) + 1) / 2, what feed_launch computes from P
__device__ __forceinline__ int ragged_half_bits(unsigned M) {
    const int bits = M > 1u ? 32 - __clz((int)(M - 1u)) : 0;
    return (max(bits, 2) + 1) >> 1;
}

// six round keys: words 0 1 2 3 of the counter (0, c1, c2, c3) and words 0 1 of (1, c1, c2, c3)
__device__ __forceinline__ void ragged_keys(unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned key[8]) {
    philox4x32_10(0u, c1, c2, c3, k0, k1, key);
    philox4x32_10(1u, c1, c2, c3, k0, k1, key + 4);
}

// columns col0 .. col0 + 3 take the points pi((col0 + i) mod M) of the shape [lo, lo + M), M >= 1, pi the keyed Feistel permutation of [0, M)
__device__ __forceinline__ void ragged_perm4(const RaggedRef &r, long long lo, unsigned M, unsigned col0, int cols, const unsigned key[8],
                                             float v[12]) {
    const int h = ragged_half_bits(M);
    unsigned at = col0 % M;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned x = i < cols ? at : 0u;                         // (< M: inside the domain, and on a cycle that comes back below M)
        do x = feistel_pass(x, h, key); while (x >= M);
        const float *pt = r.points + (size_t)(lo + (long long)x) * 3;   // lo + x < lo + M <= T
        v[3 * i] = pt[0], v[3 * i + 1] = pt[1], v[3 * i + 2] = pt[2];
        at = at + 1u == M ? 0u : at + 1u;
    }
}

struct RaggedFeedArgs {
    int S, len[4];                                               // r1 r2 r3 N
    int g[6];                                                    // as FeedArgs::g
    int groups;
    int vec;                                                     // bit k: output k takes 16-byte stores
    RaggedRef set;
    const int *order;
    long long first;
    unsigned k0, k1, t_lo, t_hi24;
    unsigned row0;
    float sigma;
    float *p[4];
    float *z[2];
};

__global__ __launch_bounds__(FEED_THREADS) void feed_batch_ragged_kernel(RaggedFeedArgs a) {
    const int q = blockIdx.x * FEED_THREADS + threadIdx.x;       // the group of row b this thread owns
    const int b = blockIdx.y;
    if (q >= a.groups) return;
    const unsigned row = a.row0 + (unsigned)b;
    if (q >= a.g[4]) {                                           // ---- noise: pdgn_feed_batch's
        const int which = q >= a.g[5];
        feed_noise_group(q - a.g[4 + which], which, b, row, a.t_lo, a.t_hi24, a.k0, a.k1, a.sigma, a.z[which]);
        return;
    }
    const int c = min(max(a.order[a.first + b], 0), a.S - 1);    // (clamped as feed_batch_kernel clamps)
    long long lo;
    unsigned M;
    ragged_range(a.set, c, lo, M);
    const int k = (q >= a.g[1]) + (q >= a.g[2]) + (q >= a.g[3]);
    const int j = q - a.g[k];
    const int r = a.len[k];
    const int cols = min(4, r - 4 * j);
    float v[12];
    if (M == 0u) {                                               // (a table CloudSet refuses: the row is zeros, nothing is read)
#pragma unroll
        for (int i = 0; i < 12; ++i) v[i] = 0.f;
    } else if (k == 3) {                                         // ---- columns 4j .. 4j+3 of p4: the points pi(4j mod M) ..
        unsigned key[8];
        ragged_keys(row, a.t_lo, FEED_TAG_PERM | (a.t_hi24 << 8), a.k0, a.k1, key);
        ragged_perm4(a.set, lo, M, (unsigned)(4 * j), cols, key, v);
    } else {                                                     // ---- a sub-resolution: i = umulhi(word, M), with replacement from the whole shape
        unsigned w[4];
        philox4x32_10((unsigned)j, row, a.t_lo, (unsigned)k | (a.t_hi24 << 8), a.k0, a.k1, w);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float *pt = a.set.points + (size_t)(lo + (long long)__umulhi(w[i], M)) * 3;
            v[3 * i] = pt[0], v[3 * i + 1] = pt[1], v[3 * i + 2] = pt[2];
        }
    }
    float *dst = a.p[k] + (size_t)b * 3 * r + 4 * j;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        store4(dst + (size_t)ch * r, cols, (a.vec >> k) & 1, v[ch], v[3 + ch], v[6 + ch], v[9 + ch]);
}

struct RaggedSampleArgs {
    int S, n, groups, vec;
    RaggedRef set;
    unsigned k0, k1, d_lo, d_hi24;
    float *out;
};

__global__ __launch_bounds__(FEED_THREADS) void sample_ragged_kernel(RaggedSampleArgs a) {
    const int j = blockIdx.x * FEED_THREADS + threadIdx.x;       // columns 4j .. 4j+3
    if (j >= a.groups) return;
    const int cols = min(4, a.n - 4 * j);
    for (int s = blockIdx.y; s < a.S; s += gridDim.y) {
        long long lo;
        unsigned M;
        ragged_range(a.set, s, lo, M);
        float v[12];
        if (M == 0u) {
#pragma unroll
            for (int i = 0; i < 12; ++i) v[i] = 0.f;
        } else {
            unsigned key[8];
            ragged_keys((unsigned)s, a.d_lo, FEED_TAG_RAGGED | (a.d_hi24 << 8), a.k0, a.k1, key);
            ragged_perm4(a.set, lo, M, (unsigned)(4 * j), cols, key, v);
        }
        float *dst = a.out + ((size_t)s * a.n + (size_t)4 * j) * 3;                           // 48 contiguous bytes
        if (a.vec) {                                             // (n a multiple of 4 and the base 16-byte aligned: so is every group)
            float4 *d4 = reinterpret_cast<float4 *>(dst);
            d4[0] = make_float4(v[0], v[1], v[2], v[3]), d4[1] = make_float4(v[4], v[5], v[6], v[7]), d4[2] = make_float4(v[8], v[9], v[10], v[11]);
        } else {
#pragma unroll
            for (int i = 0; i < 12; ++i)
                if (i < 3 * cols) dst[i] = v[i];
        }
    }
}

// what both ragged entry points refuse of the set itself.  T <= 2^31 - 1: a shape's count, the domain of its permutation and the operand of
// the multiply-high, is one 31-bit number; the offsets into points, 3 (lo + x), are 64-bit, so 3 T itself has no bound of its own
static bool ragged_invalid(int S, const float *points, const long long *off, long long T, RaggedRef &r) {
    if (S < 1 || !points || !off) return true;
    if (((uintptr_t)points & 3) || ((uintptr_t)off & 7)) return true;
    if (T < 1 || T > 0x7fffffffLL) return true;
    r.points = points, r.off = off, r.T = T;
    return false;
}

extern "C" int pdgn_feed_batch_ragged(int B, int S, int N, int r1, int r2, int r3, const float *points, const long long *off, long long T,
                                      const int32_t *order, long long first, unsigned long long seed, unsigned long long t, long long row0,
                                      float sigma, float *p1, float *p2, float *p3, float *p4, float *z1, float *z2, pdgn_stream_t stream) {
    RaggedFeedArgs a;
    if (feed_args_invalid(B, S, N, r1, r2, r3, order, first, row0, p1, p2, p3, p4, z1, z2)) return PDGN_ERR_INVALID;
    if (ragged_invalid(S, points, off, T, a.set)) return PDGN_ERR_INVALID;
    a.S = S;
    const int len[4] = {r1, r2, r3, N};
    float *const out[4] = {p1, p2, p3, p4};
    int at = 0;
    a.vec = 0;
    for (int k = 0; k < 4; ++k) {
        a.len[k] = len[k], a.g[k] = at, a.p[k] = out[k];
        at += (len[k] + 3) / 4;
        if (len[k] % 4 == 0 && !((uintptr_t)out[k] & 15)) a.vec |= 1 << k;
    }
    a.g[4] = at, a.g[5] = at + FEED_NOISE_DIM / 4;
    a.groups = at + 2 * (FEED_NOISE_DIM / 4);
    a.order = order, a.first = first;
    a.k0 = (unsigned)seed, a.k1 = (unsigned)(seed >> 32);
    a.t_lo = (unsigned)t, a.t_hi24 = (unsigned)(t >> 32) & 0xffffffu;
    a.row0 = (unsigned)row0;
    a.sigma = sigma;
    a.z[0] = z1, a.z[1] = z2;
    hipLaunchKernelGGL(feed_batch_ragged_kernel, dim3(cdiv(a.groups, FEED_THREADS), B), dim3(FEED_THREADS), 0, (hipStream_t)stream, a);
    return pdgn_launch_status();
}

extern "C" int pdgn_sample_ragged(int S, int n, const float *points, const long long *off, long long T, unsigned long long seed,
                                  unsigned long long draw, float *out, pdgn_stream_t stream) {
    RaggedSampleArgs a;
    if (ragged_invalid(S, points, off, T, a.set)) return PDGN_ERR_INVALID;
    if (n < 1 || n > 0x7fffff00 || !out || ((uintptr_t)out & 3)) return PDGN_ERR_INVALID;
    a.S = S, a.n = n, a.groups = (n + 3) / 4;
    a.vec = n % 4 == 0 && !((uintptr_t)out & 15);
    a.k0 = (unsigned)seed, a.k1 = (unsigned)(seed >> 32);
    a.d_lo = (unsigned)draw, a.d_hi24 = (unsigned)(draw >> 32) & 0xffffffu;
    a.out = out;
    hipLaunchKernelGGL(sample_ragged_kernel, dim3(cdiv(a.groups, FEED_THREADS), min(S, 65535)), dim3(FEED_THREADS), 0, (hipStream_t)stream, a);
    return pdgn_launch_status();
}
