// winding.hip -- generalized winding numbers (Jacobson, Kavan, Sorkine-Hornung 2013): pdgn_winding_number sums, for every point of a cloud,
// the solid angles that the live faces of one shape subtend at it, over 4 pi: 1 inside a closed, consistently oriented surface, 0 outside
// (include/pdgn_hip.h).  The faces are the records of pdgn_mesh_dist_prepare (csrc/meshrec.h), unchanged.  No
// inline assembly, no atomics of any kind, plain vector stores, nothing allocated.
//
// THE RESULT.  Per point p, over the live faces f of the shape:
//     T = sum of t_f as int64,   t_f = llrint((double)h_f * 2^32),   h_f half the signed solid angle of face f at p, in [-pi, pi]
//     w = (float)((double)T * K),   K = 0x1.45f306dc9c883p-35, the double nearest 1 / (2^33 pi)
//     inside = T >= T_HALF,   T_HALF = 13493037705 = llrint(pi 2^32):  w >= 1/2 as an integer comparison
// A point with a non-finite coordinate, and a point for which any face gave a non-finite h_f, gives T = INT64_MIN, w = NaN (0x7FC00000),
// inside = 0: "bad" is an OR over the faces.  A shape with no live face gives T = 0, w = 0.  A sum of integers and an OR do not depend on
// the order of their members: slot order, chunking, the split of a shape's chunks over workgroups, point order and launch geometry change
// no bit.  |t_f| <= pi 2^32 < 2^34, so a shape may have up to 2^28 faces before a partial sum could reach 2^62.
//
// NORMATIVE ORDER of h_f (tests/winding_mirror.py restates it in numpy; every fp32 operation below is one rounding -- __fadd_rn / __fsub_rn /
// __fmul_rn / __fdiv_rn, and sqrtf for the roots: the correctly rounded one, never __fsqrt_rn, see csrc/auction.hip -- nothing contracted;
// dot3 and cross exactly as in csrc/meshdist.hip).  The van Oosterom-Strackee formula (1983):
//     face (a, b, c);  A = a - p,  B = b - p,  C = c - p
//     la = sqrt(dot3(A, A)),  lb = sqrt(dot3(B, B)),  lc = sqrt(dot3(C, C))
//     num = dot3(A, cross(B, C))
//     den = ((la * lb) * lc + dot3(A, B) * lc) + (dot3(B, C) * la + dot3(C, A) * lb)
//     h = natan2(num, den)
// natan2(y, x), fp32 (the reduction and the polynomial are those of Cephes' atanf, Moshier 1992; PI = 0x40490FDB, PI_2 = 0x3FC90FDB,
// PI_4 = 0x3F490FDB, TAN_PI_8 = 0x3ED413CD as bit patterns):
//     ax = |x|, ay = |y|;  mx = fmaxf(ax, ay), mn = fminf(ax, ay);  r = mn / mx                                  (in [0, 1])
//     big = r > TAN_PI_8;  z = big ? (r - 1) / (r + 1) : r                                                        (|z| <= tan(pi / 8))
//     zz = z * z
//     q = ((8.05374449538e-2f * zz + -1.38776856032e-1f) * zz + 1.99777106478e-1f) * zz + -3.33329491539e-1f
//     v = (q * zz) * z + z;   if big: v = PI_4 + v
//     if ay > ax: v = PI_2 - v;   if x < 0: v = PI - v;   if y < 0: v = -v
//     if y == 0: v = 0            (whatever x is: a point on a face's plane or at a vertex, and a degenerate face, take the mean of both
//                                  sides -- the term is exactly 0 and the sign of a zero never matters)
//     if x or y is NaN: v = NaN   (0x7FC00000; and r = inf / inf is NaN by itself: coordinates whose products overflow mark the point bad)
// Its largest error against float64 arctan2 is 1.13 * 2^-22 over the sweeps of tests/test_winding_host.py (numpy's float32 arctan2: 1.32).
//
// SHAPE OF THE LAUNCH.  THE WALK of csrc/meshrec.h, with one thing added: a workgroup owns a run of 256 points of one cloud and one PART
// of the shape's chunks.  With nchunks of them and `parts` parts, part k owns the chunks [k nchunks / parts, (k + 1) nchunks / parts) --
// possibly none.  Nothing can be culled: every live face is evaluated at every point.
//   parts = 1: the workgroup writes T, w and inside itself.  One launch.
//   parts > 1: it writes its partial sum (INT64_MIN where bad -- no sum of fewer than 2^28 terms reaches it) to workspace[part][point], and a
//   second launch of one thread per point adds the parts and writes T, w and inside.  Every workspace entry is written by exactly one
//   workgroup before it is read, so nothing is zeroed beforehand and there are no atomics.
#include "meshrec.h"

#define WN_THREADS MESHREC_THREADS                               // (wn_finish_kernel's too)
#define WN_MAX_BLOCKS (1 << 23)                                  // workgroups per launch: 2^31 threads
#define WN_MAX_FACES (1 << 28)
#define WN_MAX_SPLITS 4096
#define WN_TARGET_BLOCKS 2048                                    // splits = 0: eight workgroups for each of the 256 CUs, every SIMD full
#define WN_T_HALF 13493037705LL                                  // llrint(pi 2^32)
#define WN_T_BAD INT64_MIN
#define WN_K 0x1.45f306dc9c883p-35                               // the double nearest 1 / (2^33 pi)

// NORMATIVE ORDER: natan2
__device__ __forceinline__ float wn_atan2(float y, float x) {
    const float PI = __uint_as_float(0x40490FDBu), PI_2 = __uint_as_float(0x3FC90FDBu), PI_4 = __uint_as_float(0x3F490FDBu);
    const float TAN_PI_8 = __uint_as_float(0x3ED413CDu);
    const float ax = fabsf(x), ay = fabsf(y);
    const float r = __fdiv_rn(fminf(ax, ay), fmaxf(ax, ay));
    const bool big = r > TAN_PI_8;
    const float z = big ? __fdiv_rn(__fsub_rn(r, 1.f), __fadd_rn(r, 1.f)) : r;
    const float zz = __fmul_rn(z, z);
    float q = __fadd_rn(__fmul_rn(8.05374449538e-2f, zz), -1.38776856032e-1f);
    q = __fadd_rn(__fmul_rn(q, zz), 1.99777106478e-1f);
    q = __fadd_rn(__fmul_rn(q, zz), -3.33329491539e-1f);
    float v = __fadd_rn(__fmul_rn(__fmul_rn(q, zz), z), z);
    if (big) v = __fadd_rn(PI_4, v);
    if (ay > ax) v = __fsub_rn(PI_2, v);
    if (x < 0.f) v = __fsub_rn(PI, v);
    if (y < 0.f) v = -v;
    if (y == 0.f) v = 0.f;
    if (x != x || y != y) v = __uint_as_float(MESHREC_NAN_BITS);
    return v;
}

// NORMATIVE ORDER: h_f of the face (a, b, c) at p
// (spelled in scalars: through MdVec and md_sub / md_cross / md_dotv of csrc/meshrec.h, the same operations, the compiler pairs them
// differently into packed instructions and the walk's loop is one instruction in 200 longer, 0.4 % of the kernel's time, measured)
__device__ __forceinline__ float wn_half_angle(float px, float py, float pz, float4 a, float4 b, float4 c) {
    const float Ax = __fsub_rn(a.x, px), Ay = __fsub_rn(a.y, py), Az = __fsub_rn(a.z, pz);
    const float Bx = __fsub_rn(b.x, px), By = __fsub_rn(b.y, py), Bz = __fsub_rn(b.z, pz);
    const float Cx = __fsub_rn(c.x, px), Cy = __fsub_rn(c.y, py), Cz = __fsub_rn(c.z, pz);
    const float la = sqrtf(dot3_rn(Ax, Ay, Az, Ax, Ay, Az)), lb = sqrtf(dot3_rn(Bx, By, Bz, Bx, By, Bz)), lc = sqrtf(dot3_rn(Cx, Cy, Cz, Cx, Cy, Cz));
    const float nx = __fsub_rn(__fmul_rn(By, Cz), __fmul_rn(Bz, Cy)), ny = __fsub_rn(__fmul_rn(Bz, Cx), __fmul_rn(Bx, Cz)),
                nz = __fsub_rn(__fmul_rn(Bx, Cy), __fmul_rn(By, Cx));
    const float num = dot3_rn(Ax, Ay, Az, nx, ny, nz);
    const float ab = dot3_rn(Ax, Ay, Az, Bx, By, Bz), bc = dot3_rn(Bx, By, Bz, Cx, Cy, Cz), ca = dot3_rn(Cx, Cy, Cz, Ax, Ay, Az);
    const float den = __fadd_rn(__fadd_rn(__fmul_rn(__fmul_rn(la, lb), lc), __fmul_rn(ab, lc)), __fadd_rn(__fmul_rn(bc, la), __fmul_rn(ca, lb)));
    return wn_atan2(num, den);
}

// THE RESULT: w and inside from T
__device__ __forceinline__ void wn_store(long long T, size_t at, long long *__restrict__ out_T, float *__restrict__ out_w,
                                         int32_t *__restrict__ out_in) {
    out_T[at] = T;
    out_w[at] = T == WN_T_BAD ? __uint_as_float(MESHREC_NAN_BITS) : (float)((double)T * WN_K);
    if (out_in) out_in[at] = T >= WN_T_HALF ? 1 : 0;
}

// SHAPE OF THE LAUNCH above.  blockIdx.x = (cloud * runs + run) * parts + part.
__global__ __launch_bounds__(WN_THREADS) void wn_sum_kernel(int n, int S, int F, int runs, int parts, long long total, const float *__restrict__ xyz,
                                                            const int32_t *__restrict__ shape, const int32_t *__restrict__ face_off,
                                                            const float4 *__restrict__ rec, long long *__restrict__ partial,
                                                            long long *__restrict__ out_T, float *__restrict__ out_w,
                                                            int32_t *__restrict__ out_in) {
    __shared__ float4 s_rec[3 * MESHREC_CHUNK];
    const int tid = threadIdx.x, lane = tid & (PDGN_WAVE - 1);
    const int part = blockIdx.x % parts, cr = blockIdx.x / parts;
    const int c = cr / runs, i = (cr % runs) * WN_THREADS + tid;
    const bool mine = i < n;
    const MdVec p = meshrec_point(xyz, c, n, i);
    bool bad = !(isfinite(p.x) && isfinite(p.y) && isfinite(p.z));
    const MeshrecRange r = meshrec_range<false>(shape, face_off, nullptr, c, S, F);
    const int f0 = r.f0, slots = r.f1 - r.f0, nchunks = (slots + MESHREC_CHUNK - 1) / MESHREC_CHUNK;
    const int k0 = (int)((long long)part * nchunks / parts), k1 = (int)((long long)(part + 1) * nchunks / parts);
    long long T = 0;
    for (int k = k0; k < k1; ++k) {
        const int j0 = k * MESHREC_CHUNK, cnt = min(MESHREC_CHUNK, slots - j0);
        if (k > k0) __syncthreads();                               // everyone is done reading the previous chunk
        meshrec_stage(rec, f0 + j0, cnt, s_rec);
        __syncthreads();
        for (int s0 = 0; s0 < cnt; s0 += MESHREC_GROUP) {
            // (s0 + lane < MESHREC_CHUNK: a staged record, dead past cnt)
            meshrec_walk(s_rec, s0, __ballot(meshrec_face(s_rec[3 * (s0 + lane)]) >= 0), [&](const float4 *f) {
                const float h = wn_half_angle(p.x, p.y, p.z, f[0], f[1], f[2]);
                const bool ok = isfinite(h);
                bad |= !ok;
                T += ok ? __double2ll_rn((double)h * 4294967296.0) : 0LL;
            });
        }
    }
    if (mine) {
        const size_t at = (size_t)c * n + i;
        if (bad) T = WN_T_BAD;
        if (parts == 1) wn_store(T, at, out_T, out_w, out_in);
        else partial[(size_t)part * total + at] = T;
    }
}

// parts > 1: one thread per point adds the parts
__global__ __launch_bounds__(WN_THREADS) void wn_finish_kernel(long long total, int parts, const long long *__restrict__ partial,
                                                               long long *__restrict__ out_T, float *__restrict__ out_w,
                                                               int32_t *__restrict__ out_in) {
    const long long at = (long long)blockIdx.x * WN_THREADS + threadIdx.x;
    if (at >= total) return;
    long long T = 0;
    bool bad = false;
    for (int k = 0; k < parts; ++k) {
        const long long t = partial[(size_t)k * total + at];
        bad |= t == WN_T_BAD;
        T += t == WN_T_BAD ? 0LL : t;
    }
    wn_store(bad ? WN_T_BAD : T, (size_t)at, out_T, out_w, out_in);
}

// ---------------------------------------------------------------------------- entry points (host-side checks only before any launch)
static bool wn_sizes_ok(int b, int n, int faces) {
    return b >= 1 && n >= 1 && faces >= 1 && faces <= WN_MAX_FACES && (long long)b * n < (1LL << 31);
}

extern "C" long long pdgn_winding_half_turn(void) { return WN_T_HALF; }

extern "C" int pdgn_winding_splits(int b, int n, int faces) {
    if (!wn_sizes_ok(b, n, faces)) return PDGN_ERR_INVALID;
    const long long blocks = (long long)b * cdiv(n, WN_THREADS), chunks = cdiv(faces, MESHREC_CHUNK);
    long long parts = (WN_TARGET_BLOCKS + blocks - 1) / blocks;
    if (parts > chunks / 2) parts = chunks / 2;                    // a part has at least two chunks: single chunks divide unevenly
    if (parts > WN_MAX_SPLITS) parts = WN_MAX_SPLITS;
    return parts < 1 ? 1 : (int)parts;
}

extern "C" long long pdgn_winding_workspace_bytes(int b, int n, int F, int splits) {
    if (!wn_sizes_ok(b, n, F) || splits < 0 || splits > WN_MAX_SPLITS) return PDGN_ERR_INVALID;
    const int parts = splits ? splits : pdgn_winding_splits(b, n, F);
    return parts > 1 ? 8LL * parts * b * n : 0;
}

extern "C" int pdgn_winding_number(int b, int n, int S, int F, const float *xyz, const int32_t *shape, const int32_t *face_off,
                                   const float *records, int splits, long long *workspace, long long *T, float *w, int32_t *inside,
                                   pdgn_stream_t stream) {
    if (S < 1 || !wn_sizes_ok(b, n, F) || splits < 0 || splits > WN_MAX_SPLITS) return PDGN_ERR_INVALID;
    const int parts = splits ? splits : pdgn_winding_splits(b, n, F);
    const int runs = cdiv(n, WN_THREADS);
    if ((long long)b * runs * parts > WN_MAX_BLOCKS) return PDGN_ERR_INVALID;
    if (!xyz || !shape || !face_off || !records || !T || !w || (parts > 1 && !workspace)) return PDGN_ERR_INVALID;
    if (!pdgn_aligned(xyz, 4) || !pdgn_aligned(shape, 4) || !pdgn_aligned(face_off, 4) || !pdgn_aligned(records, 16) || !pdgn_aligned(workspace, 8) ||
        !pdgn_aligned(T, 8) || !pdgn_aligned(w, 4) || !pdgn_aligned(inside, 4))
        return PDGN_ERR_INVALID;
    hipLaunchKernelGGL(wn_sum_kernel, dim3((unsigned)((long long)b * runs * parts)), dim3(WN_THREADS), 0, (hipStream_t)stream, n, S, F, runs,
                       parts, (long long)b * n, xyz, shape, face_off, (const float4 *)records, workspace, T, w, inside);
    int rc = pdgn_launch_status();
    if (rc || parts == 1) return rc;
    const long long total = (long long)b * n;
    hipLaunchKernelGGL(wn_finish_kernel, dim3((unsigned)cdiv(total, WN_THREADS)), dim3(WN_THREADS), 0, (hipStream_t)stream, total, parts,
                       workspace, T, w, inside);
    return pdgn_launch_status();
}
