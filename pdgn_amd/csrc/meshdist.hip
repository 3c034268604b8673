// meshdist.hip -- point-to-surface distance: pdgn_mesh_dist_prepare writes a mesh set's faces as records with the boxes of their groups,
// pdgn_point_mesh_distance finds, for every point of a cloud, the closest point of the live faces of one shape (include/pdgn_hip.h;
// DESIGN.md section 7t; the metric is PU-Net's P2F, Yu et al. 2018).  No inline assembly, no float atomics, plain vector stores, nothing
// allocated.
//
// THE RESULT.  Per point p, over the live faces f of the shape: the lexicographic minimum of (d2_f, f), f the face's index in the caller's
// array -- as one unsigned compare on key = bits(d2_f) << 32 | f (d2_f is a sum of squares: never negative, never -0).  A NaN d2_f never
// wins (a candidate is taken only where d2_f == d2_f and its key is below the best key, which starts at 2^64 - 1).  A point with a
// non-finite coordinate, and a point for which no face was taken, gives d2 = NaN (0x7FC00000), face = -1, closest = NaN.  The minimum of a
// set does not depend on the order of its members: slot order, chunking, culling and launch geometry change no bit.
//
// NORMATIVE ORDER of d2_f and its closest point q_f (tests/p2m_mirror.py restates it in numpy; every fp32 operation below is one rounding --
// __fadd_rn / __fsub_rn / __fmul_rn / __fdiv_rn -- nothing contracted; dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z: dot3_rn of csrc/common.h, as in
// csrc/normals.hip and csrc/reconstruct.hip; cross(u, v) = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x), two products and one
// difference each).
// CLAMPS are fminf(fmaxf(x, lo), hi): fmaxf / fminf return the other operand where one is NaN (the mirror: np.fmax / np.fmin, never
// np.maximum), so a clamped value is never NaN where lo and hi are finite.
//     face (a, b, c);  lo = min(min(a, b), c),  hi = max(max(a, b), c) per component
//     for the edges (s, e) = (a, b), (b, c), (c, a), k = 0, 1, 2:
//         u_k = e - s,  w_k = p - s
//         t = dot3(w_k, u_k) / dot3(u_k, u_k),  t = clamp(t, 0, 1)
//         q = s + u_k * t,  q = clamp(q, lo, hi) per component
//         d = p - q,  d2 = dot3(d, d)
//         k = 0 sets (best d2, best q); k = 1, 2 replace them where d2 < best d2            (the first edge wins ties)
//     plane:  n = cross(u_0, c - a),  nn = dot3(n, n)
//         counts = nn > 0  and  dot3(n, cross(u_k, w_k)) >= 0 for k = 0, 1, 2               (a NaN fails its comparison)
//         r = p - (best q of the edges),  h = dot3(n, r) / nn,  q = p - n * h,  q = clamp(q, lo, hi),  d = p - q,  d2 = dot3(d, d)
//         where it counts and d2 < best d2 it replaces them
// Why this form and not the barycentric region walk (Ericson, Real-Time Collision Detection 5.1.5) in fp32: on slivers the region tests
// of that routine are differences of nearly equal products and pick a far vertex; here every candidate is a point of the face's box and a
// wrong "counts" costs at most the gap between the plane candidate and the nearest edge (DESIGN.md section 7t has the measured errors).
//
// RECORDS and THE WALK: csrc/meshrec.h, which csrc/winding.hip shares.  The distance kernel adds the boxes of the groups to the walk: thread
// t < 4 stages the box of group t of the chunk beside the records, and the three levels of culling below decide what is visited.
//
// CULLING, exact under rounding (the pattern of imls_skips in csrc/reconstruct.hip).  For a box [flo, fhi] that holds the boxes of a set
// of faces and a box [plo, phi] that holds a set of points:
//     m_a = max(max(flo_a - phi_a, plo_a - fhi_a), 0),   LB = dot3(m, m)
//   * every q_f is clamped into its face's box, so flo_a <= q_a <= fhi_a, and plo_a <= p_a <= phi_a;
//   * a correctly rounded subtraction is monotone in either operand and odd, so |p_a - q_a| rounded is at least m_a, each difference
//     rounded the same way;
//   * products and sums of non-negative numbers, rounded, are monotone: d2_f = dot3(d, d) >= dot3(m, m) = LB for every face of the set and
//     every point of the box.  Overflow keeps the chain (inf is the largest value; the boxes of live faces and live points are finite, an
//     empty box is (+inf, -inf) and gives LB = +inf without an inf - inf).
// A set is left out where LB > best, STRICTLY: on equality a face of a lower index could still win the tie.  Three levels use it: a group
// against the wave's point box and the largest best of its live lanes (recomputed per group), a face against the same, and in the walk a
// face against the lane's own point and best.  A lane without a live point carries best = -1, so it takes no part and is never evaluated.
// cull = 0 visits every live face at every point.
#include "meshrec.h"

#define MD_MAX_BLOCKS (1 << 23)                                  // workgroups per launch: 2^31 threads

__device__ __forceinline__ float md_clamp(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

__device__ __forceinline__ float md_min3(float a, float b, float c) { return fminf(fminf(a, b), c); }
__device__ __forceinline__ float md_max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

__device__ __forceinline__ float md_wave_min(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, PDGN_WAVE));
    return v;
}

__device__ __forceinline__ float md_wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, PDGN_WAVE));
    return v;
}

// CULLING above: the lower bound of d2_f between the boxes [flo, fhi] and [plo, phi]
__device__ __forceinline__ float md_lower(float flx, float fly, float flz, float fhx, float fhy, float fhz, float plx, float ply, float plz,
                                          float phx, float phy, float phz) {
    const float mx = fmaxf(fmaxf(__fsub_rn(flx, phx), __fsub_rn(plx, fhx)), 0.f);
    const float my = fmaxf(fmaxf(__fsub_rn(fly, phy), __fsub_rn(ply, fhy)), 0.f);
    const float mz = fmaxf(fmaxf(__fsub_rn(flz, phz), __fsub_rn(plz, fhz)), 0.f);
    return dot3_rn(mx, my, mz, mx, my, mz);
}

__device__ __forceinline__ MdVec md_clampv(MdVec q, MdVec lo, MdVec hi) {
    return {md_clamp(q.x, lo.x, hi.x), md_clamp(q.y, lo.y, hi.y), md_clamp(q.z, lo.z, hi.z)};
}

// one edge of NORMATIVE ORDER: its candidate (d2, q) from u = e - s and w = p - s
__device__ __forceinline__ float md_edge(MdVec p, MdVec s, MdVec u, MdVec w, MdVec lo, MdVec hi, MdVec &q) {
    const float t = md_clamp(__fdiv_rn(md_dotv(w, u), md_dotv(u, u)), 0.f, 1.f);
    q = {__fadd_rn(s.x, __fmul_rn(u.x, t)), __fadd_rn(s.y, __fmul_rn(u.y, t)), __fadd_rn(s.z, __fmul_rn(u.z, t))};
    q = md_clampv(q, lo, hi);
    const MdVec d = md_sub(p, q);
    return md_dotv(d, d);
}

// NORMATIVE ORDER: d2_f and q_f of the face (a, b, c) with the box [lo, hi]
__device__ __forceinline__ float md_face(MdVec p, MdVec a, MdVec b, MdVec c, MdVec lo, MdVec hi, MdVec &best_q) {
    const MdVec u0 = md_sub(b, a), u1 = md_sub(c, b), u2 = md_sub(a, c);
    const MdVec w0 = md_sub(p, a), w1 = md_sub(p, b), w2 = md_sub(p, c);
    MdVec q;
    float best = md_edge(p, a, u0, w0, lo, hi, best_q);
    float d2 = md_edge(p, b, u1, w1, lo, hi, q);
    if (d2 < best) best = d2, best_q = q;
    d2 = md_edge(p, c, u2, w2, lo, hi, q);
    if (d2 < best) best = d2, best_q = q;
    const MdVec n = md_cross(u0, md_sub(c, a));
    const float nn = md_dotv(n, n);
    const bool counts = nn > 0.f && md_dotv(n, md_cross(u0, w0)) >= 0.f && md_dotv(n, md_cross(u1, w1)) >= 0.f &&
                        md_dotv(n, md_cross(u2, w2)) >= 0.f;
    const float h = __fdiv_rn(md_dotv(n, md_sub(p, best_q)), nn);
    q = {__fsub_rn(p.x, __fmul_rn(n.x, h)), __fsub_rn(p.y, __fmul_rn(n.y, h)), __fsub_rn(p.z, __fmul_rn(n.z, h))};
    q = md_clampv(q, lo, hi);
    const MdVec d = md_sub(p, q);
    d2 = md_dotv(d, d);
    if (counts && d2 < best) best = d2, best_q = q;
    return best;
}

// RECORDS above.  One wave per group.
__global__ __launch_bounds__(MESHREC_THREADS) void md_prepare_kernel(int S, int V, int F, int G, const float *__restrict__ verts,
                                                                const int32_t *__restrict__ faces, const int32_t *__restrict__ face_off,
                                                                const int32_t *__restrict__ group_off, const int32_t *__restrict__ live,
                                                                const int32_t *__restrict__ order, float4 *__restrict__ rec,
                                                                float4 *__restrict__ grp) {
    const int lane = threadIdx.x & (PDGN_WAVE - 1);
    const int g = blockIdx.x * (MESHREC_THREADS / PDGN_WAVE) + (threadIdx.x >> 6);
    if (g >= G) return;                                            // (uniform per wave; no barrier in this kernel)
    int lo = 0, hi = S - 1;                                        // the shape whose groups hold g: the first s with group_off[s + 1] > g
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (group_off[mid + 1] > g) hi = mid;
        else lo = mid + 1;
    }
    const int s = lo;
    const long long slot = (long long)face_off[s] + (long long)(g - group_off[s]) * MESHREC_GROUP + lane;
    const bool in = slot >= face_off[s] && slot < face_off[s + 1] && slot < F;
    const float inf = __builtin_inff();
    float blx = inf, bly = inf, blz = inf, bhx = -inf, bhy = -inf, bhz = -inf;
    if (in) {
        const int f = order ? order[slot] : (int)slot;
        bool ok = f >= 0 && f < F;
        int ia = 0, ib = 0, ic = 0;
        if (ok) {
            ia = faces[(size_t)f * 3], ib = faces[(size_t)f * 3 + 1], ic = faces[(size_t)f * 3 + 2];
            ok = live[f] != 0 && ia >= 0 && ia < V && ib >= 0 && ib < V && ic >= 0 && ic < V;
        }
        float4 a = make_float4(0.f, 0.f, 0.f, __int_as_float(-1)), b = make_float4(0.f, 0.f, 0.f, 0.f), c = b;
        if (ok) {
            a = make_float4(verts[(size_t)ia * 3], verts[(size_t)ia * 3 + 1], verts[(size_t)ia * 3 + 2], __int_as_float(f));
            b = make_float4(verts[(size_t)ib * 3], verts[(size_t)ib * 3 + 1], verts[(size_t)ib * 3 + 2], 0.f);
            c = make_float4(verts[(size_t)ic * 3], verts[(size_t)ic * 3 + 1], verts[(size_t)ic * 3 + 2], 0.f);
            blx = md_min3(a.x, b.x, c.x), bly = md_min3(a.y, b.y, c.y), blz = md_min3(a.z, b.z, c.z);
            bhx = md_max3(a.x, b.x, c.x), bhy = md_max3(a.y, b.y, c.y), bhz = md_max3(a.z, b.z, c.z);
        }
        rec[slot * 3] = a, rec[slot * 3 + 1] = b, rec[slot * 3 + 2] = c;
    }
    blx = md_wave_min(blx), bly = md_wave_min(bly), blz = md_wave_min(blz);
    bhx = md_wave_max(bhx), bhy = md_wave_max(bhy), bhz = md_wave_max(bhz);
    if (lane == 0) grp[(size_t)g * 2] = make_float4(blx, bly, blz, 0.f), grp[(size_t)g * 2 + 1] = make_float4(bhx, bhy, bhz, 0.f);
}

__global__ __launch_bounds__(MESHREC_THREADS) void md_distance_kernel(int n, int S, int F, int G, int runs, const float *__restrict__ xyz,
                                                                      const int32_t *__restrict__ shape,
                                                                      const int32_t *__restrict__ face_off,
                                                                      const int32_t *__restrict__ group_off,
                                                                      const float4 *__restrict__ rec, const float4 *__restrict__ grp,
                                                                      int cull, float *__restrict__ out_d2,
                                                                      int32_t *__restrict__ out_face, float *__restrict__ out_q) {
    __shared__ float4 s_rec[3 * MESHREC_CHUNK];
    __shared__ float4 s_grp[2 * (MESHREC_CHUNK / MESHREC_GROUP)];
    const int tid = threadIdx.x, lane = tid & (PDGN_WAVE - 1);
    const int c = blockIdx.x / runs, i = (blockIdx.x % runs) * MESHREC_THREADS + tid;
    const bool mine = i < n;
    const float inf = __builtin_inff(), nan = __uint_as_float(MESHREC_NAN_BITS);
    const MdVec p = meshrec_point(xyz, c, n, i);
    const bool live = mine && isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
    const MeshrecRange r = meshrec_range<true>(shape, face_off, group_off, c, S, F);
    const int f0 = r.f0, g0 = r.g0, slots = r.f1 - r.f0;
    // the box of the wave's live points
    const float plx = md_wave_min(live ? p.x : inf), ply = md_wave_min(live ? p.y : inf), plz = md_wave_min(live ? p.z : inf);
    const float phx = md_wave_max(live ? p.x : -inf), phy = md_wave_max(live ? p.y : -inf), phz = md_wave_max(live ? p.z : -inf);
    unsigned long long key = ~0ULL;
    float best = live ? inf : -1.f;
    MdVec best_q = {nan, nan, nan};
    for (int j0 = 0; j0 < slots; j0 += MESHREC_CHUNK) {
        const int cnt = min(MESHREC_CHUNK, slots - j0);
        if (j0) __syncthreads();                                   // everyone is done reading the previous chunk
        meshrec_stage(rec, f0 + j0, cnt, s_rec);
        if (tid < MESHREC_CHUNK / MESHREC_GROUP) {
            const long long g = (long long)g0 + j0 / MESHREC_GROUP + tid;
            float4 glo = make_float4(inf, inf, inf, 0.f), ghi = make_float4(-inf, -inf, -inf, 0.f);
            if (tid * MESHREC_GROUP < cnt && g < G) glo = grp[g * 2], ghi = grp[g * 2 + 1];
            s_grp[2 * tid] = glo, s_grp[2 * tid + 1] = ghi;
        }
        __syncthreads();
        for (int s0 = 0; s0 < cnt; s0 += MESHREC_GROUP) {
            float wmax = 0.f;
            if (cull) {
                wmax = md_wave_max(best);
                const float4 glo = s_grp[2 * (s0 / MESHREC_GROUP)], ghi = s_grp[2 * (s0 / MESHREC_GROUP) + 1];
                if (md_lower(glo.x, glo.y, glo.z, ghi.x, ghi.y, ghi.z, plx, ply, plz, phx, phy, phz) > wmax) continue;      // (uniform)
            }
            const float4 ra = s_rec[3 * (s0 + lane)];               // (s0 + lane < MESHREC_CHUNK: a staged record, dead past cnt)
            bool visit = meshrec_face(ra) >= 0;
            if (cull && visit) {
                const float4 rb = s_rec[3 * (s0 + lane) + 1], rc = s_rec[3 * (s0 + lane) + 2];
                visit = !(md_lower(md_min3(ra.x, rb.x, rc.x), md_min3(ra.y, rb.y, rc.y), md_min3(ra.z, rb.z, rc.z), md_max3(ra.x, rb.x, rc.x),
                                   md_max3(ra.y, rb.y, rc.y), md_max3(ra.z, rb.z, rc.z), plx, ply, plz, phx, phy, phz) > wmax);
            }
            unsigned long long todo = __ballot(visit);             // meshrec_walk's loop, spelled out (csrc/meshrec.h says why)
            while (todo) {
                const int jj = s0 + __builtin_ctzll(todo);         // uniform: the lowest slot still to visit
                todo &= todo - 1;
                const float4 fa = s_rec[3 * jj], fb = s_rec[3 * jj + 1], fc = s_rec[3 * jj + 2];
                const MdVec a = {fa.x, fa.y, fa.z}, b = {fb.x, fb.y, fb.z}, cc = {fc.x, fc.y, fc.z};
                const MdVec lo = {md_min3(a.x, b.x, cc.x), md_min3(a.y, b.y, cc.y), md_min3(a.z, b.z, cc.z)};
                const MdVec hi = {md_max3(a.x, b.x, cc.x), md_max3(a.y, b.y, cc.y), md_max3(a.z, b.z, cc.z)};
                if (cull && md_lower(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, p.x, p.y, p.z, p.x, p.y, p.z) > best) continue;
                MdVec q;
                const float d2 = md_face(p, a, b, cc, lo, hi, q);
                const unsigned long long k = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)meshrec_face(fa);
                if (d2 == d2 && k < key) key = k, best = d2, best_q = q;
            }
        }
    }
    if (mine) {
        const bool found = live && key != ~0ULL;
        const size_t at = (size_t)c * n + i;
        out_d2[at] = found ? best : nan;
        out_face[at] = found ? (int32_t)(key & 0xFFFFFFFFu) : -1;
        if (out_q) {
            out_q[at * 3] = found ? best_q.x : nan;
            out_q[at * 3 + 1] = found ? best_q.y : nan;
            out_q[at * 3 + 2] = found ? best_q.z : nan;
        }
    }
}

// ---------------------------------------------------------------------------- entry points (host-side checks only before any launch)
static bool md_mesh_ok(int S, int F, int G) {
    return S >= 1 && F >= 1 && G >= 1 && 3LL * F < (1LL << 31) && (long long)G <= (long long)F / MESHREC_GROUP + S;
}

extern "C" int pdgn_mesh_dist_group(void) { return MESHREC_GROUP; }

extern "C" int pdgn_mesh_dist_chunk(void) { return MESHREC_CHUNK; }

extern "C" long long pdgn_mesh_dist_workspace_floats(int S, int F) {
    if (S < 1 || F < 1 || 3LL * F >= (1LL << 31)) return PDGN_ERR_INVALID;
    return 12LL * F + 8LL * ((long long)F / MESHREC_GROUP + S);
}

extern "C" int pdgn_mesh_dist_prepare(int S, int V, int F, int G, const float *verts, const int32_t *faces, const int32_t *face_off,
                                      const int32_t *group_off, const int32_t *live, const int32_t *order, float *records, float *groups,
                                      pdgn_stream_t stream) {
    if (!md_mesh_ok(S, F, G) || V < 1 || 3LL * V >= (1LL << 31)) return PDGN_ERR_INVALID;
    if (!verts || !faces || !face_off || !group_off || !live || !records || !groups) return PDGN_ERR_INVALID;
    if (!pdgn_aligned(verts, 4) || !pdgn_aligned(faces, 4) || !pdgn_aligned(face_off, 4) || !pdgn_aligned(group_off, 4) || !pdgn_aligned(live, 4) ||
        !pdgn_aligned(order, 4) || !pdgn_aligned(records, 16) || !pdgn_aligned(groups, 16))
        return PDGN_ERR_INVALID;
    hipLaunchKernelGGL(md_prepare_kernel, dim3(cdiv(G, MESHREC_THREADS / PDGN_WAVE)), dim3(MESHREC_THREADS), 0, (hipStream_t)stream, S, V, F, G, verts,
                       faces, face_off, group_off, live, order, (float4 *)records, (float4 *)groups);
    return pdgn_launch_status();
}

extern "C" int pdgn_point_mesh_distance(int b, int n, int S, int F, int G, const float *xyz, const int32_t *shape, const int32_t *face_off,
                                        const int32_t *group_off, const float *records, const float *groups, int cull, float *d2,
                                        int32_t *face, float *closest, pdgn_stream_t stream) {
    if (!md_mesh_ok(S, F, G) || b < 1 || n < 1 || (long long)b * n >= (1LL << 31) || cull < 0 || cull > 1) return PDGN_ERR_INVALID;
    if ((long long)b * cdiv(n, MESHREC_THREADS) > MD_MAX_BLOCKS) return PDGN_ERR_INVALID;
    if (!xyz || !shape || !face_off || !group_off || !records || !groups || !d2 || !face) return PDGN_ERR_INVALID;
    if (!pdgn_aligned(xyz, 4) || !pdgn_aligned(shape, 4) || !pdgn_aligned(face_off, 4) || !pdgn_aligned(group_off, 4) || !pdgn_aligned(records, 16) ||
        !pdgn_aligned(groups, 16) || !pdgn_aligned(d2, 4) || !pdgn_aligned(face, 4) || !pdgn_aligned(closest, 4))
        return PDGN_ERR_INVALID;
    const int runs = cdiv(n, MESHREC_THREADS);
    hipLaunchKernelGGL(md_distance_kernel, dim3((unsigned)((long long)b * runs)), dim3(MESHREC_THREADS), 0, (hipStream_t)stream, n, S, F, G, runs,
                       xyz, shape, face_off, group_off, (const float4 *)records, (const float4 *)groups, cull, d2, face, closest);
    return pdgn_launch_status();
}
