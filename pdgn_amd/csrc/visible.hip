// visible.hip -- pdgn_mesh_visibility: which faces of a triangle mesh can be seen from a ring of viewpoints.  Per (shape, view) an
// orthographic depth buffer in LDS and a per-face depth test against it; bit v of mask[f] says that face f passes in view v.  The
// faces whose mask is 0 get weight 0 in the alias table (pdgn_amd/meshes.py), so the feed kernel never draws from them: the surface
// sampled is the one that can be seen.  Runs once per run or once per `pack`.
//
// THE DEFINITION (normative; tests/visible_mirror.py spells the same function in numpy).  Shape c has the frame (centre ctr, radius
// rho); view v has the rows e_x, e_y, e_z; the image is R x R pixels.
//   Snap.   For a vertex p:  d = p - ctr;  x = ((e_x0 d0 + e_x1 d1) + e_x2 d2), y and z likewise with e_y and e_z; every fp32
//           subtraction, product and sum is rounded on its own, never contracted.  With s = R 2^7 (exact in fp32):
//             X = (int) clamp(rint((x / rho) s), -s, s) + s         in [0, 2^8 R]: pixel units with 8 sub-pixel bits
//             Y likewise;   Z = (int) clamp(rint((z / rho) 2^20), -2^20, 2^20) + 2^20      in [0, 2^21]; a smaller Z is nearer the eye
//           (x / rho is the correctly rounded fp32 quotient, rint rounds halves to even, a NaN clamps to the lower end.)  After the snap
//           nothing is floating point.
//   Dead.   A face of zero area in 3D is skipped in both passes: e1 = v1 - v0, e2 = v2 - v0 and n = e1 x e2 (n_x = e1_y e2_z - e1_z e2_y,
//           ...) in fp64, every operation rounded on its own, all three components zero -- the host's face_areas(verts, faces) == 0.  So
//           is a face that names a vertex outside [0, V).
//   Pass 1. Every pixel starts at 0xffffffff.  With edge(A, B, P) = (B.x - A.x)(P.y - A.y) - (B.y - A.y)(P.x - A.x) in int64: A2 =
//           edge(P0, P1, P2); where A2 < 0, P1 and P2 (and their Z) change places and A2 its sign.  A face with A2 != 0 looks at the
//           pixel centres C = ((2 px + 1) 2^7, (2 py + 1) 2^7), 0 <= px, py < R, of its bounding box: C is COVERED when w0 = edge(P1, P2, C),
//           w1 = edge(P2, P0, C) and w2 = edge(P0, P1, C) are all >= 0 (edges inclusive, faces two-sided: no back-face culling); there
//           Zp = floor((w0 Z0 + w1 Z1 + w2 Z2) / A2)  (below 2^55) and  buf[py R + px] = min(buf[py R + px], Zp).
//           A face with A2 = 0, or one that covers no centre, writes nothing: it cannot occlude.
//   Pass 2. After one barrier.  A face that covers centres PASSES when Zp <= buf + PDGN_VISIBLE_BIAS_COVER at any of them.  A face that
//           covers none (edge-on in this view, or smaller than a pixel) is tested once, at the pixel (min(Xc >> 8, R - 1), min(Yc >> 8, R - 1))
//           that holds the integer centroid Xc = floor((X0 + X1 + X2) / 3), Yc likewise, with Zc = floor((Z0 + Z1 + Z2) / 3): it passes when
//           Zc <= buf + pdgn_mesh_visibility_bias_small(R) = floor(3 2^20 / R), where an empty pixel (0xffffffff) lets everything pass.
//           A face that passes ORs 1 << v into mask[f].
// Everything the result depends on is an integer minimum or an integer OR: two runs agree bit for bit and a permutation of a shape's
// faces permutes its masks.
//
// THE KERNEL.  One workgroup of 256 threads per (shape, view), view fastest in the grid, so that the NV workgroups that gather the same
// vertices run next to each other and hit in L2.  The depth buffer is dynamic LDS, 4 R^2 bytes (64 KB at R = 128: two workgroups per
// CU; 144 KB at R = 192: one), beside the sweep's static 1 KB.  The two passes are the same sweep of the shape's faces (csrc/raster.h,
// THE SWEEP: a lane per small face, a wave per large one, the exact division) with atomicMin (ds_min_u32) in the first and a compare in
// the second.
//
// pdgn_mesh_face_votes: WHICH SIDE of a face the views see (tests/face_orient_mirror.py spells it in numpy).  A face
// seen mostly from its back is stored the wrong way round (Takayama et al. 2014, orientation of facets by ray casting).
// THE DEFINITION (normative).  Snap, Dead and Pass 1 are the ones above, word for word: the same depth buffer.
//   Side.   For a live face in view v, S = edge(P0, P1, P2) on the snapped integers in the STORED vertex order, before Pass 1's swap.
//           S < 0: the view sees the FRONT, the side from which the stored vertices run counter-clockwise, the side the normal e1 x e2
//           points to (the view looks along +e_z of a right-handed basis, so such a face has e_z . n < 0 and a negative edge function).
//           S > 0: the view sees the BACK.  S = 0: the face is edge-on in this view and has no vote here.
//   Pass 2. After one barrier.  A face that covers centres counts n = the number of ALL its covered centres with Zp <= buf +
//           PDGN_VISIBLE_BIAS_COVER (no early stop).  A face with S != 0 that covers none counts n = 1 when it passes the fallback test
//           above, else 0.  votes[f][S > 0] += n: column 0 the front, column 1 the back.
//   Mask.   Where mask is given it receives pdgn_mesh_visibility's bits exactly: bit v when n > 0, or when the fallback passes (S = 0
//           included).
// Everything the result depends on is an integer minimum, an integer sum or an OR: two runs agree bit for bit and a permutation of a
// shape's faces permutes its rows.  A count is at most NV R^2 < 2^21: uint32 holds it.
// THE KERNEL is the one above with another second pass (vis_vote_pass): the per-lane counts of a large face are summed over the wave in
// the sweep's fold hook, and one lane per (face, view) adds the face's n to its word with one integer atomicAdd (global_atomic_add_u32,
// no return); the LDS buffer is only read in this pass.  Same grid, same LDS, same occupancy as the visibility kernel.
#include "raster.h"

#define VIS_THREADS RASTER_THREADS
#define VIS_EMPTY 0xffffffffu

struct VisArgs {
    const float *verts;
    const int32_t *faces, *face_off;
    const float *frame, *views;
    uint32_t *mask, *votes;                                      // votes: pdgn_mesh_face_votes' (F,2); there mask may be null
    int V, F, NV, R, bias_small;
};

struct VisView {
    float ex[3], ey[3], ez[3], c[3], rho;
    int R;
};

__device__ __forceinline__ float vis_dot(const float *e, float d0, float d1, float d2) {
    return __fadd_rn(__fadd_rn(__fmul_rn(e[0], d0), __fmul_rn(e[1], d1)), __fmul_rn(e[2], d2));
}

__device__ __forceinline__ int vis_quant(float t, float rho, float s) {
    const float q = rintf(__fmul_rn(t / rho, s));
    return (int)fminf(fmaxf(q, -s), s) + (int)s;                 // (fmaxf drops a NaN: the lower end)
}

__device__ __forceinline__ void vis_snap(const VisView &w, const float *p, int &X, int &Y, int &Z) {
    const float d0 = __fsub_rn(p[0], w.c[0]), d1 = __fsub_rn(p[1], w.c[1]), d2 = __fsub_rn(p[2], w.c[2]);
    const float s = (float)(w.R << 7);
    X = vis_quant(vis_dot(w.ex, d0, d1, d2), w.rho, s);
    Y = vis_quant(vis_dot(w.ey, d0, d1, d2), w.rho, s);
    Z = vis_quant(vis_dot(w.ez, d0, d1, d2), w.rho, 1048576.f);
}

// Gather and snap face f.  False: the face is dead (zero area in 3D, or an index outside the vertices).  side: the sign of S =
// edge(P0, P1, P2) in the stored vertex order, before the set-up's swap (-1: the view sees the front, +1: the back, 0: edge-on).
__device__ __forceinline__ bool vis_load(const VisArgs &a, const VisView &w, int f, RasterFace &t, int &side) {
    const int i0 = a.faces[3 * (size_t)f], i1 = a.faces[3 * (size_t)f + 1], i2 = a.faces[3 * (size_t)f + 2];
    if ((unsigned)i0 >= (unsigned)a.V || (unsigned)i1 >= (unsigned)a.V || (unsigned)i2 >= (unsigned)a.V) return false;
    const float *q0 = a.verts + 3 * (size_t)i0, *q1 = a.verts + 3 * (size_t)i1, *q2 = a.verts + 3 * (size_t)i2;
    const float p0[3] = {q0[0], q0[1], q0[2]}, p1[3] = {q1[0], q1[1], q1[2]}, p2[3] = {q2[0], q2[1], q2[2]};
    {
        const double ux = __dsub_rn((double)p1[0], (double)p0[0]), uy = __dsub_rn((double)p1[1], (double)p0[1]), uz = __dsub_rn((double)p1[2], (double)p0[2]);
        const double vx = __dsub_rn((double)p2[0], (double)p0[0]), vy = __dsub_rn((double)p2[1], (double)p0[1]), vz = __dsub_rn((double)p2[2], (double)p0[2]);
        const double nx = __dsub_rn(__dmul_rn(uy, vz), __dmul_rn(uz, vy));
        const double ny = __dsub_rn(__dmul_rn(uz, vx), __dmul_rn(ux, vz));
        const double nz = __dsub_rn(__dmul_rn(ux, vy), __dmul_rn(uy, vx));
        if (nx == 0.0 && ny == 0.0 && nz == 0.0) return false;
    }
    vis_snap(w, p0, t.x0, t.y0, t.z0);
    vis_snap(w, p1, t.x1, t.y1, t.z1);
    vis_snap(w, p2, t.x2, t.y2, t.z2);
    const long long stored = raster_edge(t.x0, t.y0, t.x1, t.y1, t.x2, t.y2);
    side = (stored > 0) - (stored < 0);
    raster_setup<8>(t, 0, w.R - 1);
    return true;
}

__device__ __forceinline__ bool vis_fallback(const RasterFace &t, const unsigned *buf, int R, int bias_small) {
    const int px = min((t.x0 + t.x1 + t.x2) / 3 >> 8, R - 1), py = min((t.y0 + t.y1 + t.y2) / 3 >> 8, R - 1);
    return (long long)((t.z0 + t.z1 + t.z2) / 3) <= (long long)buf[py * R + px] + bias_small;
}

extern __shared__ unsigned vis_buf[];

// One pass over the faces [f0, f1).  TEST false: pass 1, minima into the buffer.  TEST true: pass 2, the depth test; a face that passes
// at one of its covered centres (the scan stops there), or at its fallback pixel where it covers none, ORs `bit` into its mask.
template <bool TEST>
__device__ __forceinline__ void vis_pass(const VisArgs &a, const VisView &w, int f0, int f1, unsigned bit, int *s_list, int *s_cnt) {
    const int R = w.R;
    int side;
    raster_sweep<8>(
        f0, f1, VIS_THREADS, s_list, s_cnt, [&](int f, RasterFace &t) { return vis_load(a, w, f, t, side); },
        [&](int px, int py, long long zp) {
            if (TEST) return zp <= (long long)vis_buf[py * R + px] + PDGN_VISIBLE_BIAS_COVER;
            atomicMin(vis_buf + py * R + px, (unsigned)zp);
            return false;
        },
        [&](int f, const RasterFace &t, bool covered, bool passed) {
            if (TEST && (covered ? passed : vis_fallback(t, vis_buf, R, a.bias_small))) atomicOr(a.mask + f, bit);
        });
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;                 // (the next pass starts from parity 0 again)
    __syncthreads();
}

// Pass 2 of pdgn_mesh_face_votes over the faces [f0, f1): every covered centre that passes the depth test is counted, in the lane that
// looked at it (no visit stops the scan); the 64 partials of a large face are summed in the sweep's fold, so that `done` -- one lane per
// face on either path -- holds the face's n and adds it to the column its stored order names.  Integer adds to distinct words per face:
// the NV workgroups of a shape meet on a face's two words in any order, with one result.
__device__ __forceinline__ void vis_vote_pass(const VisArgs &a, const VisView &w, int f0, int f1, unsigned bit, int *s_list, int *s_cnt) {
    const int R = w.R;
    int side;
    unsigned n;
    raster_sweep<8>(
        f0, f1, VIS_THREADS, s_list, s_cnt,
        [&](int f, RasterFace &t) {
            n = 0;
            return vis_load(a, w, f, t, side);
        },
        [&](int px, int py, long long zp) {
            n += zp <= (long long)vis_buf[py * R + px] + PDGN_VISIBLE_BIAS_COVER;
            return false;
        },
        [&](int f, const RasterFace &t, bool covered, bool) {
            const bool fell = !covered && vis_fallback(t, vis_buf, R, a.bias_small);
            const unsigned count = covered ? n : (unsigned)(fell && side != 0);
            if (count) atomicAdd(a.votes + 2 * (size_t)f + (side > 0), count);
            if (a.mask && (count || fell)) atomicOr(a.mask + f, bit);
        },
        [&] { n = raster_wave_sum(n); });
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
}

template <bool VOTES>
__global__ __launch_bounds__(VIS_THREADS) void visible_kernel(VisArgs a) {
    __shared__ int s_list[VIS_THREADS];
    __shared__ int s_cnt[2];
    const int tid = threadIdx.x;
    const int shape = blockIdx.x / a.NV, view = blockIdx.x - shape * a.NV;
    VisView w;
    const float *e = a.views + 9 * view, *fr = a.frame + 4 * (size_t)shape;
#pragma unroll
    for (int i = 0; i < 3; ++i) w.ex[i] = e[i], w.ey[i] = e[3 + i], w.ez[i] = e[6 + i], w.c[i] = fr[i];
    w.rho = fr[3], w.R = a.R;
    const int f0 = max(a.face_off[shape], 0), f1 = min(a.face_off[shape + 1], a.F);
    for (int i = tid; i < a.R * a.R; i += VIS_THREADS) vis_buf[i] = VIS_EMPTY;
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    vis_pass<false>(a, w, f0, f1, 0u, s_list, s_cnt);            // (its last sweep ends with the barrier between the passes)
    if (VOTES) vis_vote_pass(a, w, f0, f1, 1u << view, s_list, s_cnt);
    else vis_pass<true>(a, w, f0, f1, 1u << view, s_list, s_cnt);
}

extern "C" int pdgn_mesh_visibility_bias_cover(void) { return PDGN_VISIBLE_BIAS_COVER; }

extern "C" int pdgn_mesh_visibility_bias_small(int R) {
    if (R < PDGN_VISIBLE_MIN_RES || R > PDGN_VISIBLE_MAX_RES) return PDGN_ERR_INVALID;
    return (3 << 20) / R;
}

// Both entry points: the checks, the memsets and the launch.  votes null: pdgn_mesh_visibility (mask required); else pdgn_mesh_face_votes
// (mask optional).
template <bool VOTES>
static int vis_launch(int S, int V, int F, const float *verts, const int32_t *faces, const int32_t *face_off, const float *frame,
                      const float *views, int NV, int R, uint32_t *mask, uint32_t *votes, pdgn_stream_t stream) {
    // host-side checks: nothing is launched and nothing written before all of them have passed
    if (S < 1 || V < 1 || F < 1 || NV < 1 || NV > PDGN_VISIBLE_MAX_VIEWS || R < PDGN_VISIBLE_MIN_RES || R > PDGN_VISIBLE_MAX_RES)
        return PDGN_ERR_INVALID;
    if (3LL * V > 0x7fffffffLL || 3LL * F > 0x7fffffffLL || (long long)S * NV > 0x7fffffffLL) return PDGN_ERR_INVALID;
    if (!verts || !faces || !face_off || !frame || !views || (VOTES ? !votes : !mask)) return PDGN_ERR_INVALID;
    if (((uintptr_t)verts | (uintptr_t)faces | (uintptr_t)face_off | (uintptr_t)frame | (uintptr_t)views | (uintptr_t)mask | (uintptr_t)votes) & 3)
        return PDGN_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    {   // the radii, read back once (16 S bytes; the stream is waited for): a frame the snap would divide by is refused here
        float *host = (float *)malloc(sizeof(float) * 4 * (size_t)S);
        if (!host) return PDGN_ERR_INVALID;
        hipError_t e = hipStreamSynchronize(s);
        if (e == hipSuccess) e = hipMemcpy(host, frame, sizeof(float) * 4 * (size_t)S, hipMemcpyDeviceToHost);
        bool ok = e == hipSuccess;
        for (int c = 0; ok && c < S; ++c) ok = host[4 * c + 3] > 0.f && host[4 * c + 3] <= 3.4028234e38f;      // (false for a NaN)
        free(host);
        if (e != hipSuccess) return (int)e;
        if (!ok) return PDGN_ERR_INVALID;
    }
    VisArgs a;
    a.verts = verts, a.faces = faces, a.face_off = face_off, a.frame = frame, a.views = views, a.mask = mask, a.votes = votes;
    a.V = V, a.F = F, a.NV = NV, a.R = R, a.bias_small = (3 << 20) / R;
    const size_t lds = (size_t)R * R * 4;
    if (lds > 48 * 1024) {                                       // (beside it the kernel's static 1 KB: the attribute is the dynamic part alone)
        hipError_t e = hipFuncSetAttribute((const void *)visible_kernel<VOTES>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipError_t e = mask ? hipMemsetAsync(mask, 0, sizeof(uint32_t) * (size_t)F, s) : hipSuccess;
    if (e == hipSuccess && VOTES) e = hipMemsetAsync(votes, 0, sizeof(uint32_t) * 2 * (size_t)F, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(visible_kernel<VOTES>, dim3(S * NV), dim3(VIS_THREADS), lds, s, a);
    return pdgn_launch_status();
}

extern "C" int pdgn_mesh_visibility(int S, int V, int F, const float *verts, const int32_t *faces, const int32_t *face_off,
                                    const float *frame, const float *views, int NV, int R, uint32_t *mask, pdgn_stream_t stream) {
    return vis_launch<false>(S, V, F, verts, faces, face_off, frame, views, NV, R, mask, nullptr, stream);
}

extern "C" int pdgn_mesh_face_votes(int S, int V, int F, const float *verts, const int32_t *faces, const int32_t *face_off,
                                    const float *frame, const float *views, int NV, int R, uint32_t *mask, uint32_t *votes,
                                    pdgn_stream_t stream) {
    return vis_launch<true>(S, V, F, verts, faces, face_off, frame, views, NV, R, mask, votes, stream);
}
