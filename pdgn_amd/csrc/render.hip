// render.hip -- pdgn_render_sheet: a contact sheet of point clouds as one 8-bit grey image, one cell per (sample, cloud list).
// What a training run shows of itself at a snapshot (pdgn_amd/report.py): the generator's four resolutions next to real clouds.
//
// One launch sequence per sheet, three kernels on the caller's stream:
//   clear    every pixel's key <- 0xffffffff                                         (16-byte stores)
//   splat    one thread per point: project with a fixed __fmaf_rn chain, quantise the depth to 24 bits,
//            key = depth << 8 | shade, integer atomicMin on every pixel of the point's disc that lies inside its own cell
//   resolve  key -> grey (the key's low byte) or the background; four pixels per thread   (16-byte loads, 4-byte stores)
// The smallest key of a pixel does not depend on the order the points arrive in, so the image is a pure function of the
// arguments, bit for bit.  No float atomics, no LDS.  tests/render_mirror.py spells the same function in numpy.
//
// pdgn_render_sheet_lit: the same sheet with a splat kernel of its own that takes a column's shade from its normals where it has some --
// two-sided headlight shading, c = |n . l| as (nx lx + ny ly) + nz lz with every operation rounded on its own, 0 where !(c >= 0), 1 where
// c > 1, shade = 48 + (unsigned)(207 c) -- under the same key, the same atomicMin and the same clear and resolve kernels; a column without
// normals takes the depth shade above, byte for byte.  tests/normals_mirror.py spells it.
//
// pdgn_render_sheet_mesh (the second half of this file): columns of triangle meshes beside the columns of clouds, rasterised exactly in
// integers into the same keys.  Its definition heads that half; tests/mesh_render_mirror.py spells it.
#include "raster.h"

#define RENDER_THREADS 256
#define RENDER_MAX_COLS 8
#define RENDER_MAX_RADIUS 16
#define RENDER_EMPTY 0xffffffffu
#define RENDER_BACKGROUND 0

struct RenderArgs {
    const float *cloud[RENDER_MAX_COLS];
    int n[RENDER_MAX_COLS];
    int channel_major;                                           // bit c: cloud c is (rows, 3, n) instead of (rows, n, 3)
    int rows, cols, cell, radius;
    float m[12];
    unsigned *key;
};

__global__ __launch_bounds__(RENDER_THREADS) void render_clear_kernel(unsigned *key, long long total) {
    const long long i = ((long long)blockIdx.x * RENDER_THREADS + threadIdx.x) * 4;
    if (i + 3 < total) {
        *reinterpret_cast<uint4 *>(key + i) = make_uint4(RENDER_EMPTY, RENDER_EMPTY, RENDER_EMPTY, RENDER_EMPTY);
    } else {
        for (long long j = i; j < total; ++j) key[j] = RENDER_EMPTY;
    }
}

__global__ __launch_bounds__(RENDER_THREADS) void render_splat_kernel(RenderArgs a) {
    const int c = blockIdx.z, b = blockIdx.y;
    const int p = blockIdx.x * RENDER_THREADS + threadIdx.x;
    const int n = a.n[c];
    if (p >= n) return;
    const bool cm = (a.channel_major >> c) & 1;
    const float *src = a.cloud[c] + (size_t)b * 3 * n + (cm ? (size_t)p : (size_t)3 * p);
    const size_t cs = cm ? (size_t)n : 1;
    const float x = src[0], y = src[cs], z = src[2 * cs];
    const float u = __fmaf_rn(a.m[2], z, __fmaf_rn(a.m[1], y, __fmaf_rn(a.m[0], x, a.m[3])));
    const float v = __fmaf_rn(a.m[6], z, __fmaf_rn(a.m[5], y, __fmaf_rn(a.m[4], x, a.m[7])));
    const float d = __fmaf_rn(a.m[10], z, __fmaf_rn(a.m[9], y, __fmaf_rn(a.m[8], x, a.m[11])));
    const float fu = floorf(u), fv = floorf(v);
    const float lo = -(float)(a.radius + 1), hi = (float)(a.cell + a.radius + 1);
    if (!(fu > lo && fu < hi && fv > lo && fv < hi) || !(d == d)) return;          // no pixel of the disc in the cell (or a NaN)
    const int iu = (int)fu, iv = (int)fv;
    const float dc = fminf(fmaxf(d, 0.f), 1.f);
    const unsigned q = min((unsigned)(dc * 16777216.f), 0xffffffu);                 // 24-bit depth, 0 = nearest
    const unsigned k = (q << 8) | (255u - (q >> 17));                              // shade: 255 (nearest) .. 128 (farthest)
    const int r = a.radius, r2 = r * r;
    const size_t width = (size_t)a.cols * a.cell;
    unsigned *cellkey = a.key + ((size_t)b * a.cell) * width + (size_t)c * a.cell;
    for (int dy = -r; dy <= r; ++dy) {
        const int py = iv + dy;
        if (py < 0 || py >= a.cell) continue;
        for (int dx = -r; dx <= r; ++dx) {
            const int px = iu + dx;
            if (px < 0 || px >= a.cell || dx * dx + dy * dy > r2) continue;
            atomicMin(cellkey + (size_t)py * width + px, k);
        }
    }
}

struct RenderLitArgs {
    RenderArgs r;
    const float *normal[RENDER_MAX_COLS];                        // (rows, n, 3) point-major per column, or null: the depth shade
    float l[3];
};

// render_splat_kernel with the shade of a column that has normals taken from them; everything else is that kernel's, line for line
__global__ __launch_bounds__(RENDER_THREADS) void render_splat_lit_kernel(RenderLitArgs la) {
    const RenderArgs &a = la.r;
    const int c = blockIdx.z, b = blockIdx.y;
    const int p = blockIdx.x * RENDER_THREADS + threadIdx.x;
    const int n = a.n[c];
    if (p >= n) return;
    const bool cm = (a.channel_major >> c) & 1;
    const float *src = a.cloud[c] + (size_t)b * 3 * n + (cm ? (size_t)p : (size_t)3 * p);
    const size_t cs = cm ? (size_t)n : 1;
    const float x = src[0], y = src[cs], z = src[2 * cs];
    const float u = __fmaf_rn(a.m[2], z, __fmaf_rn(a.m[1], y, __fmaf_rn(a.m[0], x, a.m[3])));
    const float v = __fmaf_rn(a.m[6], z, __fmaf_rn(a.m[5], y, __fmaf_rn(a.m[4], x, a.m[7])));
    const float d = __fmaf_rn(a.m[10], z, __fmaf_rn(a.m[9], y, __fmaf_rn(a.m[8], x, a.m[11])));
    const float fu = floorf(u), fv = floorf(v);
    const float lo = -(float)(a.radius + 1), hi = (float)(a.cell + a.radius + 1);
    if (!(fu > lo && fu < hi && fv > lo && fv < hi) || !(d == d)) return;          // no pixel of the disc in the cell (or a NaN)
    const int iu = (int)fu, iv = (int)fv;
    const float dc = fminf(fmaxf(d, 0.f), 1.f);
    const unsigned q = min((unsigned)(dc * 16777216.f), 0xffffffu);                 // 24-bit depth, 0 = nearest
    unsigned shade = 255u - (q >> 17);                                             // without normals: 255 (nearest) .. 128 (farthest)
    if (la.normal[c]) {
        const float *nr = la.normal[c] + ((size_t)b * n + p) * 3;
        float lit = fabsf(__fadd_rn(__fadd_rn(__fmul_rn(nr[0], la.l[0]), __fmul_rn(nr[1], la.l[1])), __fmul_rn(nr[2], la.l[2])));
        lit = lit >= 0.f ? lit : 0.f;                                               // (a NaN normal: the darkest shade)
        lit = lit > 1.f ? 1.f : lit;
        shade = 48u + (unsigned)__fmul_rn(207.f, lit);                              // 48 (edge on) .. 255 (facing the light)
    }
    const unsigned k = (q << 8) | shade;
    const int r = a.radius, r2 = r * r;
    const size_t width = (size_t)a.cols * a.cell;
    unsigned *cellkey = a.key + ((size_t)b * a.cell) * width + (size_t)c * a.cell;
    for (int dy = -r; dy <= r; ++dy) {
        const int py = iv + dy;
        if (py < 0 || py >= a.cell) continue;
        for (int dx = -r; dx <= r; ++dx) {
            const int px = iu + dx;
            if (px < 0 || px >= a.cell || dx * dx + dy * dy > r2) continue;
            atomicMin(cellkey + (size_t)py * width + px, k);
        }
    }
}

__device__ __forceinline__ unsigned render_grey(unsigned k) { return k == RENDER_EMPTY ? RENDER_BACKGROUND : (k & 0xffu); }

__global__ __launch_bounds__(RENDER_THREADS) void render_resolve_kernel(const unsigned *key, uint8_t *image, long long total) {
    const long long i = ((long long)blockIdx.x * RENDER_THREADS + threadIdx.x) * 4;
    if (i + 3 < total) {
        const uint4 k = *reinterpret_cast<const uint4 *>(key + i);
        *reinterpret_cast<unsigned *>(image + i) = render_grey(k.x) | (render_grey(k.y) << 8) | (render_grey(k.z) << 16) | (render_grey(k.w) << 24);
    } else {
        for (long long j = i; j < total; ++j) image[j] = (uint8_t)render_grey(key[j]);
    }
}

static bool render_shape_ok(int rows, int cols, int cell) {
    return rows > 0 && rows <= 65535 && cols > 0 && cols <= RENDER_MAX_COLS && cell > 0 && cell <= 4096 &&
           (long long)rows * cell * cols * cell <= (1LL << 30);
}

extern "C" long long pdgn_render_workspace_bytes(int rows, int cols, int cell) {
    if (!render_shape_ok(rows, cols, cell)) return PDGN_ERR_INVALID;
    return 4LL * rows * cell * cols * cell;
}

extern "C" int pdgn_render_sheet(int rows, int cols, const float *const *clouds, const int *npoints, int channel_major, const float *view,
                                 int cell, int radius, void *workspace, uint8_t *image, pdgn_stream_t stream) {
    // host-side checks only: nothing here touches the device
    if (!render_shape_ok(rows, cols, cell) || radius < 0 || radius > RENDER_MAX_RADIUS) return PDGN_ERR_INVALID;
    if (!clouds || !npoints || !view || !workspace || !image) return PDGN_ERR_INVALID;
    if (((uintptr_t)workspace & 15) || ((uintptr_t)image & 3)) return PDGN_ERR_INVALID;
    RenderArgs a;
    int nmax = 0;
    for (int c = 0; c < RENDER_MAX_COLS; ++c) {
        a.cloud[c] = c < cols ? clouds[c] : nullptr;
        a.n[c] = c < cols ? npoints[c] : 0;
        if (c < cols && (!clouds[c] || ((uintptr_t)clouds[c] & 3) || npoints[c] <= 0 || npoints[c] > (1 << 24))) return PDGN_ERR_INVALID;
        nmax = a.n[c] > nmax ? a.n[c] : nmax;
    }
    a.channel_major = channel_major, a.rows = rows, a.cols = cols, a.cell = cell, a.radius = radius;
    for (int i = 0; i < 12; ++i) a.m[i] = view[i];
    a.key = (unsigned *)workspace;
    const long long total = (long long)rows * cell * cols * cell;
    const int quads = cdiv(cdiv(total, 4), RENDER_THREADS);
    hipLaunchKernelGGL(render_clear_kernel, dim3(quads), dim3(RENDER_THREADS), 0, (hipStream_t)stream, a.key, total);
    hipLaunchKernelGGL(render_splat_kernel, dim3(cdiv(nmax, RENDER_THREADS), rows, cols), dim3(RENDER_THREADS), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(render_resolve_kernel, dim3(quads), dim3(RENDER_THREADS), 0, (hipStream_t)stream, a.key, image, total);
    return pdgn_launch_status();
}

extern "C" int pdgn_render_sheet_lit(int rows, int cols, const float *const *clouds, const float *const *normals, const int *npoints,
                                     int channel_major, const float *view, const float *light, int cell, int radius, void *workspace,
                                     uint8_t *image, pdgn_stream_t stream) {
    // host-side checks only: nothing here touches the device
    if (!render_shape_ok(rows, cols, cell) || radius < 0 || radius > RENDER_MAX_RADIUS) return PDGN_ERR_INVALID;
    if (!clouds || !normals || !npoints || !view || !light || !workspace || !image) return PDGN_ERR_INVALID;
    if (((uintptr_t)workspace & 15) || ((uintptr_t)image & 3)) return PDGN_ERR_INVALID;
    RenderLitArgs la;
    RenderArgs &a = la.r;
    int nmax = 0;
    for (int c = 0; c < RENDER_MAX_COLS; ++c) {
        a.cloud[c] = c < cols ? clouds[c] : nullptr;
        la.normal[c] = c < cols ? normals[c] : nullptr;
        a.n[c] = c < cols ? npoints[c] : 0;
        if (c < cols && (!clouds[c] || ((uintptr_t)clouds[c] & 3) || ((uintptr_t)normals[c] & 3) || npoints[c] <= 0 || npoints[c] > (1 << 24)))
            return PDGN_ERR_INVALID;
        nmax = a.n[c] > nmax ? a.n[c] : nmax;
    }
    a.channel_major = channel_major, a.rows = rows, a.cols = cols, a.cell = cell, a.radius = radius;
    for (int i = 0; i < 12; ++i) a.m[i] = view[i];
    for (int i = 0; i < 3; ++i) la.l[i] = light[i];
    a.key = (unsigned *)workspace;
    const long long total = (long long)rows * cell * cols * cell;
    const int quads = cdiv(cdiv(total, 4), RENDER_THREADS);
    hipLaunchKernelGGL(render_clear_kernel, dim3(quads), dim3(RENDER_THREADS), 0, (hipStream_t)stream, a.key, total);
    hipLaunchKernelGGL(render_splat_lit_kernel, dim3(cdiv(nmax, RENDER_THREADS), rows, cols), dim3(RENDER_THREADS), 0, (hipStream_t)stream, la);
    hipLaunchKernelGGL(render_resolve_kernel, dim3(quads), dim3(RENDER_THREADS), 0, (hipStream_t)stream, a.key, image, total);
    return pdgn_launch_status();
}

// ------------------------------------------------------------------------------------------------------------------------------------
// pdgn_render_sheet_mesh: the same sheet with columns of TRIANGLE MESHES beside the columns of clouds.  The launch
// sequence is the clear above, render_splat_lit_kernel over the cloud columns (skipped where there are none), render_mesh_kernel over the
// mesh columns, the resolve above: one key buffer, one key, one integer minimum; a column is one kind or the other.
//
// THE DEFINITION (normative; tests/mesh_render_mirror.py spells the same function in numpy).  A mesh column has verts (V,3) fp32, faces
// (F,3) int32, range (rows,3) int32 = (first, count, base) per row, an optional mask (F) int32 and a shade mode.  Row b draws the faces
// f in [max(first, 0), min(first + count, F)); a count <= 0 draws nothing.
//   Dead.   Face f is skipped where mask[f] == 0, or where one of i_k + base (k = 0, 1, 2; the sum taken in 64 bits) lies outside [0, V).
//   Snap.   Per vertex p = verts[i_k + base]: u, v, d from the 3 x 4 view by exactly the __fmaf_rn chain of render_splat_kernel.  A
//           u, v or d that is not finite kills the face.  With s = 16 cell (exact in fp32):
//             X = (int) clamp(rintf(u * 16), -s, 2 s)    pixel units with 4 sub-pixel bits, a guard band of one cell either side
//             Y likewise from v;     Z = min((unsigned)(clamp(d, 0, 1) * 16777216.f), 0xffffff)      the splat's q
//           (rintf rounds halves to even; u * 16 is one fp32 product, +-inf where it overflows, which the clamp takes.)  After the snap
//           nothing is floating point but the flat shade.
//   Cover.  With edge(A, B, P) = (B.x - A.x)(P.y - A.y) - (B.y - A.y)(P.x - A.x) in int64:  A2 = edge(P0, P1, P2); where A2 < 0, P1 and
//           P2 (and their Z) change places and A2 its sign; A2 = 0 draws nothing.  The pixel centres C = ((2 px + 1) 8, (2 py + 1) 8) of
//           the face's bounding box, clipped to 0 <= px, py < cell of the face's OWN cell, are COVERED where w0 = edge(P1, P2, C), w1 =
//           edge(P2, P0, C) and w2 = edge(P0, P1, C) are all >= 0: edges inclusive, faces two-sided, exactly as csrc/raster.h, so two
//           faces on a shared edge leave no hole and the minimum decides.  There
//             q = floor((w0 Z0 + w1 Z1 + w2 Z2) / A2),   key = q << 8 | shade,   key buffer <- min(key buffer, key).
//           BOUND: coordinates span at most 48 cell <= 3 * 2^16 (cell <= 4096), so every edge function is below 2^37 in magnitude, A2 < 2^37
//           and the numerator below 2^37 2^24 = 2^61; the quotient is at most 2^24 - 1.  The division is exact: an fp64 estimate (off by
//           less than one) corrected by the integer remainder, as raster_div of csrc/raster.h.
//   Shade.  Depth (mode 1): 255 - (q >> 17) from the pixel's own q.  Flat-lit (mode 0), one value per face from the fp32 vertices as
//           handed in, before any swap: e1 = p1 - p0, e2 = p2 - p0, n = e1 x e2 (nx = e1y e2z - e1z e2y, ny = e1z e2x - e1x e2z, nz =
//           e1x e2y - e1y e2x), every subtraction, product and sum rounded on its own, never contracted; len = sqrtf((nx nx + ny ny) + nz nz),
//           correctly rounded; c = fabsf((nx lx + ny ly) + nz lz) / len (the correctly rounded quotient); c = 0 where !(c >= 0), c = 1
//           where c > 1; shade = 48 + (unsigned)(207 c): the lit splat's constants and light vector.  A len that is 0 or not finite kills
//           the face (flat-lit columns only).  Equal depths from two faces resolve to the smaller key, the darker shade: still
//           independent of the order of the faces.
// LIMITS.  A face with a vertex on the guard band's clamp is drawn distorted (the vertex is moved onto the band's edge).  A face that
// covers no pixel centre draws nothing: no wireframe, no anti-aliasing.  The normal of a face whose edge products underflow in fp32 is
// lost (len = 0: the face is not drawn in a flat-lit column).
//
// THE KERNEL.  Grid (chunks, rows, cols), 256 threads; a workgroup sweeps the faces of its row 256 at a time, striding by the grid
// (csrc/raster.h, THE SWEEP: a lane per small face, a wave per large one; 1 KB of static LDS).  The keys go to the key buffer in global
// memory with atomicMin, as the splat's do.  No float atomics: two runs agree bit for bit.
#define MESH_THREADS RASTER_THREADS
#define MESH_MAX_CHUNKS 64

struct RenderMeshArgs {
    const float *verts[RENDER_MAX_COLS];                         // null: not a mesh column
    const int32_t *faces[RENDER_MAX_COLS], *range[RENDER_MAX_COLS], *mask[RENDER_MAX_COLS];
    int V[RENDER_MAX_COLS], F[RENDER_MAX_COLS];
    int depth_shade;                                             // bit c: column c is shaded by depth
    int rows, cols, cell;
    float m[12], l[3];
    unsigned *key;
};

// Project and snap one vertex.  False: u, v or d is not finite.
__device__ __forceinline__ bool mesh_snap(const float *m, float s, const float *p, int &X, int &Y, int &Z) {
    const float x = p[0], y = p[1], z = p[2];
    const float u = __fmaf_rn(m[2], z, __fmaf_rn(m[1], y, __fmaf_rn(m[0], x, m[3])));
    const float v = __fmaf_rn(m[6], z, __fmaf_rn(m[5], y, __fmaf_rn(m[4], x, m[7])));
    const float d = __fmaf_rn(m[10], z, __fmaf_rn(m[9], y, __fmaf_rn(m[8], x, m[11])));
    if (!(fabsf(u) <= 3.4028234e38f && fabsf(v) <= 3.4028234e38f && fabsf(d) <= 3.4028234e38f)) return false;
    X = (int)fminf(fmaxf(rintf(__fmul_rn(u, 16.f)), -s), 2.f * s);
    Y = (int)fminf(fmaxf(rintf(__fmul_rn(v, 16.f)), -s), 2.f * s);
    const float dc = fminf(fmaxf(d, 0.f), 1.f);
    Z = (int)min((unsigned)(dc * 16777216.f), 0xffffffu);
    return true;
}

// Gather, snap and shade face f of column c (shade: the flat shade, 0 in a column shaded by depth).  False: the face is dead.
__device__ __forceinline__ bool mesh_load(const RenderMeshArgs &a, int c, int base, int f, RasterFace &t, unsigned &shade) {
    if (a.mask[c] && a.mask[c][f] == 0) return false;
    const int32_t *fi = a.faces[c] + 3 * (size_t)f;
    const long long i0 = (long long)fi[0] + base, i1 = (long long)fi[1] + base, i2 = (long long)fi[2] + base;
    const long long V = a.V[c];
    if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) return false;
    const float *q0 = a.verts[c] + 3 * (size_t)i0, *q1 = a.verts[c] + 3 * (size_t)i1, *q2 = a.verts[c] + 3 * (size_t)i2;
    const float p0[3] = {q0[0], q0[1], q0[2]}, p1[3] = {q1[0], q1[1], q1[2]}, p2[3] = {q2[0], q2[1], q2[2]};
    const float s = (float)(a.cell << 4);
    if (!mesh_snap(a.m, s, p0, t.x0, t.y0, t.z0) || !mesh_snap(a.m, s, p1, t.x1, t.y1, t.z1) || !mesh_snap(a.m, s, p2, t.x2, t.y2, t.z2))
        return false;
    shade = 0;
    if (!((a.depth_shade >> c) & 1)) {
        const float ux = __fsub_rn(p1[0], p0[0]), uy = __fsub_rn(p1[1], p0[1]), uz = __fsub_rn(p1[2], p0[2]);
        const float vx = __fsub_rn(p2[0], p0[0]), vy = __fsub_rn(p2[1], p0[1]), vz = __fsub_rn(p2[2], p0[2]);
        const float nx = __fsub_rn(__fmul_rn(uy, vz), __fmul_rn(uz, vy));
        const float ny = __fsub_rn(__fmul_rn(uz, vx), __fmul_rn(ux, vz));
        const float nz = __fsub_rn(__fmul_rn(ux, vy), __fmul_rn(uy, vx));
        const float len = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(nx, nx), __fmul_rn(ny, ny)), __fmul_rn(nz, nz)));
        if (!(len > 0.f && len <= 3.4028234e38f)) return false;                      // (false for a NaN too)
        float lit = __fdiv_rn(fabsf(__fadd_rn(__fadd_rn(__fmul_rn(nx, a.l[0]), __fmul_rn(ny, a.l[1])), __fmul_rn(nz, a.l[2]))), len);
        lit = lit >= 0.f ? lit : 0.f;
        lit = lit > 1.f ? 1.f : lit;
        shade = 48u + (unsigned)__fmul_rn(207.f, lit);
    }
    raster_setup<4>(t, 0, a.cell - 1);
    return true;
}

__global__ __launch_bounds__(MESH_THREADS) void render_mesh_kernel(RenderMeshArgs a) {
    __shared__ int s_list[MESH_THREADS];
    __shared__ int s_cnt[2];
    const int c = blockIdx.z, b = blockIdx.y;
    if (!a.verts[c]) return;                                     // a cloud column (the whole workgroup leaves)
    const int32_t *rg = a.range[c] + 3 * (size_t)b;
    const int first = rg[0], count = rg[1], vbase = rg[2];
    const long long f0 = max(first, 0), f1 = min((long long)first + max(count, 0), (long long)a.F[c]);
    const bool depth = (a.depth_shade >> c) & 1;
    const size_t width = (size_t)a.cols * a.cell;
    unsigned *cellkey = a.key + ((size_t)b * a.cell) * width + (size_t)c * a.cell;      // the cell's first pixel
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    unsigned shade;                                              // of the face this thread last loaded
    raster_sweep<4>(
        f0 + (long long)blockIdx.x * MESH_THREADS, f1, (long long)gridDim.x * MESH_THREADS, s_list, s_cnt,
        [&](int f, RasterFace &t) { return mesh_load(a, c, vbase, f, t, shade); },
        [&](int px, int py, long long z) {
            const unsigned q = (unsigned)z;
            atomicMin(cellkey + (size_t)py * width + px, (q << 8) | (depth ? 255u - (q >> 17) : shade));
            return false;
        },
        [](int, const RasterFace &, bool, bool) {});
}

extern "C" int pdgn_render_sheet_mesh(int rows, int cols, const float *const *clouds, const float *const *normals, const int *npoints,
                                      int channel_major, const float *const *mesh_verts, const int32_t *const *mesh_faces,
                                      const int32_t *const *mesh_range, const int32_t *const *mesh_mask, const int *mesh_nverts,
                                      const int *mesh_nfaces, const int *mesh_shade, const float *view, const float *light, int cell, int radius,
                                      void *workspace, uint8_t *image, pdgn_stream_t stream) {
    // host-side checks only: nothing here touches the device
    if (!render_shape_ok(rows, cols, cell) || radius < 0 || radius > RENDER_MAX_RADIUS) return PDGN_ERR_INVALID;
    if (!clouds || !normals || !npoints || !view || !light || !workspace || !image) return PDGN_ERR_INVALID;
    if (!mesh_verts || !mesh_faces || !mesh_range || !mesh_nverts || !mesh_nfaces || !mesh_shade) return PDGN_ERR_INVALID;
    if (((uintptr_t)workspace & 15) || ((uintptr_t)image & 3)) return PDGN_ERR_INVALID;
    RenderLitArgs la;
    RenderArgs &a = la.r;
    RenderMeshArgs ma;
    int nmax = 0, fmax = 0, nmesh = 0;
    ma.depth_shade = 0;
    for (int c = 0; c < RENDER_MAX_COLS; ++c) {
        const bool mesh = c < cols && mesh_verts[c];
        const bool cloud = c < cols && !mesh;
        a.cloud[c] = cloud ? clouds[c] : nullptr;
        la.normal[c] = cloud ? normals[c] : nullptr;
        a.n[c] = cloud ? npoints[c] : 0;                         // (a mesh column: the splat's threads all leave at once)
        if (cloud && (!clouds[c] || ((uintptr_t)clouds[c] & 3) || ((uintptr_t)normals[c] & 3) || npoints[c] <= 0 || npoints[c] > (1 << 24)))
            return PDGN_ERR_INVALID;
        nmax = a.n[c] > nmax ? a.n[c] : nmax;
        ma.verts[c] = mesh ? mesh_verts[c] : nullptr;
        ma.faces[c] = mesh ? mesh_faces[c] : nullptr;
        ma.range[c] = mesh ? mesh_range[c] : nullptr;
        ma.mask[c] = mesh && mesh_mask ? mesh_mask[c] : nullptr;
        ma.V[c] = mesh ? mesh_nverts[c] : 0;
        ma.F[c] = mesh ? mesh_nfaces[c] : 0;
        if (mesh) {
            if (!ma.range[c] || (((uintptr_t)ma.verts[c] | (uintptr_t)ma.faces[c] | (uintptr_t)ma.range[c] | (uintptr_t)ma.mask[c]) & 3))
                return PDGN_ERR_INVALID;
            if (ma.V[c] < 1 || ma.V[c] > (1 << 28) || ma.F[c] < 0 || ma.F[c] > (1 << 28) || (ma.F[c] > 0 && !ma.faces[c])) return PDGN_ERR_INVALID;
            if (mesh_shade[c] != 0 && mesh_shade[c] != 1) return PDGN_ERR_INVALID;
            ma.depth_shade |= mesh_shade[c] << c;
            fmax = ma.F[c] > fmax ? ma.F[c] : fmax;
            ++nmesh;
        }
    }
    if (!nmesh) return PDGN_ERR_INVALID;
    a.channel_major = channel_major, a.rows = rows, a.cols = cols, a.cell = cell, a.radius = radius;
    ma.rows = rows, ma.cols = cols, ma.cell = cell;
    for (int i = 0; i < 12; ++i) a.m[i] = ma.m[i] = view[i];
    for (int i = 0; i < 3; ++i) la.l[i] = ma.l[i] = light[i];
    a.key = ma.key = (unsigned *)workspace;
    const long long total = (long long)rows * cell * cols * cell;
    const int quads = cdiv(cdiv(total, 4), RENDER_THREADS);
    hipLaunchKernelGGL(render_clear_kernel, dim3(quads), dim3(RENDER_THREADS), 0, (hipStream_t)stream, a.key, total);
    if (nmax > 0)
        hipLaunchKernelGGL(render_splat_lit_kernel, dim3(cdiv(nmax, RENDER_THREADS), rows, cols), dim3(RENDER_THREADS), 0, (hipStream_t)stream, la);
    if (fmax > 0) {
        const int chunks = cdiv(fmax, MESH_THREADS) < MESH_MAX_CHUNKS ? cdiv(fmax, MESH_THREADS) : MESH_MAX_CHUNKS;
        hipLaunchKernelGGL(render_mesh_kernel, dim3(chunks, rows, cols), dim3(MESH_THREADS), 0, (hipStream_t)stream, ma);
    }
    hipLaunchKernelGGL(render_resolve_kernel, dim3(quads), dim3(RENDER_THREADS), 0, (hipStream_t)stream, a.key, image, total);
    return pdgn_launch_status();
}
