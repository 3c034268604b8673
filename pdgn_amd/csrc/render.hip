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
#include "common.h"

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
