// repulsion.hip -- every point of a cloud against every other point of the same cloud: the repulsion regulariser of the generator's
// loss, its gradient, and the nearest-neighbour distances of the spacing statistics (include/pdgn_hip.h: pdgn_repulsion; DESIGN.md
// section 7p).  No BLAS, no atomics.
//
// NORMATIVE OPERATION ORDER (tests/repulsion_mirror.py restates it in numpy; every operation below is one fp32 rounding:
// __fsub_rn / __fmul_rn / __fadd_rn, nothing contracted).  One cloud x of n points, inv = 1 / h^2; for point i:
//
//     s = gx = gy = gz = 0,  nn2 = +inf
//     for j = 0 .. n-1 ascending, j != i:
//         dx = x_i.x - x_j.x,  dy = x_i.y - x_j.y,  dz = x_i.z - x_j.z
//         d2 = (dx*dx + dy*dy) + dz*dz
//         nn2 = d2 < nn2 ? d2 : nn2
//         t  = 1 - d2*inv
//         if !(t <= 0):  s = s + t*t;  gx = gx + t*dx;  gy = gy + t*dy;  gz = gz + t*dz
//     s_i = s,  nn2_i = nn2,  grad_i = (coef*gx, coef*gy, coef*gz)
//
// `!(t <= 0)` and not `t > 0`: a NaN coordinate gives a NaN d2, a NaN t that passes, and so a NaN s_i and a NaN gradient -- for the point
// that has it and for every other point of its cloud, and for no point of another cloud.  An infinite coordinate takes whatever path
// this code takes (d2 = +inf: t = -inf, the pair is outside; inf - inf: NaN, as above).
//
// The reduction (second launch, one workgroup): cloud c is summed by ONE wave,
//     lane l:  p_l = ((s[l] + s[l + 64]) + s[l + 128]) + ...           (starting from 0.0f, i ascending)
//     for off = 32, 16, 8, 4, 2, 1:  p_l = p_l + p_(l xor off)          (all lanes end with the same value P_c)
//     per_cloud[c] = (float)((double)P_c / (double)n)
//     loss = (float)(T / (double)(b n)),   T = ((double)P_0 + (double)P_1) + ...   (from 0.0, c ascending)
//
// SHAPE.  One thread per point i; the cloud passes through LDS in chunks of RP_CHUNK points, 16 bytes each (x, y, z, pad): every lane
// reads the same x_j, one ds_read_b128 at a uniform address -- a broadcast, conflict-free -- per ~20 VALU operations.  The order over
// j is each thread's own, so block size, grid size and chunk length change no bit.  Block size: the largest of 256 / 128 / 64 that
// still gives the chip a workgroup per CU (35 x 256 points: 140 one-wave workgroups, not 35 of four waves).  16 bytes of LDS per staged
// point (dynamic: min(n, RP_CHUNK) points, 16 KB at most) and 51 VGPRs, nothing spilled: ten workgroups fit a CU at the large levels, the
// wave slots bound the small ones.
#include "common.h"

#include <math.h>

#define RP_CHUNK 1024
#define RP_RED_THREADS 1024

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void repulsion_kernel(int n, const float *__restrict__ xyz, float inv, float coef,
                                                          float *__restrict__ s_out, float *__restrict__ grad,
                                                          float *__restrict__ nn2_out) {
    extern __shared__ float4 pts[];                                // min(n, RP_CHUNK) points: the small levels keep more workgroups per CU
    const int c = blockIdx.y;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    const bool live = i < n;
    const float *cloud = xyz + (size_t)c * n * 3;
    float xi = 0.f, yi = 0.f, zi = 0.f;
    if (live) xi = cloud[3 * i], yi = cloud[3 * i + 1], zi = cloud[3 * i + 2];
    float s = 0.f, gx = 0.f, gy = 0.f, gz = 0.f, nn2 = INFINITY;
    float *flat = reinterpret_cast<float *>(pts);
    for (int j0 = 0; j0 < n; j0 += RP_CHUNK) {
        const int cnt = min(RP_CHUNK, n - j0);
        if (j0) __syncthreads();                                   // everyone is done reading the previous chunk
        for (int e = threadIdx.x; e < 3 * cnt; e += BLOCK) flat[(e / 3) * 4 + e % 3] = cloud[3 * j0 + e];
        __syncthreads();
        const int skip = i - j0;                                   // this thread's own point, as an index into the chunk (or outside it)
#pragma unroll 4
        for (int jj = 0; jj < cnt; ++jj) {
            const float4 p = pts[jj];
            const float dx = __fsub_rn(xi, p.x), dy = __fsub_rn(yi, p.y), dz = __fsub_rn(zi, p.z);
            const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
            const float t = __fsub_rn(1.0f, __fmul_rn(d2, inv));
            const bool other = jj != skip;
            const bool in = other && !(t <= 0.f);
            nn2 = (other && d2 < nn2) ? d2 : nn2;
            s = in ? __fadd_rn(s, __fmul_rn(t, t)) : s;
            gx = in ? __fadd_rn(gx, __fmul_rn(t, dx)) : gx;
            gy = in ? __fadd_rn(gy, __fmul_rn(t, dy)) : gy;
            gz = in ? __fadd_rn(gz, __fmul_rn(t, dz)) : gz;
        }
    }
    if (!live) return;
    const size_t at = (size_t)c * n + i;
    s_out[at] = s;
    if (nn2_out) nn2_out[at] = nn2;
    if (grad) {
        grad[3 * at] = __fmul_rn(coef, gx);
        grad[3 * at + 1] = __fmul_rn(coef, gy);
        grad[3 * at + 2] = __fmul_rn(coef, gz);
    }
}

// One workgroup of 16 waves; wave w sums the clouds w, w + 16, ... (each in the order of the header), thread 0 adds a round's sixteen
// totals to T in cloud order.
__global__ __launch_bounds__(RP_RED_THREADS) void repulsion_reduce_kernel(int b, int n, const float *__restrict__ s,
                                                                         float *__restrict__ loss, float *__restrict__ per_cloud) {
    constexpr int WAVES = RP_RED_THREADS / PDGN_WAVE;
    __shared__ float tot[WAVES];
    const int wave = threadIdx.x / PDGN_WAVE, lane = lane_id();
    double T = 0.0;
    for (int c0 = 0; c0 < b; c0 += WAVES) {
        const int c = c0 + wave;
        if (c < b) {
            const float *row = s + (size_t)c * n;
            float p = 0.f;
#pragma unroll 8                                                 // eight loads in flight; the additions keep their order
            for (int i = lane; i < n; i += PDGN_WAVE) p = __fadd_rn(p, row[i]);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) p = __fadd_rn(p, __shfl_xor(p, off, 64));
            if (lane == 0) {
                tot[wave] = p;
                if (per_cloud) per_cloud[c] = (float)((double)p / (double)n);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int w = 0; w < WAVES && c0 + w < b; ++w) T += (double)tot[w];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(T / ((double)b * (double)n));
}

// dxyz = g[0] * grad: the saved gradient times the upstream scalar
__global__ __launch_bounds__(256) void repulsion_bwd_kernel(long long count, const float *__restrict__ grad, const float *__restrict__ g,
                                                            float *__restrict__ dxyz) {
    const float up = g[0];
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += (long long)gridDim.x * blockDim.x)
        dxyz[k] = __fmul_rn(up, grad[k]);
}


void rp_reduce_launch(int b, int n, const float *s, float *loss, float *per_cloud, hipStream_t st) {
    hipLaunchKernelGGL(repulsion_reduce_kernel, dim3(1), dim3(RP_RED_THREADS), 0, st, b, n, s, loss, per_cloud);
}

extern "C" int pdgn_repulsion_chunk(void) { return RP_CHUNK; }

extern "C" int pdgn_repulsion(int b, int n, const float *xyz, float inv_h2, float coef, float *s, float *loss, float *per_cloud,
                              float *grad, float *nn2, pdgn_stream_t stream) {
    if (b < 1 || n < 1 || n > PDGN_REPULSION_MAX_N || (long long)b * n > (1LL << 28)) return PDGN_ERR_INVALID;
    if (!isfinite(inv_h2) || !(inv_h2 > 0.f) || !isfinite(coef)) return PDGN_ERR_INVALID;
    if (!xyz || !s || !loss) return PDGN_ERR_INVALID;
    if (!pdgn_aligned(xyz, 4) || !pdgn_aligned(s, 4) || !pdgn_aligned(loss, 4) || !pdgn_aligned(per_cloud, 4) || !pdgn_aligned(grad, 4) ||
        !pdgn_aligned(nn2, 4))
        return PDGN_ERR_INVALID;
    // the largest workgroup that still leaves one per CU (256 of them); 64 where even that does not
    const int block = (long long)b * cdiv(n, 256) >= 256 ? 256 : (long long)b * cdiv(n, 128) >= 256 ? 128 : 64;
    const unsigned lds = (unsigned)(n < RP_CHUNK ? n : RP_CHUNK) * sizeof(float4);
    // grid.y carries the cloud: at most 65535 of them per launch
    for (int c0 = 0; c0 < b; c0 += 65535) {
        const int cb = b - c0 < 65535 ? b - c0 : 65535;
        const float *x0 = xyz + (size_t)c0 * n * 3;
        float *s0 = s + (size_t)c0 * n, *g0 = grad ? grad + (size_t)c0 * n * 3 : nullptr, *n0 = nn2 ? nn2 + (size_t)c0 * n : nullptr;
        const dim3 grid(cdiv(n, block), cb);
        if (block == 256)
            hipLaunchKernelGGL(repulsion_kernel<256>, grid, dim3(256), lds, (hipStream_t)stream, n, x0, inv_h2, coef, s0, g0, n0);
        else if (block == 128)
            hipLaunchKernelGGL(repulsion_kernel<128>, grid, dim3(128), lds, (hipStream_t)stream, n, x0, inv_h2, coef, s0, g0, n0);
        else
            hipLaunchKernelGGL(repulsion_kernel<64>, grid, dim3(64), lds, (hipStream_t)stream, n, x0, inv_h2, coef, s0, g0, n0);
    }
    rp_reduce_launch(b, n, s, loss, per_cloud, (hipStream_t)stream);
    return pdgn_launch_status();
}

extern "C" int pdgn_repulsion_backward(long long count, const float *grad, const float *g, float *dxyz, pdgn_stream_t stream) {
    if (count < 1 || !grad || !g || !dxyz) return PDGN_ERR_INVALID;
    if (!pdgn_aligned(grad, 4) || !pdgn_aligned(g, 4) || !pdgn_aligned(dxyz, 4)) return PDGN_ERR_INVALID;
    const int grid = (int)(count < 256LL * 1024 ? cdiv(count, 256) : 1024);
    hipLaunchKernelGGL(repulsion_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, count, grad, g, dxyz);
    return pdgn_launch_status();
}
