// loss_small.hip -- the scalar ends of the step's losses as single launches.
//
// The adversarial terms are nn.MSELoss against a constant (models/PDGNet_v2.py:186-190, 246-250: mse(D(x), 1) / mse(D(x), 0)
// on a (B, 1) score), the local-pair terms sums of Chamfer minima (utils/chamfer_loss.py:16-20).  As torch ops each is two
// launches forward (elementwise + reduction, or reduction + scale) and two backward (a zero-filled or expanded gradient + the
// elementwise adjoint) -- 24 such terms per iteration, every launch ~10 us of host time on the issuing thread.  One workgroup
// each way; the sums run in a fixed order (deterministic).
#include "common.h"

#define LS_THREADS 1024

__device__ __forceinline__ float ls_block_sum(float v) {
    __shared__ float red[LS_THREADS / PDGN_WAVE];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane_id() == 0) red[threadIdx.x / PDGN_WAVE] = v;
    __syncthreads();
    float s = 0.f;
    if (threadIdx.x == 0)
        for (int w = 0; w < LS_THREADS / PDGN_WAVE; ++w) s += red[w];
    return s;                                                      // valid in thread 0
}

// out[0] = scale * sum x
__global__ __launch_bounds__(LS_THREADS) void scaled_sum_kernel(long long n, const float *__restrict__ x, float scale,
                                                               float *__restrict__ out) {
    float s = 0.f;
    for (long long i = threadIdx.x; i < n; i += LS_THREADS) s += x[i];
    s = ls_block_sum(s);
    if (threadIdx.x == 0) out[0] = scale * s;
}

// out[0] = scale * mean (x - t)^2
__global__ __launch_bounds__(LS_THREADS) void mse_const_fwd_kernel(long long n, const float *__restrict__ x, float t, float scale,
                                                                  float *__restrict__ out) {
    float s = 0.f;
    for (long long i = threadIdx.x; i < n; i += LS_THREADS) {
        const float d = x[i] - t;
        s = __fmaf_rn(d, d, s);
    }
    s = ls_block_sum(s);
    if (threadIdx.x == 0) out[0] = scale * (s / (float)n);
}

// two integer block sums at once: wave shuffles, then the sixteen wave totals through shared memory; valid in thread 0
__device__ __forceinline__ void ls_block_sum2(int &a, int &b) {
    __shared__ int red2[2][LS_THREADS / PDGN_WAVE];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64), b += __shfl_xor(b, off, 64);
    if (lane_id() == 0) red2[0][threadIdx.x / PDGN_WAVE] = a, red2[1][threadIdx.x / PDGN_WAVE] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        a = b = 0;
        for (int w = 0; w < LS_THREADS / PDGN_WAVE; ++w) a += red2[0][w], b += red2[1][w];
    }
}

// mse_const_fwd_kernel (the float sum in its order: out[0] is the same bits) + count = (#{x > bnd}, #{x < bnd}, n), STORED:
// the adaptive augmentation's statistic on D's scores of the real batch (include/pdgn_hip.h).  NaN and x == bnd count to neither.
__global__ __launch_bounds__(LS_THREADS) void mse_const_count_fwd_kernel(long long n, const float *__restrict__ x, float t, float scale,
                                                                        float bnd, float *__restrict__ out, int *__restrict__ count) {
    float s = 0.f;
    int pos = 0, neg = 0;
    for (long long i = threadIdx.x; i < n; i += LS_THREADS) {
        const float v = x[i];
        const float d = v - t;
        s = __fmaf_rn(d, d, s);
        pos += v > bnd;
        neg += v < bnd;
    }
    s = ls_block_sum(s);
    ls_block_sum2(pos, neg);
    if (threadIdx.x == 0) {
        out[0] = scale * (s / (float)n);
        count[0] = pos, count[1] = neg, count[2] = (int)n;
    }
}

// dx = g[0] * scale * 2 (x - t) / n
__global__ __launch_bounds__(256) void mse_const_bwd_kernel(long long n, const float *__restrict__ x, float t, float scale,
                                                            const float *__restrict__ g, float *__restrict__ dx) {
    const float c = g[0] * scale * 2.0f / (float)n;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        dx[i] = c * (x[i] - t);
}

// ---- the hinge and the non-saturating logistic objectives (include/pdgn_hip.h: pdgn_gan_term): siblings of the mse_const trio above,
// the same launch shapes and the same summation order.  kind and role are uniform over the launch.  Every operation is its own fp32
// rounding (-ffp-contract=off).  A NaN score stays a NaN term: `v > 0 ? v : 0` alone would turn it into 0.
__device__ __forceinline__ float gan_f(float x, int kind, int role) {
    if (kind == PDGN_GAN_HINGE) {
        if (role == PDGN_GAN_G) return -x;
        const float v = role == PDGN_GAN_D_REAL ? 1.0f - x : 1.0f + x;
        return v > 0.f ? v : (v == v ? 0.f : v);
    }
    const float t = role == PDGN_GAN_D_FAKE ? x : -x;              // softplus(t) = max(t, 0) + log1p(exp(-|t|)): no overflow
    return fmaxf(t, 0.f) + log1pf(expf(-fabsf(t)));
}

// sigma(t) from e = exp(-|t|) in (0, 1]: never inf / inf; a NaN t fails `t >= 0` and gives NaN / NaN
__device__ __forceinline__ float gan_sigmoid(float t) {
    const float e = expf(-fabsf(t));
    return t >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);
}

// d f / d x; the hinge's kink (v == 0) has derivative 0: the forward's own `v > 0`
__device__ __forceinline__ float gan_df(float x, int kind, int role) {
    if (kind == PDGN_GAN_HINGE) {
        if (role == PDGN_GAN_G) return x == x ? -1.0f : x;
        const float v = role == PDGN_GAN_D_REAL ? 1.0f - x : 1.0f + x;
        const float d = role == PDGN_GAN_D_REAL ? -1.0f : 1.0f;
        return v > 0.f ? d : (v == v ? 0.f : v);
    }
    return role == PDGN_GAN_D_FAKE ? gan_sigmoid(x) : -gan_sigmoid(-x);
}

// out[0] = scale * mean f(x)
__global__ __launch_bounds__(LS_THREADS) void gan_term_fwd_kernel(long long n, const float *__restrict__ x, int kind, int role, float scale,
                                                                 float *__restrict__ out) {
    float s = 0.f;
    for (long long i = threadIdx.x; i < n; i += LS_THREADS) s += gan_f(x[i], kind, role);
    s = ls_block_sum(s);
    if (threadIdx.x == 0) out[0] = scale * (s / (float)n);
}

// gan_term_fwd_kernel (the float sum in its order: out[0] is the same bits) + mse_const_count_fwd_kernel's counts, stored the same way
__global__ __launch_bounds__(LS_THREADS) void gan_term_count_fwd_kernel(long long n, const float *__restrict__ x, int kind, int role,
                                                                       float scale, float bnd, float *__restrict__ out,
                                                                       int *__restrict__ count) {
    float s = 0.f;
    int pos = 0, neg = 0;
    for (long long i = threadIdx.x; i < n; i += LS_THREADS) {
        const float v = x[i];
        s += gan_f(v, kind, role);
        pos += v > bnd;
        neg += v < bnd;
    }
    s = ls_block_sum(s);
    ls_block_sum2(pos, neg);
    if (threadIdx.x == 0) {
        out[0] = scale * (s / (float)n);
        count[0] = pos, count[1] = neg, count[2] = (int)n;
    }
}

// dx = (g[0] * scale / n) * f'(x)
__global__ __launch_bounds__(256) void gan_term_bwd_kernel(long long n, const float *__restrict__ x, int kind, int role, float scale,
                                                           const float *__restrict__ g, float *__restrict__ dx) {
    const float c = g[0] * scale / (float)n;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        dx[i] = c * gan_df(x[i], kind, role);
}

static bool gan_args_ok(long long n, int kind, int role, const void *a, const void *b, const void *c) {
    if (n < 1 || (kind != PDGN_GAN_HINGE && kind != PDGN_GAN_LOGISTIC) || role < PDGN_GAN_D_REAL || role > PDGN_GAN_G) return false;
    if (!a || !b || !c) return false;
    return !(((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 3);
}

extern "C" int pdgn_gan_term(long long n, const float *x, int kind, int role, float scale, float *out, pdgn_stream_t stream) {
    if (!gan_args_ok(n, kind, role, x, out, out)) return PDGN_ERR_INVALID;
    hipLaunchKernelGGL(gan_term_fwd_kernel, dim3(1), dim3(LS_THREADS), 0, (hipStream_t)stream, n, x, kind, role, scale, out);
    return pdgn_launch_status();
}

extern "C" int pdgn_gan_term_count(long long n, const float *x, int kind, int role, float scale, float boundary, float *out, int32_t *count,
                                   pdgn_stream_t stream) {
    if (!gan_args_ok(n, kind, role, x, out, count) || n > 0x7fffffffLL) return PDGN_ERR_INVALID;
    hipLaunchKernelGGL(gan_term_count_fwd_kernel, dim3(1), dim3(LS_THREADS), 0, (hipStream_t)stream, n, x, kind, role, scale, boundary, out,
                       count);
    return pdgn_launch_status();
}

extern "C" int pdgn_gan_term_backward(long long n, const float *x, int kind, int role, float scale, const float *g, float *dx,
                                      pdgn_stream_t stream) {
    if (!gan_args_ok(n, kind, role, x, g, dx)) return PDGN_ERR_INVALID;
    const int grid = (int)(n < 256 * 64 ? cdiv(n, 256) : 64);
    hipLaunchKernelGGL(gan_term_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, n, x, kind, role, scale, g, dx);
    return pdgn_launch_status();
}

extern "C" int pdgn_scaled_sum(long long n, const float *x, float scale, float *out, pdgn_stream_t stream) {
    if (n < 0) return PDGN_ERR_INVALID;
    hipLaunchKernelGGL(scaled_sum_kernel, dim3(1), dim3(LS_THREADS), 0, (hipStream_t)stream, n, x, scale, out);
    return pdgn_launch_status();
}

extern "C" int pdgn_mse_const(long long n, const float *x, float target, float scale, float *out, pdgn_stream_t stream) {
    if (n < 1) return PDGN_ERR_INVALID;
    hipLaunchKernelGGL(mse_const_fwd_kernel, dim3(1), dim3(LS_THREADS), 0, (hipStream_t)stream, n, x, target, scale, out);
    return pdgn_launch_status();
}

extern "C" int pdgn_mse_const_count(long long n, const float *x, float target, float scale, float boundary, float *out, int32_t *count,
                                    pdgn_stream_t stream) {
    if (n < 1 || n > 0x7fffffffLL || !x || !out || !count) return PDGN_ERR_INVALID;
    if (((uintptr_t)x | (uintptr_t)out | (uintptr_t)count) & 3) return PDGN_ERR_INVALID;
    hipLaunchKernelGGL(mse_const_count_fwd_kernel, dim3(1), dim3(LS_THREADS), 0, (hipStream_t)stream, n, x, target, scale, boundary, out,
                       count);
    return pdgn_launch_status();
}

extern "C" int pdgn_mse_const_backward(long long n, const float *x, float target, float scale, const float *g, float *dx,
                                       pdgn_stream_t stream) {
    if (n < 1) return PDGN_ERR_INVALID;
    const int grid = (int)(n < 256 * 64 ? cdiv(n, 256) : 64);
    hipLaunchKernelGGL(mse_const_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, n, x, target, scale, g, dx);
    return pdgn_launch_status();
}
