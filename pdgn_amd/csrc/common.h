// common.h -- shared helpers for the gfx950 kernels of libpdgn_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pdgn_hip.h"

#define PDGN_WAVE 64

static inline int pdgn_launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// Squared distance exactly as the reference kernels compute it after nvcc's FMA
// contraction (knnquery_cuda_kernel.cu:31, interpolation_cuda_kernel.cu:156):
// fma(dz,dz, fma(dy,dy, dx*dx)) with d = q - p.  The CPU oracle spells the same chain.
__device__ __forceinline__ float sqdist3(float qx, float qy, float qz, float px, float py, float pz) {
    float dx = qx - px, dy = qy - py, dz = qz - pz;
    return __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, __fmul_rn(dx, dx)));
}

// dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z, every product and sum rounded on its own: the dot product of every geometry kernel whose
// result is pinned bit for bit (normals, orient, reconstruct, meshdist, winding)
__device__ __forceinline__ float dot3_rn(float ax, float ay, float az, float bx, float by, float bz) {
    return __fadd_rn(__fadd_rn(__fmul_rn(ax, bx), __fmul_rn(ay, by)), __fmul_rn(az, bz));
}

// Whether a pointer an entry point was handed sits on a multiple of `to` bytes (a power of two); a null pointer does
static inline bool pdgn_aligned(const void *p, uintptr_t to) { return !((uintptr_t)p & (to - 1)); }

__device__ __forceinline__ int lane_id() { return threadIdx.x & (PDGN_WAVE - 1); }

// Host-side launchers one kernel file offers another (defined once, linked by name; each enqueues on `s` and allocates nothing).
// det.hip: CSR transpose of idx (b, E) over nt targets in ws = [cnt b*nt][rowptr b*(nt+1)][edges b*E] (det_ints(b, nt, E) ints, b <= 65535);
// every row lists its edges in INCREASING edge id, an index outside [0, nt) is in no row.
long long det_ints(long long b, long long nt, long long E);
int det_transpose(int b, int nt, long long E, const int32_t *idx, int *ws, int **rowptr, int **edges, hipStream_t s);
// repulsion.hip: the fixed-order means of a (b, n) array (that file's header block: one wave per cloud, the xor tree, fp64 across clouds)
void rp_reduce_launch(int b, int n, const float *s, float *loss, float *per_cloud, hipStream_t st);
