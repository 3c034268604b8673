// fps.hip -- pdgn_fps_order / pdgn_feed_fps_pyramid: farthest-point sampling with the cloud in registers.
// The iteration is furthestsampling's (sampling_cuda_kernel.cu:59-168; pointops_extra.hip keeps that launcher as it is):
// "mind = min(mind, d(last, .)); last = argmax mind", m - 1 times.  pointops_extra.hip re-reads the cloud and `temp` from
// global memory in every round and takes two barriers per round; this kernel is the one that sits in front of every
// training iteration (data.BatchFeeder, subsample="fps"), so a round here touches registers and 32 bytes of LDS per wave.
//
// One workgroup of FPS_THREADS = 512 (two waves per SIMD: a single wave issues a vector instruction every 4 cycles, two
// share the SIMD at 2) per cloud.  Thread t holds the PPT points i = s * 512 + t, s < PPT: x, y, z and the running
// minimum, 4 PPT registers, for the whole call.  Slots with i >= n hold minimum 0 and never change.
//
// A round:  every thread updates its PPT minima against the last point and keeps the largest
//     key = (bits of the fp32 minimum) << 32 | (0xFFFFFFFF - i)
// together with that point's coordinates.  The minimum is not negative, so its bits order as the value does: an unsigned max
// over keys is the largest minimum with ties to the lowest index (pdgn_furthestsampling's rule).  A slot beyond n has the
// key 0 << 32 | (0xFFFFFFFF - i), i >= n: below every real key, whatever the real minima are.  Keys are distinct.
// The wave's max goes through DPP (four steps inside a row of 16, two row broadcasts, one readlane); the one lane that owns it
// writes key and coordinates to its wave's LDS slot; ONE barrier; every wave reads the 8 slots (lane l slot l & 7), reduces
// them with three more DPP steps, and reads the winner's coordinates from the slot of the wave that owns the index.  Two
// alternating slot sets: a wave can reach round j + 2's write only after barrier j + 1, which every wave passes only after
// it has used (the next scan depends on them) what it read in round j.
// The winner's coordinates travel with the key, so the pyramid's gather p_k[b,:,j] = p4[b,:,order[b,j]] is three stores of
// values already in registers.
#include "common.h"
#include "philox.h"

#define FPS_THREADS 512
#define FPS_WAVES (FPS_THREADS / PDGN_WAVE)
#define FPS_MAX_PPT (PDGN_FPS_MAX_N / FPS_THREADS)
static_assert(FPS_WAVES == 8, "the cross-wave stage reduces 8 slots with three DPP steps");
static_assert(FPS_MAX_PPT == 16, "the dispatch below instantiates PPT = 1 2 4 8 16");

struct FpsArgs {
    int n, m;
    const float *src;                                            // pdgn_fps_order: xyz (b,n,3); the pyramid: p4 (B,3,N)
    const int32_t *start;                                        // pdgn_fps_order only, nullable
    int32_t *order;                                              // (b,m); the pyramid: nullable
    int r[3];                                                    // the pyramid's level sizes, r[2] = m
    float *p[3];
    unsigned k0, k1, t_lo, t_hi24, row0;
};

typedef unsigned long long u64;

// the value of another lane (DPP control CTRL) where the control and the row mask give one, else this lane's own
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ u64 dpp_u64(u64 v) {
    const int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
    const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xF, false);
    const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xF, false);
    return ((u64)ohi << 32) | olo;
}

template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ u64 dpp_max(u64 v) {
    const u64 o = dpp_u64<CTRL, ROW_MASK>(v);
    return o > v ? o : v;
}

#define DPP_QUAD_XOR1 0xB1                                       // quad_perm:[1,0,3,2]
#define DPP_QUAD_XOR2 0x4E                                       // quad_perm:[2,3,0,1]
#define DPP_ROW_HALF_MIRROR 0x141                                // lane l of a row <- lane 7 - l of its half
#define DPP_ROW_MIRROR 0x140                                     // lane l of a row <- lane 15 - l
#define DPP_ROW_BCAST15 0x142                                    // lane 15 of each row -> the next row
#define DPP_ROW_BCAST31 0x143                                    // lane 31 -> rows 2 and 3

// max over the 8 lanes of each aligned group of 8, in every lane of the group
__device__ __forceinline__ u64 max8_u64(u64 v) {
    v = dpp_max<DPP_QUAD_XOR1>(v);
    v = dpp_max<DPP_QUAD_XOR2>(v);
    return dpp_max<DPP_ROW_HALF_MIRROR>(v);
}

// max over the wave, uniform
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
    v = dpp_max<DPP_ROW_MIRROR>(max8_u64(v));                    // every lane: its row's max
    v = dpp_max<DPP_ROW_BCAST15, 0xA>(v);                        // rows 1 and 3: max with the row before
    v = dpp_max<DPP_ROW_BCAST31, 0xC>(v);                        // row 3: max of all four
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
    return ((u64)hi << 32) | lo;
}

// PYRAMID = false: pdgn_fps_order (point-major loader, indices out); true: pdgn_feed_fps_pyramid (channel-major loader, Philox
// start, the three levels out)
template <int PPT, bool PYRAMID>
__global__ __launch_bounds__(FPS_THREADS) void fps_reg_kernel(FpsArgs a) {
    __shared__ uint4 s_head[2][FPS_WAVES];                       // key low, key high, x, y
    __shared__ float s_z[2][FPS_WAVES];
    const int bs = blockIdx.x, tid = threadIdx.x, lane = tid & (PDGN_WAVE - 1), wave = tid >> 6;
    const int n = a.n, m = a.m;
    const float *src = a.src + (size_t)bs * n * 3;
    float px[PPT], py[PPT], pz[PPT], mind[PPT];
#pragma unroll
    for (int s = 0; s < PPT; ++s) {
        const int i = s * FPS_THREADS + tid;
        const bool real = i < n;
        px[s] = real ? src[PYRAMID ? i : 3 * i] : 0.f;
        py[s] = real ? src[PYRAMID ? n + i : 3 * i + 1] : 0.f;
        pz[s] = real ? src[PYRAMID ? 2 * n + i : 3 * i + 2] : 0.f;
        mind[s] = real ? 1e10f : 0.f;                            // (1e10: what pointops.py:24 fills `temp` with)
    }
    int cur;
    if (PYRAMID) {
        unsigned w[4];
        philox4x32_10(0u, a.row0 + (unsigned)bs, a.t_lo, (unsigned)PDGN_FEED_TAG_FPS | (a.t_hi24 << 8), a.k0, a.k1, w);
        cur = (int)__umulhi(w[0], (unsigned)n);
    } else {
        cur = a.start ? min(max(a.start[bs], 0), n - 1) : 0;     // (in range by contract; clamped so that a bad one cannot read outside xyz)
    }
    float cx = src[PYRAMID ? cur : 3 * cur], cy = src[PYRAMID ? n + cur : 3 * cur + 1], cz = src[PYRAMID ? 2 * n + cur : 3 * cur + 2];
    int32_t *order = a.order ? a.order + (size_t)bs * m : nullptr;
    for (int j = 0;; ++j) {
        // ---- column j of the outputs is the point (cur; cx cy cz)
        if (tid == 0 && order) order[j] = cur;
        if (PYRAMID && tid < 3) {
            const float v = tid == 0 ? cx : tid == 1 ? cy : cz;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (j < a.r[k]) a.p[k][((size_t)bs * 3 + tid) * a.r[k] + j] = v;
        }
        if (j + 1 >= m) break;                                   // (uniform)
        // ---- this thread's PPT minima against the last point; its largest key
        u64 best = 0;
        float bx = 0.f, by = 0.f, bz = 0.f;
#pragma unroll
        for (int s = 0; s < PPT; ++s) {
            const float d = fminf(sqdist3(px[s], py[s], pz[s], cx, cy, cz), mind[s]);
            mind[s] = d;
            const u64 key = ((u64)__float_as_uint(d) << 32) | (0xFFFFFFFFu - (unsigned)(s * FPS_THREADS + tid));
            if (key > best) best = key, bx = px[s], by = py[s], bz = pz[s];
        }
        // ---- the wave's: its owner (keys are distinct: one lane) publishes key and coordinates
        const u64 wmax = wave_max_u64(best);
        const int set = j & 1;
        if (best == wmax) {
            s_head[set][wave] = make_uint4((unsigned)best, (unsigned)(best >> 32), __float_as_uint(bx), __float_as_uint(by));
            s_z[set][wave] = bz;
        }
        __syncthreads();
        // ---- the workgroup's, in every wave
        const uint4 mine = s_head[set][lane & (FPS_WAVES - 1)];
        const u64 gmax = max8_u64(((u64)mine.y << 32) | mine.x);
        cur = __builtin_amdgcn_readfirstlane((int)(0xFFFFFFFFu - (unsigned)gmax));
        const int owner = (cur & (FPS_THREADS - 1)) >> 6;        // the wave of thread cur % 512
        const uint4 head = s_head[set][owner];
        cx = __uint_as_float(head.z), cy = __uint_as_float(head.w), cz = s_z[set][owner];
    }
}

template <bool PYRAMID>
static int fps_launch(int b, const FpsArgs &a, pdgn_stream_t stream) {
    const int ppt = cdiv(a.n, FPS_THREADS);
    const dim3 grid(b), block(FPS_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (ppt <= 1) hipLaunchKernelGGL((fps_reg_kernel<1, PYRAMID>), grid, block, 0, s, a);
    else if (ppt <= 2) hipLaunchKernelGGL((fps_reg_kernel<2, PYRAMID>), grid, block, 0, s, a);
    else if (ppt <= 4) hipLaunchKernelGGL((fps_reg_kernel<4, PYRAMID>), grid, block, 0, s, a);
    else if (ppt <= 8) hipLaunchKernelGGL((fps_reg_kernel<8, PYRAMID>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((fps_reg_kernel<16, PYRAMID>), grid, block, 0, s, a);
    return pdgn_launch_status();
}

extern "C" int pdgn_fps_order(int b, int n, int m, const float *xyz, const int32_t *start, int32_t *order, pdgn_stream_t stream) {
    // host-side checks only: nothing here touches the device
    if (b < 0 || n < 1 || n > PDGN_FPS_MAX_N || m < 1 || m > n) return PDGN_ERR_INVALID;
    if (b == 0) return 0;
    if (!xyz || !order || (((uintptr_t)xyz | (uintptr_t)order | (uintptr_t)start) & 3)) return PDGN_ERR_INVALID;
    FpsArgs a = {};
    a.n = n, a.m = m, a.src = xyz, a.start = start, a.order = order;
    return fps_launch<false>(b, a, stream);
}

extern "C" int pdgn_feed_fps_pyramid(int B, int N, int r1, int r2, int r3, const float *p4, unsigned long long seed, unsigned long long t,
                                     long long row0, float *p1, float *p2, float *p3, int32_t *order_out, pdgn_stream_t stream) {
    // host-side checks only: nothing here touches the device
    if (B < 1 || N < 1 || N > PDGN_FPS_MAX_N || r1 < 1 || r1 > r2 || r2 > r3 || r3 > N) return PDGN_ERR_INVALID;
    if (row0 < 0 || row0 + B > 0x100000000LL) return PDGN_ERR_INVALID;                        // the global row is one 32-bit counter word
    if (!p4 || !p1 || !p2 || !p3) return PDGN_ERR_INVALID;
    if (((uintptr_t)p4 | (uintptr_t)p1 | (uintptr_t)p2 | (uintptr_t)p3 | (uintptr_t)order_out) & 3) return PDGN_ERR_INVALID;
    FpsArgs a = {};
    a.n = N, a.m = r3, a.src = p4, a.order = order_out;
    a.r[0] = r1, a.r[1] = r2, a.r[2] = r3;
    a.p[0] = p1, a.p[1] = p2, a.p[2] = p3;
    a.k0 = (unsigned)seed, a.k1 = (unsigned)(seed >> 32);
    a.t_lo = (unsigned)t, a.t_hi24 = (unsigned)(t >> 32) & 0xffffffu;
    a.row0 = (unsigned)row0;
    return fps_launch<true>(B, a, stream);
}
