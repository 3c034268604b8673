// orient.hip -- pdgn_orient_normals: a consistent sign for every normal of a cloud, by propagation along a minimum spanning tree of the
// symmetrised neighbour graph (Hoppe et al. 1992; include/pdgn_hip.h).  The normals are the caller's
// (pdgn_estimate_normals, sign mode 0), the neighbour lists too (pdgn_knnquery).  One launch, nothing allocated, no float atomics.
//
// NORMATIVE RULES (tests/orient_mirror.py restates them in numpy; every fp32 operation below is one rounding, nothing contracted;
// dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z as in csrc/normals.hip).  One cloud: x (n,3), g (n,3), idx (n,k).
//
//   1  live      point i is live iff x_i and g_i are six finite numbers.  A dead point keeps o_i = g_i bit for bit, parent -2, and takes
//                no part in the graph.
//   2  edges     for a live u and a slot s, v = idx[u][s]: ignored where v is outside [0, n) (never dereferenced), v == u, or v is dead;
//                otherwise {u, v} is an undirected edge.  Repeats and edges seen from both ends count as one.
//   3  weight    w = 1 - |dot3(g_u, g_v)|, w = 0 where !(w > 0); wbits = the bits of w (they order as w does).  Symmetric bit for bit,
//                independent of the signs chosen so far.
//   4  rounds    best[u] = 2^64 - 1 for every live u, the tree empty.  Until every live point is in the tree:
//                a  choose, among the live points outside the tree, the u with the smallest (best[u] >> 32, u)
//                b  best[u] >> 32 == 0xFFFFFFFF: nothing outside touches the tree.  Drop u; take the live outside point with the largest
//                   x.z instead (compared as fp32 values, ties to the lowest index); parent -1, components += 1, o = -g iff g.z < 0
//                   (the top of a closed surface: its outward normal points up).
//                   Otherwise p = (uint32)best[u] is the parent; o_u = -g_u iff dot3(g_u, o_p) < 0; weak += 1 iff
//                   best[u] >> 32 > bits(0.5f) (a tree edge across more than 60 degrees: the sign there is a guess).
//                c  flipped += 1 where the sign changed; u joins; for every edge {u, t}, t outside: best[t] = min(best[t], wbits << 32 | u)
//   5  stats     (components, flipped, weak, dead) per cloud.
//
// Every update is a minimum over packed integer keys, so the order in which edges are visited cannot matter: the result is the same
// for every run, and the reverse adjacency below may be filled in whatever order the atomics resolve.
//
// SHAPE.  The rounds of a cloud are sequential (Prim), the clouds independent: ONE workgroup of ORI_THREADS = 512 per cloud, as
// csrc/fps.hip and csrc/auction.hip.  In LDS: best[] (8 n bytes), the normals' bits (12 n), the offsets of the reverse rows (4 n + 4)
// and their fill cursors (4 n), one live bit and one sign bit per point: 28 n bytes and a little, 115 KB at PDGN_ORIENT_MAX_N = 4096
// (beyond the 64 KB a launch gets unasked: hipFuncSetAttribute, as the auction).  Thread t owns the points s * 512 + t and keeps their
// "outside the tree" bits in one register.
// Prologue: load, live bits by ballot; in-degrees with LDS integer atomics over all n k slots; an exclusive scan; the reverse rows
// (for every valid slot (u -> v) the entry u in row v) into the caller's workspace, n k ints per cloud.  The same workgroup reads them
// back after a fence and a barrier: nothing crosses workgroups.
// A round: every thread takes the smallest key of its outside points, the wave's minimum goes through DPP (the steps of fps.hip, on
// `<`), one LDS slot per wave, barrier, every wave reduces the 8 slots.  Then all threads read the winner's parent and normal (LDS
// broadcasts) and decide the sign alike; the threads split the winner's forward row (k slots, checked by rule 2) and its reverse row
// (valid by construction) and take atomicMin on the 64-bit LDS keys; second barrier.  The root search is a second reduction of the
// same form on (ordered bits of x.z, ~index), and runs only when a component starts.
#include "common.h"

#include <math.h>

#define ORI_THREADS 512
#define ORI_WAVES (ORI_THREADS / PDGN_WAVE)
#define ORI_MAX_PPT (PDGN_ORIENT_MAX_N / ORI_THREADS)
static_assert(ORI_WAVES == 8, "the cross-wave stage reduces 8 slots with three DPP steps");
static_assert(ORI_MAX_PPT <= 32, "a thread's outside bits are one register");

typedef unsigned long long u64;

#define ORI_NONE 0xFFFFFFFFFFFFFFFFull
#define ORI_HI 0xFFFFFFFF00000000ull
#define ORI_WEAK_BITS 0x3F000000u                                // bits(0.5f)

struct OriArgs {
    int n, k;
    const float *xyz;
    const int32_t *idx;
    const float *gin;                                            // may be == out
    float *out;
    int32_t *parent, *stats;                                     // nullable
    int32_t *ws;                                                 // n k ints per cloud
};

// ---- the DPP reductions of csrc/fps.hip, on `<` (a local copy: fps.hip stays as it is)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ u64 ori_dpp_u64(u64 v) {
    const int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
    const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xF, false);
    const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xF, false);
    return ((u64)ohi << 32) | olo;
}

template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ u64 ori_dpp_min(u64 v) {
    const u64 o = ori_dpp_u64<CTRL, ROW_MASK>(v);
    return o < v ? o : v;
}

#define ORI_QUAD_XOR1 0xB1                                       // quad_perm:[1,0,3,2]
#define ORI_QUAD_XOR2 0x4E                                       // quad_perm:[2,3,0,1]
#define ORI_ROW_HALF_MIRROR 0x141                                // lane l of a row <- lane 7 - l of its half
#define ORI_ROW_MIRROR 0x140                                     // lane l of a row <- lane 15 - l
#define ORI_ROW_BCAST15 0x142                                    // lane 15 of each row -> the next row
#define ORI_ROW_BCAST31 0x143                                    // lane 31 -> rows 2 and 3

// min over the 8 lanes of each aligned group of 8, in every lane of the group
__device__ __forceinline__ u64 ori_min8(u64 v) {
    v = ori_dpp_min<ORI_QUAD_XOR1>(v);
    v = ori_dpp_min<ORI_QUAD_XOR2>(v);
    return ori_dpp_min<ORI_ROW_HALF_MIRROR>(v);
}

// min over the wave, uniform
__device__ __forceinline__ u64 ori_wave_min(u64 v) {
    v = ori_dpp_min<ORI_ROW_MIRROR>(ori_min8(v));                // every lane: its row's min
    v = ori_dpp_min<ORI_ROW_BCAST15, 0xA>(v);                    // rows 1 and 3: min with the row before
    v = ori_dpp_min<ORI_ROW_BCAST31, 0xC>(v);                    // row 3: min of all four
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
    return ((u64)hi << 32) | lo;
}

// the workgroup's minimum of one key per thread, uniform: `slot` holds one entry per wave.  ONE barrier; the caller keeps another
// barrier between this call's reads and the next write of the same slots.
__device__ __forceinline__ u64 ori_block_min(u64 v, u64 *slot) {
    const u64 w = ori_wave_min(v);
    if (lane_id() == 0) slot[threadIdx.x >> 6] = w;
    __syncthreads();
    const u64 m = ori_min8(slot[lane_id() & (ORI_WAVES - 1)]);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)m);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(m >> 32));
    return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ bool ori_bit(const unsigned *words, int i) { return (words[i >> 5] >> (i & 31)) & 1u; }

// bytes of dynamic LDS for a cloud of n points (the kernel's carve-up below)
static size_t ori_lds_bytes(int n) { return (size_t)n * 28 + 4 + (size_t)cdiv(n, 64) * 16; }

__global__ __launch_bounds__(ORI_THREADS) void orient_kernel(OriArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ori_lds[];
    __shared__ u64 s_slot[ORI_WAVES];                            // the round's reduction
    __shared__ u64 s_root[ORI_WAVES];                            // the root search's
    __shared__ int s_wsum[ORI_WAVES];
    __shared__ int s_dead;
    const int n = a.n, k = a.k, tid = threadIdx.x, lane = tid & (PDGN_WAVE - 1), wave = tid >> 6;
    const int words = 2 * ((n + 63) >> 6);
    u64 *best = (u64 *)ori_lds;                                  // n
    unsigned *g = (unsigned *)(best + n);                        // 3 n: the normals' bits, point-major
    int *roff = (int *)(g + 3 * n);                              // n + 1: reverse row v is rev[roff[v] .. roff[v + 1])
    int *cur = roff + n + 1;                                     // n: in-degree, then fill cursor
    unsigned *livew = (unsigned *)(cur + n);                     // one bit per point
    unsigned *flipw = livew + words;
    const size_t cloud = (size_t)blockIdx.x * n;
    const float *x = a.xyz + cloud * 3;
    const int32_t *idx = a.idx + cloud * k;
    int32_t *rev = a.ws + cloud * k;
    int32_t *parent = a.parent ? a.parent + cloud : nullptr;
    const int ppt = (n + ORI_THREADS - 1) / ORI_THREADS;

    // ---- prologue 1: the normals into LDS, live bits, best = none
    if (tid == 0) s_dead = 0;
    for (int w = tid; w < words; w += ORI_THREADS) flipw[w] = 0u;
    __syncthreads();
    unsigned outside = 0u;                                       // bit s: point s * 512 + tid is live and not yet in the tree
    int dead = 0;
    for (int s = 0; s < ppt; ++s) {
        const int i = s * ORI_THREADS + tid;
        bool live = false;
        if (i < n) {
            const float gx = a.gin[(cloud + i) * 3], gy = a.gin[(cloud + i) * 3 + 1], gz = a.gin[(cloud + i) * 3 + 2];
            live = isfinite(x[3 * i]) && isfinite(x[3 * i + 1]) && isfinite(x[3 * i + 2]) && isfinite(gx) && isfinite(gy) && isfinite(gz);
            g[3 * i] = __float_as_uint(gx), g[3 * i + 1] = __float_as_uint(gy), g[3 * i + 2] = __float_as_uint(gz);
            best[i] = ORI_NONE;
            cur[i] = 0;
            if (live) outside |= 1u << s;
            else {
                ++dead;
                if (parent) parent[i] = -2;
            }
        }
        const u64 m = __ballot(live);
        const int i0 = s * ORI_THREADS + wave * PDGN_WAVE;       // (a multiple of 64: two whole words)
        if (lane == 0 && i0 < n) livew[i0 >> 5] = (unsigned)m, livew[(i0 >> 5) + 1] = (unsigned)(m >> 32);
    }
    if (dead) atomicAdd(&s_dead, dead);
    __syncthreads();
    const int nlive = n - s_dead;

    // ---- prologue 2: in-degrees of the valid slots (rule 2)
    const int slots = n * k;
    for (int e = tid; e < slots; e += ORI_THREADS) {
        const int u = e / k, v = idx[e];
        if ((unsigned)v < (unsigned)n && v != u && ori_bit(livew, u) && ori_bit(livew, v)) atomicAdd(&cur[v], 1);
    }
    __syncthreads();

    // ---- prologue 3: exclusive scan; thread t owns the `ppt` consecutive points from t * ppt on
    {
        const int lo = min(tid * ppt, n), hi = min(lo + ppt, n);
        int sum = 0;
        for (int i = lo; i < hi; ++i) sum += cur[i];
        int inc = sum;
#pragma unroll
        for (int off = 1; off < PDGN_WAVE; off <<= 1) {
            const int o = __shfl_up(inc, off);
            if (lane >= off) inc += o;
        }
        if (lane == PDGN_WAVE - 1) s_wsum[wave] = inc;
        __syncthreads();
        int run = inc - sum;
        for (int w = 0; w < wave; ++w) run += s_wsum[w];
        for (int i = lo; i < hi; ++i) {
            const int d = cur[i];
            roff[i] = run, cur[i] = run;
            run += d;
        }
        if (tid == ORI_THREADS - 1) roff[n] = run;               // (its points are the last ones, or none: the total)
    }
    __syncthreads();

    // ---- prologue 4: the reverse rows
    for (int e = tid; e < slots; e += ORI_THREADS) {
        const int u = e / k, v = idx[e];
        if ((unsigned)v < (unsigned)n && v != u && ori_bit(livew, u) && ori_bit(livew, v)) rev[atomicAdd(&cur[v], 1)] = u;
    }
    __threadfence_block();
    __syncthreads();

    // ---- the rounds
    int components = 0, flipped = 0, weak = 0;                   // (uniform: every thread counts alike)
    for (int round = 0; round < nlive; ++round) {
        // a: choose
        u64 mine = ORI_NONE;
        for (int s = 0; s < ppt; ++s)
            if ((outside >> s) & 1u) {
                const int i = s * ORI_THREADS + tid;
                const u64 key = (best[i] & ORI_HI) | (unsigned)i;
                mine = key < mine ? key : mine;
            }
        const u64 win = ori_block_min(mine, s_slot);
        int u = (int)(unsigned)win;
        bool flip;
        int par;
        if ((unsigned)(win >> 32) == 0xFFFFFFFFu) {
            // b: a component starts at the highest outside point.  Largest (ordered bits of z, ~i) = smallest of the complement.
            u64 top = ORI_NONE;
            for (int s = 0; s < ppt; ++s)
                if ((outside >> s) & 1u) {
                    const int i = s * ORI_THREADS + tid;
                    const unsigned zb = __float_as_uint(__fadd_rn(x[3 * i + 2], 0.0f));         // (-0 becomes +0: they compare equal)
                    const unsigned ord = zb ^ ((zb >> 31) ? 0xFFFFFFFFu : 0x80000000u);         // orders as the value does
                    const u64 key = ~(((u64)ord << 32) | (0xFFFFFFFFu - (unsigned)i));
                    top = key < top ? key : top;
                }
            u = (int)(unsigned)ori_block_min(top, s_root);       // low word: ~(~i) = i
            par = -1;
            ++components;
            flip = __uint_as_float(g[3 * u + 2]) < 0.f;
        } else {
            const u64 b = best[u];
            par = (int)(unsigned)b;
            const unsigned sp = ori_bit(flipw, par) ? 0x80000000u : 0u;
            const float d = dot3_rn(__uint_as_float(g[3 * u]), __uint_as_float(g[3 * u + 1]), __uint_as_float(g[3 * u + 2]),
                                    __uint_as_float(g[3 * par] ^ sp), __uint_as_float(g[3 * par + 1] ^ sp),
                                    __uint_as_float(g[3 * par + 2] ^ sp));
            flip = d < 0.f;
            weak += (unsigned)(b >> 32) > ORI_WEAK_BITS;
        }
        // c: update
        flipped += flip;
        if ((u & (ORI_THREADS - 1)) == tid) outside &= ~(1u << (u / ORI_THREADS));
        if (tid == 0) {
            if (flip) flipw[u >> 5] |= 1u << (u & 31);           // (read from the next round on: behind the barrier below)
            if (parent) parent[u] = par;
        }
        const float ux = __uint_as_float(g[3 * u]), uy = __uint_as_float(g[3 * u + 1]), uz = __uint_as_float(g[3 * u + 2]);
        const int r0 = roff[u], nrev = roff[u + 1] - r0;
        for (int e = tid; e < k + nrev; e += ORI_THREADS) {
            int t;
            if (e < k) {
                t = idx[(size_t)u * k + e];
                if (!((unsigned)t < (unsigned)n && t != u && ori_bit(livew, t))) continue;
            } else {
                t = rev[r0 + (e - k)];
            }
            // (a t inside the tree takes the minimum too: its key is never read again)
            float w = __fsub_rn(1.0f, fabsf(dot3_rn(ux, uy, uz, __uint_as_float(g[3 * t]), __uint_as_float(g[3 * t + 1]),
                                                    __uint_as_float(g[3 * t + 2]))));
            w = w > 0.f ? w : 0.f;
            atomicMin(&best[t], ((u64)__float_as_uint(w) << 32) | (unsigned)u);
        }
        __syncthreads();
    }

    // ---- the outputs: the sign bit alone changes
    for (int s = 0; s < ppt; ++s) {
        const int i = s * ORI_THREADS + tid;
        if (i < n) {
            const unsigned sg = ori_bit(flipw, i) ? 0x80000000u : 0u;
            float *o = a.out + (cloud + i) * 3;
            o[0] = __uint_as_float(g[3 * i] ^ sg), o[1] = __uint_as_float(g[3 * i + 1] ^ sg), o[2] = __uint_as_float(g[3 * i + 2] ^ sg);
        }
    }
    if (tid == 0 && a.stats) {
        int32_t *st = a.stats + (size_t)blockIdx.x * 4;
        st[0] = components, st[1] = flipped, st[2] = weak, st[3] = n - nlive;
    }
}

static bool ori_shape_ok(int b, int n, int k) {
    return b >= 1 && n >= 1 && n <= PDGN_ORIENT_MAX_N && k >= 1 && k <= PDGN_NORMALS_MAX_K && (long long)b * n <= (1LL << 28);
}

extern "C" long long pdgn_orient_workspace_ints(int b, int n, int k) {
    if (!ori_shape_ok(b, n, k)) return PDGN_ERR_INVALID;
    return (long long)b * n * k;
}

extern "C" int pdgn_orient_normals(int b, int n, int k, const float *xyz, const int32_t *idx, const float *normals_in, float *normals_out,
                                   int32_t *parent, int32_t *stats, int32_t *workspace, pdgn_stream_t stream) {
    // host-side checks only: nothing here touches the device
    if (!ori_shape_ok(b, n, k)) return PDGN_ERR_INVALID;
    if (!xyz || !idx || !normals_in || !normals_out || !workspace) return PDGN_ERR_INVALID;
    if (((uintptr_t)xyz | (uintptr_t)idx | (uintptr_t)normals_in | (uintptr_t)normals_out | (uintptr_t)parent | (uintptr_t)stats |
         (uintptr_t)workspace) & 3)
        return PDGN_ERR_INVALID;
    OriArgs a = {};
    a.n = n, a.k = k, a.xyz = xyz, a.idx = idx, a.gin = normals_in, a.out = normals_out, a.parent = parent, a.stats = stats, a.ws = workspace;
    const size_t lds = ori_lds_bytes(n);
    if (lds > 60 * 1024) {  // with the kernel's static 0.2 KB the total nears the 64 KB a launch gets unasked: opt in
        hipError_t e = hipFuncSetAttribute((const void *)orient_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(orient_kernel, dim3(b), dim3(ORI_THREADS), lds, (hipStream_t)stream, a);
    return pdgn_launch_status();
}
