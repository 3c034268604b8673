// auction.hip -- pdgn_auction_assign / _assign_indexed / _cost_grad: the exact earth mover's distance between two clouds of n
// points as an assignment problem on integer costs.  No reference counterpart: the reference has
// approxmatch only (structural.hip restates it).  tests/auction_mirror.py is this file in numpy, element for element.
//
// Costs.  cmax = the diagonal of the bounding box of both clouds (an upper bound of every pairwise distance), q = cmax * 2^-20,
//     C_ij = rint(sqrt((dx*dx + dy*dy) + dz*dz) / q),  d = a_i - b_j,  every fp32 operation rounded on its own,
// recomputed from the coordinates whenever a bidder looks at an object: no n x n matrix exists.  S_ij = C_ij * (n + 1), so that
// the last phase's eps = 1 leaves n * eps < n + 1 = one unit of C: the assignment is an optimum of the integer problem.
//
// Auction (Bertsekas, forward, eps-scaling).  Prices are unsigned 64-bit, start at 0 and only rise.  eps = max(1, (n + 1) * 2^20 / 4),
// divided by 5 per phase down to 1; a phase starts with nobody assigned and the prices of the phase before.  A Jacobi round:
//   scan     one WAVE per unassigned bidder i (late rounds have a handful of bidders: their cost follows the number of bids):
//            lane l looks at the objects j = l, l + 64, ..; key = (S_ij + price_j) << 11 | ((j - i) mod n); the two smallest keys
//            of the wave (two DPP reductions) give the best object j1 -- among equal values the first one at or after the
//            bidder's own index, so that bidders with identical rows spread over objects instead of all raising one --
//            and the second best value w2.  bid = price_j1 + (w2 - w1) + eps; lane 0 does a 64-bit LDS atomic max of
//            bid << 11 | (2047 - i) on the object's slot: the highest bid, the lowest bidder among equal bids.  Slots are never
//            cleared: a later bid exceeds the object's price, which is the largest bid ever made on it.
//   resolve  one LANE per bidder of the round: the winner takes the object (owner, price, assignment) and puts the bidder it
//            displaced on the next round's list; a loser puts itself there.  The list's order is arrival order, and nothing
//            depends on it: the outcome of a round is a function of the SET of bidders.
// Two barriers per round, three where waves share a bidder: with at most half as many bidders as waves (the long tail of every
// phase) 2, 4, .. 16 waves scan one bidder's objects in slices and one lane merges their two smallest keys.
// Every loop that depends on the data is capped: a phase runs at most 16 n + 64 rounds, a pair makes at most
// pdgn_auction_max_bids(n) bids, and a bid of 2^51 or more (the packed keys hold 52 bits of value) counts as a cap.  A capped pair
// keeps what it has assigned, the rest is completed in index order, status = 1.  A pair without a finite positive quantum (all
// points equal, a coordinate or the diagonal not finite, a computed diagonal below 2^-106: its squares are denormal for extents
// below 2^-63 and vanish near 2^-75) gets the identity and status = 2 before any loop.
//
// One workgroup per pair, everything in LDS: 56 bytes per point (six coordinate planes, price, bid slot, owner, assignment, two
// bidder lists) -- 112 KB at n = 2048 = PDGN_AUCTION_MAX_N -- and 256 / 512 / 1024 threads for n <= 256 / 1024 / 2048.
#include <math.h>

#include "common.h"

#define AUC_QBITS 20
#define AUC_EPS_DIV 5
#define AUC_ROT_BITS 11
#define AUC_ROT_MASK ((1u << AUC_ROT_BITS) - 1)
#define AUC_PRICE_BITS 51
static_assert(PDGN_AUCTION_MAX_N == 1 << AUC_ROT_BITS, "a rotation and an inverted bidder index take AUC_ROT_BITS bits of a key");
static_assert(AUC_PRICE_BITS + 1 + AUC_ROT_BITS <= 64, "value + price below 2^52, shifted by the index bits, fits 64 bits");

typedef unsigned long long u64;

static inline u64 auction_eps0(int n) {
    const u64 e = ((u64)(n + 1) << AUC_QBITS) / 4;
    return e > 1 ? e : 1;
}

static inline int auction_phases(int n) {
    int count = 1;
    for (u64 e = auction_eps0(n); e > 1; e = e / AUC_EPS_DIV > 1 ? e / AUC_EPS_DIV : 1) ++count;
    return count;
}

extern "C" int pdgn_auction_quantum_bits(void) { return AUC_QBITS; }

extern "C" long long pdgn_auction_max_bids(int n) {
    if (n < 1 || n > PDGN_AUCTION_MAX_N) return PDGN_ERR_INVALID;
    return 64LL * n * auction_phases(n);
}

struct AucArgs {
    int n, max_rounds;
    long long max_bids;
    const float *xyz1, *xyz2;
    const int32_t *ia, *ib;                                      // nullable: pair p = (cloud p, cloud p)
    int32_t *assign;                                             // nullable
    float *cost;
    int32_t *status;
    long long *bids;                                             // nullable
};

// the value of another lane (DPP control CTRL) where the control and the row mask give one, else this lane's own (fps.hip's)
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ u64 auc_dpp_min(u64 v) {
    const int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
    const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xF, false);
    const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xF, false);
    const u64 o = ((u64)ohi << 32) | olo;
    return o < v ? o : v;
}

// min over the wave, uniform
__device__ __forceinline__ u64 wave_min_u64(u64 v) {
    v = auc_dpp_min<0xB1>(v);                                    // quad_perm:[1,0,3,2]
    v = auc_dpp_min<0x4E>(v);                                    // quad_perm:[2,3,0,1]
    v = auc_dpp_min<0x141>(v);                                   // row_half_mirror
    v = auc_dpp_min<0x140>(v);                                   // row_mirror: every lane its row's min
    v = auc_dpp_min<0x142, 0xA>(v);                              // row_bcast:15 into rows 1 and 3
    v = auc_dpp_min<0x143, 0xC>(v);                              // row_bcast:31 into rows 2 and 3: lane 63 has all four
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
    return ((u64)hi << 32) | lo;
}

// |a - b|^2 in the one order the mirror spells.  Its root is sqrtf (correctly rounded: v_sqrt_f32 and a one-ulp correction), never
// __fsqrt_rn, which hipcc lowers to the bare instruction: one ulp of a distance is 2^-4 of a quantum at the far end of the range
__device__ __forceinline__ float auc_sq(float px, float py, float pz, float qx, float qy, float qz) {
    const float dx = __fsub_rn(px, qx), dy = __fsub_rn(py, qy), dz = __fsub_rn(pz, qz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// bidder i's bid from the two smallest keys of its row: on the best object, at its price plus the margin to the second best plus eps
__device__ __forceinline__ void auc_bid(int i, int n, u64 g1, u64 g2, u64 eps, const u64 *price, u64 *slot, int *asg, int *cap) {
    int j1 = i + (int)((unsigned)g1 & AUC_ROT_MASK);
    if (j1 >= n) j1 -= n;
    const u64 bid = price[j1] + ((g2 >> AUC_ROT_BITS) - (g1 >> AUC_ROT_BITS)) + eps;
    if (bid >> AUC_PRICE_BITS) {
        *cap = 1;
    } else {
        atomicMax(&slot[j1], (bid << AUC_ROT_BITS) | (AUC_ROT_MASK - (unsigned)i));
        asg[i] = ~j1;
    }
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void auction_kernel(AucArgs a) {
    constexpr int WAVES = THREADS / PDGN_WAVE;
    extern __shared__ __attribute__((aligned(16))) unsigned char auc_lds[];
    __shared__ float s_box[WAVES][6];
    __shared__ int s_bad[WAVES];
    __shared__ int s_cnt[2];
    __shared__ int s_cap;
    __shared__ u64 s_part[WAVES][2];                              // a wave's two smallest keys, where waves share a bidder
    const int n = a.n, np = (n + 1) & ~1;                         // plane stride: 8-byte planes stay aligned
    u64 *price = (u64 *)auc_lds, *slot = price + np;
    float *ax = (float *)(slot + np), *ay = ax + np, *az = ay + np, *bx = az + np, *by = bx + np, *bz = by + np;
    int *owner = (int *)(bz + np), *asg = owner + np, *list0 = asg + np, *list1 = list0 + np;
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & (PDGN_WAVE - 1), wave = tid >> 6;
    const float *A = a.xyz1 + (size_t)(a.ia ? a.ia[pair] : pair) * n * 3;
    const float *B = a.xyz2 + (size_t)(a.ib ? a.ib[pair] : pair) * n * 3;

    // ---- the clouds into LDS; their bounding box and whether every coordinate is finite
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int bad = 0;
    for (int i = tid; i < n; i += THREADS) {
        const float p[6] = {A[3 * i], A[3 * i + 1], A[3 * i + 2], B[3 * i], B[3 * i + 1], B[3 * i + 2]};
        ax[i] = p[0], ay[i] = p[1], az[i] = p[2], bx[i] = p[3], by[i] = p[4], bz[i] = p[5];
        price[i] = 0, slot[i] = 0;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            bad |= !(fabsf(p[c]) < INFINITY);
            lo[c % 3] = fminf(lo[c % 3], p[c]), hi[c % 3] = fmaxf(hi[c % 3], p[c]);
        }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) lo[c] = fminf(lo[c], __shfl_xor(lo[c], off)), hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], off));
        bad |= __shfl_xor(bad, off);
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s_box[wave][c] = lo[c], s_box[wave][3 + c] = hi[c];
        s_bad[wave] = bad;
    }
    if (tid == 0) s_cap = 0;
    __syncthreads();
    for (int w = 0; w < WAVES; ++w) {
#pragma unroll
        for (int c = 0; c < 3; ++c) lo[c] = fminf(lo[c], s_box[w][c]), hi[c] = fmaxf(hi[c], s_box[w][3 + c]);
        bad |= s_bad[w];
    }
    const float ex = __fsub_rn(hi[0], lo[0]), ey = __fsub_rn(hi[1], lo[1]), ez = __fsub_rn(hi[2], lo[2]);
    const float cmax = bad ? NAN : sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)), __fmul_rn(ez, ez)));
    const float q = __fmul_rn(cmax, 0x1p-20f);
    const bool finite = cmax < INFINITY;                         // (false for NaN)
    const bool degenerate = __builtin_amdgcn_readfirstlane(!(finite && q >= 0x1p-126f));

    long long bids = 0;
    int capped = 0;
    if (degenerate || n == 1) {
        for (int i = tid; i < n; i += THREADS) asg[i] = i;
    } else {
        u64 eps = ((u64)(n + 1) << AUC_QBITS) / 4;               // (n >= 2: at least 2^18 * 3)
        const unsigned scale = (unsigned)(n + 1);
        for (;;) {
            // ---- a phase: nobody assigned, the prices stay
            for (int i = tid; i < n; i += THREADS) owner[i] = -1, asg[i] = -1, list0[i] = i;
            if (tid == 0) s_cnt[0] = n;
            __syncthreads();
            int rounds = 0, cur = 0;
            for (;;) {
                const int cnt = __builtin_amdgcn_readfirstlane(s_cnt[cur]);
                if (cnt == 0) break;
                if (rounds >= a.max_rounds || bids + cnt > a.max_bids) {
                    capped = 1;
                    break;
                }
                ++rounds, bids += cnt;
                if (tid == 0) s_cnt[cur ^ 1] = 0;
                const int *list = cur ? list1 : list0;
                int *next = cur ? list0 : list1;
                // ---- scan: a wave per bidder; with at most half as many bidders as waves, `share` waves per bidder, each on its
                // own slice of the objects (the long tail of a phase is rounds of one or two bidders: one wave would walk all n
                // objects while fifteen wait), their two smallest keys merged behind one more barrier
                int share = 1;
                while (2 * share * cnt <= WAVES) share *= 2;     // (uniform)
                for (int e = wave / share; e < cnt; e += WAVES / share) {
                    const int i = __builtin_amdgcn_readfirstlane(list[e]);
                    const float px = ax[i], py = ay[i], pz = az[i];
                    u64 b1 = ~0ull, b2 = ~0ull;
                    for (int j = (wave % share) * PDGN_WAVE + lane; j < n; j += share * PDGN_WAVE) {
                        const float d = sqrtf(auc_sq(px, py, pz, bx[j], by[j], bz[j]));
                        const unsigned c = (unsigned)rintf(__fdiv_rn(d, q));
                        int rot = j - i;
                        rot += (rot >> 31) & n;                  // (j - i) mod n
                        const u64 key = (((u64)c * scale + price[j]) << AUC_ROT_BITS) | (unsigned)rot;
                        if (key < b1) b2 = b1, b1 = key;
                        else if (key < b2) b2 = key;
                    }
                    const u64 g1 = wave_min_u64(b1);
                    const u64 g2 = wave_min_u64(b1 == g1 ? b2 : b1);   // keys are distinct: one lane owns g1
                    if (lane == 0) {
                        if (share == 1) auc_bid(i, n, g1, g2, eps, price, slot, asg, &s_cap);
                        else s_part[wave][0] = g1, s_part[wave][1] = g2;
                    }
                }
                if (share > 1) {
                    __syncthreads();
                    if (tid < cnt) {                             // (share > 1: cnt <= WAVES / 2; bidder e's waves are e share .. e share + share - 1)
                        u64 g1 = ~0ull, g2 = ~0ull;
                        for (int g = 0; g < share; ++g) {
                            const u64 p1 = s_part[tid * share + g][0], p2 = s_part[tid * share + g][1];
                            if (p1 < g1) g2 = g1 < p2 ? g1 : p2, g1 = p1;
                            else g2 = g2 < p1 ? g2 : p1;
                        }
                        auc_bid(list[tid], n, g1, g2, eps, price, slot, asg, &s_cap);
                    }
                }
                __syncthreads();
                if (__builtin_amdgcn_readfirstlane(s_cap)) {     // (written before the barrier only)
                    capped = 1;
                    break;
                }
                // ---- resolve: a lane per bidder
                for (int e = tid; e < cnt; e += THREADS) {
                    const int i = list[e], j1 = ~asg[i];
                    const u64 key = slot[j1];
                    if ((int)(AUC_ROT_MASK - ((unsigned)key & AUC_ROT_MASK)) == i) {
                        const int old = owner[j1];
                        owner[j1] = i, price[j1] = key >> AUC_ROT_BITS, asg[i] = j1;
                        if (old >= 0) asg[old] = -1, next[atomicAdd(&s_cnt[cur ^ 1], 1)] = old;
                    } else {
                        asg[i] = -1, next[atomicAdd(&s_cnt[cur ^ 1], 1)] = i;
                    }
                }
                __syncthreads();
                cur ^= 1;
            }
            if (capped || eps == 1) break;
            eps = eps / AUC_EPS_DIV > 1 ? eps / AUC_EPS_DIV : 1;
            __syncthreads();                                     // every thread has read the empty list's count
        }
        if (capped) {
            // ---- the rest in index order on both sides (owner and the non-negative assignments agree at every barrier)
            __syncthreads();
            if (tid == 0) {
                int j = 0;
                for (int i = 0; i < n; ++i) {
                    if (asg[i] >= 0) continue;
                    while (j < n - 1 && owner[j] >= 0) ++j;
                    asg[i] = j, owner[j] = i;
                }
            }
        }
    }
    __syncthreads();

    // ---- outputs; the cost of the assignment in fp32: lane l adds i = l, l + 64, .. in order, then a fixed tree over the lanes
    if (a.assign)
        for (int i = tid; i < n; i += THREADS) a.assign[(size_t)pair * n + i] = asg[i];
    if (wave == 0) {
        float sum = 0.f;
        for (int i = lane; i < n; i += PDGN_WAVE) {
            const int j = asg[i];
            sum = __fadd_rn(sum, sqrtf(auc_sq(ax[i], ay[i], az[i], bx[j], by[j], bz[j])));
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) sum = __fadd_rn(sum, __shfl_xor(sum, off));
        if (lane == 0) {
            a.cost[pair] = finite ? sum : NAN;
            a.status[pair] = degenerate ? 2 : capped;
            if (a.bids) a.bids[pair] = bids;
        }
    }
}

static int auction_launch(int pairs, const AucArgs &a, pdgn_stream_t stream) {
    const int np = (a.n + 1) & ~1;
    const size_t lds = (size_t)np * 56;                          // (beside it the kernel's static LDS: the attribute below is the dynamic part alone)
    hipStream_t s = (hipStream_t)stream;
#define AUC_LAUNCH(T)                                                                                                              \
    do {                                                                                                                           \
        if (T == 1024) { /* n > 1024: with the kernel's static 0.7 KB the total passes the 64 KB a launch gets unasked from n = 1158 */ \
            hipError_t e = hipFuncSetAttribute((const void *)auction_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            if (e != hipSuccess) return (int)e;                                                                                    \
        }                                                                                                                          \
        hipLaunchKernelGGL(auction_kernel<T>, dim3(pairs), dim3(T), lds, s, a);                                                    \
    } while (0)
    if (a.n <= 256) AUC_LAUNCH(256);
    else if (a.n <= 1024) AUC_LAUNCH(512);
    else AUC_LAUNCH(1024);
#undef AUC_LAUNCH
    return pdgn_launch_status();
}

static bool auction_fill(AucArgs &a, int n) {
    if (n < 1 || n > PDGN_AUCTION_MAX_N) return false;
    a.n = n, a.max_rounds = 16 * n + 64, a.max_bids = pdgn_auction_max_bids(n);
    return true;
}

extern "C" int pdgn_auction_assign(int b, int n, const float *xyz1, const float *xyz2, int32_t *assign, float *cost, int32_t *status,
                                   long long *bids, pdgn_stream_t stream) {
    // host-side checks only: nothing here touches the device
    AucArgs a = {};
    if (b < 0 || !auction_fill(a, n)) return PDGN_ERR_INVALID;
    if (b == 0) return 0;
    if (!xyz1 || !xyz2 || !assign || !cost || !status) return PDGN_ERR_INVALID;
    if ((((uintptr_t)xyz1 | (uintptr_t)xyz2 | (uintptr_t)assign | (uintptr_t)cost | (uintptr_t)status) & 3) || ((uintptr_t)bids & 7))
        return PDGN_ERR_INVALID;
    a.xyz1 = xyz1, a.xyz2 = xyz2, a.assign = assign, a.cost = cost, a.status = status, a.bids = bids;
    return auction_launch(b, a, stream);
}

extern "C" int pdgn_auction_assign_indexed(int npairs, int n, const float *xyz1, const int32_t *ia, const float *xyz2, const int32_t *ib,
                                           float *cost, int32_t *status, pdgn_stream_t stream) {
    // host-side checks only: nothing here touches the device
    AucArgs a = {};
    if (npairs < 0 || !auction_fill(a, n)) return PDGN_ERR_INVALID;
    if (npairs == 0) return 0;
    if (!xyz1 || !xyz2 || !ia || !ib || !cost || !status) return PDGN_ERR_INVALID;
    if (((uintptr_t)xyz1 | (uintptr_t)xyz2 | (uintptr_t)ia | (uintptr_t)ib | (uintptr_t)cost | (uintptr_t)status) & 3) return PDGN_ERR_INVALID;
    a.xyz1 = xyz1, a.xyz2 = xyz2, a.ia = ia, a.ib = ib, a.cost = cost, a.status = status;
    return auction_launch(npairs, a, stream);
}

// grad1[i] = g (a_i - b_pi(i)) / sqrt(max(|a_i - b_pi(i)|^2, 1e-20)), grad2[pi(i)] = -grad1[i]: pi is a bijection, so every row of
// both gradients is written exactly once and nothing is added.  An index outside [0, n) (not an assignment) writes no row.
__global__ __launch_bounds__(256) void auction_grad_kernel(int n, long long total, const float *xyz1, const float *xyz2, const int32_t *assign,
                                                           const float *g, float *grad1, float *grad2) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long long pair = t / n;
    const int j = assign[t];
    if (j < 0 || j >= n) return;
    const float *p = xyz1 + t * 3, *r = xyz2 + (pair * n + j) * 3;
    const float dx = p[0] - r[0], dy = p[1] - r[1], dz = p[2] - r[2];
    const float s = g[pair] / sqrtf(fmaxf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)), 1e-20f));
    float *o1 = grad1 + t * 3, *o2 = grad2 + (pair * n + j) * 3;
    o1[0] = dx * s, o1[1] = dy * s, o1[2] = dz * s;
    o2[0] = -(dx * s), o2[1] = -(dy * s), o2[2] = -(dz * s);
}

extern "C" int pdgn_auction_cost_grad(int b, int n, const float *xyz1, const float *xyz2, const int32_t *assign, const float *g,
                                      float *grad1, float *grad2, pdgn_stream_t stream) {
    // host-side checks only: nothing here touches the device
    if (b < 0 || n < 1 || n > PDGN_AUCTION_MAX_N) return PDGN_ERR_INVALID;
    if (b == 0) return 0;
    if (!xyz1 || !xyz2 || !assign || !g || !grad1 || !grad2) return PDGN_ERR_INVALID;
    if (((uintptr_t)xyz1 | (uintptr_t)xyz2 | (uintptr_t)assign | (uintptr_t)g | (uintptr_t)grad1 | (uintptr_t)grad2) & 3) return PDGN_ERR_INVALID;
    const long long total = (long long)b * n;
    hipLaunchKernelGGL(auction_grad_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, n, total, xyz1, xyz2, assign, g,
                       grad1, grad2);
    return pdgn_launch_status();
}
