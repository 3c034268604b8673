// meshrec.h -- the face records of a mesh set and the walk over them, once: pdgn_mesh_dist_prepare (csrc/meshdist.hip) writes the records,
// md_distance_kernel (csrc/meshdist.hip) and wn_sum_kernel (csrc/winding.hip) read them.  The layout and the sizes below are the only
// statement of either; a kernel that consumes the records includes this header and so cannot disagree with the one that wrote them.
//
// RECORDS (pdgn_mesh_dist_prepare).  Slot i of the record array holds face order[i] (order = NULL: face i): three 16-byte words
// (a, bits(f)), (b, 0), (c, 0), f = -1 for a dead slot.  Slots keep inside their shape's range; a group is MESHREC_GROUP = 64 consecutive
// slots counted from the start of the shape's range, group_off[s] the index of shape s's first group, and per group two 16-byte words hold
// the box of its live faces (+inf / -inf for none).  One wave writes one group: lane l gathers slot l, the box is reduced across the lanes.
//
// THE WALK.  One thread per query point; a workgroup of MESHREC_THREADS = 256 owns a run of 256 points of one cloud.  The shape's records
// pass through LDS in chunks of MESHREC_CHUNK = 256 slots counted from the start of the shape's range, thread t staging slot j0 + t.  A
// wave takes the chunk one group at a time: lane l decides whether slot l of the group is to be visited by this wave (it is live; the
// distance kernel also culls), a ballot collects the decisions, and the wave walks the set bits, reading each surviving face's three words
// at a uniform address (broadcasts).
#pragma once
#include "common.h"

#include <math.h>

#define MESHREC_THREADS 256
#define MESHREC_CHUNK 256
#define MESHREC_GROUP 64
#define MESHREC_NAN_BITS 0x7FC00000u
static_assert(MESHREC_CHUNK == MESHREC_THREADS, "thread t stages slot j0 + t");
static_assert(MESHREC_GROUP == PDGN_WAVE, "lane l of a wave holds slot l of a group");
static_assert(MESHREC_CHUNK % MESHREC_GROUP == 0, "a chunk is whole groups");

struct MdVec {
    float x, y, z;
};

__device__ __forceinline__ MdVec md_sub(MdVec a, MdVec b) { return {__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y), __fsub_rn(a.z, b.z)}; }

__device__ __forceinline__ MdVec md_cross(MdVec u, MdVec v) {
    return {__fsub_rn(__fmul_rn(u.y, v.z), __fmul_rn(u.z, v.y)), __fsub_rn(__fmul_rn(u.z, v.x), __fmul_rn(u.x, v.z)),
            __fsub_rn(__fmul_rn(u.x, v.y), __fmul_rn(u.y, v.x))};
}

__device__ __forceinline__ float md_dotv(MdVec a, MdVec b) { return dot3_rn(a.x, a.y, a.z, b.x, b.y, b.z); }

// the face a slot's first word names; negative: a dead slot
__device__ __forceinline__ int meshrec_face(float4 first) { return __float_as_int(first.w); }

// point i of cloud c of xyz (clouds, n, 3); NaN for a thread without one (i >= n)
__device__ __forceinline__ MdVec meshrec_point(const float *__restrict__ xyz, int c, int n, int i) {
    const float nan = __uint_as_float(MESHREC_NAN_BITS);
    MdVec p = {nan, nan, nan};
    if (i < n) {
        const size_t at = ((size_t)c * n + i) * 3;
        p = {xyz[at], xyz[at + 1], xyz[at + 2]};
    }
    return p;
}

// The slots [f0, f1) of shape[c] (uniform per workgroup) and, with GROUPS, g0 = group_off[shape[c]], the index of its first group;
// anything out of range is a shape without faces, f0 = f1 = 0.  Without GROUPS group_off is not read and g0 is 0.
struct MeshrecRange {
    int f0, f1, g0;
};

template <bool GROUPS>
__device__ __forceinline__ MeshrecRange meshrec_range(const int32_t *shape, const int32_t *face_off, const int32_t *group_off, int c, int S,
                                                      int F) {
    const int s = shape[c];
    int f0 = 0, f1 = 0, g0 = 0;
    if (s >= 0 && s < S) {
        f0 = face_off[s], f1 = face_off[s + 1], g0 = GROUPS ? group_off[s] : 0;
        if (f0 < 0 || f1 > F || f1 < f0 || g0 < 0) f0 = f1 = 0;
    }
    return {f0, f1, g0};
}

// Thread t stages slot first + t of rec into s_rec (3 MESHREC_CHUNK words), a dead slot where t >= cnt.  Barriers are the caller's.
__device__ __forceinline__ void meshrec_stage(const float4 *__restrict__ rec, int first, int cnt, float4 *s_rec) {
    const int tid = threadIdx.x;
    float4 a = make_float4(0.f, 0.f, 0.f, __int_as_float(-1)), b = make_float4(0.f, 0.f, 0.f, 0.f), c = b;
    if (tid < cnt) {
        const size_t at = (size_t)(first + tid) * 3;
        a = rec[at], b = rec[at + 1], c = rec[at + 2];
    }
    s_rec[3 * tid] = a, s_rec[3 * tid + 1] = b, s_rec[3 * tid + 2] = c;
}

// The set bits of todo (uniform: a ballot over the group that starts at staged slot s0), lowest first: visit(w) with w[0], w[1], w[2] the
// three words of each such slot, still in LDS.  The winding kernel's walk.  The distance kernel spells the same loop out in its own text:
// its body leaves early where it culls, and handed over as a functor it cost 1.5 to 5 % of that kernel's time (measured; the compiler
// lays the loop out differently).
template <class Visit>
__device__ __forceinline__ void meshrec_walk(const float4 *s_rec, int s0, unsigned long long todo, Visit visit) {
    while (todo) {
        const int jj = s0 + __builtin_ctzll(todo);                 // uniform: the lowest slot still to visit
        todo &= todo - 1;
        visit(s_rec + 3 * jj);
    }
}
