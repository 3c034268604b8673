// raster.h -- the exact integer scan conversion of a triangle, once: the face record, the edge function, the set-up, the exact division,
// the scan of a face's box and the sweep of a workgroup over a range of faces.  csrc/visible.hip (SUB = 8 sub-pixel bits, depth minima into
// an LDS buffer, then a depth test) and the mesh half of csrc/render.hip (SUB = 4, keys into global memory) are its two callers; their
// THE DEFINITION blocks state what is computed, and everything here is spelled so that both hold bit for bit.  Nothing below knows which
// of the two is calling: what differs is a template parameter or a functor.
//
// THE SWEEP.  A workgroup of RASTER_THREADS = 256 takes its faces 256 at a time, a lane per face: a face whose clipped bounding box holds
// at most RASTER_SMALL_BOX pixels is rasterised by its lane (a surface-nets face at R = 64 in a 128-pixel cell covers a handful); a larger
// one is appended to an LDS list and, after a barrier, taken by a whole wave whose lanes stride over the pixels of its box (a face as large
// as a 128 x 128 image is 16 384 centres: 256 per lane).  The list's counter has two copies used in turn (s_cnt[par]): the copy of the NEXT
// turn is cleared by thread 0 after the first barrier of this turn, when its last readers -- the waves of the turn before -- have all passed
// the barrier that ended that turn, so a turn costs two barriers and the list never needs a third.  The division by A2 is an fp64 estimate
// corrected by one step either way with the integer remainder: exact.
#pragma once
#include "common.h"

#define RASTER_THREADS 256
#define RASTER_WAVES (RASTER_THREADS / PDGN_WAVE)
#define RASTER_SMALL_BOX 32

struct RasterFace {
    int x0, y0, z0, x1, y1, z1, x2, y2, z2;
    int bx, by, bw, bh;                                          // the clipped pixel box; bw * bh = 0: no centre to look at
    long long a2;
    double ra2;
};

__device__ __forceinline__ long long raster_edge(int ax, int ay, int bx, int by, int px, int py) {
    return (long long)(bx - ax) * (py - ay) - (long long)(by - ay) * (px - ax);
}

// From the nine snapped integers of t: A2, P1 and P2 (with their Z) changing places where it is negative, the box of the pixel centres
// (2 p + 1) 2^(SUB - 1) that lie inside the face's bounding box with clip_lo <= p <= clip_hi, and 1 / A2.  A2 = 0 leaves the box empty.
// (Visibility's coordinates are never negative, so its lower clip of 0 changes nothing there; the previews' guard band needs it.)
template <int SUB>
__device__ __forceinline__ void raster_setup(RasterFace &t, int clip_lo, int clip_hi) {
    constexpr int HALF = 1 << (SUB - 1);
    t.a2 = raster_edge(t.x0, t.y0, t.x1, t.y1, t.x2, t.y2);
    if (t.a2 < 0) {
        int s;
        s = t.x1, t.x1 = t.x2, t.x2 = s;
        s = t.y1, t.y1 = t.y2, t.y2 = s;
        s = t.z1, t.z1 = t.z2, t.z2 = s;
        t.a2 = -t.a2;
    }
    t.bw = t.bh = 0, t.bx = t.by = 0, t.ra2 = 0.0;
    if (t.a2 != 0) {
        // the centres (2 p + 1) HALF inside [lo, hi]: p from ceil((lo - HALF) / 2 HALF) to floor((hi - HALF) / 2 HALF), clipped
        const int xlo = min(t.x0, min(t.x1, t.x2)), xhi = max(t.x0, max(t.x1, t.x2));
        const int ylo = min(t.y0, min(t.y1, t.y2)), yhi = max(t.y0, max(t.y1, t.y2));
        const int px0 = max((xlo + HALF - 1) >> SUB, clip_lo), px1 = min((xhi - HALF) >> SUB, clip_hi);
        const int py0 = max((ylo + HALF - 1) >> SUB, clip_lo), py1 = min((yhi - HALF) >> SUB, clip_hi);
        if (px1 >= px0 && py1 >= py0) t.bx = px0, t.by = py0, t.bw = px1 - px0 + 1, t.bh = py1 - py0 + 1;
        t.ra2 = 1.0 / (double)t.a2;
    }
}

// floor(num / den) for 0 <= num < 2^61, 0 < den < 2^37 and a quotient below 2^24: the fp64 estimate is off by less than one.  The bound
// is the previews' (render.hip, BOUND); visibility's -- num < 2^55, den < 2^34, a quotient of at most 2^21 -- lies inside it.
__device__ __forceinline__ long long raster_div(long long num, long long den, double rden) {
    long long q = (long long)((double)num * rden);
    long long r = num - q * den;
    if (r < 0) --q, r += den;
    if (r >= den) ++q;
    return q;
}

// The pixels start, start + step, ... (row-major in the box) of face t.  At every covered centre: covered = true and visit(px, py, z) with
// z = floor((w0 Z0 + w1 Z1 + w2 Z2) / A2); a visit that returns true ends the scan, which then returns true.
template <int SUB, class Visit>
__device__ __forceinline__ bool raster_scan(const RasterFace &t, int start, int step, bool &covered, Visit visit) {
    const int n = t.bw * t.bh;
    const int qy = step / t.bw, qx = step - qy * t.bw;
    int iy = start / t.bw, ix = start - iy * t.bw;
    for (int k = start; k < n; k += step) {
        const int px = t.bx + ix, py = t.by + iy;
        const int cx = (2 * px + 1) << (SUB - 1), cy = (2 * py + 1) << (SUB - 1);
        const long long w0 = raster_edge(t.x1, t.y1, t.x2, t.y2, cx, cy);
        const long long w1 = raster_edge(t.x2, t.y2, t.x0, t.y0, cx, cy);
        const long long w2 = t.a2 - w0 - w1;                     // = edge(P0, P1, C): the three sum to A2 identically
        if ((w0 | w1 | w2) >= 0) {
            covered = true;
            if (visit(px, py, raster_div(w0 * t.z0 + w1 * t.z1 + w2 * t.z2, t.a2, t.ra2))) return true;
        }
        ix += qx, iy += qy;
        if (ix >= t.bw) ix -= t.bw, ++iy;
    }
    return false;
}

// THE SWEEP above over the faces f0 + tid, f0 + tid + stride, ... below f1 (Index: int or long long, the caller's own width).  s_list
// (RASTER_THREADS ints) and s_cnt (two, both 0 on entry, with a barrier between their clearing and this call) are the workgroup's LDS;
// every thread of the workgroup calls, and the last thing the call does is a barrier.  load(f, t) gathers and sets up face f and says
// whether it is alive; visit is raster_scan's; done(f, t, covered, stopped) runs once per live face after its scan, in one lane, with
// whether any of its centres was covered and whether any visit stopped.  The counter of the last turn is left holding its count: a caller
// that sweeps again clears both first.  fold() is the one hook that every lane of a wave reaches after it has scanned its share of a large
// face, before lane 0 calls done: a caller whose visit keeps a per-lane partial (a count) folds the 64 of them there; a lane-per-face
// scan has nothing to fold and does not call it.
template <int SUB, class Index, class Load, class Visit, class Done, class Fold>
__device__ __forceinline__ void raster_sweep(Index f0, Index f1, Index stride, int *s_list, int *s_cnt, Load load, Visit visit, Done done, Fold fold) {
    const int tid = threadIdx.x, lane = tid & (PDGN_WAVE - 1), wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int par = 0;
    for (Index base = f0; base < f1; base += stride, par ^= 1) {
        // ---- a lane per face: the small ones here, the large ones onto the list
        const Index f = base + tid;
        RasterFace t;
        if (f < f1 && load((int)f, t)) {
            const int n = t.bw * t.bh;
            if (n > RASTER_SMALL_BOX) {
                s_list[atomicAdd(&s_cnt[par], 1)] = (int)f;
            } else {
                bool covered = false, stopped = false;
                if (n > 0) stopped = raster_scan<SUB>(t, 0, 1, covered, visit);
                done((int)f, t, covered, stopped);
            }
        }
        __syncthreads();
        // ---- a wave per large face
        const int cnt = s_cnt[par];
        if (tid == 0) s_cnt[par ^ 1] = 0;                        // (last read before the barrier that ended the previous sweep)
        for (int e = wave; e < cnt; e += RASTER_WAVES) {
            const int g = __builtin_amdgcn_readfirstlane(s_list[e]);
            load(g, t);                                          // (it was alive when it was listed)
            bool covered = false;
            const bool stopped = raster_scan<SUB>(t, lane, PDGN_WAVE, covered, visit);
            const bool any_stopped = __any(stopped), any_covered = __any(covered);
            fold();
            if (lane == 0) done(g, t, any_covered, any_stopped);
        }
        __syncthreads();
    }
}

// The sweep of a caller without per-lane partials.
template <int SUB, class Index, class Load, class Visit, class Done>
__device__ __forceinline__ void raster_sweep(Index f0, Index f1, Index stride, int *s_list, int *s_cnt, Load load, Visit visit, Done done) {
    raster_sweep<SUB>(f0, f1, stride, s_list, s_cnt, load, visit, done, [] {});
}

// The sum of one unsigned per lane over the 64 lanes of a wave, in every lane (all 64 call).
__device__ __forceinline__ unsigned raster_wave_sum(unsigned v) {
#pragma unroll
    for (int d = PDGN_WAVE / 2; d > 0; d >>= 1) v += (unsigned)__shfl_xor((int)v, d, PDGN_WAVE);
    return v;
}
