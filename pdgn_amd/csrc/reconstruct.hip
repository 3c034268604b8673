// reconstruct.hip -- from oriented points to a triangle mesh: pdgn_imls_grid, an implicit-moving-least-squares signed-distance field on a
// regular grid, and pdgn_surface_nets_count / _emit, the surface-nets iso-surface of such a field (Hoppe et al. 1992 for the pipeline,
// Kolluri 2005 for the field, Gibson 1998 for the mesh; include/pdgn_hip.h).  No inline assembly, no float atomics,
// plain vector stores, nothing allocated.
//
// NORMATIVE ORDER (tests/reconstruct_mirror.py restates it in numpy; every fp32 operation below is one rounding -- __fadd_rn / __fsub_rn /
// __fmul_rn / __fdiv_rn -- nothing contracted; dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z as in csrc/normals.hip).
//
// THE FIELD.  One cloud: x (n,3), g (n,3) oriented normals, origin o, voxel v, inv = 1 / h^2, R nodes per axis.
//     node (i,j,k) has the id (i R + j) R + k and the position p_a = o_a + (float)i_a * v
//     point j is live iff its six values are finite; a dead point is skipped
//     sw = sf = +0
//     for j ascending over the live points:
//         d = p - x_j,  d2 = dot3(d, d),  t = 1 - d2 * inv
//         where t > 0:  w = t * t,  sw = sw + w,  sf = sf + w * dot3(d, g_j)
//     f = sw > 0 ? sf / sw : NaN with the bits 0x7FC00000            (an invalid node: no point within h)
//
// THE MESH.  C = R - 1 cells per axis, cell id (i C + j) C + k, corner (a,b,c) of a cell is node (i+a, j+b, k+c).  A node is inside iff
// f < 0 (f = +-0 is outside), invalid iff f is NaN.
//     active cell  all eight corners valid, 1 to 7 of them inside
//     its vertex   the 12 edges in the order axis A = 0, 1, 2 and, within A, offsets (u,v) = (0,0), (1,0), (0,1), (1,1) on the axes
//                  A1 = (A+1)%3, A2 = (A+2)%3.  On an edge whose ends differ in "inside": t = f0 / (f0 - f1) (f0 the low end), the crossing
//                  in cell-local coordinates is (t on A, u on A1, v on A2).  The three coordinates are summed in edge order from +0, the
//                  crossings counted as m:  pos_a = o_a + v * ((float)cell_a + sum_a / (float)m)
//     quads        node N and axis A with N + e_A in range, both ends valid and differing in "inside".  The four cells
//                  N + u e_A1 + w e_A2, (u,w) = (-1,-1), (0,-1), (0,0), (-1,0); where all four are in range and active: q is that order if
//                  N is inside, the reverse if not, the triangles (q0,q1,q2), (q0,q2,q3) -- counter-clockwise seen from outside.
//                  Otherwise no quad is written and the edge counts as open.
//     order        vertices by ascending cell id; faces by ascending key 3 (node id) + A, two per quad; int32 indices into the cloud's own
//                  vertices
//     counters     per cloud: vertices, faces, open edges, invalid nodes
//
// SHAPE OF THE FIELD KERNEL.  One thread per node; a workgroup of IMLS_THREADS = 512 owns a cube of 8 x 8 x 8 nodes, each of its eight
// waves a brick of 4 x 4 x 4 (lane = (li 4 + lj) 4 + lk).  The cloud passes through LDS in chunks of IMLS_CHUNK = 512 points, thread t
// staging point j0 + t as two 16-byte records (x, y, z, live) and (gx, gy, gz, 0).  A wave then takes the chunk 64 points at a time:
// lane l decides whether point l of the 64 is to be visited by this wave, a ballot collects the decisions, and the wave walks the set
// bits of the ballot from the lowest up -- ascending j -- reading each surviving point's two records at a uniform address (broadcasts).
// The order over j is each thread's own, so grid, block and chunk sizes change no bit.
//
// CULLING.  A term with w = 0 changes no bit (the sums start at +0 and t > 0 fails), so a wave may leave out every point for which
// t <= 0 holds at all nodes of its brick, as long as the others keep their order.  The test (imls_skips) needs no slack:
//   * p_a is monotone in the index (a rounded product by v > 0 and a rounded sum are monotone), so the brick's nodes lie in the box
//     [lo_a, hi_a] of its first and its last in-range node, bounds included, in fp32 exactly;
//   * a correctly rounded subtraction is monotone in either operand and odd, so for every node |p_a - x_a| rounded is at least
//     m_a = max(lo_a - x_a, x_a - hi_a, 0), each difference rounded the same way;
//   * products and sums of non-negative numbers, rounded, are monotone: dot3(d, d) >= dot3(m, m); so are d2 * inv for inv > 0 and 1 - it,
//     the other way round.  Hence t(node) <= T = 1 - dot3(m, m) * inv for every node of the brick, and T <= 0 proves all of them.
// Overflow keeps the chain (inf is the largest value; no inf - inf or 0 * inf can arise from finite x, finite positive inv).  The mirror's
// `brick_skips` is the same expression; the bit-for-bit tests run with the culling on and off: the entry point's `cull` = 0 visits every
// live point at every node (measurement, tests).
//
// SHAPE OF THE EXTRACTION.  pdgn_surface_nets_count: a clearing launch for the counters, one thread per node marking active cells (a cell
// is filed under its lowest corner's node id, which orders as the cell id does) and counting invalid nodes, one thread per node counting
// its quads (0 .. 3) and open edges from those marks; counters through integer atomics (LDS, then one global add per workgroup).  The
// caller scans both arrays per cloud (torch.cumsum on int32) and hands the inclusive sums to pdgn_surface_nets_emit, where a thread per
// node writes its cell's vertex and its node's quads at their ranks: the order is by index whatever the launch geometry.
#include "common.h"

#include <math.h>

#define IMLS_THREADS 512
#define IMLS_CHUNK 512
#define IMLS_EDGE 8                                              // the workgroup's cube
#define IMLS_BRICK 4                                             // the wave's brick
#define IMLS_MAX_BLOCKS (1 << 22)                                // workgroups per launch: 2^31 threads
#define SN_THREADS 256
#define SN_TURNS 8                                               // chunks of SN_THREADS nodes per counting workgroup
#define RECON_NAN_BITS 0x7FC00000u
static_assert(IMLS_CHUNK == IMLS_THREADS, "thread t stages point j0 + t");
static_assert(IMLS_CHUNK % PDGN_WAVE == 0, "a wave takes the chunk 64 points at a time");

__device__ __forceinline__ float rc_pos(float o, int i, float v) { return __fadd_rn(o, __fmul_rn((float)i, v)); }

// CULLING above: true where t <= 0 is proven for every node of the box [lo, hi]
__device__ __forceinline__ bool imls_skips(float x, float y, float z, float lox, float loy, float loz, float hix, float hiy, float hiz,
                                           float inv) {
    const float mx = fmaxf(fmaxf(__fsub_rn(lox, x), __fsub_rn(x, hix)), 0.f);
    const float my = fmaxf(fmaxf(__fsub_rn(loy, y), __fsub_rn(y, hiy)), 0.f);
    const float mz = fmaxf(fmaxf(__fsub_rn(loz, z), __fsub_rn(z, hiz)), 0.f);
    const float T = __fsub_rn(1.0f, __fmul_rn(dot3_rn(mx, my, mz, mx, my, mz), inv));
    return !(T > 0.f);
}

__global__ __launch_bounds__(IMLS_THREADS) void imls_kernel(int n, int R, int per_axis, const float *__restrict__ xyz,
                                                            const float *__restrict__ normals, const float *__restrict__ grid,
                                                            float *__restrict__ field, int cull) {
    __shared__ float4 rec[2 * IMLS_CHUNK];
    const int tid = threadIdx.x, lane = tid & (PDGN_WAVE - 1), wave = tid >> 6;
    const int per_cloud = per_axis * per_axis * per_axis;
    const int c = blockIdx.x / per_cloud, cube = blockIdx.x % per_cloud;
    const int ci = cube / (per_axis * per_axis), cj = (cube / per_axis) % per_axis, ck = cube % per_axis;
    // the wave's brick and the thread's node
    const int bi = ci * IMLS_EDGE + (wave >> 2) * IMLS_BRICK, bj = cj * IMLS_EDGE + ((wave >> 1) & 1) * IMLS_BRICK,
              bk = ck * IMLS_EDGE + (wave & 1) * IMLS_BRICK;
    const int i = bi + (lane >> 4), j = bj + ((lane >> 2) & 3), k = bk + (lane & 3);
    const bool wave_on = bi < R && bj < R && bk < R;                 // (uniform per wave: a brick past the grid visits nothing)
    const bool mine = i < R && j < R && k < R;
    const float *gr = grid + (size_t)c * 5;
    const float ox = gr[0], oy = gr[1], oz = gr[2], v = gr[3], inv = gr[4];
    const float px = rc_pos(ox, i, v), py = rc_pos(oy, j, v), pz = rc_pos(oz, k, v);
    // the brick's box: its first node and its last node inside the grid
    const float lox = rc_pos(ox, bi, v), loy = rc_pos(oy, bj, v), loz = rc_pos(oz, bk, v);
    const float hix = rc_pos(ox, min(bi + IMLS_BRICK - 1, R - 1), v), hiy = rc_pos(oy, min(bj + IMLS_BRICK - 1, R - 1), v),
                hiz = rc_pos(oz, min(bk + IMLS_BRICK - 1, R - 1), v);
    const float *x = xyz + (size_t)c * n * 3, *g = normals + (size_t)c * n * 3;
    float sw = 0.f, sf = 0.f;
    for (int j0 = 0; j0 < n; j0 += IMLS_CHUNK) {
        const int cnt = min(IMLS_CHUNK, n - j0);
        if (j0) __syncthreads();                                   // everyone is done reading the previous chunk
        {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
            if (tid < cnt) {
                const size_t at = (size_t)(j0 + tid) * 3;
                a.x = x[at], a.y = x[at + 1], a.z = x[at + 2];
                b.x = g[at], b.y = g[at + 1], b.z = g[at + 2];
                const bool live = isfinite(a.x) && isfinite(a.y) && isfinite(a.z) && isfinite(b.x) && isfinite(b.y) && isfinite(b.z);
                a.w = live ? 1.f : 0.f;
            }
            rec[2 * tid] = a, rec[2 * tid + 1] = b;
        }
        __syncthreads();
        if (!wave_on) continue;                                    // (the barriers above are reached by every wave all the same)
        for (int s0 = 0; s0 < cnt; s0 += PDGN_WAVE) {
            const float4 q = rec[2 * (s0 + lane)];                 // (s0 + lane < IMLS_CHUNK: a staged record, live = 0 past cnt)
            bool visit = q.w != 0.f;
            if (cull) visit = visit && !imls_skips(q.x, q.y, q.z, lox, loy, loz, hix, hiy, hiz, inv);
            unsigned long long todo = __ballot(visit);
            while (todo) {
                const int jj = s0 + __builtin_ctzll(todo);         // uniform: the lowest point still to visit
                todo &= todo - 1;
                const float4 p = rec[2 * jj], gn = rec[2 * jj + 1];
                const float dx = __fsub_rn(px, p.x), dy = __fsub_rn(py, p.y), dz = __fsub_rn(pz, p.z);
                const float d2 = dot3_rn(dx, dy, dz, dx, dy, dz);
                const float t = __fsub_rn(1.0f, __fmul_rn(d2, inv));
                const float w = __fmul_rn(t, t);
                const float term = __fmul_rn(w, dot3_rn(dx, dy, dz, gn.x, gn.y, gn.z));
                const bool in = t > 0.f;
                sw = in ? __fadd_rn(sw, w) : sw;
                sf = in ? __fadd_rn(sf, term) : sf;
            }
        }
    }
    if (mine) field[(size_t)c * R * R * R + ((size_t)i * R + j) * R + k] = sw > 0.f ? __fdiv_rn(sf, sw) : __uint_as_float(RECON_NAN_BITS);
}

// ---------------------------------------------------------------------------- surface nets
__device__ __forceinline__ bool sn_nan(float f) { return f != f; }

// the workgroup's sums of two per-thread counts into two counters of its cloud: LDS integer atomics per wave, one global add each
__device__ __forceinline__ void sn_block_add(int a, int b, int32_t *dst_a, int32_t *dst_b) {
    __shared__ int s_sum[2];
    if (threadIdx.x == 0) s_sum[0] = 0, s_sum[1] = 0;
    __syncthreads();
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64), b += __shfl_xor(b, off, 64);
    if (lane_id() == 0) {
        if (a) atomicAdd(&s_sum[0], a);
        if (b) atomicAdd(&s_sum[1], b);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_sum[0]) atomicAdd(dst_a, s_sum[0]);
        if (s_sum[1]) atomicAdd(dst_b, s_sum[1]);
    }
}

__global__ __launch_bounds__(SN_THREADS) void sn_clear_kernel(long long count, int32_t *stats) {
    const long long e = (long long)blockIdx.x * SN_THREADS + threadIdx.x;
    if (e < count) stats[e] = 0;
}

// vflag[node] = 1 where the cell whose lowest corner the node is exists and is active; counters 0 (vertices) and 3 (invalid nodes).
// A workgroup takes SN_TURNS chunks of SN_THREADS nodes, so that its two global adds stand for that many: most workgroups of a grid
// hold invalid nodes, and the adds of one cloud all go to one address.
__global__ __launch_bounds__(SN_THREADS) void sn_cells_kernel(int R, const float *__restrict__ field, int32_t *__restrict__ vflag,
                                                              int32_t *__restrict__ stats) {
    const int nodes = R * R * R, C = R - 1;
    const size_t base = (size_t)blockIdx.y * nodes;
    const float *f = field + base;
    int actives = 0, invalids = 0;
    for (int turn = 0; turn < SN_TURNS; ++turn) {
        const long long at = ((long long)blockIdx.x * SN_TURNS + turn) * SN_THREADS + threadIdx.x;
        if (at >= nodes) break;
        const int node = (int)at;
        const int i = node / (R * R), j = (node / R) % R, k = node % R;
        invalids += sn_nan(f[node]);
        int active = 0;
        if (i < C && j < C && k < C) {
            bool valid = true;
            int nin = 0;
#pragma unroll
            for (int corner = 0; corner < 8; ++corner) {
                const float fc = f[node + ((corner >> 2) * R + ((corner >> 1) & 1)) * R + (corner & 1)];
                valid = valid && !sn_nan(fc);
                nin += fc < 0.f;
            }
            active = valid && nin >= 1 && nin <= 7;
        }
        vflag[base + node] = active;
        actives += active;
    }
    sn_block_add(actives, invalids, stats + (size_t)blockIdx.y * 4, stats + (size_t)blockIdx.y * 4 + 3);
}

// Whether the grid edge from `node` along axis A is crossed, and, if so, the node ids of the four cells around it (cells[s] in the
// order of the header) where they all exist and are active.  -> 0: not crossed, 1: a quad, 2: open
__device__ __forceinline__ int sn_edge(int R, const float *f, const int32_t *vflag, int node, const int coord[3], int A, int cells[4]) {
    const int C = R - 1;
    const int stride[3] = {R * R, R, 1};
    if (coord[A] + 1 >= R) return 0;
    const float f0 = f[node], f1 = f[node + stride[A]];
    if (sn_nan(f0) || sn_nan(f1) || ((f0 < 0.f) == (f1 < 0.f))) return 0;
    const int A1 = (A + 1) % 3, A2 = (A + 2) % 3;
    const int du[4] = {-1, 0, 0, -1}, dw[4] = {-1, -1, 0, 0};
    bool all = true;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int c1 = coord[A1] + du[s], c2 = coord[A2] + dw[s];
        const bool in = c1 >= 0 && c1 < C && c2 >= 0 && c2 < C;     // (on axis A the cell's index is the node's, below C already)
        cells[s] = node + du[s] * stride[A1] + dw[s] * stride[A2];
        all = all && in && vflag[in ? cells[s] : node] != 0;
    }
    return all ? 1 : 2;
}

// qcnt[node] = the quads of the node's three edges; counters 1 (faces) and 2 (open edges); SN_TURNS chunks per workgroup as above
__global__ __launch_bounds__(SN_THREADS) void sn_quads_kernel(int R, const float *__restrict__ field, const int32_t *__restrict__ vflag,
                                                              int32_t *__restrict__ qcnt, int32_t *__restrict__ stats) {
    const int nodes = R * R * R;
    const size_t base = (size_t)blockIdx.y * nodes;
    int faces = 0, opens = 0;
    for (int turn = 0; turn < SN_TURNS; ++turn) {
        const long long at = ((long long)blockIdx.x * SN_TURNS + turn) * SN_THREADS + threadIdx.x;
        if (at >= nodes) break;
        const int node = (int)at;
        const int coord[3] = {node / (R * R), (node / R) % R, node % R};
        int cells[4], quads = 0;
#pragma unroll
        for (int A = 0; A < 3; ++A) {
            const int e = sn_edge(R, field + base, vflag + base, node, coord, A, cells);
            quads += e == 1, opens += e == 2;
        }
        qcnt[base + node] = quads;
        faces += 2 * quads;
    }
    sn_block_add(faces, opens, stats + (size_t)blockIdx.y * 4 + 1, stats + (size_t)blockIdx.y * 4 + 2);
}

struct SnEmitArgs {
    int R;
    const float *field, *grid;
    const int32_t *vflag, *vscan, *qcnt, *qscan, *vert_off, *face_off;
    long long total_verts, total_faces;
    float *verts;
    int32_t *faces;
};

__global__ __launch_bounds__(SN_THREADS) void sn_emit_kernel(SnEmitArgs a) {
    const int R = a.R, nodes = R * R * R;
    const int node = blockIdx.x * SN_THREADS + threadIdx.x;
    if (node >= nodes) return;
    const int c = blockIdx.y;
    const size_t base = (size_t)c * nodes;
    const float *f = a.field + base;
    const int32_t *vflag = a.vflag + base, *vscan = a.vscan + base;
    const int coord[3] = {node / (R * R), (node / R) % R, node % R};
    if (vflag[node]) {
        // the vertex of the cell whose lowest corner this node is
        float fc[2][2][2];
#pragma unroll
        for (int corner = 0; corner < 8; ++corner)
            fc[corner >> 2][(corner >> 1) & 1][corner & 1] = f[node + ((corner >> 2) * R + ((corner >> 1) & 1)) * R + (corner & 1)];
        float sum[3] = {0.f, 0.f, 0.f};
        int m = 0;
#pragma unroll
        for (int A = 0; A < 3; ++A) {
            const int A1 = (A + 1) % 3, A2 = (A + 2) % 3;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int u = e & 1, w = e >> 1;
                int lo[3], hi[3];
                lo[A] = 0, lo[A1] = u, lo[A2] = w;
                hi[A] = 1, hi[A1] = u, hi[A2] = w;
                const float f0 = fc[lo[0]][lo[1]][lo[2]], f1 = fc[hi[0]][hi[1]][hi[2]];
                if ((f0 < 0.f) != (f1 < 0.f)) {
                    float local[3];
                    local[A] = __fdiv_rn(f0, __fsub_rn(f0, f1)), local[A1] = (float)u, local[A2] = (float)w;
                    sum[0] = __fadd_rn(sum[0], local[0]), sum[1] = __fadd_rn(sum[1], local[1]), sum[2] = __fadd_rn(sum[2], local[2]);
                    ++m;
                }
            }
        }
        const float *gr = a.grid + (size_t)c * 4;
        const float v = gr[3], mf = (float)m;
        const long long dst = (long long)a.vert_off[c] + (vscan[node] - 1);
        if (dst >= 0 && dst < a.total_verts) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax)
                a.verts[dst * 3 + ax] = __fadd_rn(gr[ax], __fmul_rn(v, __fadd_rn((float)coord[ax], __fdiv_rn(sum[ax], mf))));
        }
    }
    const int mine = a.qcnt[base + node];
    if (mine) {
        long long dst = (long long)a.face_off[c] + 2LL * (a.qscan[base + node] - mine);
        const bool inside = f[node] < 0.f;
        int cells[4];
#pragma unroll
        for (int A = 0; A < 3; ++A) {
            if (sn_edge(R, f, vflag, node, coord, A, cells) != 1) continue;
            const int q0 = vscan[cells[inside ? 0 : 3]] - 1, q1 = vscan[cells[inside ? 1 : 2]] - 1, q2 = vscan[cells[inside ? 2 : 1]] - 1,
                      q3 = vscan[cells[inside ? 3 : 0]] - 1;
            if (dst >= 0 && dst + 1 < a.total_faces) {
                int32_t *o = a.faces + dst * 3;
                o[0] = q0, o[1] = q1, o[2] = q2, o[3] = q0, o[4] = q2, o[5] = q3;
            }
            dst += 2;
        }
    }
}

// ---------------------------------------------------------------------------- entry points (host-side checks only before any launch)

static bool rc_shape_ok(int b, int R) {
    return b >= 1 && R >= PDGN_RECON_MIN_R && R <= PDGN_RECON_MAX_R && (long long)b * R * R * R < (1LL << 31);
}

// origin finite, voxel finite and positive (and, with five values per cloud, inv too)
static bool rc_grid_ok(int b, const float *host, int per) {
    for (long long e = 0; e < (long long)b * per; ++e) {
        if (!isfinite(host[e])) return false;
        if (e % per >= 3 && !(host[e] > 0.f)) return false;
    }
    return true;
}

extern "C" int pdgn_imls_chunk(void) { return IMLS_CHUNK; }

extern "C" int pdgn_imls_grid(int b, int n, int R, const float *xyz, const float *normals, const float *grid, const float *grid_host,
                              int cull, float *field, pdgn_stream_t stream) {
    if (!rc_shape_ok(b, R) || n < 1 || cull < 0 || cull > 1) return PDGN_ERR_INVALID;
    if (!xyz || !normals || !grid || !grid_host || !field) return PDGN_ERR_INVALID;
    if (!pdgn_aligned(xyz, 4) || !pdgn_aligned(normals, 4) || !pdgn_aligned(grid, 4) || !pdgn_aligned(grid_host, 4) || !pdgn_aligned(field, 4))
        return PDGN_ERR_INVALID;
    if (!rc_grid_ok(b, grid_host, 5)) return PDGN_ERR_INVALID;
    const int per_axis = cdiv(R, IMLS_EDGE);
    const int per_cloud = per_axis * per_axis * per_axis;           // (at most 32^3)
    // at most IMLS_MAX_BLOCKS workgroups per launch: a grid whose threads pass 2^32 is refused by the runtime, and R = 9 rounds up to
    // 16^3 threads per cloud, so b R^3 < 2^31 alone does not keep a single launch below that
    const int clouds = IMLS_MAX_BLOCKS / per_cloud;
    for (int c0 = 0; c0 < b; c0 += clouds) {
        const int cb = b - c0 < clouds ? b - c0 : clouds;
        hipLaunchKernelGGL(imls_kernel, dim3((unsigned)cb * per_cloud), dim3(IMLS_THREADS), 0, (hipStream_t)stream, n, R, per_axis,
                           xyz + (size_t)c0 * n * 3, normals + (size_t)c0 * n * 3, grid + (size_t)c0 * 5, field + (size_t)c0 * R * R * R, cull);
    }
    return pdgn_launch_status();
}

extern "C" int pdgn_surface_nets_count(int b, int R, const float *field, int32_t *vflag, int32_t *qcnt, int32_t *stats,
                                       pdgn_stream_t stream) {
    if (!rc_shape_ok(b, R)) return PDGN_ERR_INVALID;
    if (!field || !vflag || !qcnt || !stats) return PDGN_ERR_INVALID;
    if (!pdgn_aligned(field, 4) || !pdgn_aligned(vflag, 4) || !pdgn_aligned(qcnt, 4) || !pdgn_aligned(stats, 4)) return PDGN_ERR_INVALID;
    const int nodes = R * R * R;
    hipLaunchKernelGGL(sn_clear_kernel, dim3(cdiv(4LL * b, SN_THREADS)), dim3(SN_THREADS), 0, (hipStream_t)stream, 4LL * b, stats);
    // grid.y carries the cloud: at most 65535 of them per launch
    for (int c0 = 0; c0 < b; c0 += 65535) {
        const int cb = b - c0 < 65535 ? b - c0 : 65535;
        const size_t at = (size_t)c0 * nodes;
        const dim3 grid(cdiv(nodes, SN_THREADS * SN_TURNS), cb);
        hipLaunchKernelGGL(sn_cells_kernel, grid, dim3(SN_THREADS), 0, (hipStream_t)stream, R, field + at, vflag + at, stats + (size_t)c0 * 4);
        hipLaunchKernelGGL(sn_quads_kernel, grid, dim3(SN_THREADS), 0, (hipStream_t)stream, R, field + at, vflag + at, qcnt + at,
                           stats + (size_t)c0 * 4);
    }
    return pdgn_launch_status();
}

extern "C" int pdgn_surface_nets_emit(int b, int R, const float *field, const float *grid, const float *grid_host, const int32_t *vflag,
                                      const int32_t *vscan, const int32_t *qcnt, const int32_t *qscan, const int32_t *vert_off,
                                      const int32_t *face_off, long long total_verts, long long total_faces, long long vert_capacity,
                                      long long face_capacity, float *verts, int32_t *faces, pdgn_stream_t stream) {
    if (!rc_shape_ok(b, R)) return PDGN_ERR_INVALID;
    if (!field || !grid || !grid_host || !vflag || !vscan || !qcnt || !qscan || !vert_off || !face_off) return PDGN_ERR_INVALID;
    if (!pdgn_aligned(field, 4) || !pdgn_aligned(grid, 4) || !pdgn_aligned(grid_host, 4) || !pdgn_aligned(vflag, 4) || !pdgn_aligned(vscan, 4) ||
        !pdgn_aligned(qcnt, 4) || !pdgn_aligned(qscan, 4) || !pdgn_aligned(vert_off, 4) || !pdgn_aligned(face_off, 4) ||
        !pdgn_aligned(verts, 4) || !pdgn_aligned(faces, 4))
        return PDGN_ERR_INVALID;
    const long long most = 0x7FFFFFFFLL / 3;
    if (total_verts < 0 || total_faces < 0 || total_verts > most || total_faces > most) return PDGN_ERR_INVALID;
    if (vert_capacity < total_verts || face_capacity < total_faces) return PDGN_ERR_INVALID;
    if ((total_verts && !verts) || (total_faces && !faces)) return PDGN_ERR_INVALID;
    if (!rc_grid_ok(b, grid_host, 4)) return PDGN_ERR_INVALID;
    const int nodes = R * R * R;
    for (int c0 = 0; c0 < b; c0 += 65535) {
        const int cb = b - c0 < 65535 ? b - c0 : 65535;
        const size_t at = (size_t)c0 * nodes;
        SnEmitArgs a = {};
        a.R = R, a.field = field + at, a.grid = grid + (size_t)c0 * 4, a.vflag = vflag + at, a.vscan = vscan + at, a.qcnt = qcnt + at;
        a.qscan = qscan + at, a.vert_off = vert_off + c0, a.face_off = face_off + c0, a.total_verts = total_verts;
        a.total_faces = total_faces, a.verts = verts, a.faces = faces;
        hipLaunchKernelGGL(sn_emit_kernel, dim3(cdiv(nodes, SN_THREADS), cb), dim3(SN_THREADS), 0, (hipStream_t)stream, a);
    }
    return pdgn_launch_status();
}
