// gemm_plan.h -- the launch model of the dense contractions (gemm_nt.hip, gemm_x3.hip and its two other translation units), once:
// the tile tables of the two kernel families and, as ordinary functions over a tile record WITH THE CU COUNT AS AN ARGUMENT, what
// a launch will do (plan), the data-parallel grid, the stream-K tail's layout and workspace, the weight gradients' k slices, the
// two pick rules and x2_pays.  No HIP header: the file compiles with any C++ compiler and its answers can be stepped through on a
// machine without a GPU.  tests/gemm_cases.py restates this arithmetic in Python; the cost formulas are IEEE double, evaluated
// in the order written here (the build has -ffp-contract=off), so the restatement reproduces the picks exactly -- change both.
#pragma once
#include <cstdlib>

#define NT_BK 32                      // reduction depth of a chunk
#define NT_GROUP_M 8                  // tile rows per group of the XCD-aware tile order

struct GemmTile {
    int bm, bn, wg_per_cu;
    int stat_div;                     // a statistics partial covers bm / stat_div rows (one per wave row)
    double rate;                      // chunk-rate divisor: the flop / us a CU sustains on this tile's loop
    double ov;                        // what a tile costs on top of its own chunks (ring fill, output), in chunks
    int tpw_chunks;                   // chunks of work a workgroup of the data-parallel launch keeps behind one ring fill
    bool tpw_env;                     // PDGN_NT_TPW overrides the tiles per workgroup (measurement; the fp32 family only)
};
// Calibrated on MI355X (tools/gemm_shapes.py, tools/x3_check.py).  x3 (gemm_x3.hip): 256 x 128 (144 KB of LDS), 128 x 128 (96 KB)
// one workgroup per CU, 128 x 64 (72 KB) two.  fp32 (gemm_nt.hip): 256 x 128 (96 KB) one per CU, 128 x 128 (64 KB) and 160 x 64
// (56 KB; 35840 = 224 x 160) two, 128 x 64 (48 KB, < 168 registers) three; a CU multiplies ~0.56 Mflop / us there, 0.95 of it on
// the tiles with fewer than 16 blocks per wave.
constexpr GemmTile X3_TILES[3] = {{256, 128, 1, 2, 760e3, 2.0, 64, false}, {128, 128, 1, 2, 660e3, 2.0, 64, false},
                                  {128, 64, 2, 2, 540e3, 2.0, 64, false}};
constexpr GemmTile FP32_TILES[4] = {{256, 128, 1, 4, 0.56e6 * 1.0, 2.5, 32, true}, {128, 128, 2, 2, 0.56e6 * 1.0, 2.5, 32, true},
                                    {160, 64, 2, 2, 0.56e6 * 0.95, 2.5, 32, true}, {128, 64, 3, 2, 0.56e6 * 0.95, 2.5, 32, true}};

static inline int plan_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// what the launch will do: tiles, slots, whether a stream-K tail follows the whole rounds
struct GemmPlan {
    int tiles_m, tiles_n, kchunks, grid_dp, dp_tiles, grid_sk;
    long long sk_per_wg;
    double cost;                      // launch model, microseconds
};

// Workgroups of the data-parallel launch: at least one per slot, and more -- each then walks fewer tiles -- so that the hardware
// hands them out as CUs come free (the kernel shares the chip with the step's other streams; a static assignment over exactly
// `slots` workgroups lets one delayed workgroup hold up the launch): enough tiles per workgroup to keep ~tpw_chunks chunks of
// work behind one ring fill.
static inline int gemm_dp_grid(const GemmTile &t, long long tiles, int slots, int kc) {
    static const int tpw_env = [] { const char *e = getenv("PDGN_NT_TPW"); return e ? atoi(e) : 0; }();
    const int forced = t.tpw_env ? tpw_env : 0;
    int tpw = forced > 0 ? forced : (t.tpw_chunks + kc - 1) / kc;
    tpw = tpw < 1 ? 1 : (tpw > 8 ? 8 : tpw);
    if (forced >= 1000) return (int)(tiles < slots ? tiles : slots);               // measurement: one workgroup per slot
    const long long g = (tiles + tpw - 1) / tpw;
    const long long lo = tiles < slots ? tiles : slots;
    return (int)(g < lo ? lo : g);
}
static inline double gemm_chunk_us(const GemmTile &t, int w) { return 2.0 * t.bm * t.bn * NT_BK * w / t.rate; }

// Launch model: the w workgroups sharing a CU share its rate; a tile costs ov chunks on top of its own; the atomics of a partial
// tile are added at ~1.3 TB/s chip-wide.
static inline GemmPlan gemm_plan(const GemmTile &t, long long m, int n, int k, bool allow_sk, int cus) {
    GemmPlan pl;
    pl.tiles_m = plan_cdiv(m, t.bm);
    pl.tiles_n = plan_cdiv(n, t.bn);
    pl.kchunks = plan_cdiv(k, NT_BK);
    const long long T = (long long)pl.tiles_m * pl.tiles_n;
    const int slots = cus * t.wg_per_cu, KC = pl.kchunks;
    const long long rounds = T / slots, tail = T - rounds * slots;
    const double ov = t.ov;
    const double full = (double)rounds * (KC + ov) * gemm_chunk_us(t, t.wg_per_cu);
    // data-parallel only: the last, partial round runs ceil(tail / cus) workgroups on its busiest CU
    pl.dp_tiles = (int)T;
    pl.grid_dp = gemm_dp_grid(t, T, slots, KC);
    pl.grid_sk = 0;
    pl.sk_per_wg = 0;
    pl.cost = full + (tail ? (KC + ov) * gemm_chunk_us(t, (int)((tail + cus - 1) / cus)) : 0.0);
    if (allow_sk && tail > 0) {
        // stream-K tail over g workgroups: every slot, one per CU, or fewer with at least 16 chunks each
        const long long iters = tail * KC;
        const long long cand[3] = {(long long)slots, (long long)cus, iters / 16};
        for (int ci = 0; ci < 3; ++ci) {
            long long g = cand[ci] < 1 ? 1 : (cand[ci] > slots ? slots : cand[ci]);
            g = g < iters ? g : iters;
            const long long per = (iters + g - 1) / g;
            if (per < 8 && g > 1) continue;                        // short ranges: the atomics cost more than they balance
            g = (iters + per - 1) / per;
            const double zero_rows = (double)(m - (long long)((rounds * slots) / (NT_GROUP_M * pl.tiles_n)) * NT_GROUP_M * t.bm);
            const double c = full + (per + ov) * gemm_chunk_us(t, (int)((g + cus - 1) / cus)) + (double)(g + tail) * t.bm * t.bn * 4 / 1.3e6 +
                             zero_rows * n * 4 / 3.0e6 + 4.0;
            if (c < pl.cost) {
                pl.cost = c;
                pl.dp_tiles = (int)(rounds * slots);
                pl.grid_dp = rounds ? gemm_dp_grid(t, rounds * slots, slots, KC) : 0;
                pl.grid_sk = (int)g;
                pl.sk_per_wg = per;
            }
        }
    }
    return pl;
}

// How a stream-K tail (the leftover tiles' k ranges over all CUs) is laid out when its partial tiles go to a workspace (gemm_x3).
// Aligned: every tile's chunks in s_tail equal slices, workgroup v = (slice, tile): the workgroups that run together read the
// same chunks of different tiles.  When the tiles do not divide the CUs well (140 leftover tiles on 256 CUs: one slice each
// = 55 % of the chip, the per-point product's input gradient) the FLATTENED order instead: iteration ranges of equal length,
// a workgroup's range may span seg tiles.
struct GemmTail {
    int t_tail, s_tail, per_tail, grid, seg;
    long long per_flat, floats;
};
static inline GemmTail gemm_tail_layout(const GemmTile &tile, const GemmPlan &pl, int cus) {
    GemmTail t = {0, 0, 0, 0, 0, 0, 0};
    if (!pl.grid_sk) return t;
    const long long T = (long long)pl.tiles_m * pl.tiles_n;
    const int slots_ = cus * tile.wg_per_cu;
    t.t_tail = (int)(T - pl.dp_tiles);
    t.s_tail = slots_ / t.t_tail < 1 ? 1 : slots_ / t.t_tail;
    t.s_tail = t.s_tail > pl.kchunks ? pl.kchunks : t.s_tail;
    t.per_tail = (pl.kchunks + t.s_tail - 1) / t.s_tail;
    t.s_tail = (pl.kchunks + t.per_tail - 1) / t.per_tail;
    t.grid = t.s_tail * t.t_tail;
    const long long iters = (long long)t.t_tail * pl.kchunks;
    if (t.grid * 5 < slots_ * 4 && iters >= (long long)slots_ * 8) {         // under 80 % of the chip, and ranges of >= 8 chunks to hand out
        t.per_flat = (iters + slots_ - 1) / slots_;
        t.grid = (int)((iters + t.per_flat - 1) / t.per_flat);
        t.seg = (int)((t.per_flat + pl.kchunks - 2) / pl.kchunks) + 1;
        t.floats = (long long)t.grid * t.seg * tile.bm * tile.bn;
    } else {
        t.floats = (long long)t.grid * tile.bm * tile.bn;
    }
    return t;
}
// floats of workspace the stream-K tail of (m, n, k) wants (0: no tail)
static inline long long gemm_tail_floats(const GemmTile &t, long long m, int n, int k, bool allow_sk, int cus) {
    return gemm_tail_layout(t, gemm_plan(t, m, n, k, allow_sk, cus), cus).floats;
}

// Weight gradients (split-K over few output tiles: at most one per slot): the k slices per tile the launch hands out, the number
// of NON-EMPTY ones, and the workspace their partial tiles want (0: the launch is not a split-K one)
static inline bool gemm_at_splits(const GemmTile &t, const GemmPlan &pl, int cus) {
    return (long long)pl.tiles_m * pl.tiles_n <= cus * t.wg_per_cu;
}
static inline int gemm_at_split(const GemmTile &t, const GemmPlan &pl, int cus) {
    const long long T = (long long)pl.tiles_m * pl.tiles_n;
    const int slots = cus * t.wg_per_cu;
    return (int)(slots / T) < pl.kchunks ? (int)(slots / T) : pl.kchunks;
}
static inline int gemm_at_slices(const GemmTile &t, const GemmPlan &pl, int cus) {
    const int S = gemm_at_split(t, pl, cus), per = (pl.kchunks + S - 1) / S;
    return (pl.kchunks + per - 1) / per;
}
static inline long long gemm_at_floats(const GemmTile &t, long long m, int n, int k, int cus) {
    const GemmPlan pl = gemm_plan(t, m, n, k, true, cus);
    if (!gemm_at_splits(t, pl, cus)) return 0;
    return (long long)gemm_at_slices(t, pl, cus) * pl.tiles_m * pl.tiles_n * t.bm * t.bn;
}

// Statistics partials: [3n] rows a launch writes (tile rows x wave rows), and the rows of C each covers
static inline long long gemm_stat_rows(const GemmTile &t, long long m) { return (long long)plan_cdiv(m, t.bm) * t.stat_div; }
static inline int gemm_stat_block_rows(const GemmTile &t) { return t.bm / t.stat_div; }

// Tile configuration for a problem: `forced` (>= 0: measurement / tests), else by the launch model.
// fp32: the square tile unless another is clearly cheaper; no_tall: not the 160 x 64 tile (weight gradients).
static inline int gemm_pick_fp32(int forced, long long m, int n, int k, bool stats, bool no_tall, int cus) {
    if (forced >= 0) return (no_tall && forced == 2) ? 1 : forced;
    double c[4];
    for (int i = 0; i < 4; ++i) c[i] = gemm_plan(FP32_TILES[i], m, n, k, !stats, cus).cost;
    int best = 1;
    for (int i = 0; i < 4; ++i)
        if (c[i] < c[best] * 0.97 && !(no_tall && i == 2)) best = i;
    return best;
}
// x3: the cheapest (0 .. 2; a forced 3, the fp32 kernel's fourth, reads as 2)
static inline int gemm_pick_x3(int forced, long long m, int n, int k, bool stats, int cus) {
    if (forced >= 0) return forced > 2 ? 2 : forced;
    double c[3];
    for (int i = 0; i < 3; ++i) c[i] = gemm_plan(X3_TILES[i], m, n, k, !stats, cus).cost;
    int best = 0;
    for (int i = 1; i < 3; ++i)
        if (c[i] < c[best]) best = i;
    return best;
}

// Where the two-part form pays (measured, tools/x2_shapes.py: every contraction of an iteration alone in both forms): it halves
// the matrix-core work of a launch and needs the operands' maxima first -- a pass over every operand that does not bring them
// along.  On the 256 x 128 tile, with a reduction of at least 128 and >= 20 GFLOP, the products are the larger part of the
// launch (conv2's dense half 927 -> 782 us with both scans, its input gradient 952 -> 693, the per-point product 761 -> 610);
// the smaller tiles' launches are bound by their operand path and only pay the scans (+5 .. 100 us each).  A launch that
// would have to read more than 4.5 bytes per kflop for the maxima keeps three parts (the per-point product's input gradient:
// 1.8 GB of dY for 118 GFLOP).
static inline bool x2_pays(int mode, int cfg, long long m, int n, int k, long long scan_bytes) {
    if (mode != 2 || cfg != 0 || k < 128 || m >= (1LL << 28)) return false;
    const double flops = 2.0 * (double)m * n * k;
    static const double min_flops = [] { const char *e = getenv("PDGN_X2_MIN_GFLOP"); return (e && *e) ? atof(e) * 1e9 : 2e10; }();   // (measurement)
    return flops >= min_flops && (double)scan_bytes <= 4.5e-3 * flops;
}
