// gemm_shared.h -- what the two dense-contraction kernels (gemm_nt.hip: fp32 matrix instructions; gemm_x3.hip: fp32 operands
// split into three bf16 parts) have in common.  Device side: operand descriptors, the LDS-DMA instruction, the argument block, the
// two-part scales.  Host side: the process-wide switches, the ARGUMENT FRONT of the public entry points (one check of the common
// arguments, one of the extended epilogue -- which builds the NtEpi --, one of the weight gradient's), the one fill of the
// argument block's common part, the launch of a kernel instance, and the prototypes of what one contraction file calls in another.
// The launch model (tile tables, plan, pick rules) is gemm_plan.h, which has no HIP in it.
#pragma once
#include <type_traits>

#include "common.h"
#include "gemm_plan.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void_t;

#define NT_OOB 0x40000000u            // a byte offset past every tile descriptor (num_records < 2^30)

typedef int i32x4 __attribute__((ext_vector_type(4)));

// Buffer descriptor (raw, stride 0): offsets >= bytes read as zero / are not written.
__device__ __forceinline__ i32x4 nt_srd(const void *base, unsigned bytes) {
    const unsigned long long b = (unsigned long long)base;
    i32x4 r;
    r.x = __builtin_amdgcn_readfirstlane((int)(unsigned)b);
    r.y = __builtin_amdgcn_readfirstlane((int)((unsigned)(b >> 32) & 0xffffu));
    r.z = __builtin_amdgcn_readfirstlane((int)bytes);
    r.w = 0x00020000;
    return r;
}

// One LDS-DMA wave instruction: 64 lanes x 16 B, lane l -> LDS byte lds_base + 16 l, from descriptor offset
// voff (per lane) + soff (scalar).  Issued as inline asm so that the compiler does not order every later LDS read
// behind it with s_waitcnt vmcnt(0) -- the kernel counts these operations itself.
__device__ __forceinline__ void nt_dma16(i32x4 srd, unsigned lds_base, unsigned voff, unsigned soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                 :
                 : "s"(lds_base), "v"(voff), "s"(srd), "s"(soff)
                 : "memory", "m0");
}

struct NtArgs {
    long long M;
    int N, K, lda, ldw, ldc, ldadd;
    const float *A, *W, *bias, *addend;
    float *C, *stat_part;
    int tiles_m, tiles_n, tile_begin, tile_end, kchunks;
    long long sk_per_wg;              // stream-K launch: (tile, chunk) iterations per workgroup
    int sk_split;                     // > 0 (gemm_x3 only): split-K launch over sk_split tiles: workgroup v takes tile v % sk_split,
                                      // chunks [v / sk_split * sk_per_wg, + sk_per_wg) -- workgroups that run together share panels
    float *sk_ws;                     // gemm_x3, non-atomic instances: partial tiles (whole, pitch BN) go to this workspace instead of
                                      // into C (stream-K tail without atomics).  sk_split > 0: workgroup v's one tile at slot v;
    int sk_seg;                       // sk_seg > 0 (sk_split == 0): the FLATTENED order -- workgroup v takes (tile, chunk) iterations
                                      // [v sk_per_wg, + sk_per_wg), its i-th tile's part at slot v * sk_seg + i
    int dbg;                          // builds with -DPDGN_NT_DEBUG only (ablation: 1 = stores dropped); always 0 otherwise
    // extended epilogue (pdgn_gemm_nt_ex), applied in this order after bias / addend:
    const float *row_bias;            // + row_bias[(row / rows_per_group) * ld_rb + col]: a bias per GROUP of rows (per sample)
    int ld_rb, rows_per_group;
    unsigned rpg_magic;               // row / rows_per_group == umulhi(row, rpg_magic) (rows_per_group > 1)
    int rb_bytes;                     // extent of the row_bias table in bytes (its buffer descriptor's range, < NT_OOB)
    int act;                          // 2: LeakyReLU(0.01) on the result
    const float *gate;                // result *= (gate[row, col] > 0 ? 1 : 0.01): the LeakyReLU derivative of a saved activation
    int ldgate;
    const unsigned short *Wp;         // gemm_x3, PW instances: the second operand pre-split into three bf16 planes [N][ldw]
    long long wplane;                 // elements between the planes
    const unsigned *max_a, *max_w;    // gemm_x3, two-part (fp16) instances: the maximum of |x| (bit pattern) of every ROW of each operand as the
                                      // kernel sees it (M entries / N entries: for an operand given transposed, of every column of the
                                      // matrix in memory); row r is multiplied by 2^e_r, e_r = x2_exponent(its maximum), before the split and
                                      // the result by 2^-e_A[row] 2^-e_W[column] (pre-split second operand: its rows' maxima sit behind
                                      // its two planes; the host points max_w there)
};

// Two-part mode: an operand's scales -- one power of two PER ROW of the operand as the kernel sees it (round 6; one per operand until
// then: a block-scaled format whose block was the whole matrix).  The maxima travel as bit patterns of |x| (unsigned order =
// magnitude order, so producers combine them with integer max / atomicMax in any order: deterministic); e = 14 - floor(log2 max):
// max |x| 2^e in [2^14, 2^15) -- nothing overflows fp16, and a value keeps 22 bits while it is within 2^-16 of ITS ROW's largest.
__device__ __forceinline__ int x2_exponent(unsigned maxbits) {     // (NaN / Inf: the largest exponent field; the products carry them)
    const int e = 14 - ((int)(maxbits >> 23) - 127);
    return e > 126 ? 126 : (e < -126 ? -126 : e);
}
__device__ __forceinline__ int x2_scale_field(unsigned maxbits) {  // exponent field of 2^e: 127 + e = 268 - field(max), clamped like x2_exponent
    const int f = 268 - (int)(maxbits >> 23);
    return f < 1 ? 1 : (f > 253 ? 253 : f);
}
__device__ __forceinline__ float x2_scale(unsigned maxbits) { return __int_as_float(x2_scale_field(maxbits) << 23); }          // 2^e
__device__ __forceinline__ float x2_unscale(unsigned maxbits) { return __int_as_float((254 - x2_scale_field(maxbits)) << 23); }  // 2^-e

// ------------------------------------------------------------------ host side
static inline int nt_cus() {
    static int cached = 0;
    if (!cached) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
            return 256;
        cached = cus;
    }
    return cached;
}

// Process-wide switches of the dense contractions.  Read from the environment ONCE (first use); tests and tools change them
// through pdgn_gemm_set_mode / pdgn_gemm_set_config (no getenv per launch, no environment mutation at run time).
//   mode: 2 = products on the matrix cores, two scaled fp16 parts per value where that pays and three bf16 parts elsewhere (gemm_x3.hip,
//   default), 1 = three bf16 parts everywhere (PDGN_GEMM=x3), 0 = fp32 matrix instructions (gemm_nt.hip; PDGN_GEMM=fp32)
//   cfg:  -1 = the launch model's pick (default), 0 .. 3 = a forced tile configuration (PDGN_NT_CFG; measurement / tests)
//   shape16: per instance class of gemm_x3.hip, which bf16 matrix instruction it runs on (PDGN_X3_SHAPE / PDGN_X3_SHAPE16_MASK;
//   pdgn_gemm_set_shape)
struct NtSwitches {
    int mode, cfg, splitk, shape16, shape16_default;
};
NtSwitches &nt_switches();

// The tile configuration of a problem under the switches in force (gemm_plan.h: forced, or the launch model's pick on this device)
// and its record.  fp32: the fp32 kernel's family (mode 0, and every call gemm_nt.hip takes).
static inline int nt_pick(bool fp32, long long m, int n, int k, bool stats, bool no_tall = false) {
    return fp32 ? gemm_pick_fp32(nt_switches().cfg, m, n, k, stats, no_tall, nt_cus()) : gemm_pick_x3(nt_switches().cfg, m, n, k, stats, nt_cus());
}
static inline const GemmTile &nt_tile(bool fp32, int cfg) { return fp32 ? FP32_TILES[cfg] : X3_TILES[cfg]; }

// ---- the argument front
static inline bool nt_args_ok(long long m, int n, int k, int lda, int ldw, int ldadd, int ldc, const float *addend, bool wt) {
    return m >= 1 && n >= 4 && k >= 4 && n % 4 == 0 && k % 4 == 0 && lda % 4 == 0 && ldw % 4 == 0 && ldc % 4 == 0 &&
           lda >= k && ldw >= (wt ? n : k) && ldc >= n && (!addend || (ldadd % 4 == 0 && ldadd >= n)) && lda < (1 << 19) &&
           ldw < (1 << 19) && ldc < (1 << 19) && (long long)cdiv(m, 128) * cdiv(n, 64) < 0x7fffffffLL &&
           (!wt || (long long)k * ldw < (1LL << 27));
}
// weight gradient dW (n x k) = dY (m x n)^T X (m x k)
static inline bool nt_tn_big_args_ok(long long m, int n, int k, int ldy, int ldx) {
    return !(m < 1 || n < 4 || k < 4 || n % 4 || k % 4 || ldy % 4 || ldx % 4 || ldy < n || ldx < k || ldy >= (1 << 19) ||
             ldx >= (1 << 19) || m > 0x7fffffffLL * 16);
}
static inline int nt_tn_big_reduction(long long m) { return (int)(m > 0x7fffffff ? 0x7fffffff : m); }

struct NtEpi {                        // extended epilogue of pdgn_gemm_nt_ex (all optional)
    const float *row_bias = nullptr;
    int ld_rb = 0, rows_per_group = 1, act = 0;
    const float *gate = nullptr;
    int ldgate = 0;
    bool any() const { return row_bias || act || gate; }
};
// the extended epilogue's arguments checked and, when they are in range, taken into e (rows_per_group at least 1)
static inline bool nt_epi_ok(long long m, int n, const float *row_bias, int ld_rb, int rows_per_group, int act, const float *gate,
                             int ldgate, NtEpi &e) {
    if ((act != 0 && act != 2) || (row_bias && (ld_rb < n || ld_rb % 4 || rows_per_group < 1)) ||
        (gate && (ldgate < n || ldgate % 4)) || m >= (1LL << 31) || (row_bias && m * rows_per_group >= (1LL << 32)) ||
        (row_bias && rows_per_group >= 1 && ((m + rows_per_group - 1) / rows_per_group) * (long long)ld_rb * 4 >= (long long)NT_OOB))
        return false;
    e.row_bias = row_bias; e.ld_rb = ld_rb; e.rows_per_group = rows_per_group > 0 ? rows_per_group : 1; e.act = act; e.gate = gate;
    e.ldgate = ldgate;
    return true;
}

// The part of the argument block that both families fill alike: the problem, the epilogue, the plan's tiling; what only gemm_x3
// uses (stream-K workspace, split-K, pre-split planes, maxima) at "none".  The tile range and sk_per_wg are the launch's.
static inline void nt_fill_args(NtArgs &a, const GemmPlan &pl, long long m, int n, int k, const float *A, int lda, const float *W, int ldw,
                                const float *bias, const float *addend, int ldadd, float *C, int ldc, float *stat_part, const NtEpi &epi) {
    a.M = m; a.N = n; a.K = k; a.lda = lda; a.ldw = ldw; a.ldc = ldc; a.ldadd = ldadd;
    a.A = A; a.W = W; a.bias = bias; a.addend = addend; a.C = C; a.stat_part = stat_part;
    a.row_bias = epi.row_bias; a.ld_rb = epi.ld_rb; a.rows_per_group = epi.rows_per_group;
    a.rpg_magic = a.rows_per_group > 1 ? (unsigned)(0x100000000ULL / (unsigned)a.rows_per_group) + 1u : 0u;
    a.rb_bytes = epi.row_bias ? (int)((((m + a.rows_per_group - 1) / a.rows_per_group - 1) * (long long)epi.ld_rb + n) * 4) : 0;
    a.act = epi.act; a.gate = epi.gate; a.ldgate = epi.ldgate;
    a.sk_split = 0; a.sk_ws = nullptr; a.sk_seg = 0; a.Wp = nullptr; a.wplane = 0; a.max_a = a.max_w = nullptr;
    a.tiles_m = pl.tiles_m; a.tiles_n = pl.tiles_n; a.kchunks = pl.kchunks;
    a.dbg = 0;
#ifdef PDGN_NT_DEBUG
    { const char *e = getenv("PDGN_NT_DBG"); a.dbg = e ? atoi(e) : 0; }
#endif
}

// A kernel instance as the launchers hand it around: its host symbol and workgroup size.  An instance that does not exist (NULL)
// is a build error, not a run-time condition: launching it aborts.
struct NtInstance {
    const void *sym;
    int threads;
};
static inline void nt_go(NtInstance f, int grid, hipStream_t s, const NtArgs &a) {
    if (!f.sym) abort();
    NtArgs args = a;
    void *params[] = {&args};
    (void)hipLaunchKernel(f.sym, dim3(grid), dim3(f.threads), params, 0, s);
}

// ---- what one contraction file calls in another
// gemm_nt.hip: the fp32-matrix-instruction forms of the public entry points; gemm_x3.hip dispatches between the two
int fp32_gemm_nt(long long m, int n, int k, const float *A, int lda, const float *W, int ldw, const float *bias,
                 const float *addend, int ldadd, float *C, int ldc, float *stat_part, pdgn_stream_t stream);
int fp32_gemm_nn(long long m, int n, int k, const float *A, int lda, const float *Wt, int ldw, const float *bias,
                 const float *addend, int ldadd, float *C, int ldc, float *stat_part, pdgn_stream_t stream);
int fp32_gemm_nt_ex(long long m, int n, int k, const float *A, int lda, const float *W, int ldw, const float *bias,
                    const float *addend, int ldadd, float *C, int ldc, float *stat_part, const float *row_bias, int ld_rb,
                    int rows_per_group, int act, const float *gate, int ldgate, int transposed_w, pdgn_stream_t stream);
int fp32_gemm_tn_big(long long m, int n, int k, const float *dY, int ldy, const float *X, int ldx, float *dW,
                     pdgn_stream_t stream);
// gemm_rp.hip: the row-panel kernel of the short-reduction, wide-result products on two-part planes
bool rp_takes(long long m, int n, int k);
int rp_launch(long long m, int n, int k, const float *A, int lda, const unsigned short *Wp, int ldw, long long wplane, float *C, int ldc,
              float *stat_part, hipStream_t s);
// gemm_x3_16.hip / gemm_x3_h2.hip: instance (tile, flags: x3_flags) of gemm_x3_kernel<..., 16> / of gemm_x3_kernel<..., 32, 2> (two fp16
// parts; the 256 x 128 tile as eight waves or four)
NtInstance x3_instance16(int cfg, int flags);
NtInstance x3_instance_h2(int flags, bool eight_waves);
