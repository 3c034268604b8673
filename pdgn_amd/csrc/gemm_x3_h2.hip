// gemm_x3_h2.hip -- the two-part instances of gemm_x3_kernel (gemm_x3.hip, template parameter NP = 2: two scaled fp16 parts per
// operand value, three partial products on v_mfma_f32_32x32x16_f16) in a translation unit of their own, built beside the bf16 forms:
// the 256 x 128 tile only (x2_pays: the launches whose time is their matrix-core work).  gemm_x3.hip's launcher reaches them through
// x3_instance_h2; the list of flag combinations is gemm_x3.hip's own (X3_INSTANCES).
#define X3_KERNEL_ONLY
#include "gemm_x3.hip"

// The 256 x 128 tile in two shapes.  Eight waves of 64 x 64 (two per SIMD; 174 vector registers): while one wave's matrix
// instructions run the other issues its split / LDS / load instructions -- the two-part loop has half the matrix-core work of the
// bf16 form to hide the same operand path behind, and one wave per SIMD no longer hides it (alone: conv2's dense half 950 -> 860 us,
// the per-point product 750 -> 715, 71680 x 1024 x 256 275 -> 253; identical results).  Four waves of 128 x 64 for the launches
// that emit BatchNorm partials: their layout (two partial rows per tile row, pdgn_gemm_nt_stat_rows) is the four-wave tile's.
typedef X3Cfg<2, 2, 4, 2, 1> X2Big8;
static_assert(X2Big8::BM == X3Big::BM && X2Big8::BN == X3Big::BN, "both shapes are the 256 x 128 tile");

NtInstance x3_instance_h2(int flags, bool eight_waves) {
    return eight_waves ? X2Big8::instance<32, 2>(flags) : X3Big::instance<32, 2>(flags);
}
