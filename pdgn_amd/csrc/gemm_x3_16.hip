// gemm_x3_16.hip -- the v_mfma_f32_16x16x32_bf16 instances of gemm_x3_kernel (gemm_x3.hip, template parameter MS = 16) in a
// translation unit of their own: 33 instances of a 192-instruction straight-line chunk take as long to compile as the 33 of the
// default form, and the two files build side by side.  gemm_x3.hip's launcher reaches them through x3_instance16; the tiles and
// the list of flag combinations are gemm_x3.hip's own (x3_tile_instance).
#define X3_KERNEL_ONLY
#include "gemm_x3.hip"

NtInstance x3_instance16(int cfg, int flags) { return x3_tile_instance<16>(cfg, flags); }
