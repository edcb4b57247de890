// One (dtype, BM x BN) instantiation of the implicit-GEMM kernel: compiled once per tile by the Makefile with
// -DPSG_TILE_BF16=0|1 -DPSG_TILE_BM=.. -DPSG_TILE_BN=..
#include "conv_gemm_kernel.h"
#ifndef PSG_TILE_BM          // (a bare `hipcc -c conv_tile.hip` still compiles: the smallest fp32 tile)
#define PSG_TILE_BF16 0
#define PSG_TILE_BM 64
#define PSG_TILE_BN 64
#endif

namespace psg {
#if PSG_TILE_BF16
typedef bf16_t tile_t;
#else
typedef float tile_t;
#endif
// What is built: the border-class form for bf16 modes 0 / 1, unsplit; the parity-class mode unsplit and not 160 wide (its tap
// tables push a 160-wide kernel past the scalar register file - one layer, the first downsample's data gradient, runs
// 128x128 instead); everything else of (MODE 0..3) x SPLITK x CLS.
template <typename T, int BM, int BN, int MODE, bool SPLITK, bool CLS> constexpr ConvKernel conv_variant() {
    if constexpr (CLS ? (sizeof(T) != 2 || MODE > 1 || SPLITK) : (MODE == 3 && (SPLITK || BN == 160))) return nullptr;
    else return conv_gemm_kernel<T, BM, BN, MODE, SPLITK, CLS>;
}
template <typename T, int BM, int BN> const ConvKernels& conv_kernels() {
#define PSG_MODE(M) {{conv_variant<T, BM, BN, M, false, false>(), conv_variant<T, BM, BN, M, false, true>()}, \
                     {conv_variant<T, BM, BN, M, true, false>(), conv_variant<T, BM, BN, M, true, true>()}}
    static const ConvKernels k = {{PSG_MODE(0), PSG_MODE(1), PSG_MODE(2), PSG_MODE(3)}, conv_splitk_finish_kernel<T>};
#undef PSG_MODE
    return k;
}
template const ConvKernels& conv_kernels<tile_t, PSG_TILE_BM, PSG_TILE_BN>();
}  // namespace psg
