// Which kernel a toist_gemm_bf16 call runs on.  Host only: integers, null-ness and the alignment of pointers -- no HIP header, so the unit
// (gemm_route.cpp) builds with a plain C++17 compiler and runs on a CPU under a sanitizer (tests/gemm_route_main.cpp).
//
// gemm_check() holds the preconditions on descriptor fields, gemm_route() is the one place that decides; toist_gemm_bf16 (gemm.hip) switches
// on the family and calls the launch function, toist_gemm_pick_tile / toist_gemm_effective_split report the same plan.  A new kernel family
// is one predicate and one step of gemm_route()'s ladder here, one enum value below and one `case` in toist_gemm_bf16.
#pragma once
#include "../../include/toist_hip.h"

namespace toist {

// block shapes the predicates share with the kernels (gemm.hip derives its LDS layouts from them)
constexpr int C3_BM = 128, C3_BK = 64, C3_NP = 28;             // conv3_kernel: output rows, k-tile, 8-row pieces of a patch buffer
constexpr int G8_BM = 128, G8_BN = 128, G8_BK = 64;            // gemm128_kernel / gemm128w_kernel
constexpr int G9_BM = 256, G9_BN = 128, G9_NS = 6;             // gemm256w_kernel: block, ring stages of 32 k-rows

enum gemm_family {
    GEMM_TILES = 0,   // gemm_kernel<BM, BN, BK, ...>: tile codes 64, 65, 128, 129, 130, 132, 133, 134 (launch_tiles_a / _b / _c)
    GEMM_CONV3,       // 131: conv3_kernel, the shared-halo 3x3
    GEMM_PANEL,       // 135: panel_kernel (ring == 1) or panel2_kernel (ring = its variant word)
    GEMM_128,         // 136: gemm128_kernel
    GEMM_128W,        // 137: gemm128w_kernel
    GEMM_256W         // 138: gemm256w_kernel
};

enum gemm_post {
    GEMM_POST_NONE = 0,
    GEMM_POST_REDUCE,     // splitk_reduce_kernel folds the k-slices into C
    GEMM_POST_EPILOGUE,   // splitk_epilogue_kernel folds them and applies the complete epilogue (TOIST_GEMM_SPLIT_EPILOGUE)
    GEMM_POST_DEFERRED    // the caller folds (TOIST_GEMM_DEFER_REDUCE, toist_splitk_reduce_batch)
};

struct gemm_verdict {
    int code;             // TOIST_OK or TOIST_EINVAL
    char msg[320];        // the refusal, as toist_last_error reports it
};

struct gemm_plan : gemm_verdict {
    int family;                       // gemm_family; of a refused plan: the family that refused
    int tile;                         // tile code, as toist_gemm_pick_tile reports it
    int ring;                         // ring / variant word for the launch function (tile >> 8; GEMM_PANEL: see above)
    int batch, batch_inner, split;    // normalised (>= 1); split = the k-slices the launch makes (toist_gemm_effective_split)
    int post;                         // gemm_post
};

// the preconditions of toist_gemm_bf16 on descriptor fields, first failure first
gemm_verdict gemm_check(const toist_gemm& desc);
// the plan for a descriptor; tile and split are answered for refused (and unchecked) descriptors too
gemm_plan gemm_route(const toist_gemm& desc);
// what epilogue_lean covers: launch_variant and launch_conv3 pick their instantiation by it
bool lean_epilogue_ok(const toist_gemm& d);

// conv_pair_kernel (toist_conv_pair_bf16): 64-row blocks, C = 256 channels with a 4C-wide intermediate
constexpr int CP_BM = 64, CP_C = 256;
// the preconditions of toist_conv_pair_bf16, first failure first
gemm_verdict pair_check(const toist_conv_pair& desc);
bool pair_applies(const toist_conv_pair& desc);
// the toist_gemm_bf16 call the pair's second product replaces: conv_pair_kernel sums the two 32-deep halves of every 64-deep k-tile apart
// exactly when that call would run on gemm128_kernel (gemm_route()), so both paths round alike at every M
toist_gemm pair_second_gemm(const toist_conv_pair& desc);

}  // namespace toist
