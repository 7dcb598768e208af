// The dispatcher of toist_gemm_bf16: preconditions, the predicates of every kernel family with the measurements behind their thresholds,
// and the one ladder that picks a family (gemm_route.h).  Plain C++: nothing here touches the GPU.
#include "gemm_route.h"

#include <cstddef>
#include <cstdio>

#include "tuning.h"

namespace toist {

static bool aligned16(const void* p) { return (((size_t)p) & 15) == 0; }

static void normalise(toist_gemm& d) {
    if (d.batch <= 0) d.batch = 1;
    if (d.batch_inner <= 0) d.batch_inner = 1;
    if (d.split_k <= 0) d.split_k = 1;
}

// records the first refusal only: what follows one is still evaluated (fields and integers, no side effects) and the plan's tile and
// split are still worked out behind it
#define GEMM_REQUIRE(v, cond, ...) \
    do { if ((v).code == TOIST_OK && !(cond)) { (v).code = TOIST_EINVAL; std::snprintf((v).msg, sizeof((v).msg), __VA_ARGS__); } } while (0)

gemm_verdict gemm_check(const toist_gemm& desc) {
    gemm_verdict v{};
    toist_gemm d = desc;
    GEMM_REQUIRE(v, d.M > 0 && d.N > 0 && d.K > 0, "toist_gemm_bf16: bad shape M=%d N=%d K=%d", d.M, d.N, d.K);
    normalise(d);
    GEMM_REQUIRE(v, d.a.ptr && d.b.ptr && d.c, "toist_gemm_bf16: null operand");
    GEMM_REQUIRE(v, aligned16(d.a.ptr) && aligned16(d.b.ptr), "toist_gemm_bf16: A/B must be 16-byte aligned");
    const toist_operand* ops[2] = {&d.a, &d.b};
    const int kinds[2] = {d.a_kind, d.b_kind == TOIST_B_CONVX ? TOIST_A_CONV : (d.b_kind == TOIST_B_KROW ? TOIST_A_KROW : TOIST_A_ROWK)};
    for (int i = 0; i < 2; ++i) {
        const toist_operand& o = *ops[i];
        GEMM_REQUIRE(v, (o.bs_outer % 8) == 0 && (o.bs_inner % 8) == 0, "toist_gemm_bf16: batch strides must be multiples of 8 elements");
        if (kinds[i] == TOIST_A_CONV || kinds[i] == TOIST_A_CONVT) {
            GEMM_REQUIRE(v, o.SC > 0 && (o.SC % 8) == 0, "toist_gemm_bf16: source channels must be a multiple of 8 (got %d)", o.SC);
            GEMM_REQUIRE(v, o.R > 0 && o.S > 0 && o.stride > 0 && o.dil > 0 && o.PH > 0 && o.PW > 0 && o.SH > 0 && o.SW > 0,
                         "toist_gemm_bf16: bad conv geometry");
        } else {
            GEMM_REQUIRE(v, o.ld > 0 && (o.ld % 8) == 0, "toist_gemm_bf16: leading dimension must be a multiple of 8 (got %d)", o.ld);
        }
    }
    if (d.b_kind == TOIST_B_CONVX) GEMM_REQUIRE(v, (d.N % 8) == 0, "toist_gemm_bf16: CONVX needs N %% 8 == 0");
    // k-major operands are read in 8-row chunks: rows beyond M/N inside the last chunk are read
    // (and discarded), so ld must cover the rounded-up extent.
    if (d.a_kind == TOIST_A_KROW) GEMM_REQUIRE(v, d.a.ld >= ((d.M + 7) & ~7), "toist_gemm_bf16: A_KROW needs lda >= roundup8(M)");
    if (d.b_kind == TOIST_B_KROW) GEMM_REQUIRE(v, d.b.ld >= ((d.N + 7) & ~7), "toist_gemm_bf16: B_KROW needs ldb >= roundup8(N)");
    const bool split_epi = (d.flags & TOIST_GEMM_SPLIT_EPILOGUE) != 0 && d.split_k > 1;
    if ((d.split_k > 1 && !split_epi) || d.epi.accumulate)
        GEMM_REQUIRE(v, d.epi.out_f32, "toist_gemm_bf16: split_k/accumulate needs an f32 output");
    if (split_epi)
        GEMM_REQUIRE(v, d.workspace != nullptr && d.batch == 1 && d.group == nullptr && (d.N % 4) == 0 && !d.epi.cmap && !d.epi.accumulate &&
                         !(d.flags & TOIST_GEMM_DEFER_REDUCE) && (d.tile & 255) != 131 && !d.a_colsum,
                     "toist_gemm_bf16: TOIST_GEMM_SPLIT_EPILOGUE needs a workspace, batch = 1, no group / row map / accumulate, N %% 4 == 0");
    if (d.a_colsum) GEMM_REQUIRE(v, d.a_kind == TOIST_A_KROW, "toist_gemm_bf16: a_colsum needs a k-major A operand");
    if (d.flags & TOIST_GEMM_COLSUM_SLICES)
        GEMM_REQUIRE(v, d.a_colsum != nullptr && d.group == nullptr && d.batch == 1 && d.split_k > 1 && !split_epi,
                     "toist_gemm_bf16: TOIST_GEMM_COLSUM_SLICES needs a_colsum, split_k > 1, batch = 1, no group and no split epilogue");
    if (d.group) GEMM_REQUIRE(v, (d.split_k <= 1 || (d.flags & TOIST_GEMM_DEFER_REDUCE)) && d.batch_inner == 1 && !d.epi.cmap && (d.tile & 255) != 131 &&
                                  d.a_kind != TOIST_A_CONVT,
                              "toist_gemm_bf16: a grouped launch takes batch_inner = 1, no cmap, a generic tile, and folds its k-slices through "
                              "toist_splitk_reduce_batch (TOIST_GEMM_DEFER_REDUCE; workspace = [problem][k-slice][M][N])");
    if (d.split_k > 1 && !split_epi) {
        GEMM_REQUIRE(v, !d.epi.scale && !d.epi.shift && !d.epi.res && d.epi.act == TOIST_ACT_NONE && !d.epi.pre_out && d.epi.drop_where == 0 &&
                         !d.epi.cmap && (d.batch == 1 || d.group != nullptr),
                     "toist_gemm_bf16: split_k only supports alpha/rscale/accumulate epilogues on a single batch (or a grouped launch)");
        GEMM_REQUIRE(v, d.workspace != nullptr && (d.N % 4) == 0 && (d.ldc % 4) == 0, "toist_gemm_bf16: split_k needs a workspace and N, ldc %% 4 == 0");
    }
    if (d.epi.act >= TOIST_ACT_MASK_POS) GEMM_REQUIRE(v, d.epi.aux != nullptr, "toist_gemm_bf16: activation %d needs aux", d.epi.act);
    if (d.a2) GEMM_REQUIRE(v, d.a_kind == TOIST_A_ROWK && aligned16(d.a2) && d.a2_from > 0 && (d.a2_from % 128) == 0 && d.split_k <= 1,
                           "toist_gemm_bf16: a2 needs a row-major A, 16-byte alignment, a2_from %% 128 == 0 and no split");
    if (d.epi.drop_where) GEMM_REQUIRE(v, d.epi.drop_p >= 0.f && d.epi.drop_p < 1.f, "toist_gemm_bf16: bad dropout p");
    return v;
}

// what epilogue_lean (and the panel kernel's epilogue) covers
bool lean_epilogue_ok(const toist_gemm& d) {
    // TOIST_LEAN_EPILOGUE: 0 = never, 1 = only scale / shift / residual / ReLU / mask, 2 (default) = also dropout, GELU, aux-based gradients, row map
    static const int level = (int)tuning_knob("TOIST_LEAN_EPILOGUE", 2);
    const toist_epilogue& e = d.epi;
    if (level == 1 && (e.drop_where || e.cmap || (e.act != TOIST_ACT_NONE && e.act != TOIST_ACT_RELU && e.act != TOIST_ACT_MASK_POS))) return false;
    if (level <= 0 || d.split_k > 1 || d.group != nullptr || d.a_colsum != nullptr) return false;
    if (e.out_f32 || e.accumulate || e.rscale || e.pre_out || e.res_div > 0) return false;
    if (e.act == TOIST_ACT_SIGMOID) return false;
    if ((d.N % 8) != 0 || (d.ldc % 8) != 0 || !aligned16(d.c) || (d.cs_outer % 8) != 0 || (d.cs_inner % 8) != 0) return false;
    if (e.res && ((e.ldr % 8) != 0 || !aligned16(e.res))) return false;
    if (e.act >= TOIST_ACT_MASK_POS && (e.aux == nullptr || (e.ldaux % 8) != 0 || !aligned16(e.aux))) return false;
    if ((e.scale && (((size_t)e.scale) & 15)) || (e.shift && (((size_t)e.shift) & 15))) return false;
    return true;
}

// panel_kernel / panel2_kernel.  Tile code 135, or picked by the dispatcher (panel_min_tiles) when the call qualifies.
static bool panel_applies(const toist_gemm& d) {
    if (d.a_kind != TOIST_A_ROWK || (d.b_kind != TOIST_B_ROWK && d.b_kind != TOIST_B_KROW)) return false;
    if (d.b_kind == TOIST_B_KROW && d.b.kin > 0) return false;
    if (d.K > 256 || (d.K % 8) != 0 || (d.a.ld % 8) != 0 || (d.b.ld % 8) != 0) return false;
    if (d.batch != 1 || d.split_k != 1 || d.group != nullptr || d.a2 != nullptr || d.a_colsum != nullptr || (d.flags & 1)) return false;
    if ((d.N + 63) / 64 > 64 || (d.M + 63) / 64 < 8) return false;      // row tiles are dealt to 8 XCDs: too few would leave XCDs idle
    if ((long long)d.M * d.a.ld >= (1ll << 30) || (long long)d.K * d.b.ld >= (1ll << 30) || (long long)d.N * d.b.ld >= (1ll << 30)) return false;   // 32-bit element offsets
    // the kernel's lean epilogue: bf16 rows in whole 16-byte chunks, per-column scale / shift, residual, {none, ReLU, aux > 0 mask}
    const toist_epilogue& e = d.epi;
    if (e.out_f32 || e.accumulate || e.rscale || e.pre_out || e.cmap || e.res_div > 0) return false;
    if (e.drop_where && !(e.drop_p >= 0.f && e.drop_p < 1.f)) return false;
    if (e.act != TOIST_ACT_NONE && e.act != TOIST_ACT_RELU && e.act != TOIST_ACT_MASK_POS) return false;
    if ((d.N % 8) != 0 || (d.ldc % 8) != 0 || !aligned16(d.c) || (long long)d.M * d.ldc >= (1ll << 31)) return false;
    if (e.res && ((e.ldr % 8) != 0 || !aligned16(e.res) || (long long)d.M * e.ldr >= (1ll << 31))) return false;
    if (e.act == TOIST_ACT_MASK_POS && ((e.ldaux % 8) != 0 || !aligned16(e.aux) || (long long)d.M * e.ldaux >= (1ll << 31))) return false;
    if ((e.scale && (((size_t)e.scale) & 15)) || (e.shift && (((size_t)e.shift) & 15))) return false;
    return true;
}

static long long panel_min_tiles() {   // (32 -- the 800-query decoder linears, 52 tiles -- measured 559.8 -> 563.8 images/s over two noisy rounds: not taken)
    static const long long v = tuning_knob("TOIST_PANEL_MIN_TILES", 128);
    return v;
}

// panel2_kernel: what panel_applies admits, with byte offsets that fit the 2 GiB buffer descriptors of the DMA / store path
static bool panel2_applies(const toist_gemm& d) {
    if (!panel_applies(d)) return false;
    const long long lim = 1ll << 30;
    if ((long long)d.M * d.ldc >= lim) return false;
    if (d.epi.res && (long long)d.M * d.epi.ldr >= lim) return false;
    if (d.epi.act == TOIST_ACT_MASK_POS && (long long)d.M * d.epi.ldaux >= lim) return false;
    return true;
}

// conv3_kernel: true when the halo kernel covers this call (the dispatcher then never looks at the tile code)
static bool conv3_applies(const toist_gemm& d) {
    const bool fwd = d.a_kind == TOIST_A_CONV && d.b_kind == TOIST_B_ROWK;
    const bool dgr = d.a_kind == TOIST_A_CONVT && d.b_kind == TOIST_B_KROW;
    if (!fwd && !dgr) return false;
    const toist_operand& a = d.a;
    if (a.R != 3 || a.S != 3 || a.stride != 1 || a.pad != 1 || a.dil != 1) return false;
    if (a.PH != a.SH || a.PW != a.SW || (a.SC % C3_BK) != 0 || d.K != 9 * a.SC) return false;
    if (C3_BM + 2 * (a.SW + 1) > C3_NP * 8) return false;            // patch rows must fit the 28 pieces
    if (d.batch != 1 || d.split_k != 1 || d.a_colsum != nullptr) return false;
    if ((long long)d.M * a.SC >= (1ll << 30)) return false;           // 32-bit element offsets
    if (fwd && d.b.ld != d.K) return false;
    if (dgr && (d.b.kin != a.SC || (d.N % 8) != 0)) return false;
    return d.M >= 2048;                                                // tiny grids: the generic 64x64 tiles fill more CUs
}

// drop k-slices that would own no k-tile
static int clamp_split(int split_k, int K, int tile) {
    const int bk0 = (tile == 64 || tile == 128) ? 32 : 64;
    const int ktiles = (K + bk0 - 1) / bk0;
    if (ktiles < 1) return 1;                                 // (K <= 0: refused by gemm_check(); the queries answer one slice)
    if (split_k < 1) split_k = 1;
    if (split_k > ktiles) split_k = ktiles;
    const int kper = (ktiles + split_k - 1) / split_k;
    return (ktiles + kper - 1) / kper;
}

// gemm128_kernel (tile code 136): one problem, K a multiple of 64 with at least 4 k-tiles, bf16 rows finished by {alpha, scale, shift,
// residual, ReLU | aux > 0 mask}.  Operands: row-major A with row-major or plain k-major B (1x1 convolutions, nn.Linear and their data
// gradients); convolution gather of stride 1 or 2 with row-major weights (forward); its stride-1 transposed gather on a same-size plane with the
// two-level k-major weights (data gradient) -- up to 16 taps, source channels a multiple of 64.
static bool gemm128_applies(const toist_gemm& d) {
    const bool plain = d.a_kind == TOIST_A_ROWK && (d.b_kind == TOIST_B_ROWK || (d.b_kind == TOIST_B_KROW && d.b.kin == 0));
    const bool fwd = d.a_kind == TOIST_A_CONV && d.b_kind == TOIST_B_ROWK;
    const bool dgr = d.a_kind == TOIST_A_CONVT && d.b_kind == TOIST_B_KROW;
    if (!plain && !fwd && !dgr) return false;
    if (d.K < 256 || (d.K % 64) != 0 || (d.b.ld % 8) != 0) return false;
    if (d.batch != 1 || d.split_k != 1 || d.group != nullptr || d.a2 != nullptr || d.a_colsum != nullptr || (d.flags & 1)) return false;
    const long long lim = 1ll << 30;
    if ((long long)d.K * d.b.ld >= lim || (long long)d.N * d.b.ld >= lim) return false;       // 32-bit byte offsets
    if (plain) {
        if ((d.a.ld % 8) != 0 || (long long)d.M * d.a.ld >= lim) return false;
    } else {
        const toist_operand& a = d.a;
        if ((a.stride != 1 && !fwd) || a.stride < 1 || a.stride > 2 || a.R * a.S > 16 || (a.SC % 64) != 0 || d.K != a.R * a.S * a.SC) return false;
        if (a.PH <= 0 || a.PW <= 0) return false;               // (the queries also answer for descriptors gemm_check() refuses)
        if ((long long)(d.M / (a.PH * a.PW) + 1) * a.SH * a.SW * a.SC >= lim) return false;
        if (fwd && d.b.ld != d.K) return false;
        if (dgr && (a.PH != a.SH || a.PW != a.SW || d.b.kin != a.SC)) return false;
        if (dgr && (a.pad - (a.R - 1) * a.dil > 0 || a.pad - (a.S - 1) * a.dil > 0)) return false;   // the shifted base must not lie beyond tap (0, 0)
    }
    const toist_epilogue& e = d.epi;
    if (!lean_epilogue_ok(d) || e.drop_where || e.cmap) return false;
    if (e.act != TOIST_ACT_NONE && e.act != TOIST_ACT_RELU && e.act != TOIST_ACT_MASK_POS) return false;
    if ((d.N % 8) != 0) return false;                     // ldc / ldr / ldaux % 8 and 16-byte bases: lean_epilogue_ok above
    return true;
}

// Where the dispatcher picks it (profiles/r03_gemm128_us.txt): one block per CU, so it needs about a chip of 128 x 128 tiles and a deep
// reduction to amortise its prologue / k-fold epilogue.  Gathers: every stride-1 3x3 of layers 2-4 at the bench batch (-1 .. -16 us per
// launch against the 64 x 64 tiles and the halo kernel).  Plain GEMMs: K >= 768 from 150 tiles on (12800 x 256 x 1024: 14.7 / 15.5 vs
// 18.2 / 20.3 us forward / data gradient, 12800 x 512 x 1024: 25.4 / 27.5 vs 29.2 / 31.8, 4096^3: 150 vs 169); K = 512 loses (two rounds of
// 8 k-tiles do not amortise the fixed costs), 100 tiles are a draw.
static bool gemm128_pays(const toist_gemm& d) {
    static const int on = (int)tuning_knob("TOIST_GEMM128", 1);
    if (!on || !gemm128_applies(d)) return false;
    const long long tiles = (long long)((d.M + G8_BM - 1) / G8_BM) * ((d.N + G8_BN - 1) / G8_BN);
    if (d.a_kind != TOIST_A_ROWK) return tiles >= 96 && (d.N % G8_BN) == 0;
    return d.K >= 768 && tiles >= 150;
}

// gemm128w_kernel (tile code 137): weight gradients -- k-major A (dy [pixels][Co]), B = k-major rows (1x1) or the stride-1 same-size
// gather with whole 128-column tiles inside a tap; f32 output with alpha / rscale / accumulate, or k-slice partials; grouped or single.
static bool gemm128w_applies(const toist_gemm& d) {
    if (d.a_kind != TOIST_A_KROW) return false;
    const bool plain = d.b_kind == TOIST_B_KROW && d.b.kin == 0, gather = d.b_kind == TOIST_B_CONVX;
    if (!plain && !gather) return false;
    if ((d.K % 64) != 0 || (d.M % 8) != 0 || (d.N % 8) != 0 || (d.a.ld % 8) != 0) return false;
    if (d.batch_inner != 1 || (d.batch != 1 && d.group == nullptr) || d.a2 != nullptr || d.a_colsum != nullptr || (d.flags & (1 | TOIST_GEMM_SPLIT_EPILOGUE))) return false;
    const int split = clamp_split(d.split_k, d.K, 65);                                  // the slices the launch will really make
    const int ktiles = d.K / 64, kper = (ktiles + split - 1) / split;
    if (kper < 4 || (long long)(split - 1) * kper + 4 > ktiles) return false;          // every k-slice holds at least 4 k-tiles
    if (split > 1 && d.workspace == nullptr) return false;
    const long long lim = 1ll << 30;
    if ((long long)d.K * d.a.ld >= lim) return false;                                   // 32-bit byte offsets
    if (plain) {
        if ((d.b.ld % 8) != 0 || (long long)d.K * d.b.ld >= lim) return false;
    } else {
        const toist_operand& b = d.b;
        if (b.stride < 1 || b.stride > 2 || (b.SC % 128) != 0 || d.N != b.R * b.S * b.SC) return false;
        if (b.stride == 1 && (b.PH != b.SH || b.PW != b.SW)) return false;                 // stride 1: the same-size plane trick (address = pixel + constant)
        if (b.PH <= 0 || b.PW <= 0 || (d.K % (b.PH * b.PW)) != 0) return false;
        if ((long long)(d.K / (b.PH * b.PW) + 1) * b.SH * b.SW * b.SC + (long long)b.SW * (b.pad + 1) * b.SC >= lim) return false;
    }
    const toist_epilogue& e = d.epi;
    if (!e.out_f32 || e.scale || e.shift || e.res || e.pre_out || e.act != TOIST_ACT_NONE || e.drop_where || e.cmap || e.res_div > 0) return false;
    if ((d.ldc % 4) != 0 || (((size_t)d.c) & 15) != 0) return false;
    return true;
}

// where it replaces the grouped / split tiles the host asked for (profiles/r03_gemm128w_us.txt)
static bool gemm128w_pays(const toist_gemm& d) {
    static const int on = (int)tuning_knob("TOIST_GEMM128W", 1);
    if (!on || !gemm128w_applies(d)) return false;
    const long long wgs = (long long)((d.M + G8_BM - 1) / G8_BM) * ((d.N + G8_BN - 1) / G8_BN) * d.batch * clamp_split(d.split_k, d.K, 65);
    return wgs >= 128 && (d.M % 64) == 0 && (d.N % 128) == 0;
}

// gemm256w_kernel (tile code 138): what gemm128w_kernel takes, with M a multiple of 256 and k-slices of at least 6 x 32 rows
static bool gemm256w_applies(const toist_gemm& d) {
    if (!gemm128w_applies(d) || (d.M % G9_BM) != 0 || (d.N % G9_BN) != 0) return false;
    const int split = clamp_split(d.split_k, d.K, 65);
    const int k64 = d.K / 64, kper = (k64 + split - 1) / split;
    return 2 * (k64 - (split - 1) * kper) >= G9_NS;      // the last (shortest) slice fills the ring
}

static bool gemm256w_pays(const toist_gemm& d) {
    static const int on = (int)tuning_knob("TOIST_GEMM256W", 1);
    if (!on || !gemm256w_applies(d)) return false;
    const long long wgs = (long long)(d.M / G9_BM) * (d.N / G9_BN) * d.batch * clamp_split(d.split_k, d.K, 65);
    return wgs >= 128;
}

// the big generic tiles the host asks for on (grouped) weight gradients -- and the automatic choice -- give way to the 128x128 kernel
static int wgrad_tile_replaced(const toist_gemm& d) {       // 0 = no, else 137 / 138
    const int t = d.tile & 255;
    if (!((t == 0 || t == 129 || t == 130 || t == 134) && d.a_kind == TOIST_A_KROW)) return 0;
    if (gemm256w_pays(d)) return 138;
    return gemm128w_pays(d) ? 137 : 0;
}

// tile code the dispatcher picks for tile == 0
static int auto_tile(const toist_gemm& d) {
    // measured on MI355X (tools/sweep_gemm.py): 128x128x64 only pays once >= ~4 tiles per CU exist and K
    // is deep; below that 64x64x64 tiles keep more workgroups (and DMA) in flight.
    const long long t128 = (long long)((d.M + 127) / 128) * ((d.N + 127) / 128) * d.batch * d.split_k;
    // (round 2: the 128x64 tile beats 128x128 on every large problem measured -- 4096^3: 675 vs 555 TFLOP/s, 8192 x 8192 x 2048: 708 vs 443;
    // 128x128 needs 231-247 VGPRs, two waves per SIMD)
    static const int big_tile = (int)tuning_knob("TOIST_BIG_TILE", 130);
    if (t128 >= 1024 && d.K >= 1024) return big_tile;
    if (d.K > 64 && d.N <= 32 && d.M >= 4096) return 132;   // a 64-wide tile would idle half (or more) of its MFMA columns
    if (d.K > 64 && d.M <= 32 && d.N >= 128) return 133;
    // Wave quantisation of the 64x64 grid: four two-slot workgroups fit a CU (1024 slots; three before the occupancy hint of gemm_kernel,
    // when 800 tiles -- ResNet layer3 at batch 8 -- were a full round plus a 4 % one and this rule bought 28 -> 21 us).  When the last
    // round would be < 1/4 full and there are at most two full ones, 64x128 tiles (half the workgroups, half the A traffic through LDS)
    // finish in fewer rounds: 17000 x 256 x 1024 25.8 -> 21.2 us, 20000 x 256 x 1024 26.6 -> 22.1, 12800 x 384 x 1024 25.9 -> 22.1; at
    // 1.5-1.6 rounds (12800 x 512 x 1024) the 64x64 grid stays ahead (29.3 vs 31.0), as it does below one round (tools/dbg/gemm_tiles.py).
    const long long t64 = (long long)((d.M + 63) / 64) * ((d.N + 63) / 64) * d.batch * d.split_k;
    const long long rounds = t64 / 1024, last = t64 - rounds * 1024;
    static const bool wide = tuning_knob("TOIST_TILE_64x128", 1) != 0;
    if (wide && d.K >= 512 && (d.N % 128) == 0 && rounds >= 1 && rounds <= 2 && last * 4 < 1024 &&
        (d.a_kind == TOIST_A_ROWK || d.a_kind == TOIST_A_CONV) && !d.group)
        return 134;
    // (a nearly full single round -- 800 tiles of 1024 -- stays on 64x64: 64x128 there measured 552 vs 556 images/s for the conv gathers, 546 with row-major A too)
    return (d.K > 64) ? 65 : 64;
}

// what launch_tiles_a / _b / _c and launch_tile (gemm.hip) are instantiated for: a new generic tile or operand pair is added there AND here
// tile codes: 64 = 64x64x32, 65 = 64x64x64, 128 = 128x128x32, 129 = 128x128x64, 130 = 128x64x64, 132 = 128x32x64, 133 = 32x128x64, 134 = 64x128x64
static bool generic_tile(int tile) { return tile == 64 || tile == 65 || (tile >= 128 && tile <= 134 && tile != 131); }
static bool generic_operands(int ak, int bk) {
    return bk == TOIST_B_KROW ? (ak >= TOIST_A_ROWK && ak <= TOIST_A_CONVT)      // (A_CONV x B_KROW: parity classes of a strided dgrad)
                              : (bk == TOIST_B_ROWK && (ak == TOIST_A_ROWK || ak == TOIST_A_CONV)) || (bk == TOIST_B_CONVX && ak == TOIST_A_KROW);
}

gemm_plan gemm_route(const toist_gemm& desc) {
    toist_gemm d = desc;
    normalise(d);
    gemm_plan r{};
    r.batch = d.batch, r.batch_inner = d.batch_inner;
    r.ring = d.tile >> 8;   // 0 = pick; else slots of the DMA ring (2..4)
    const int code = d.tile & 255;
    const bool panel_sized = (long long)((d.M + 63) / 64) * ((d.N + 63) / 64) >= panel_min_tiles();
    if (d.tile == 136 || (d.tile == 0 && gemm128_pays(d))) {
        r.family = GEMM_128, r.tile = 136;
        GEMM_REQUIRE(r, gemm128_applies(d), "toist_gemm_bf16: the 128x128 kernel does not cover this call");
    } else if (d.tile == 131 || (d.tile == 0 && d.a_kind == TOIST_A_CONVT && conv3_applies(d))) {
        // the 3x3 shared-halo kernel: picked for dgrad (measured 395 vs 351 TFLOP/s on layer 3), explicit tile code 131 otherwise
        // (forward: 384 vs 451 for the generic tiles)
        r.family = GEMM_CONV3, r.tile = 131;
        GEMM_REQUIRE(r, conv3_applies(d), "toist_gemm_bf16: the 3x3 halo kernel does not cover this call");
    } else if (code == 135 || (d.tile == 0 && panel_sized && panel_applies(d))) {
        r.family = GEMM_PANEL, r.tile = 135;
        GEMM_REQUIRE(r, panel_applies(d), "toist_gemm_bf16: the short-K panel kernel does not cover this call");
        // tile word 135 | variant << 8: variant 1 = the round-2 kernel, otherwise panel2_kernel (see launch_panel2); 255 = its own pick
        static const int def_variant = (int)tuning_knob("TOIST_PANEL_VARIANT", 0);
        const int variant = r.ring ? r.ring : def_variant;
        r.ring = (variant == 1 || !panel2_applies(d)) ? 1 : variant == 255 ? 0 : variant;
    } else {
        r.tile = code;
        if (code == 137) GEMM_REQUIRE(r, gemm128w_applies(d), "toist_gemm_bf16: the 128x128 weight-gradient kernel does not cover this call");
        if (code == 138) GEMM_REQUIRE(r, gemm256w_applies(d), "toist_gemm_bf16: the 256x128 weight-gradient kernel does not cover this call");
        if (const int wt = wgrad_tile_replaced(d)) r.tile = wt;
        if (r.tile == 0) r.tile = auto_tile(d);
        r.family = r.tile == 137 ? GEMM_128W : r.tile == 138 ? GEMM_256W : GEMM_TILES;
    }
    r.split = clamp_split(d.split_k, d.K, r.tile);      // 1 wherever a family takes no split
    r.post = r.split <= 1 ? GEMM_POST_NONE : (d.flags & TOIST_GEMM_DEFER_REDUCE) ? GEMM_POST_DEFERRED
           : (d.flags & TOIST_GEMM_SPLIT_EPILOGUE) ? GEMM_POST_EPILOGUE : GEMM_POST_REDUCE;
    if (r.family == GEMM_TILES || r.family == GEMM_128W || r.family == GEMM_256W) {
        if (d.flags & TOIST_GEMM_COLSUM_SLICES)      // the caller sized a_colsum (and its fold) by toist_gemm_effective_split: one row per slice
            GEMM_REQUIRE(r, r.split > 1, "toist_gemm_bf16: TOIST_GEMM_COLSUM_SLICES with a split that clamps to 1 (see toist_gemm_effective_split)");
        if (d.b_kind == TOIST_B_KROW && d.b.kin > 0) GEMM_REQUIRE(r, (d.b.kin % 8) == 0, "toist_gemm_bf16: kin %% 8 != 0");
    }
    if (r.family == GEMM_TILES) {
        GEMM_REQUIRE(r, generic_tile(r.tile), "toist_gemm_bf16: bad tile code %d", r.tile);
        GEMM_REQUIRE(r, generic_operands(d.a_kind, d.b_kind), "toist_gemm_bf16: unsupported operand kinds a=%d b=%d", d.a_kind, d.b_kind);
    }
    return r;
}

// ---- toist_conv_pair_bf16 ----
gemm_verdict pair_check(const toist_conv_pair& d) {
    gemm_verdict v{};
    const long long lim = 1ll << 30;      // byte offsets of the DMA / buffer-store path stay below 2 GiB
    GEMM_REQUIRE(v, d.M > 0 && d.C == CP_C, "toist_conv_pair_bf16: bad shape M=%d C=%d (C = %d only)", d.M, d.C, CP_C);
    GEMM_REQUIRE(v, d.dgrad == 0 || d.dgrad == 1, "toist_conv_pair_bf16: dgrad = %d (0 or 1)", d.dgrad);
    GEMM_REQUIRE(v, d.a && d.w_first && d.w_second && d.mid && d.out, "toist_conv_pair_bf16: null operand");
    GEMM_REQUIRE(v, d.res != nullptr, "toist_conv_pair_bf16: res is required");
    if (d.dgrad) {
        GEMM_REQUIRE(v, d.aux_mid && d.aux_out, "toist_conv_pair_bf16: the data gradient needs aux_mid and aux_out");
        GEMM_REQUIRE(v, !d.shift_mid && !d.shift_out, "toist_conv_pair_bf16: the data gradient takes no shift");
    } else {
        GEMM_REQUIRE(v, !d.aux_mid && !d.aux_out, "toist_conv_pair_bf16: aux_mid / aux_out belong to the data gradient (dgrad = 1)");
    }
    GEMM_REQUIRE(v, aligned16(d.a) && aligned16(d.w_first) && aligned16(d.w_second) && aligned16(d.res) && aligned16(d.mid) && aligned16(d.out) &&
                        aligned16(d.aux_mid) && aligned16(d.aux_out) && aligned16(d.shift_mid) && aligned16(d.shift_out),
                 "toist_conv_pair_bf16: every pointer must be 16-byte aligned");
    const int C = CP_C, C4 = 4 * CP_C;
    GEMM_REQUIRE(v, d.lda >= C && d.ldout >= C && d.ldmid >= C4 && d.ldr >= C4 && (d.lda % 8) == 0 && (d.ldout % 8) == 0 && (d.ldmid % 8) == 0 && (d.ldr % 8) == 0,
                 "toist_conv_pair_bf16: leading dimensions must cover the row and be multiples of 8 (lda=%d ldmid=%d ldr=%d ldout=%d)", d.lda, d.ldmid,
                 d.ldr, d.ldout);
    if (d.dgrad)
        GEMM_REQUIRE(v, d.ldaux_mid >= C4 && d.ldaux_out >= C && (d.ldaux_mid % 8) == 0 && (d.ldaux_out % 8) == 0,
                     "toist_conv_pair_bf16: leading dimensions must cover the row and be multiples of 8 (ldaux_mid=%d ldaux_out=%d)", d.ldaux_mid, d.ldaux_out);
    const long long rows = (long long)((d.M + CP_BM - 1) / CP_BM) * CP_BM;
    GEMM_REQUIRE(v, rows * d.lda < lim && rows * d.ldmid < lim && rows * d.ldr < lim && rows * d.ldout < lim &&
                        (!d.dgrad || (rows * d.ldaux_mid < lim && rows * d.ldaux_out < lim)),
                 "toist_conv_pair_bf16: M = %d rows exceed the 2 GiB byte offsets of the kernel", d.M);
    return v;
}

bool pair_applies(const toist_conv_pair& desc) { return pair_check(desc).code == TOIST_OK; }

toist_gemm pair_second_gemm(const toist_conv_pair& p) {
    toist_gemm d{};
    d.M = p.M, d.N = p.C, d.K = 4 * p.C;
    d.a_kind = TOIST_A_ROWK, d.b_kind = p.dgrad ? TOIST_B_KROW : TOIST_B_ROWK;
    d.a.ptr = p.mid, d.a.ld = p.ldmid;
    d.b.ptr = p.w_second, d.b.ld = p.dgrad ? p.C : 4 * p.C;
    d.c = p.out, d.ldc = p.ldout;
    d.batch = d.batch_inner = d.split_k = 1;
    d.epi.alpha = 1.f;
    d.epi.shift = p.shift_out;
    d.epi.act = p.dgrad ? TOIST_ACT_MASK_POS : TOIST_ACT_RELU;
    d.epi.aux = p.aux_out, d.epi.ldaux = p.dgrad ? p.ldaux_out : 0;
    return d;
}

}  // namespace toist

extern "C" int toist_gemm_pick_tile(const toist_gemm* desc) { return desc == nullptr ? 0 : toist::gemm_route(*desc).tile; }

extern "C" int toist_gemm_effective_split(const toist_gemm* desc) {
    if (desc == nullptr) return 0;
    toist_gemm d = *desc;
    if (d.workspace == nullptr) d.workspace = (float*)16;      // asked BEFORE the caller sizes the scratch: "a workspace will be there"
    return toist::gemm_route(d).split;
}
