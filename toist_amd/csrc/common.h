// Shared device/host helpers for the TOIST hot-path kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <cstdlib>
#include <type_traits>

#include "../../include/toist_hip.h"
#include "tuning.h"

typedef unsigned short bf16_t;  // raw bfloat16 bits
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(8))) short s16x8_t;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2_t;
typedef __attribute__((address_space(3))) s16x4_t* lds_v4;  // LDS operand of ds_read_b64_tr_b16

namespace toist {

// ---- error plumbing (host) -------------------------------------------------
void set_last_error(const char* fmt, ...);
int check_launch(const char* what);  // hipGetLastError -> TOIST_EHIP / TOIST_OK

#define TOIST_REQUIRE(cond, ...)                  \
    do {                                          \
        if (!(cond)) {                            \
            ::toist::set_last_error(__VA_ARGS__); \
            return TOIST_EINVAL;                  \
        }                                         \
    } while (0)

// ---- per-device one-time kernel attributes (> 64 KiB of dynamic LDS) ----------------------
// hipFuncSetAttribute is per device; a process that drives several devices must set it on each.  Lock-free and idempotent: two
// threads racing on the first launch both set the same value.  `done` = one bit per device ordinal.
template <typename F>
inline bool lds_attr_once_flag(std::atomic<unsigned long long>& done, F&& set) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return true;
    if (!set()) return false;
    done.fetch_or(bit, std::memory_order_release);
    return true;
}
template <typename F>
inline bool lds_attr_once(int slot, F&& set) {
    static std::atomic<unsigned long long> done[8];
    return lds_attr_once_flag(done[slot & 7], static_cast<F&&>(set));
}

// ---- bf16 <-> f32 ------------------------------------------------------------
__device__ __forceinline__ float bf2f(bf16_t h) { return __uint_as_float(((unsigned)h) << 16); }

// float -> bfloat16, round-to-nearest-even (torch's cast): gfx950 converts in hardware, two values per
// v_cvt_pk_bf16_f32 -- the hand-rolled rounding was 5-6 VALU operations per value in every epilogue
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_native_t;

__device__ __forceinline__ bf16_t f2bf(float f) { return __builtin_bit_cast(bf16_t, (__bf16)f); }

__device__ __forceinline__ unsigned pack2bf(float lo, float hi) {
    const bf16x2_native_t v = {(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(unsigned, v);
}

// ---- bf16 pack / unpack: eight values = one 16-byte access ---------------------------------
__device__ __forceinline__ void unpack8(const uint4& u, float* f) {
    f[0] = __uint_as_float(u.x << 16); f[1] = __uint_as_float(u.x & 0xffff0000u);
    f[2] = __uint_as_float(u.y << 16); f[3] = __uint_as_float(u.y & 0xffff0000u);
    f[4] = __uint_as_float(u.z << 16); f[5] = __uint_as_float(u.z & 0xffff0000u);
    f[6] = __uint_as_float(u.w << 16); f[7] = __uint_as_float(u.w & 0xffff0000u);
}
__device__ __forceinline__ uint4 pack8(const float* f) {
    return make_uint4(pack2bf(f[0], f[1]), pack2bf(f[2], f[3]), pack2bf(f[4], f[5]), pack2bf(f[6], f[7]));
}

// ---- wave (64-lane) reductions -------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- lane-group reductions -------------------------------------------------------
// sum over the 16 lanes of a row group (lanes 16 r .. 16 r + 15 of the wave)
__device__ __forceinline__ float group16_sum(float v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 8, 64);
    return v;
}
// sum over a workgroup of THREADS threads; `red` = THREADS / 64 floats of LDS.  The wave partials are added in wave order by every thread:
// the order is part of the result (csrc/segm.hip and csrc/optim.hip pair their four partials instead and keep their own)
template <int THREADS>
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < THREADS / 64; ++i) t += red[i];
    return t;
}

// ---- compile-time unrolling ------------------------------------------------------
template <int N, typename F>
__device__ __forceinline__ void unrolled(F&& f) {      // f(integral_constant<int, 0>) .. f(integral_constant<int, N - 1>): indices stay compile-time
    if constexpr (N > 0) {
        unrolled<N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
}

// ---- LDS transposed reads and MFMA fragments ---------------------------------------
// two ds_read_b64_tr_b16 = one bf16 MFMA operand of a k-major LDS tile
__device__ __forceinline__ bf16x8_t tr_pair(const bf16_t* lo_ptr, const bf16_t* hi_ptr) {
    const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)lo_ptr);
    const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)hi_ptr);
    return __builtin_bit_cast(bf16x8_t, (s16x8_t)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}
__device__ __forceinline__ bf16x8_t frag_of(unsigned a, unsigned b, unsigned c, unsigned d) {
    const u32x4_t u = {a, b, c, d};
    return __builtin_bit_cast(bf16x8_t, u);
}

// ---- elementwise dropout hash ----------------------------------------------------
// counter-based RNG for dropout: one 32-bit hash per (seed, element index).
// Forward and backward regenerate the same keep-mask from (seed, index).
__device__ __forceinline__ unsigned hash_u32(unsigned long long seed, unsigned long long idx) {
    // two-round 32-bit mixer (multiply / xor-shift, full avalanche) over the element index, keyed by the 64-bit seed.  The previous
    // splitmix64 finaliser cost ~25 VALU operations per element in 64-bit multiplies -- visible in every kernel that drops out.
    unsigned x = (unsigned)idx ^ (unsigned)seed;
    // the seed enters twice (xor before round 1, a multiplied copy before round 2): masks of different seeds are not index-shifted copies
    const unsigned key = ((unsigned)(seed >> 32) ^ ((unsigned)seed * 0x9E3779B9u)) + (unsigned)(idx >> 32) * 0x85EBCA6Bu;
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= key;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
// keep with probability 1-p ; thresh = (unsigned)(p * 2^32)
__device__ __forceinline__ bool dropout_keep(unsigned long long seed, unsigned long long idx, unsigned thresh) {
    return hash_u32(seed, idx) >= thresh;
}

// ---- attention: softmax constant and dropout hash ------------------------------------
constexpr float LOG2E = 1.4426950408889634f;    // the cores form exp2((s - m) * scale * log2(e))

// The ONE definition the attention forward (csrc/attn2.hip), the key-owning backward (csrc/attn2_bwd_body.h) and the XCD-resident decoder
// (csrc/xdec.hip) draw their keep mask from: the backward regenerates the forward's mask, so both must hash alike.
// One 32-bit hash decides two adjacent keys of a score row: element (row, key) -> pair (row * ld + key) >> 1, field key & 1 (bits 0-15 /
// 16-31), kept when field >= round(p * 65536).  Two multiply rounds on the full-rate 24-bit multiplier (v_mad_u32_u24; a 32-bit
// v_mul_lo_u32 occupies the vector pipe four times as long); keep rate, field / neighbour / stride correlations measured in
// tools/r4/hash_quality.py.
__device__ __forceinline__ unsigned pair_hash(unsigned pair, unsigned s0, unsigned s1) {
    unsigned a = pair ^ s0;
    a ^= a >> 12;               // the 24-bit multiply below only sees bits 0-23: fold the upper bits in first (pairs 2^24 apart otherwise share 99.9 % of their masks)
    unsigned h = __umul24(a, 0x9E3779u) + s1;
    h ^= h >> 15;
    h = __umul24(h, 0x85EBCBu) + (a >> 8);
    h ^= h >> 13;
    return h;
}

}  // namespace toist
