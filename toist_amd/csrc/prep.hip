// Device-side image preparation: what the reference does on the host between the decoded uint8 image and the model's input
// (datasets/transforms.py: hflip / crop / resize = Pillow's Image.resize(BILINEAR), ToTensor, Normalize; util/misc.py:185-209:
// NestedTensor.from_tensor_list's padding and mask) as ONE launch per batch whose every size comes from a device table.
//
// Pillow's 8-bit resampler is integer arithmetic on coefficients computed in double precision: the host builds, per axis, the bounds
// (first tap, tap count) and the int32 coefficients (22 fractional bits) of every output index; a pass is
//     out = clip((2^21 + sum_j pixel[lo + j] * k_j) >> 22, 0, 255)        stored as uint8
// horizontal first, its uint8 result the vertical pass's input.  The kernel does that integer work only, so its pixels EQUAL Pillow's.
//
// A 256-thread workgroup owns a PT_H x PT_W tile of output pixels of one image.  It resamples the source rows the tile needs
// horizontally into LDS (uint8, interleaved RGB), at most PT_CHUNK rows at a time, and accumulates the vertical pass out of LDS in
// int32 registers across the chunks (integer sums: the split changes nothing); the horizontally resampled image never goes to HBM.
// A thread owns 4 consecutive x of PT_H / 16 rows: 3 dwords of LDS per tap, one 16-byte store per plane in the final mode.
//   final mode        : fp32 planar [B, 3, Hp, Wp] through a 3 x 256 table of (v / 255 - mean) / std that the host fills with torch, and
//                       the bool mask [B, Hp, Wp]; the whole capacity is written (zeros / True outside the image): no memset precedes it
//   intermediate mode : uint8 HWC at a per-image offset (the image between the two resizes of the reference's second training branch)
#include "common.h"

namespace toist {

static constexpr int PT_THREADS = 256;
static constexpr int PT_W = 64, PT_H = 32;        // output tile
static constexpr int PT_ROWS = PT_H / 16;         // output rows per thread
static constexpr int PT_CHUNK = 64;               // horizontally resampled source rows held in LDS at a time (64 x 192 B = 12 KiB)
static constexpr int PT_ROWB = PT_W * 3;          // bytes of one LDS row

struct PrepRow {        // one image: TOIST_PREP_DESC_WORDS int32 (include/toist_hip.h)
    int src_off, src_h, src_w, src_stride, flip, crop_y, crop_x, crop_h, crop_w, out_h, out_w, ksize_h, ksize_v, bounds_h, coef_h, bounds_v, coef_v,
        dst_off, reserved0, reserved1;
};
static_assert(sizeof(PrepRow) == TOIST_PREP_DESC_WORDS * 4, "descriptor layout");

// Everything a workgroup reads from a descriptor row is checked against the capacities here, on the device: a row that does not fit is an
// EMPTY image (padding only / nothing written), never an out-of-bounds access.  The host checks the same before it launches.
__device__ __forceinline__ bool prep_row_ok(const PrepRow& d, long long src_bytes, long long arena_words, int cap_h, int cap_w, bool inter,
                                            long long dst_bytes) {
    if (d.out_h <= 0 || d.out_w <= 0 || d.out_h > cap_h || d.out_w > cap_w) return false;
    if (d.src_h <= 0 || d.src_w <= 0 || d.src_off < 0 || d.src_stride < d.src_w * 3) return false;
    if ((long long)d.src_off + (long long)(d.src_h - 1) * d.src_stride + (long long)d.src_w * 3 > src_bytes) return false;
    if (d.crop_x < 0 || d.crop_y < 0 || d.crop_w <= 0 || d.crop_h <= 0 || (long long)d.crop_x + d.crop_w > d.src_w ||
        (long long)d.crop_y + d.crop_h > d.src_h)
        return false;
    if (d.ksize_h <= 0 || d.ksize_v <= 0 || d.bounds_h < 0 || d.coef_h < 0 || d.bounds_v < 0 || d.coef_v < 0) return false;
    if ((long long)d.bounds_h + 2ll * d.out_w > arena_words || (long long)d.coef_h + (long long)d.out_w * d.ksize_h > arena_words) return false;
    if ((long long)d.bounds_v + 2ll * d.out_h > arena_words || (long long)d.coef_v + (long long)d.out_h * d.ksize_v > arena_words) return false;
    if (inter && (d.dst_off < 0 || (long long)d.dst_off + (long long)d.out_h * d.out_w * 3 > dst_bytes)) return false;
    return true;
}

// (first tap, tap count) of output index i, clamped to the input extent and to ksize: a bad table cannot index outside the image
__device__ __forceinline__ void prep_bounds(const int32_t* __restrict__ bounds, int i, int extent, int ksize, int& lo, int& n) {
    lo = bounds[2 * i];
    n = bounds[2 * i + 1];
    lo = lo < 0 ? 0 : (lo > extent ? extent : lo);
    n = n > ksize ? ksize : n;
    n = n > extent - lo ? extent - lo : n;
    n = n < 0 ? 0 : n;
}

__device__ __forceinline__ int prep_clip8(int acc) {
    const int v = acc >> 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// grid: (ceil(cap_w / PT_W), ceil(cap_h / PT_H), batch capacity)
__global__ __launch_bounds__(PT_THREADS) void image_prep_kernel(const uint8_t* __restrict__ src, long long src_bytes, const int32_t* __restrict__ desc,
                                                                 const int32_t* __restrict__ arena, long long arena_words,
                                                                 const float* __restrict__ lut, int cap_h, int cap_w, float* __restrict__ out,
                                                                 uint8_t* __restrict__ mask, uint8_t* dst_u8, long long dst_bytes) {
    __shared__ __attribute__((aligned(16))) uint8_t hbuf[PT_CHUNK * PT_ROWB];
    __shared__ float s_lut[3 * 256];
    const bool inter = dst_u8 != nullptr;
    const int img = blockIdx.z, tx0 = blockIdx.x * PT_W, ty0 = blockIdx.y * PT_H, tid = threadIdx.x;
    const PrepRow d = *reinterpret_cast<const PrepRow*>(desc + (size_t)img * TOIST_PREP_DESC_WORDS);
    const bool ok = prep_row_ok(d, src_bytes, arena_words, cap_h, cap_w, inter, dst_bytes);       // uniform over the workgroup
    const bool live = ok && tx0 < d.out_w && ty0 < d.out_h;                                     // the tile holds pixels of the image
    if (inter && !live) return;

    const int q = tid & 15, r0 = tid >> 4;        // the thread's x quad and its first row inside the tile
    const int x0 = tx0 + q * 4;
    int acc[PT_ROWS][12];
#pragma unroll
    for (int r = 0; r < PT_ROWS; ++r)
#pragma unroll
        for (int e = 0; e < 12; ++e) acc[r][e] = 1 << 21;

    if (live) {
        if (!inter)
            for (int i = tid; i < 3 * 256; i += PT_THREADS) s_lut[i] = lut[i];
        const int32_t *bh = arena + d.bounds_h, *ch = arena + d.coef_h, *bv = arena + d.bounds_v, *cv = arena + d.coef_v;
        const int ty_last = min(ty0 + PT_H, d.out_h) - 1;
        int ylo, yhi, n_;
        prep_bounds(bv, ty0, d.crop_h, d.ksize_v, ylo, n_);
        prep_bounds(bv, ty_last, d.crop_h, d.ksize_v, yhi, n_);
        yhi += n_;
        // the thread's own rows of the vertical pass
        int vlo[PT_ROWS], vn[PT_ROWS];
#pragma unroll
        for (int r = 0; r < PT_ROWS; ++r) {
            const int y = ty0 + r0 + 16 * r;
            vlo[r] = 0;
            vn[r] = 0;
            if (y < d.out_h) prep_bounds(bv, y, d.crop_h, d.ksize_v, vlo[r], vn[r]);
        }
        const uint8_t* base = src + d.src_off;
        const int tw = min(PT_W, d.out_w - tx0);
        // the thread's own column of the horizontal pass
        const int xl = tid % PT_W;
        int hlo = 0, hn = 0;
        if (xl < tw) prep_bounds(bh, tx0 + xl, d.crop_w, d.ksize_h, hlo, hn);
        const int32_t* hk = ch + (size_t)(tx0 + xl) * d.ksize_h;
        __syncthreads();        // the normalisation table is in LDS
        for (int c0 = ylo; c0 < yhi; c0 += PT_CHUNK) {
            const int rows = min(PT_CHUNK, yhi - c0);
            __syncthreads();        // the previous chunk has been consumed
            // horizontal pass: source rows [c0, c0 + rows) of the (flipped, cropped) image -> LDS, one thread per (row, x), 3 channels
            for (int r = tid / PT_W; r < rows; r += PT_THREADS / PT_W) {
                int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
                if (xl < tw) {
                    const uint8_t* row = base + (size_t)(d.crop_y + c0 + r) * d.src_stride;
                    for (int j = 0; j < hn; ++j) {
                        const int xs = d.crop_x + hlo + j;
                        const uint8_t* p = row + (size_t)(d.flip ? d.src_w - 1 - xs : xs) * 3;
                        const int kj = hk[j];
                        a0 += (int)p[0] * kj;
                        a1 += (int)p[1] * kj;
                        a2 += (int)p[2] * kj;
                    }
                }
                uint8_t* h = hbuf + r * PT_ROWB + xl * 3;
                h[0] = (uint8_t)prep_clip8(a0);
                h[1] = (uint8_t)prep_clip8(a1);
                h[2] = (uint8_t)prep_clip8(a2);
            }
            __syncthreads();
            // vertical pass: the taps of this chunk
#pragma unroll
            for (int r = 0; r < PT_ROWS; ++r) {
                const int y = ty0 + r0 + 16 * r;
                const int j0 = max(0, c0 - vlo[r]), j1 = min(vn[r], c0 + rows - vlo[r]);
                const int32_t* k = cv + (size_t)y * d.ksize_v;
                for (int j = j0; j < j1; ++j) {
                    const int kj = k[j];
                    const uint32_t* h = reinterpret_cast<const uint32_t*>(hbuf + (vlo[r] + j - c0) * PT_ROWB + q * 12);
                    const uint32_t w0 = h[0], w1 = h[1], w2 = h[2];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc[r][e] += (int)((w0 >> (8 * e)) & 255u) * kj;
                        acc[r][4 + e] += (int)((w1 >> (8 * e)) & 255u) * kj;
                        acc[r][8 + e] += (int)((w2 >> (8 * e)) & 255u) * kj;
                    }
                }
            }
        }
    }

    if (inter) {
        uint8_t* dst = dst_u8 + d.dst_off;
#pragma unroll
        for (int r = 0; r < PT_ROWS; ++r) {
            const int y = ty0 + r0 + 16 * r;
            if (y >= d.out_h) continue;
#pragma unroll
            for (int e = 0; e < 12; ++e)
                if (x0 + e / 3 < d.out_w) dst[((size_t)y * d.out_w + x0 + e / 3) * 3 + e % 3] = (uint8_t)prep_clip8(acc[r][e]);
        }
        return;
    }

    // final mode: every quad of the capacity is written (cap_w % 4 == 0: a quad never straddles the row end)
    if (x0 >= cap_w) return;
    const int oh = ok ? d.out_h : 0, ow = ok ? d.out_w : 0;
#pragma unroll
    for (int r = 0; r < PT_ROWS; ++r) {
        const int y = ty0 + r0 + 16 * r;
        if (y >= cap_h) continue;
        f32x4_t v[3];
        uint32_t m = 0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const bool in = y < oh && x0 + p < ow;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][p] = in ? s_lut[c * 256 + prep_clip8(acc[r][p * 3 + c])] : 0.f;
            m |= (in ? 0u : 1u) << (8 * p);
        }
        const size_t px = (size_t)y * cap_w + x0, plane = (size_t)cap_h * cap_w;
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4_t*>(out + ((size_t)img * 3 + c) * plane + px) = v[c];
        *reinterpret_cast<uint32_t*>(mask + (size_t)img * plane + px) = m;
    }
}

}  // namespace toist

using namespace toist;

extern "C" int toist_image_prep(const uint8_t* src, long long src_bytes, const int32_t* desc, const int32_t* arena, long long arena_words, const float* lut,
                                int batch_cap, int cap_h, int cap_w, float* out, uint8_t* mask, uint8_t* dst_u8, long long dst_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    TOIST_REQUIRE(batch_cap >= 0 && batch_cap <= 65535 && cap_h > 0 && cap_w > 0 && (cap_h + PT_H - 1) / PT_H <= 65535, "toist_image_prep: bad capacity");
    if (batch_cap == 0) return TOIST_OK;
    TOIST_REQUIRE(src && desc && arena && src_bytes > 0 && arena_words > 0, "toist_image_prep: null source, descriptor table or coefficient arena");
    TOIST_REQUIRE((out != nullptr) != (dst_u8 != nullptr), "toist_image_prep: exactly one of the fp32 output (final mode) and the uint8 output (intermediate mode)");
    TOIST_REQUIRE((((size_t)desc | (size_t)arena) & 3) == 0, "toist_image_prep: the descriptor table and the arena hold int32");
    if (out) {
        TOIST_REQUIRE(mask && lut, "toist_image_prep: the final mode needs the mask and the 3 x 256 normalisation table");
        TOIST_REQUIRE((cap_w % 4) == 0 && ((size_t)out & 15) == 0 && ((size_t)mask & 3) == 0,
                      "toist_image_prep: the final mode stores 16 bytes at a time: cap_w %% 4 == 0 (got %d) and a 16-byte aligned output", cap_w);
    } else {
        TOIST_REQUIRE(dst_bytes > 0, "toist_image_prep: the intermediate mode needs the capacity of its output");
    }
    const dim3 grid((cap_w + PT_W - 1) / PT_W, (cap_h + PT_H - 1) / PT_H, batch_cap);
    hipLaunchKernelGGL(image_prep_kernel, grid, dim3(PT_THREADS), 0, stream, src, src_bytes, desc, arena, arena_words, lut, cap_h, cap_w, out, mask, dst_u8,
                       dst_bytes);
    return check_launch("toist_image_prep");
}
