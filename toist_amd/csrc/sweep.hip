// Task-sweep assembly: the P cross-modal sequences of a sweep of T captions over B images in ONE launch (replaces the three torch.cat of
// Transformer.encode_native, reference models/transformer.py:143-148, for a batch whose rows are (image, caption) PAIRS).  Pair p takes its image rows
// from image pair_image[p] and its caption rows from caption pair_caption[p]; both tables live on the device, so one captured launch serves any pairing.
//     tokens [P, S, D] bf16 : rows 0 .. HW-1 = img_tok[i], rows HW .. S-1 = txt_tok[t]          (S = HW + L)
//     pos    [P, S, D] bf16 : rows 0 .. HW-1 = img_pos[i], rows HW .. S-1 = 0
//     key_pad [P, S] bytes  : img_pad[i] | txt_pad[t]
// A pure copy: every output byte is written (no memset before the launch), every element is bit-equal to its source.  A table entry outside [0, B) /
// [0, T) is never used as an index: that pair becomes zeros (key_pad 0 as well) and p + 1 goes into *status with atomicMax -- a captured launch reads
// tables the host rewrote after the capture, so the guard sits on the device.
// Half a wave owns one row: 32 lanes x 16 bytes = the 512 bytes of a d_model = 256 row in one access each way; the rows go round the grid in a stride
// loop.  Traffic: 2 * P*S*D*2 bytes out, P*HW*D*2*2 + P*L*D*2 in (L2 serves the repeats of an image): ~48 MB + ~46 MB at B = 8, T = 14, 640 x 640.
#include "common.h"

namespace toist {

static constexpr int SW_THREADS = 256;
static constexpr int SW_LANES = 32;                         // lanes of one row
static constexpr int SW_ROWS = SW_THREADS / SW_LANES;       // rows of one workgroup pass
static constexpr int SW_MAX_BLOCKS = 1024;                  // 4 workgroups per CU of 256

__global__ __launch_bounds__(SW_THREADS) void sweep_assemble_kernel(const uint4* __restrict__ img_tok, const uint4* __restrict__ img_pos,
                                                                     const uint8_t* __restrict__ img_pad, int B, int HW,
                                                                     const uint4* __restrict__ txt_tok, const uint8_t* __restrict__ txt_pad, int T, int L,
                                                                     const int32_t* __restrict__ pair_image, const int32_t* __restrict__ pair_caption,
                                                                     int rows, int V, uint4* __restrict__ tokens, uint4* __restrict__ pos,
                                                                     uint8_t* __restrict__ key_pad, int32_t* __restrict__ status) {
    const int S = HW + L;
    const int lane = threadIdx.x & (SW_LANES - 1);
    for (long long r = (long long)blockIdx.x * SW_ROWS + (threadIdx.x / SW_LANES); r < rows; r += (long long)gridDim.x * SW_ROWS) {
        const int p = (int)r / S, s = (int)r - p * S;                 // r < rows < 2^31 (the stride alone may step past it)
        const int i = pair_image[p], t = pair_caption[p];
        const bool ok = (unsigned)i < (unsigned)B && (unsigned)t < (unsigned)T;
        const bool image_row = s < HW;
        // (computed only from checked indices)
        const size_t src_row = !ok ? 0 : image_row ? (size_t)i * HW + s : (size_t)t * L + (s - HW);
        const uint4* tok_src = (image_row ? img_tok : txt_tok) + src_row * V;
        const uint4* pos_src = img_pos + (image_row ? src_row : 0) * V;
        uint4* tok_dst = tokens + (size_t)r * V;
        uint4* pos_dst = pos + (size_t)r * V;
        for (int c = lane; c < V; c += SW_LANES) {
            uint4 tv = make_uint4(0u, 0u, 0u, 0u), pv = make_uint4(0u, 0u, 0u, 0u);
            if (ok) {
                tv = tok_src[c];
                if (image_row) pv = pos_src[c];
            }
            tok_dst[c] = tv;
            pos_dst[c] = pv;
        }
        if (lane == 0) {
            key_pad[r] = !ok ? (uint8_t)0 : image_row ? img_pad[src_row] : txt_pad[src_row];
            if (!ok && s == 0) atomicMax(status, p + 1);
        }
    }
}

// The gradient of the assembly with respect to its token inputs (the shared-image training step, MDETR.encode_pairs): an image's tokens receive the
// sum of the image rows of its pairs, a caption's tokens the sum of the caption rows of its pairs.
//     d_img[i, s, :] = bf16( sum over p ascending, pair_image[p]   == i, of float(d_seq[p, s,      :]) )
//     d_txt[t, l, :] = bf16( sum over p ascending, pair_caption[p] == t, of float(d_seq[p, HW + l, :]) )
// A gather, not a scatter: half a wave owns one OUTPUT row (the B*HW image rows first, the T*L caption rows behind them) and finds the row's pairs
// by scanning the two pair tables, which the host may have rewritten since a capture -- there is no inverse table to keep in step.  The scan is
// uniform over the lanes of a row and reads 8 bytes per pair from the L1 (P is 8 .. 16 in a training step; any P is correct, nothing is staged on
// chip).  One fp32 accumulator per element, pairs added in ascending order, one rounding at the end: no atomics, one defined value.  Every output
// element is written (an image or caption without a pair gets zeros; no memset before the launch).  A pair with a table entry outside [0, B) /
// [0, T) is never used as an index and adds to neither output (the forward zeroed its sequence and raised the status word).
__global__ __launch_bounds__(SW_THREADS) void sweep_assemble_bwd_kernel(const uint4* __restrict__ d_seq, int B, int HW, int T, int L,
                                                                         const int32_t* __restrict__ pair_image,
                                                                         const int32_t* __restrict__ pair_caption, int P, int V, long long img_rows,
                                                                         long long rows, uint4* __restrict__ d_img, uint4* __restrict__ d_txt) {
    const int S = HW + L;
    const int lane = threadIdx.x & (SW_LANES - 1);
    for (long long r = (long long)blockIdx.x * SW_ROWS + (threadIdx.x / SW_LANES); r < rows; r += (long long)gridDim.x * SW_ROWS) {
        const bool image_row = r < img_rows;
        const int q = (int)(image_row ? r : r - img_rows);            // the row inside its output: q < B*HW or q < T*L, both below 2^31
        const int per = image_row ? HW : L;
        const int owner = q / per, s = q - owner * per;               // image i (or caption t) and the token row inside it
        const size_t seq_row = image_row ? s : HW + s;
        uint4* dst = (image_row ? d_img : d_txt) + (size_t)q * V;
        for (int c = lane; c < V; c += SW_LANES) {
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int p = 0; p < P; ++p) {
                const int i = pair_image[p], t = pair_caption[p];
                if ((unsigned)i >= (unsigned)B || (unsigned)t >= (unsigned)T || (image_row ? i : t) != owner) continue;
                const uint4 g = d_seq[((size_t)p * S + seq_row) * V + c];
                acc[0] += __uint_as_float(g.x << 16);
                acc[1] += __uint_as_float(g.x & 0xFFFF0000u);
                acc[2] += __uint_as_float(g.y << 16);
                acc[3] += __uint_as_float(g.y & 0xFFFF0000u);
                acc[4] += __uint_as_float(g.z << 16);
                acc[5] += __uint_as_float(g.z & 0xFFFF0000u);
                acc[6] += __uint_as_float(g.w << 16);
                acc[7] += __uint_as_float(g.w & 0xFFFF0000u);
            }
            dst[c] = make_uint4(pack2bf(acc[0], acc[1]), pack2bf(acc[2], acc[3]), pack2bf(acc[4], acc[5]), pack2bf(acc[6], acc[7]));
        }
    }
}

// Row gather by a pair table: dst[p, :] = src[pair_image[p], :] for rows of `words` elements of WORD (16, 4 or 1 bytes: the launcher takes the widest
// that divides the row's byte count and both base addresses, so any row size and alignment is served).  One element per thread and trip, the
// elements go round the grid in a stride loop; the table entry of a row comes out of the L1.  A pure copy: every output element is written, a pair
// whose entry is outside [0, n_images) is never used as an index, becomes zeros and puts p + 1 into *status (atomicMax), as in the assembly above.
template <typename WORD>
__global__ __launch_bounds__(SW_THREADS) void sweep_gather_kernel(const WORD* __restrict__ src, const int32_t* __restrict__ pair_image, int n_images,
                                                                   long long words, long long total, WORD* __restrict__ dst,
                                                                   int32_t* __restrict__ status) {
    for (long long e = (long long)blockIdx.x * SW_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * SW_THREADS) {
        const long long p = e / words, c = e - p * words;
        const int i = pair_image[p];
        WORD v{};
        if ((unsigned)i < (unsigned)n_images) v = src[(size_t)i * words + c];          // (computed only from a checked index)
        else if (c == 0) atomicMax(status, (int)p + 1);
        dst[e] = v;
    }
}

}  // namespace toist

using namespace toist;

extern "C" int toist_sweep_gather(const void* src, const int32_t* pair_image, int n_images, int P, long long row_bytes, void* dst, int32_t* status,
                                  void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    TOIST_REQUIRE(n_images > 0 && P >= 0 && row_bytes > 0, "toist_sweep_gather: bad extents n_images=%d P=%d row_bytes=%lld", n_images, P, row_bytes);
    TOIST_REQUIRE(row_bytes < (1ll << 40) && (long long)n_images * row_bytes < (1ll << 46), "toist_sweep_gather: rows of %lld bytes are too long", row_bytes);
    if (P == 0) return TOIST_OK;
    TOIST_REQUIRE(src && pair_image && dst && status, "toist_sweep_gather: null pointer");
    const uintptr_t low = (uintptr_t)src | (uintptr_t)dst | (uintptr_t)row_bytes;
    const int wb = (low & 15) == 0 ? 16 : (low & 3) == 0 ? 4 : 1;
    const long long words = row_bytes / wb, total = words * P;
    const long long want = (total + SW_THREADS - 1) / SW_THREADS;
    const dim3 grid((unsigned)(want < SW_MAX_BLOCKS ? want : SW_MAX_BLOCKS));
    if (wb == 16)
        hipLaunchKernelGGL(sweep_gather_kernel<uint4>, grid, dim3(SW_THREADS), 0, stream, (const uint4*)src, pair_image, n_images, words, total, (uint4*)dst, status);
    else if (wb == 4)
        hipLaunchKernelGGL(sweep_gather_kernel<uint32_t>, grid, dim3(SW_THREADS), 0, stream, (const uint32_t*)src, pair_image, n_images, words, total,
                           (uint32_t*)dst, status);
    else
        hipLaunchKernelGGL(sweep_gather_kernel<uint8_t>, grid, dim3(SW_THREADS), 0, stream, (const uint8_t*)src, pair_image, n_images, words, total,
                           (uint8_t*)dst, status);
    return check_launch("toist_sweep_gather");
}

extern "C" int toist_sweep_assemble(const void* img_tok, const void* img_pos, const uint8_t* img_pad, int B, int HW, const void* txt_tok,
                                    const uint8_t* txt_pad, int T, int L, const int32_t* pair_image, const int32_t* pair_caption, int P, int D,
                                    void* tokens, void* pos, uint8_t* key_pad, int32_t* status, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    TOIST_REQUIRE(B > 0 && HW > 0 && T > 0 && L > 0 && P >= 0 && D > 0, "toist_sweep_assemble: bad extents B=%d HW=%d T=%d L=%d P=%d D=%d", B, HW, T, L, P, D);
    TOIST_REQUIRE(D % 8 == 0, "toist_sweep_assemble: D=%d is not a multiple of 8 (rows move as 16-byte accesses)", D);
    const long long S = (long long)HW + L, rows = (long long)P * S;
    TOIST_REQUIRE(S < (1ll << 31) && rows < (1ll << 31) && (long long)B * HW < (1ll << 31) && (long long)T * L < (1ll << 31),
                  "toist_sweep_assemble: P*(HW+L), B*HW and T*L must stay below 2^31 (P=%d HW=%d L=%d B=%d T=%d)", P, HW, L, B, T);
    if (P == 0) return TOIST_OK;
    TOIST_REQUIRE(img_tok && img_pos && img_pad && txt_tok && txt_pad && pair_image && pair_caption && tokens && pos && key_pad && status,
                  "toist_sweep_assemble: null pointer");
    TOIST_REQUIRE((((uintptr_t)img_tok | (uintptr_t)img_pos | (uintptr_t)txt_tok | (uintptr_t)tokens | (uintptr_t)pos) & 15) == 0,
                  "toist_sweep_assemble: the bf16 arrays must be 16-byte aligned");
    const long long want = (rows + SW_ROWS - 1) / SW_ROWS;
    const dim3 grid((unsigned)(want < SW_MAX_BLOCKS ? want : SW_MAX_BLOCKS));
    hipLaunchKernelGGL(sweep_assemble_kernel, grid, dim3(SW_THREADS), 0, stream, (const uint4*)img_tok, (const uint4*)img_pos, img_pad, B, HW,
                       (const uint4*)txt_tok, txt_pad, T, L, pair_image, pair_caption, (int)rows, D / 8, (uint4*)tokens, (uint4*)pos, key_pad, status);
    return check_launch("toist_sweep_assemble");
}

extern "C" int toist_sweep_assemble_bwd(const void* d_seq, const int32_t* pair_image, const int32_t* pair_caption, int P, int B, int HW, int T, int L,
                                        int D, void* d_img, void* d_txt, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    TOIST_REQUIRE(B > 0 && HW > 0 && T > 0 && L > 0 && P >= 0 && D > 0, "toist_sweep_assemble_bwd: bad extents B=%d HW=%d T=%d L=%d P=%d D=%d", B, HW, T, L, P,
                  D);
    TOIST_REQUIRE(D % 8 == 0, "toist_sweep_assemble_bwd: D=%d is not a multiple of 8 (rows move as 16-byte accesses)", D);
    const long long S = (long long)HW + L;
    TOIST_REQUIRE(S < (1ll << 31) && (long long)P * S < (1ll << 31) && (long long)B * HW < (1ll << 31) && (long long)T * L < (1ll << 31),
                  "toist_sweep_assemble_bwd: P*(HW+L), B*HW and T*L must stay below 2^31 (P=%d HW=%d L=%d B=%d T=%d)", P, HW, L, B, T);
    if (!d_img && !d_txt) return TOIST_OK;             // both sides frozen: nothing to write
    TOIST_REQUIRE(P == 0 || (d_seq && pair_image && pair_caption), "toist_sweep_assemble_bwd: null pointer");
    TOIST_REQUIRE((((uintptr_t)d_seq | (uintptr_t)d_img | (uintptr_t)d_txt) & 15) == 0, "toist_sweep_assemble_bwd: the bf16 arrays must be 16-byte aligned");
    const long long img_rows = d_img ? (long long)B * HW : 0, rows = img_rows + (d_txt ? (long long)T * L : 0);
    const long long want = (rows + SW_ROWS - 1) / SW_ROWS;
    const dim3 grid((unsigned)(want < SW_MAX_BLOCKS ? want : SW_MAX_BLOCKS));
    hipLaunchKernelGGL(sweep_assemble_bwd_kernel, grid, dim3(SW_THREADS), 0, stream, (const uint4*)d_seq, B, HW, T, L, pair_image, pair_caption, P, D / 8,
                       img_rows, rows, (uint4*)d_img, (uint4*)d_txt);
    return check_launch("toist_sweep_assemble_bwd");
}
