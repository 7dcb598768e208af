// Device-side target masks: what the reference does on the host to a target's masks (datasets/transforms.py: hflip 62-80 flip(-1), resize 118-138
// F.interpolate(mode="nearest"), crop 18-59 slicing; util/misc.py:185-209 the zero padding of NestedTensor.from_tensor_list) as ONE launch per batch
// whose every size comes from a device table.
//
// A nearest resize is an index map, and so are flip and crop: the host composes the whole plan of an image into one table of source rows and one of
// source columns (toist_amd/preprocess.py: mask_index_tables).  The source masks travel at the ORIGINAL size with one bit per pixel; the kernel is
// a gather from those bits into the bytes (0 / 1) that the mask-loss kernels read, so its bytes EQUAL the host pipeline's.
//
// A 256-thread workgroup owns a TM_H x TM_W tile of one slot's capacity.  It loads the tile's slice of the column table coalesced (one entry per
// thread) and of the row table into LDS, entries outside the source already marked; a thread then owns 16 adjacent bytes of TM_H / 16 rows and
// stores each as one 16-byte vector (4-byte vectors or single bytes where the row's address or the row's end do not allow it: any cap_w works).
// The source words come through the cache -- a source mask is a few tens of KB.  Up to a 2x reduction a thread's 16 columns lie in two adjacent words
// of a source row: it loads those for all its rows up front; otherwise it reloads a word whenever the column leaves it.
#include "common.h"

namespace toist {

static constexpr int TM_THREADS = 256;
static constexpr int TM_W = 256, TM_H = 64;       // output tile: TM_W == TM_THREADS (one column-table entry per thread)
static constexpr int TM_VEC = 16;                 // adjacent output bytes per thread and row
static constexpr int TM_ROWS = TM_H / (TM_THREADS / (TM_W / TM_VEC));        // output rows per thread
static_assert(TM_W == TM_THREADS && TM_H <= TM_THREADS && TM_ROWS * (TM_THREADS / (TM_W / TM_VEC)) == TM_H, "tile shape");

struct TmaskRow {        // one slot: TOIST_TMASK_DESC_WORDS int32 (include/toist_hip.h)
    int src_off, src_h, src_w, src_stride_words, out_h, out_w, tab_y, tab_x;
};
static_assert(sizeof(TmaskRow) == TOIST_TMASK_DESC_WORDS * 4, "descriptor layout");

// Everything a workgroup reads from a descriptor row is checked against the capacities here, on the device: a row that does not fit is an all-zero
// slot, never an out-of-bounds access.  The table ENTRIES are checked where they are read.  The host checks the same before it launches.
__device__ __forceinline__ bool tmask_row_ok(const TmaskRow& d, long long src_bytes, long long arena_words, int cap_h, int cap_w) {
    if (d.out_h <= 0 || d.out_w <= 0 || d.out_h > cap_h || d.out_w > cap_w) return false;
    if (d.src_h <= 0 || d.src_w <= 0 || d.src_off < 0 || (d.src_off & 3) != 0) return false;
    if ((long long)d.src_stride_words * 32 < (long long)d.src_w) return false;
    if ((long long)d.src_off + (long long)d.src_h * d.src_stride_words * 4 > src_bytes) return false;
    if (d.tab_y < 0 || d.tab_x < 0) return false;
    if ((long long)d.tab_y + d.out_h > arena_words || (long long)d.tab_x + d.out_w > arena_words) return false;
    return true;
}

// grid: (ceil(cap_w / TM_W), ceil(cap_h / TM_H), slots)
__global__ __launch_bounds__(TM_THREADS) void target_masks_kernel(const uint8_t* __restrict__ src, long long src_bytes, const int32_t* __restrict__ desc,
                                                                   const int32_t* __restrict__ arena, long long arena_words, int cap_h, int cap_w,
                                                                   uint8_t* __restrict__ dst) {
    __shared__ __attribute__((aligned(16))) int s_x[TM_W];        // source column of every column of the tile; -1 = reads as 0
    __shared__ int s_y[TM_H];                                     // source row of every row of the tile; -1 = reads as 0
    const int slot = blockIdx.z, tx0 = blockIdx.x * TM_W, ty0 = blockIdx.y * TM_H, tid = threadIdx.x;
    const TmaskRow d = *reinterpret_cast<const TmaskRow*>(desc + (size_t)slot * TOIST_TMASK_DESC_WORDS);
    if (d.out_h == 0) return;                                                                 // a dead slot: nothing is written
    const bool ok = tmask_row_ok(d, src_bytes, arena_words, cap_h, cap_w);                    // uniform over the workgroup
    const bool live = ok && tx0 < d.out_w && ty0 < d.out_h;                                   // the tile holds pixels of the mask
    if (live) {
        int sx = -1;
        if (tx0 + tid < d.out_w) {
            sx = arena[(size_t)d.tab_x + tx0 + tid];
            if (sx < 0 || sx >= d.src_w) sx = -1;
        }
        s_x[tid] = sx;
        if (tid < TM_H) {
            int sy = -1;
            if (ty0 + tid < d.out_h) {
                sy = arena[(size_t)d.tab_y + ty0 + tid];
                if (sy < 0 || sy >= d.src_h) sy = -1;
            }
            s_y[tid] = sy;
        }
    }
    __syncthreads();

    const int q = tid % (TM_W / TM_VEC), r0 = tid / (TM_W / TM_VEC);        // the thread's 16-byte column group and its first row inside the tile
    const int x0 = tx0 + q * TM_VEC;
    if (x0 >= cap_w) return;
    const int n = min(TM_VEC, cap_w - x0);                                  // bytes of the group inside the row
    int sxs[TM_VEC];
#pragma unroll
    for (int e = 0; e < TM_VEC; ++e) sxs[e] = -1;
    if (live) {
#pragma unroll
        for (int e = 0; e < TM_VEC; ++e) sxs[e] = s_x[q * TM_VEC + e];
    }
    // the usual case -- no reduction beyond 2x: the 16 columns read at most two adjacent words of a source row.  Then the rows' words are loaded up front,
    // independent of each other (w0 = the lower word of the pair); any other spread of columns reloads a word per change.
    int w0 = 0x7fffffff, w1 = -1;
#pragma unroll
    for (int e = 0; e < TM_VEC; ++e)
        if (sxs[e] >= 0) {
            w0 = min(w0, sxs[e] >> 5);
            w1 = max(w1, sxs[e] >> 5);
        }
    const bool any = w1 >= 0, pair = any && w1 - w0 <= 1;
    const bool hi_in = pair && w0 + 1 < d.src_stride_words;                 // the upper word lies inside the row
    const uint32_t* words = reinterpret_cast<const uint32_t*>(src + (live ? d.src_off : 0));
    uint8_t* slot_base = dst + (size_t)slot * (size_t)cap_h * (size_t)cap_w;
    // the pair path without a branch per column: each column's bit position inside its word, whether that word is the upper one, and the bytes of
    // the group that hold a pixel at all
    int bit[TM_VEC];
    bool upper[TM_VEC];
    uint32_t holds[TM_VEC / 4];
#pragma unroll
    for (int k = 0; k < TM_VEC / 4; ++k) holds[k] = 0u;
#pragma unroll
    for (int e = 0; e < TM_VEC; ++e) {
        const bool in = pair && sxs[e] >= 0;
        bit[e] = in ? (sxs[e] & 31) : 0;
        upper[e] = in && (sxs[e] >> 5) != w0;
        holds[e >> 2] |= (in ? 1u : 0u) << (8 * (e & 3));
    }
    int sys[TM_ROWS];
    uint32_t lo[TM_ROWS], hi[TM_ROWS];
#pragma unroll
    for (int r = 0; r < TM_ROWS; ++r) {
        const int yl = r0 + (TM_H / TM_ROWS) * r;
        sys[r] = (live && any && ty0 + yl < cap_h) ? s_y[yl] : -1;
        lo[r] = hi[r] = 0u;
        if (pair && sys[r] >= 0) {
            const uint32_t* row = words + (size_t)sys[r] * d.src_stride_words;
            lo[r] = row[w0];
            hi[r] = hi_in ? row[w0 + 1] : 0u;
        }
    }
#pragma unroll
    for (int r = 0; r < TM_ROWS; ++r) {
        const int yl = r0 + (TM_H / TM_ROWS) * r, y = ty0 + yl;
        if (y >= cap_h) continue;
        uint32_t v[TM_VEC / 4];
#pragma unroll
        for (int k = 0; k < TM_VEC / 4; ++k) v[k] = 0u;
        if (pair) {
#pragma unroll
            for (int e = 0; e < TM_VEC; ++e) v[e >> 2] |= (((upper[e] ? hi[r] : lo[r]) >> bit[e]) & 1u) << (8 * (e & 3));
#pragma unroll
            for (int k = 0; k < TM_VEC / 4; ++k) v[k] &= holds[k];
        } else if (sys[r] >= 0) {
            const uint32_t* row = words + (size_t)sys[r] * d.src_stride_words;
            int at = -1;
            uint32_t w = 0u;
#pragma unroll
            for (int e = 0; e < TM_VEC; ++e) {
                const int sx = sxs[e];
                if (sx >= 0) {
                    if ((sx >> 5) != at) {
                        at = sx >> 5;
                        w = row[at];
                    }
                    v[e >> 2] |= ((w >> (sx & 31)) & 1u) << (8 * (e & 3));
                }
            }
        }
        uint8_t* p = slot_base + (size_t)y * cap_w + x0;
        if (n == TM_VEC && ((size_t)p & 15) == 0) {
            u32x4_t o = {v[0], v[1], v[2], v[3]};
            *reinterpret_cast<u32x4_t*>(p) = o;
        } else {
#pragma unroll
            for (int k = 0; k < TM_VEC / 4; ++k) {
                if (4 * k + 4 <= n && ((size_t)(p + 4 * k) & 3) == 0) {
                    *reinterpret_cast<uint32_t*>(p + 4 * k) = v[k];
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (4 * k + b < n) p[4 * k + b] = (uint8_t)((v[k] >> (8 * b)) & 255u);
                }
            }
        }
    }
}

}  // namespace toist

using namespace toist;

extern "C" int toist_target_masks(const uint8_t* src, long long src_bytes, const int32_t* desc, const int32_t* arena, long long arena_words, int slots,
                                  int cap_h, int cap_w, uint8_t* dst, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    TOIST_REQUIRE(slots >= 0 && slots <= 65535, "toist_target_masks: bad slot count %d", slots);
    if (slots == 0) return TOIST_OK;
    TOIST_REQUIRE(src && desc && arena && dst, "toist_target_masks: null source, descriptor table, table arena or output");
    TOIST_REQUIRE(cap_h > 0 && cap_w > 0 && (cap_h + TM_H - 1) / TM_H <= 65535, "toist_target_masks: bad capacity %d x %d", cap_h, cap_w);
    TOIST_REQUIRE(src_bytes > 0 && arena_words > 0, "toist_target_masks: empty source or table arena");
    TOIST_REQUIRE((((size_t)desc | (size_t)arena | (size_t)src) & 3) == 0,
                  "toist_target_masks: the descriptor table, the arena and the packed source hold 32-bit words (4-byte aligned)");
    const dim3 grid((cap_w + TM_W - 1) / TM_W, (cap_h + TM_H - 1) / TM_H, slots);
    hipLaunchKernelGGL(target_masks_kernel, grid, dim3(TM_THREADS), 0, stream, src, src_bytes, desc, arena, arena_words, cap_h, cap_w, dst);
    return check_launch("toist_target_masks");
}
