// Polygon annotations rasterised on the device: maskApi.c rleFrPoly as the host restates it (toist_amd/coco_eval.py: polygon_to_mask), in the sort-free,
// edge-parallel formulation that tests/test_cpu_polygon_masks.py: parallel_polygon_mask holds against it.  ONE launch per batch whose every size comes
// from device tables (include/toist_hip.h: toist_polygon_masks).
//
// Every (edge, step d >= 1) pair is independent work: it compares point d of the edge's trace on the 5x grid with point d - 1 of THAT edge; where the
// trace enters another grid column that is the left edge of a pixel column, the crossing (bx, by) toggles one bit of a zeroed plane.  A prefix-XOR down
// each column of the plane is the polygon's mask; an object's polygons are merged by union.  Columns never mix, so a workgroup owns one (object, strip
// of PM_STRIP columns): a toggle plane and an accumulated plane of PM_ROWS x PM_STRIP bits in LDS.  It walks the object's polygons one at a time --
// each wave takes every fourth edge, its lanes the steps; crossings outside the strip are dropped -- then scans the toggle plane (rows in 128 chunks per
// word column: chunk parities, a shuffle scan over the chunks, a second pass), ORs it into the accumulated plane and clears it.
//
// The arithmetic is the host's, operation for operation, in IEEE fp64: this unit is compiled with -ffp-contract=off, because `ys + s * t + .5` rounds
// the product before the sum (tests/golden/polygon_masks.npz holds polygons whose mask changes under a fused multiply-add).
#include "common.h"

namespace toist {

static constexpr int PM_THREADS = 256;
static constexpr int PM_WAVES = PM_THREADS / 64;
static constexpr int PM_STRIP = TOIST_POLY_STRIP;              // pixel columns of a workgroup
static constexpr int PM_SW = PM_STRIP / 32;                    // 32-bit words of a plane row
static constexpr int PM_ROWS = TOIST_POLY_MAX_ROWS;            // rows of a plane: the tallest image
static constexpr int PM_CHUNKS = PM_THREADS / PM_SW;           // row chunks of the column scan, one per thread and word column
static_assert(PM_SW == 2 && PM_STRIP == 32 * PM_SW, "the scan below pairs lanes: two word columns per row");
static_assert(2 * PM_ROWS * PM_SW * 4 <= 64 * 1024, "two planes in the default LDS allocation");

struct PolyRow {        // one object slot: TOIST_POLY_DESC_WORDS int32 (include/toist_hip.h)
    int dst_off, h, w, stride_words, poly_first, poly_count, reserved0, reserved1;
};
static_assert(sizeof(PolyRow) == TOIST_POLY_DESC_WORDS * 4, "descriptor layout");

// One step of one edge: the crossing between point d - 1 and point d (in the ORIGINAL direction of the edge), toggled into the plane when its pixel
// column lies in [x0, x0 + PM_STRIP).  xs .. ye are already flipped so that the major coordinate runs upwards; t counts along it.
__device__ __forceinline__ void poly_point(bool major_x, long long xs, long long ys, double s, long long t, long long& u, long long& v) {
    if (major_x) {
        u = t + xs;
        v = (long long)((double)ys + s * (double)t + .5);          // product rounded, then the two sums: int(ys + s * t + .5)
    } else {
        u = (long long)((double)xs + s * (double)t + .5);
        v = t + ys;
    }
}

__device__ __forceinline__ void poly_step(bool major_x, bool flip, long long xs, long long ys, double s, long long length, long long d, int h, int w,
                                          int x0, uint32_t* __restrict__ tog) {
    const long long tj = flip ? length - d : d, tp = flip ? length - d + 1 : d - 1;
    long long uj, vj, up, vp;
    poly_point(major_x, xs, ys, s, tj, uj, vj);
    poly_point(major_x, xs, ys, s, tp, up, vp);
    if (uj == up) return;
    double xd = (double)(uj < up ? uj : uj - 1);
    xd = (xd + .5) / 5.0 - .5;
    if (floor(xd) != xd || xd < 0 || xd > (double)(w - 1)) return;
    const long long bx = (long long)xd;
    if (bx < x0 || bx >= x0 + PM_STRIP) return;
    double yd = (double)(vj < vp ? vj : vp);
    yd = (yd + .5) / 5.0 - .5;
    yd = fmin(fmax(yd, 0.0), (double)h);
    const long long by = (long long)ceil(yd);
    if (by >= h) return;                                            // by == h toggles nothing
    const int c = (int)(bx - x0);
    atomicXor(&tog[(int)by * PM_SW + (c >> 5)], 1u << (c & 31));
}

// grid: (ceil(cap_w / PM_STRIP), slots)
template <bool DENSE>
__global__ __launch_bounds__(PM_THREADS) void polygon_masks_kernel(const int32_t* __restrict__ desc, const int32_t* __restrict__ polys, int poly_cap,
                                                                    const int32_t* __restrict__ verts, int vert_cap, int cap_h, int cap_w,
                                                                    uint8_t* __restrict__ dst, long long dst_bytes) {
    __shared__ uint32_t s_tog[PM_ROWS * PM_SW];        // crossings of the polygon at hand
    __shared__ uint32_t s_acc[PM_ROWS * PM_SW];        // union of the object's polygons
    __shared__ uint32_t s_wave[PM_WAVES][PM_SW];
    const int slot = (int)blockIdx.y, strip = (int)blockIdx.x, x0 = strip * PM_STRIP, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PolyRow d = *reinterpret_cast<const PolyRow*>(desc + (size_t)slot * TOIST_POLY_DESC_WORDS);
    if (d.h == 0) return;                                                                      // a dead slot: nothing is written
    // everything read from the row is checked against the capacities here; a row that does not fit writes nothing (the host checks the same)
    if (d.h < 0 || d.w <= 0 || d.h > PM_ROWS || d.h > cap_h || d.w > cap_w || d.poly_first < 0 || d.poly_count < 0 ||
        (long long)d.poly_first + d.poly_count > poly_cap)
        return;
    const int h = d.h, w = d.w;
    int words;                                         // 32-bit words of an output row that this strip owns
    if (DENSE) {
        if ((long long)(slot + 1) * cap_h * cap_w > dst_bytes || x0 >= w) return;
        words = min(PM_SW, (w - x0 + 31) >> 5);
    } else {
        if (d.dst_off < 0 || (d.dst_off & 3) != 0 || (long long)d.stride_words * 32 < (long long)w || d.stride_words > (int)gridDim.x * PM_SW ||
            (long long)d.dst_off + (long long)h * d.stride_words * 4 > dst_bytes)
            return;
        words = min(PM_SW, d.stride_words - strip * PM_SW);            // signed: a strip behind the row owns none; pad words behind w are included
        if (words <= 0) return;
    }
    for (int i = tid; i < h * PM_SW; i += PM_THREADS) s_tog[i] = s_acc[i] = 0u;
    __syncthreads();

    if (x0 < w) {
        const int cw = tid & (PM_SW - 1), chunk = tid / PM_SW;
        const int rpc = (h + PM_CHUNKS - 1) / PM_CHUNKS;                                       // rows per chunk
        const int r0 = min(chunk * rpc, h), r1 = min(r0 + rpc, h);
        for (int p = 0; p < d.poly_count; ++p) {
            const int vf = polys[(size_t)(d.poly_first + p) * TOIST_POLY_REC_WORDS], vn = polys[(size_t)(d.poly_first + p) * TOIST_POLY_REC_WORDS + 1];
            if (vf < 0 || vn <= 0 || (long long)vf + vn > vert_cap) continue;                  // uniform over the workgroup
            for (int j = wave; j < vn; j += PM_WAVES) {
                const int jn = j + 1 == vn ? 0 : j + 1;
                long long xs = verts[2 * (size_t)(vf + j)], ys = verts[2 * (size_t)(vf + j) + 1];
                long long xe = verts[2 * (size_t)(vf + jn)], ye = verts[2 * (size_t)(vf + jn) + 1];
                const long long dx = xe > xs ? xe - xs : xs - xe, dy = ys > ye ? ys - ye : ye - ys;
                const bool major_x = dx >= dy;
                const bool flip = major_x ? xs > xe : ys > ye;                                 // which neighbour is the "previous" point
                if (flip) {
                    long long q = xs; xs = xe; xe = q;
                    q = ys; ys = ye; ye = q;
                }
                const long long length = major_x ? dx : dy;
                if (length == 0) continue;
                const double s = major_x ? (double)(ye - ys) / (double)dx : (double)(xe - xs) / (double)dy;
                for (long long dd = 1 + lane; dd <= length; dd += 64) poly_step(major_x, flip, xs, ys, s, length, dd, h, w, x0, s_tog);
            }
            __syncthreads();
            // prefix-XOR down the columns, a word column at a time: the parity of every chunk, an exclusive scan over the chunks (lanes 2 apart hold
            // the same word column), then the running parity through the chunk's rows
            uint32_t part = 0u;
            for (int r = r0; r < r1; ++r) part ^= s_tog[r * PM_SW + cw];
            uint32_t incl = part;
#pragma unroll
            for (int o = PM_SW; o < 64; o <<= 1) {
                const uint32_t y = __shfl_up(incl, o, 64);
                if (lane >= o) incl ^= y;
            }
            if (lane >= 64 - PM_SW) s_wave[wave][cw] = incl;                                   // the wave's parity per word column
            __syncthreads();
            uint32_t run = incl ^ part;
            for (int wv = 0; wv < wave; ++wv) run ^= s_wave[wv][cw];
            for (int r = r0; r < r1; ++r) {
                run ^= s_tog[r * PM_SW + cw];
                s_acc[r * PM_SW + cw] |= run;
                s_tog[r * PM_SW + cw] = 0u;
            }
            __syncthreads();
        }
    }

    if (DENSE) {
        // the live h x w region as bytes 0 / 1: a thread writes 4 adjacent bytes, as one word where the address allows
        uint8_t* base = dst + (size_t)slot * (size_t)cap_h * (size_t)cap_w;
        const int groups = PM_STRIP / 4;
        for (int i = tid; i < h * groups; i += PM_THREADS) {
            const int r = i / groups, c = (i % groups) * 4, x = x0 + c;
            if (x >= w) continue;
            const uint32_t nib = (s_acc[r * PM_SW + (c >> 5)] >> (c & 31)) & 15u;
            const uint32_t v = (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
            uint8_t* q = base + (size_t)r * cap_w + x;
            if (x + 4 <= w && ((size_t)q & 3) == 0) {
                *reinterpret_cast<uint32_t*>(q) = v;
            } else {
                for (int b = 0; b < 4 && x + b < w; ++b) q[b] = (uint8_t)((v >> (8 * b)) & 255u);
            }
        }
    } else {
        // pack_mask_bits' layout: row-major, pixel x = bit (x & 31) of little-endian word (x >> 5); every word of every live row, pad bits as zeros
        uint32_t* out = reinterpret_cast<uint32_t*>(dst + d.dst_off);
        for (int i = tid; i < h * PM_SW; i += PM_THREADS) {
            const int r = i / PM_SW, k = i % PM_SW;
            if (k < words) out[(size_t)r * d.stride_words + strip * PM_SW + k] = s_acc[i];
        }
    }
}

}  // namespace toist

using namespace toist;

extern "C" int toist_polygon_masks(const int32_t* desc, int slots, const int32_t* polys, int poly_cap, const int32_t* verts, int vert_cap, int cap_h,
                                   int cap_w, uint8_t* dst, long long dst_bytes, int mode, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    TOIST_REQUIRE(slots >= 0 && slots <= 65535, "toist_polygon_masks: bad slot count %d", slots);
    TOIST_REQUIRE(mode == TOIST_POLY_PACKED || mode == TOIST_POLY_DENSE, "toist_polygon_masks: unknown output mode %d", mode);
    if (slots == 0) return TOIST_OK;
    TOIST_REQUIRE(desc && polys && verts && dst, "toist_polygon_masks: null descriptor table, polygon records, vertex table or output");
    TOIST_REQUIRE(poly_cap > 0 && vert_cap > 0 && dst_bytes > 0, "toist_polygon_masks: empty polygon records, vertex table or output");
    TOIST_REQUIRE(cap_h > 0 && cap_h <= PM_ROWS && cap_w > 0, "toist_polygon_masks: bad capacity %d x %d (at most %d rows)", cap_h, cap_w, PM_ROWS);
    TOIST_REQUIRE((((size_t)desc | (size_t)polys | (size_t)verts) & 3) == 0 && (mode == TOIST_POLY_DENSE || ((size_t)dst & 3) == 0),
                  "toist_polygon_masks: the tables and the packed output hold 32-bit words (4-byte aligned)");
    const dim3 grid((cap_w + PM_STRIP - 1) / PM_STRIP, slots);
    if (mode == TOIST_POLY_DENSE)
        hipLaunchKernelGGL(polygon_masks_kernel<true>, grid, dim3(PM_THREADS), 0, stream, desc, polys, poly_cap, verts, vert_cap, cap_h, cap_w, dst, dst_bytes);
    else
        hipLaunchKernelGGL(polygon_masks_kernel<false>, grid, dim3(PM_THREADS), 0, stream, desc, polys, poly_cap, verts, vert_cap, cap_h, cap_w, dst, dst_bytes);
    return check_launch("toist_polygon_masks");
}
