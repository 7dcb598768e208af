// The mask side of COCOeval for a whole batch of PostProcess rows in ONE launch: what the "segm" branch of TDODCocoEvaluator._evaluate
// (toist_amd/coco_eval.py; reference: datasets/coco_eval.py:307-332 -> maskUtils.iou -> maskApi.c rleIou) does per image with a gather of the kept
// planes, two mask_area launches and one mask_iou launch.  Row r = one image of a captured evaluation step, read in place:
//     bits     = the Q bit planes toist_mask_resize_pack_batch left at word r * capacity_words ([Q][w][ceil(h/64)], column-major, see evalmask.hip)
//     order    = toist_coco_boxes' ranking of the row's queries, so "segm" and "bbox" keep the same detections in the same order
//     dt_area  = popcount of plane order[r, d];  iou = rleIou of that plane against the row's staged ground-truth planes, row-major [D, G]
// The ground-truth planes of a whole evaluation sit on the device once (slot tables, as in evalbox.hip); a row names its slot.  Nothing is read
// from the host.  One 256-thread workgroup per (row, kept detection): the detection plane is streamed from HBM ONCE, chunk by chunk into LDS
// (TOIST_COCO_MASKS_CHUNK_WORDS words = 32 KiB; a 480 x 640 plane is 5120 words), and every chunk is intersected with the same words of the row's G
// ground-truth planes, which the row's D workgroups re-read from L2.  The work of a chunk is dealt over the four waves as (ground truth, quarter of
// the chunk) items, so one ground truth keeps all four busy; a wave's u32 partial count is reduced by shuffles and added to the ground truth's LDS
// counter.  All counts are integers: the result does not depend on the order of the reduction.  Planes start at 8-byte alignment only (w * words
// may be odd), so every global load is one 64-bit word per lane.
// Compiled with -ffp-contract=off like its neighbours that restate host arithmetic (the union is a sum of exact doubles either way).
#include "common.h"

namespace toist {

static constexpr int ER_THREADS = 256;
static constexpr int ER_WAVES = ER_THREADS / 64;
static constexpr int ER_CHUNK = TOIST_COCO_MASKS_CHUNK_WORDS;
static constexpr int ER_GROUP = 1024;                    // ground truths whose counters sit in LDS at a time; a row with more streams its plane once per group

// grid (D, R)
__global__ __launch_bounds__(ER_THREADS) void coco_masks_kernel(const uint64_t* __restrict__ bits, long long capacity_words,
                                                                const int64_t* __restrict__ row_hw, int Q, int D, const int32_t* __restrict__ order,
                                                                const int32_t* __restrict__ row_slot, const int64_t* __restrict__ slot_off, int n_slots,
                                                                const uint64_t* __restrict__ gt_bits, long long gt_words,
                                                                const int64_t* __restrict__ gt_plane_off, const int32_t* __restrict__ slot_hw,
                                                                const uint32_t* __restrict__ gt_parea, const uint8_t* __restrict__ gt_crowd, long long n_gt,
                                                                const int64_t* __restrict__ iou_off, long long iou_cap, double* __restrict__ dt_area,
                                                                double* __restrict__ iou) {
    __shared__ uint64_t s_chunk[ER_CHUNK];
    __shared__ unsigned s_acc[ER_GROUP];
    __shared__ unsigned s_part[ER_WAVES];
    const int d = blockIdx.x, r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* area_out = dt_area + (size_t)r * D + d;
    // the detection plane: a size that is not positive, planes that leave the row's capacity and a query index outside [0, Q) are never used as an
    // index -- the entry's area is 0 and the workgroup leaves (every thread reads the same words: the branch is uniform)
    const long long h = row_hw[2 * (size_t)r], w = row_hw[2 * (size_t)r + 1];
    const int q = order[(size_t)r * D + d];
    bool readable = h > 0 && w > 0 && h <= 0x7fffffffll && w <= 0x7fffffffll;
    long long plane = 0;
    if (readable) {
        plane = w * ((h + 63) >> 6);
        readable = plane <= capacity_words / Q;
    }
    if (!readable || q < 0 || q >= Q) {
        if (tid == 0) *area_out = 0.0;
        return;
    }
    // the row's ground truth: a slot outside the staged tables, planes of another size, extents that disagree with the slot or leave iou_cap, a
    // plane offset outside the arena, and any order entry of the ROW outside [0, Q) leave the row without IoU -- the host checks all before the launch
    const int slot = row_slot[r];
    long long g0 = 0, G = 0, io = 0;
    bool scored = slot >= 0 && slot < n_slots;
    if (scored) {
        g0 = slot_off[slot];
        G = slot_off[slot + 1] - g0;
        io = iou_off[r];
        scored = g0 >= 0 && G >= 0 && g0 <= n_gt && G <= n_gt - g0 && io >= 0 && iou_off[r + 1] - io == (long long)D * G && io <= iou_cap &&
                 (long long)D * G <= iou_cap - io;
        if (scored && G > 0) scored = (long long)slot_hw[2 * (size_t)slot] == h && (long long)slot_hw[2 * (size_t)slot + 1] == w;
    }
    int bad = 0;
    for (int e = tid; e < D; e += ER_THREADS) {
        const int o = order[(size_t)r * D + e];
        bad |= (o < 0 || o >= Q) ? 1 : 0;
    }
    if (scored)
        for (long long g = tid; g < G; g += ER_THREADS) {
            const long long off = gt_plane_off[g0 + g];
            bad |= (off < 0 || off > gt_words - plane) ? 1 : 0;
        }
    bad = __syncthreads_or(bad);
    if (bad || !scored) G = 0;

    const uint64_t* p = bits + (size_t)r * (size_t)capacity_words + (size_t)q * (size_t)plane;
    const long long groups = G > 0 ? (G + ER_GROUP - 1) / ER_GROUP : 1;
    unsigned mine = 0, area_d = 0;
    for (long long gg = 0; gg < groups; ++gg) {
        const long long left = G - gg * ER_GROUP;
        const int ng = (int)(left < ER_GROUP ? (left > 0 ? left : 0) : ER_GROUP);
        const long long gbase = g0 + gg * ER_GROUP;
        for (int i = tid; i < ng; i += ER_THREADS) s_acc[i] = 0;
        for (long long c0 = 0; c0 < plane; c0 += ER_CHUNK) {
            const int n = (int)(plane - c0 < ER_CHUNK ? plane - c0 : ER_CHUNK);
            __syncthreads();                                                 // the previous chunk has been read; the counters are zero
            for (int i = tid; i < n; i += ER_THREADS) {
                const uint64_t v = p[c0 + i];
                s_chunk[i] = v;
                if (gg == 0) mine += __popcll(v);
            }
            __syncthreads();
            int seg = (((n + ER_WAVES - 1) / ER_WAVES) + 63) & ~63;          // a quarter of the chunk, in whole wave strides
            seg = seg < 64 ? 64 : seg;
            const int nseg = (n + seg - 1) / seg;
            for (int e = wave; e < ng * nseg; e += ER_WAVES) {
                const int gl = e / nseg, s = e - gl * nseg;
                const uint64_t* gp = gt_bits + gt_plane_off[gbase + gl] + c0;
                const int lo = s * seg, hi = n < lo + seg ? n : lo + seg;
                unsigned acc = 0;
#pragma unroll 4
                for (int i = lo + lane; i < hi; i += 64) acc += __popcll(s_chunk[i] & gp[i]);
                acc = wave_sum(acc);
                if (lane == 0 && acc) atomicAdd(&s_acc[gl], acc);
            }
        }
        __syncthreads();                                                     // every counter of the group is complete
        if (gg == 0) {
            mine = wave_sum(mine);
            if (lane == 0) s_part[wave] = mine;
            __syncthreads();
#pragma unroll
            for (int i = 0; i < ER_WAVES; ++i) area_d += s_part[i];
        }
        for (int i = tid; i < ng; i += ER_THREADS) {                         // mask_iou_kernel's arithmetic
            const unsigned inter = s_acc[i];
            double v = 0.0;
            if (inter) {
                const double u = gt_crowd[gbase + i] ? (double)area_d : (double)area_d + (double)gt_parea[gbase + i] - (double)inter;
                v = (double)inter / u;
            }
            iou[io + (long long)d * G + gg * ER_GROUP + i] = v;
        }
        __syncthreads();                                                     // the counters have been read before the next group clears them
    }
    if (tid == 0) *area_out = (double)area_d;
}

}  // namespace toist

using namespace toist;

extern "C" int toist_coco_masks(const uint64_t* bits, long long capacity_words, const int64_t* row_hw, int R, int Q, int D, const int32_t* order,
                                const int32_t* row_slot, const int64_t* slot_off, int n_slots, const uint64_t* gt_bits, long long gt_words,
                                const int64_t* gt_plane_off, const int32_t* slot_hw, const uint32_t* gt_parea, const uint8_t* gt_crowd, long long n_gt,
                                const int64_t* iou_off, long long iou_cap, double* dt_area, double* iou, void* stream) {
    TOIST_REQUIRE(R >= 0 && R <= 65535 && Q >= 0 && D >= 0 && capacity_words >= 0 && n_slots > 0 && gt_words >= 0 && n_gt >= 0 && iou_cap >= 0,
                  "toist_coco_masks: bad extents R=%d Q=%d D=%d slots=%d capacity_words=%lld", R, Q, D, n_slots, capacity_words);
    TOIST_REQUIRE(D <= Q, "toist_coco_masks: %d kept detections of %d queries", D, Q);
    if (R == 0) return TOIST_OK;
    TOIST_REQUIRE(row_hw && row_slot && slot_off && slot_hw && iou_off, "toist_coco_masks: null table");
    if (D == 0) return TOIST_OK;
    TOIST_REQUIRE(bits && order && dt_area, "toist_coco_masks: null pointer (bits / order / dt_area)");
    TOIST_REQUIRE(n_gt == 0 || (gt_plane_off && gt_parea && gt_crowd), "toist_coco_masks: null pointer (staged ground truth)");
    TOIST_REQUIRE(gt_words == 0 || gt_bits, "toist_coco_masks: null pointer (gt_bits)");
    TOIST_REQUIRE(iou_cap == 0 || iou, "toist_coco_masks: null pointer (iou)");
    hipLaunchKernelGGL(coco_masks_kernel, dim3(D, R), dim3(ER_THREADS), 0, (hipStream_t)stream, bits, capacity_words, row_hw, Q, D, order, row_slot,
                       slot_off, n_slots, gt_bits, gt_words, gt_plane_off, slot_hw, gt_parea, gt_crowd, n_gt, iou_off, iou_cap, dt_area, iou);
    return check_launch("toist_coco_masks");
}
