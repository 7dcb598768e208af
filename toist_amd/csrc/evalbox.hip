// The box side of COCOeval for a whole batch of PostProcess rows in ONE launch: what TDODCocoEvaluator._detections and the bbox branch of
// TDODCocoEvaluator._evaluate (toist_amd/coco_eval.py; reference: datasets/coco_eval.py:291-305 convert_to_xywh + pycocotools computeIoU -> maskApi.c
// bbIou) do per image with about twenty torch launches.  Row r = one (image, caption) result of kernels.postprocess, read in place:
//     order    = the stable score-descending order of its Q queries on the scores as doubles, cut to D = min(Q, max_det)
//     dt_score, dt_area = the kept detections' scores and w * h (w, h formed in fp32 as PostProcess's consumers do, then widened)
//     iou      = bbIou of the kept detections against the row's ground truth, row-major [D, G]
//     gt_area, gt_crowd = the row's ground truth copied out of the staged tables, contiguous per row (what toist_coco_match reads)
// The ground truth of a whole evaluation sits on the device once (slot tables); a row names its slot.  Nothing is read from the host.
// One workgroup per row.  The scores sit in LDS as doubles; the rank of query d is the number of queries that come before it (Q^2 compares dealt
// over the lanes: 40 per lane at Q = 100, 4096 at the capacity of 1024), then the D x G block is dealt over the lanes.  Traffic per row: 20 Q bytes
// in, 20 D + 8 D G + 9 G bytes out -- about 1.3 MB for 112 rows of 100 queries and 10 boxes: launch-latency bound, one launch is the point.
// Compiled with -ffp-contract=off: da + ga - w * h must round the product first, as the torch ops it replaces do.
#include "common.h"

namespace toist {

static constexpr int EB_THREADS = 256;

// torch.minimum / torch.maximum: a NaN operand gives NaN
__device__ __forceinline__ double eb_min(double a, double b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }
__device__ __forceinline__ double eb_max(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// does query j (score sj) come before query d (score sd)?  torch.sort(descending=True, stable=True): NaN first, then larger scores, ties
// (-0.0 == 0.0 among them) in index order
__device__ __forceinline__ bool eb_before(double sj, int j, double sd, int d) {
    const bool nj = sj != sj, nd = sd != sd;
    if (nj || nd) return nj && (!nd || j < d);
    return sj > sd || (sj == sd && j < d);
}

__global__ __launch_bounds__(EB_THREADS) void coco_boxes_kernel(const float* __restrict__ scores, const float* __restrict__ boxes, int Q, int D,
                                                                const int32_t* __restrict__ row_slot, const int64_t* __restrict__ slot_off, int n_slots,
                                                                const double* __restrict__ gt_xywh, const double* __restrict__ gt_area,
                                                                const uint8_t* __restrict__ gt_crowd, long long n_gt,
                                                                const int64_t* __restrict__ iou_off, const int64_t* __restrict__ gt_off,
                                                                long long iou_cap, long long gt_cap, int32_t* __restrict__ order,
                                                                double* __restrict__ dt_score, double* __restrict__ dt_area, double* __restrict__ iou,
                                                                double* __restrict__ out_gt_area, uint8_t* __restrict__ out_gt_crowd) {
    __shared__ double s_score[TOIST_COCO_BOXES_MAX_Q];
    __shared__ int s_order[TOIST_COCO_BOXES_MAX_Q];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float* sc = scores + (size_t)r * Q;
    const float* bx = boxes + (size_t)r * Q * 4;
    for (int q = tid; q < Q; q += EB_THREADS) s_score[q] = (double)sc[q];
    __syncthreads();
    for (int d = tid; d < Q; d += EB_THREADS) {
        const double sd = s_score[d];
        int rank = 0;
        for (int j = 0; j < Q; ++j) rank += eb_before(s_score[j], j, sd, d) ? 1 : 0;
        if (rank < D) {
            const float w = bx[4 * d + 2] - bx[4 * d], h = bx[4 * d + 3] - bx[4 * d + 1];        // convert_to_xywh in fp32
            s_order[rank] = d;
            order[(size_t)r * D + rank] = d;
            dt_score[(size_t)r * D + rank] = sd;
            dt_area[(size_t)r * D + rank] = (double)w * (double)h;
        }
    }
    // the row's ground truth: a slot outside the staged tables is never used as an index, and a row whose extents in the batch tables disagree with
    // its slot (or leave the output capacities) writes nothing more -- the host checks both before the launch
    const int slot = row_slot[r];
    if (slot < 0 || slot >= n_slots) return;
    const int64_t g0 = slot_off[slot], G = slot_off[slot + 1] - g0;
    const int64_t io = iou_off[r], go = gt_off[r];
    if (g0 < 0 || G < 0 || g0 + G > n_gt || gt_off[r + 1] - go != G || iou_off[r + 1] - io != (int64_t)D * G) return;
    if (io < 0 || go < 0 || io + (int64_t)D * G > iou_cap || go + G > gt_cap) return;
    for (int64_t g = tid; g < G; g += EB_THREADS) {
        out_gt_area[go + g] = gt_area[g0 + g];
        out_gt_crowd[go + g] = gt_crowd[g0 + g];
    }
    __syncthreads();                                                                                // s_order is complete
    for (int64_t e = tid; e < (int64_t)D * G; e += EB_THREADS) {
        const int d = (int)(e / G);
        const int64_t g = e - (int64_t)d * G;
        const int q = s_order[d];
        const float x0 = bx[4 * q], y0 = bx[4 * q + 1];
        const float wf = bx[4 * q + 2] - x0, hf = bx[4 * q + 3] - y0;
        const double dx = (double)x0, dy = (double)y0, dw = (double)wf, dh = (double)hf;
        const double* gb = gt_xywh + (size_t)(g0 + g) * 4;
        const double gx = gb[0], gy = gb[1], gw = gb[2], gh = gb[3];
        const double da = dw * dh, ga = gw * gh;
        const double w = eb_min(dw + dx, gw + gx) - eb_max(dx, gx);
        const double h = eb_min(dh + dy, gh + gy) - eb_max(dy, gy);
        const double inter = w * h;
        const double uni = gt_crowd[g0 + g] ? da : da + ga - inter;
        iou[io + e] = (w > 0.0 && h > 0.0) ? inter / uni : 0.0;
    }
}

}  // namespace toist

using namespace toist;

extern "C" int toist_coco_boxes(const float* scores, const float* boxes, int R, int Q, int max_det, const int32_t* row_slot, const int64_t* slot_off,
                                int n_slots, const double* gt_xywh, const double* gt_area, const uint8_t* gt_crowd, long long n_gt,
                                const int64_t* iou_off, const int64_t* gt_off, long long iou_cap, long long gt_cap, int32_t* order, double* dt_score,
                                double* dt_area, double* iou, double* out_gt_area, uint8_t* out_gt_crowd, void* stream) {
    TOIST_REQUIRE(R >= 0 && Q >= 0 && max_det >= 0 && n_slots > 0 && n_gt >= 0 && iou_cap >= 0 && gt_cap >= 0,
                  "toist_coco_boxes: bad extents R=%d Q=%d max_det=%d slots=%d", R, Q, max_det, n_slots);
    TOIST_REQUIRE(Q <= TOIST_COCO_BOXES_MAX_Q, "toist_coco_boxes: %d queries exceed the kernel's capacity of %d", Q, TOIST_COCO_BOXES_MAX_Q);
    if (R == 0) return TOIST_OK;
    const int D = Q < max_det ? Q : max_det;
    TOIST_REQUIRE(row_slot && slot_off && iou_off && gt_off, "toist_coco_boxes: null table");
    TOIST_REQUIRE(Q == 0 || (scores && boxes), "toist_coco_boxes: null pointer (scores / boxes)");
    TOIST_REQUIRE(D == 0 || (order && dt_score && dt_area), "toist_coco_boxes: null pointer (order / dt_score / dt_area)");
    TOIST_REQUIRE(n_gt == 0 || (gt_xywh && gt_area && gt_crowd), "toist_coco_boxes: null pointer (staged ground truth)");
    TOIST_REQUIRE(gt_cap == 0 || (out_gt_area && out_gt_crowd), "toist_coco_boxes: null pointer (gt_area / gt_crowd outputs)");
    TOIST_REQUIRE(iou_cap == 0 || iou, "toist_coco_boxes: null pointer (iou)");
    hipLaunchKernelGGL(coco_boxes_kernel, dim3(R), dim3(EB_THREADS), 0, (hipStream_t)stream, scores, boxes, Q, D, row_slot, slot_off, n_slots, gt_xywh,
                       gt_area, gt_crowd, n_gt, iou_off, gt_off, iou_cap, gt_cap, order, dt_score, dt_area, iou, out_gt_area, out_gt_crowd);
    return check_launch("toist_coco_boxes");
}
