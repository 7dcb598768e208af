// PostProcess as ONE launch for the whole batch (reference: models/postprocessors.py:19-55): per (image, query) row
//     scores        = 1 - softmax(logits)[-1]                 (fp32, max subtracted)
//     boxes         = cxcywh -> xyxy, scaled by the image's (w, h, w, h)
//     scores_refexp = scores * sigmoid(pred_isfinal)          (only with MDETR's referring-expression head)
// The original sizes come from a DEVICE table, so the launch takes no per-batch host value and sits in a captured graph.
// One wave owns one row: lanes stride over the C class columns (coalesced), two wave reductions (max, sum); lane 0..3 write the box.
// Traffic: B*Q*(C*sizeof(logit) + 4*sizeof(box)) in, B*Q*20 (24 with refexp) bytes out -- ~0.4 MB at B = 8, Q = 100, C = 256: launch-latency
// bound, which is the point of fusing the ~10 torch launches into one.
#include "common.h"

namespace toist {

static constexpr int PP_THREADS = 256;

template <bool BF>
__device__ __forceinline__ float pp_load(const void* p, size_t i) {
    if (BF) return bf2f(((const bf16_t*)p)[i]);
    return ((const float*)p)[i];
}

// grid: ceil(B*Q / 4); wave = one row
template <bool LOGITS_BF, bool BOXES_BF>
__global__ __launch_bounds__(PP_THREADS) void postprocess_kernel(const void* __restrict__ logits, const void* __restrict__ boxes, const void* __restrict__ isfinal,
                                                                  int isfinal_bf16, const int64_t* __restrict__ sizes, int B, int Q, int C,
                                                                  float* __restrict__ scores, float* __restrict__ out_boxes, float* __restrict__ scores_refexp) {
    const int row = blockIdx.x * (PP_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B * Q) return;
    const size_t base = (size_t)row * C;
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, pp_load<LOGITS_BF>(logits, base + c));
    mx = wave_max(mx);
    float sum = 0.f;
    for (int c = lane; c < C; c += 64) sum += expf(pp_load<LOGITS_BF>(logits, base + c) - mx);
    sum = wave_sum(sum);
    const float score = 1.f - expf(pp_load<LOGITS_BF>(logits, base + C - 1) - mx) / sum;
    if (lane == 0) {
        scores[row] = score;
        if (scores_refexp != nullptr) {
            const float f = isfinal_bf16 ? bf2f(((const bf16_t*)isfinal)[row]) : ((const float*)isfinal)[row];
            scores_refexp[row] = score * (1.f / (1.f + expf(-f)));
        }
    }
    if (lane < 4) {
        const int b = row / Q;
        // lanes 0, 1 -> (x0, y0) = centre - half extent; lanes 2, 3 -> (x1, y1) = centre + half extent; x scales by w, y by h
        const float centre = pp_load<BOXES_BF>(boxes, (size_t)row * 4 + (lane & 1)), extent = pp_load<BOXES_BF>(boxes, (size_t)row * 4 + 2 + (lane & 1));
        const float half = 0.5f * extent;
        const float corner = lane < 2 ? centre - half : centre + half;
        const float scale = (float)sizes[(size_t)b * 2 + ((lane & 1) ? 0 : 1)];      // table rows are (h, w)
        out_boxes[(size_t)row * 4 + lane] = corner * scale;
    }
}

}  // namespace toist

using namespace toist;

extern "C" int toist_postprocess(const void* pred_logits, int logits_bf16, const void* pred_boxes, int boxes_bf16, const void* pred_isfinal, int isfinal_bf16,
                                 const int64_t* orig_sizes, int B, int Q, int C, float* scores, float* boxes, float* scores_refexp, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    TOIST_REQUIRE(B >= 0 && Q >= 0 && C > 0 && (long long)B * Q < (1ll << 31) / 4, "toist_postprocess: bad extents B=%d Q=%d C=%d", B, Q, C);
    if (B == 0 || Q == 0) return TOIST_OK;
    TOIST_REQUIRE(pred_logits && pred_boxes && orig_sizes && scores && boxes, "toist_postprocess: null pointer");
    TOIST_REQUIRE((pred_isfinal == nullptr) == (scores_refexp == nullptr), "toist_postprocess: pred_isfinal and scores_refexp come together");
    const dim3 grid((unsigned)(((long long)B * Q + PP_THREADS / 64 - 1) / (PP_THREADS / 64)));
#define PP_LAUNCH(LB, BB)                                                                                                                               \
    hipLaunchKernelGGL((postprocess_kernel<LB, BB>), grid, dim3(PP_THREADS), 0, stream, pred_logits, pred_boxes, pred_isfinal, isfinal_bf16, orig_sizes, B, Q, C, \
                       scores, boxes, scores_refexp)
    if (logits_bf16 && boxes_bf16) PP_LAUNCH(true, true);
    else if (logits_bf16) PP_LAUNCH(true, false);
    else if (boxes_bf16) PP_LAUNCH(false, true);
    else PP_LAUNCH(false, false);
#undef PP_LAUNCH
    return check_launch("toist_postprocess");
}
