/*
 * toist_hip.h -- C ABI of the MI355X-native (gfx950) TOIST/MDETR hot path.
 *
 * The reference (AIR-DISCOVER/TOIST) has no FFI/plugin interface of its own: its hot path is stock
 * torch ops called from Python.  This header is therefore the boundary a
 * maintainer binds from Python with ctypes: plain pointers and sizes, no torch
 * types.  Each entry point names the reference call site it replaces.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller unless marked "host";
 *    the library never allocates or frees device memory and keeps no mutable global state;
 *  - every entry point only enqueues work on `stream` (a hipStream_t passed as void*) and never
 *    synchronises with the host;
 *  - return value: TOIST_OK (0) or a negative TOIST_E* code; the message for the last error of the
 *    calling thread is available from toist_last_error();
 *  - bf16 tensors are raw uint16 (upper half of an IEEE fp32), activations are row-major with the
 *    channel / feature axis innermost (NHWC for feature maps, [tokens, d] for sequences).
 */
#ifndef TOIST_HIP_H
#define TOIST_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TOIST_OK 0
#define TOIST_EINVAL (-1) /* bad shape / alignment / unsupported combination */
#define TOIST_EHIP (-2)   /* a HIP runtime call or kernel launch failed */

#define TOIST_ABI_VERSION 1

/* the library is built with -fvisibility=hidden: these entry points are its whole export table */
#if defined(__GNUC__)
#define TOIST_API __attribute__((visibility("default")))
#else
#define TOIST_API
#endif

TOIST_API int toist_version(void);
/* copies the calling thread's last error message (NUL terminated) into buf; returns its length */
TOIST_API int toist_last_error(char* buf, size_t cap);

/* ------------------------------------------------------------------------------------------------
 * Hungarian matcher.  Replaces HungarianMatcher.forward, /root/reference/models/matcher.py:39-87
 * (softmax + class/L1/GIoU cost, `.cpu()` sync, per-image scipy.optimize.linear_sum_assignment),
 * for L decoder layers x B images in one launch.
 *   logits   [L,B,Q,K] f32      boxes    [L,B,Q,4] f32 (cxcywh)
 *   tgt_boxes[Ttot,4]  f32      pos_map  [Ttot,K]  f32
 *   tgt_off  [B+1] i32 prefix sums of T_b          match_off [B+1] i32 prefix sums of min(Q,T_b)
 *   max_T    host value, max_b T_b (sizes the LDS)
 *   src_idx / tgt_idx [L, match_off[B]] i64: for image b the slice [match_off[b], match_off[b+1])
 *            holds the matched query indices (ascending) and their target indices (image-local),
 *            exactly the pair linear_sum_assignment returns for the [Q,T_b] block.
 *   status   [L*B] i32: 0 ok, 1 = cost block holds NaN/-inf (SciPy: "matrix contains invalid numeric
 *            entries"), 2 = infeasible.
 *   cost_out optional [L, B*Q, Ttot] f32 (only the per-image diagonal blocks are written).
 */
TOIST_API int toist_matcher(const float* logits, const float* boxes, const float* tgt_boxes, const float* pos_map,
                  const int32_t* tgt_off, const int32_t* match_off, int L, int B, int Q, int K, int max_T,
                  float w_class, float w_bbox, float w_giou, int64_t* src_idx, int64_t* tgt_idx,
                  int32_t* status, float* cost_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * bf16 MFMA GEMM family:  C[z][m][n] = epilogue( sum_k A[z][m][k] * B[z][n][k] ).
 * One descriptor covers nn.Linear forward/dgrad/wgrad (transformer.py:273-304,362-408, HF RoBERTa),
 * the attention batched products, and ResNet convolutions as im2col-free implicit GEMM on NHWC
 * activations (backbone.py:75 -> torchvision ResNet body; FrozenBatchNorm2d, backbone.py:48-58, is
 * the per-channel scale/shift of the epilogue).
 */
enum {
    TOIST_A_ROWK = 0,  /* A[m][k] at a + m*lda + k                                  (k contiguous) */
    TOIST_A_KROW = 1,  /* A[m][k] at a + k*lda + m                                  (m contiguous) */
    TOIST_A_CONV = 2,  /* m = output pixel (n,oy,ox), k = (r,s,c): gather from NHWC source         */
    TOIST_A_CONVT = 3  /* m = input pixel (n,iy,ix),  k = (r,s,co): transposed-conv gather (dgrad) */
};
enum {
    TOIST_B_ROWK = 0, /* B[n][k] at b + n*ldb + k */
    TOIST_B_KROW = 1, /* B[n][k] at b + (k % kin)*ldb + (k / kin)*tap_stride + n */
    TOIST_B_CONVX = 2 /* n = (r,s,c), k = output pixel: gather from NHWC source (conv wgrad) */
};
enum {
    TOIST_ACT_NONE = 0,
    TOIST_ACT_RELU = 1,
    TOIST_ACT_GELU = 2,        /* exact erf GELU */
    TOIST_ACT_SIGMOID = 3,
    TOIST_ACT_MASK_POS = 4,    /* v = aux > 0 ? v : 0           (ReLU backward)       */
    TOIST_ACT_GELU_BWD = 5,    /* v *= gelu'(aux)               (aux = pre-activation) */
    TOIST_ACT_SIGMOID_BWD = 6  /* v *= aux * (1 - aux)          (aux = sigmoid output) */
};

typedef struct toist_operand {
    const void* ptr;     /* bf16 */
    int64_t bs_outer;    /* element stride of batch index z / batch_inner */
    int64_t bs_inner;    /* element stride of batch index z % batch_inner */
    int32_t ld;          /* leading dimension in elements */
    int32_t kin;         /* B_KROW two-level k (0 = plain) */
    int64_t tap_stride;  /* B_KROW two-level k */
    /* gather geometry (CONV / CONVT / CONVX) */
    int32_t SH, SW, SC;  /* source tensor [N,SH,SW,SC] */
    int32_t PH, PW;      /* pixel space enumerated by the row (A) or k (B) index: [N,PH,PW] */
    int32_t R, S, stride, pad, dil;
} toist_operand;

typedef struct toist_epilogue {
    float alpha;          /* v = acc * alpha */
    const float* scale;   /* [N] f32 or NULL: v = v * scale[n] */
    const float* shift;   /* [N] f32 or NULL: v = v + shift[n] */
    const float* rscale;  /* [M] f32 or NULL: v = v * rscale[m] (FrozenBN scale of a conv wgrad row) */
    const void* res;      /* bf16 residual, same row map as C, or NULL */
    int32_t ldr;
    const void* aux;      /* bf16 operand of the *_BWD / MASK_POS activations */
    int32_t ldaux;
    int32_t act;          /* TOIST_ACT_* */
    void* pre_out;        /* optional bf16 copy of v before the activation (ld = ldc) */
    int32_t out_f32;      /* C is f32 instead of bf16 */
    int32_t accumulate;   /* C += v (requires out_f32); read-modify-write by the owning thread, no atomics */
    /* optional row scatter of C/res/aux: m = (n,oy,ox) in [*,cOH,cOW] -> ((n*cH + oy*cst)*cW + ox*cst) */
    int32_t cmap, cH, cW, cOH, cOW, cst;
    /* optional residual broadcast: res row = (m / res_div) * res_mod + (m % res_mod) when res_div > 0
       (one residual map shared by the res_div / res_mod consecutive row blocks, e.g. all queries of an image) */
    int32_t res_div, res_mod;
    /* dropout: where = 0 none, 1 = before the residual add, 2 = after the activation */
    int32_t drop_where;
    float drop_p;
    uint64_t drop_seed;
    const uint64_t* drop_seed_dev; /* optional device word added to drop_seed at run time, so a captured
                                      hipGraph draws a fresh mask on every replay */
} toist_epilogue;

/* Grouped launch: `batch` problems of one shape whose operands are not uniformly strided (the weight gradients of the
 * identical residual blocks of a ResNet stage: 23 x three GEMMs in layer 3, each too small to fill the chip on its own and
 * therefore split along K with a fold pass -- grouped, they run as one unsplit launch).  Entry z replaces the strided
 * batch addressing: A and B start at a / b, C (and res / aux / pre_out) is offset by c_off elements from toist_gemm.c,
 * epi.rscale by rscale_off and a_colsum by colsum_off elements.  Device memory, `batch` entries; batch_inner must be 1.
 * With split_k > 1 the workspace is [problem][k-slice][M][N] and the caller folds every problem with
 * toist_splitk_reduce_batch (TOIST_GEMM_DEFER_REDUCE). */
typedef struct toist_group {
    const void* a;
    const void* b;
    int64_t c_off;
    int64_t rscale_off;
    int64_t colsum_off;
    int64_t shift_off;        /* offset (elements) added to epi.scale / epi.shift: per-problem bias of grouped nn.Linear forwards */
} toist_group;                /* 48 bytes */

typedef struct toist_gemm {
    int32_t M, N, K;
    int32_t a_kind, b_kind;
    toist_operand a, b;
    void* c;
    int32_t ldc;
    int64_t cs_outer, cs_inner; /* batch strides of C (and res/aux/pre_out) */
    int32_t batch, batch_inner; /* z in [0,batch): outer = z / batch_inner, inner = z % batch_inner */
    int32_t split_k;            /* >= 1; > 1 needs out_f32 and `workspace`: every k-slice stores its raw f32
                                   partial tile there and a second kernel reduces them into C */
    int32_t tile;               /* 0 = auto; 64 = 64x64x32, 65 = 64x64x64, 128 = 128x128x32, 129 = 128x128x64,
                                   130 = 128x64x64, 132 = 128x32x64, 133 = 32x128x64, 134 = 64x128x64 (BM x BN x BK);
                                   131 = shared-halo 3x3 kernel, 135 = short-K panel kernel (K <= 256, row-major A; error
                                   if the call does not qualify); + 256 * ring slots (optional) */
    int32_t flags;              /* bit0: build K-strided fragments with ds_write_b16 instead of
                                   ds_read_b64_tr_b16 (validation fallback) */
    toist_epilogue epi;
    float* workspace;           /* split_k > 1: f32 scratch of >= split_k * M * N elements (caller-owned) */
    float* a_colsum;            /* optional, A_KROW only: a_colsum[m] += sum_k A[m][k]  (f32 atomics; with TOIST_GEMM_COLSUM_SLICES and
                                   split_k > 1: a_colsum[slice * M + m] = that slice's sum, no atomics) --
                                   the bias gradient of nn.Linear falls out of the wgrad GEMM's A tiles */
    const toist_group* group;   /* optional (device memory, `batch` entries): grouped launch, see toist_group */
    const void* a2;             /* optional, A_ROWK only: output columns n >= a2_from read their A rows from a2 (same ld / batch
                                   strides) -- nn.MultiheadAttention's packed in_proj applied to two inputs in one launch:
                                   q, k from x + pos, v from x (transformer.py:293-297, 370-400); a2_from % tile columns == 0 */
    int32_t a2_from;
} toist_gemm;

TOIST_API int toist_gemm_bf16(const toist_gemm* desc, void* stream);
/* writes n <= 64 host-side entries into a device table (they travel as kernel arguments: graph-capturable, no staging buffer) */
TOIST_API int toist_group_fill(const toist_group* rows, int n, toist_group* table, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Row kernels (bf16 data, f32 statistics).
 *  layernorm: nn.LayerNorm call sites transformer.py:279-280,341-345,481 and HF RoBERTa.
 *    bwd accumulates dgamma/dbeta with f32 atomics (caller zeroes them) and can also emit
 *    dx_drop = dropout-masked dx (mask regenerated from (seed, row*D+col), see toist_dropout_bf16).
 *  softmax:  the masked softmax inside nn.MultiheadAttention (transformer.py:273,337-338):
 *    scores/probs are [nbatch*H, Sq, ld] with ld >= roundup8(Sk); key_pad [nbatch,Sk] u8 (1 = pad).
 *    p_drop (optional) receives dropout(p) for the PV product.
 */
TOIST_API int toist_layernorm_fwd(const void* x, const float* gamma, const float* beta, float eps, int rows, int D,
                        void* y, float* mean, float* rstd, const void* add, void* y2, void* stream);
/*  optional second output y2 = y + add (both bf16 [rows, D]): the `src + pos` / `tgt + query_pos` that the next attention
 *  feeds to its q / k projections (transformer.py:293, 366, 386) without a separate elementwise launch */
TOIST_API int toist_layernorm_bwd(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                        int rows, int D, void* dx, float* dgamma, float* dbeta, void* dx_drop, float drop_p,
                        uint64_t seed, const uint64_t* seed_dev, float* partials, int partial_blocks, void* stream);
/* `partials` (optional, instead of dgamma / dbeta): f32 [2][partial_blocks][D] per-block sums of dy*xhat and dy, written with plain
 * stores (no contended atomics) for the caller to fold -- toist_splitk_reduce_batch with splits = partial_blocks, M = 1, N = D.
 * partial_blocks = toist_layernorm_bwd_blocks(rows). */
TOIST_API int toist_layernorm_bwd_blocks(int rows);
TOIST_API int toist_softmax_fwd(const void* scores, const uint8_t* key_pad, int nbatch, int H, int Sq, int Sk, int ld,
                      void* p, void* p_drop, float drop_p, uint64_t seed, const uint64_t* seed_dev, void* stream);
TOIST_API int toist_softmax_bwd(const void* p, const void* dp, int rows, int Sk, int ld, void* ds, float drop_p,
                      uint64_t seed, const uint64_t* seed_dev, void* stream);
/* every dropout seed is `seed + (seed_dev ? *seed_dev : 0)`: seed_dev is an optional device word */
/* out[n] += sum_m g[m][n]  (bias gradient; out is f32, caller zeroes it) */
TOIST_API int toist_colsum(const void* g, int M, int N, int ld, float* out, void* stream);
/* out = a + b, b broadcast with period b_period elements (with_pos_embed, transformer.py:287-288) */
TOIST_API int toist_add_bf16(const void* a, const void* b, int64_t n, int64_t b_period, void* out, void* stream);
/* out = dropout(x): keep iff hash(seed, flat index) >= p*2^32, kept values scaled by 1/(1-p) */
TOIST_API int toist_dropout_bf16(const void* x, int64_t n, float p, uint64_t seed, const uint64_t* seed_dev, void* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Backbone-side layout / pooling kernels (NHWC bf16).
 *  pack_image : f32 NCHW [N,C<=8,H,W] -> bf16 NHWC [N,H,W,8] (zero padded channels): the stem operand
 *  maxpool    : 3x3 / stride 2 / pad 1 (ResNet stem, reached through backbone.py:87-89)
 *  unpack     : bf16 NHWC [N,HW,C] -> f32 NCHW [N,C,HW] for API-edge feature maps
 */
TOIST_API int toist_pack_image(const float* nchw, int N, int C, int H, int W, void* nhwc8, void* stream);
TOIST_API int toist_maxpool3x3s2(const void* in, int N, int H, int W, int C, void* out, void* stream);
TOIST_API int toist_unpack_nhwc(const void* nhwc, int N, int HW, int C, float* nchw, void* stream);
/* RoBERTa position ids (cumsum(id != pad) * (id != pad) + pad) and key-padding bytes (attention_mask != 1) of a tokenized batch [B, L] in one launch
 * (HF create_position_ids_from_input_ids / the text branch of transformer.py:129-138) */
TOIST_API int toist_text_prep(const int64_t* ids, const int64_t* attention_mask, int B, int L, int64_t pad_id, int64_t* pos_ids, uint8_t* key_pad, void* stream);
/* diagnostic: slots[idx] = the device's constant-rate clock (100 MHz ticks) when everything ordered before this launch on `stream` is done
 * (dates the branches of a replayed hipGraph without a profiler: bench.py --stamps; no reference counterpart) */
TOIST_API int toist_stamp(uint64_t* slots, int idx, void* stream);

/* ResNet stem in one launch (torchvision ResNet.conv1 / bn1 / relu / maxpool as used by /root/reference/models/backbone.py:64-91; frozen there):
 * image f32 NCHW [N, C <= 8, H, W] -> conv 7x7 / stride 2 / pad 3 with `weight` bf16 [64][7][7][8] (KRSC, channels padded to 8, FrozenBN scale
 * folded in) + shift[64] (f32, may be NULL) + ReLU -> max-pool 3x3 / stride 2 / pad 1 -> out bf16 NHWC [N, PH, PW, 64],
 * OH = (H - 1) / 2 + 1, PH = (OH - 1) / 2 + 1 (likewise for the width).  Replaces toist_pack_image + a toist_gemm_bf16 gather + toist_maxpool3x3s2. */
TOIST_API int toist_stem_fwd(const float* image, const void* weight, const float* shift, int N, int C, int H, int W, void* out, void* stream);

/* PositionEmbeddingSine.forward (position_encoding.py:30-49; normalize=True, scale=2*pi):
 * mask [B,H,W] u8 (1 = padded pixel) -> bf16 [B, H*W, 2*num_pos_feats] tokens and/or f32
 * [B, 2*num_pos_feats, H, W] (either output may be NULL). */
TOIST_API int toist_sine_position(const uint8_t* mask, int B, int H, int W, int num_pos_feats, float temperature, void* out_tok,
                        float* out_nchw, void* stream);
/* the same encoding as the token-major bf16 rows of a [B, rows_per_image, 2F] sequence buffer, rows_per_image >= H*W: the rows behind an image's
 * H*W tokens (the caption tokens of the cross-modal encoder input) are zero (transformer.py:139 torch.zeros_like(text_memory_resized)) */
TOIST_API int toist_sine_position_seq(const uint8_t* mask, int B, int H, int W, int num_pos_feats, float temperature, void* out_tok, int rows_per_image,
                                      void* stream);

/* RoBERTa input embeddings (HF RobertaEmbeddings, called at transformer.py:130):
 * out[t] = word[ids[t]] + type0 + pos[pos_ids[t]] (f32 tables -> bf16 [n,D]); bwd scatter-adds the
 * bf16 gradient rows into the dense f32 table gradients with atomics (any of them may be NULL). */
TOIST_API int toist_embed_fwd(const int64_t* ids, const int64_t* pos_ids, const float* word, const float* pos, const float* type0,
                    int n, int D, void* out, void* stream);
TOIST_API int toist_embed_bwd(const void* g, const int64_t* ids, const int64_t* pos_ids, int n, int D, int64_t pad_id, float* dword,
                    float* dpos, float* dtype0, void* stream); /* rows whose id == pad_id get no gradient (padding_idx) */
/* Row-sparse gradient slots.  A slot of numel fp32 elements comes with `touched`, one byte per `chunk` elements (slot-relative,
 * ceil(numel / chunk) bytes); invariant: every element outside a chunk whose byte is set is +0.
 *   toist_embed_bwd_sparse  toist_embed_bwd that also keeps the invariant: the wave that owns a table row (first token with that id, id != pad_id)
 *                           stores 1 into the byte of every chunk the row overlaps, id*D / chunk .. ((id+1)*D - 1) / chunk.  touched_word /
 *                           touched_pos: the bytes of dword / dpos, either may be NULL (that gradient is then written as by toist_embed_bwd).
 *   toist_sparse_clear      one workgroup per chunk of up to two slots (numel1 == 0: one slot): a chunk whose byte is set is zeroed and its
 *                           byte cleared; the others cost a byte read.  Afterwards both slots are +0 throughout and every byte is clear. */
TOIST_API int toist_embed_bwd_sparse(const void* g, const int64_t* ids, const int64_t* pos_ids, int n, int D, int64_t pad_id, float* dword,
                    float* dpos, float* dtype0, uint8_t* touched_word, uint8_t* touched_pos, int chunk, void* stream);
TOIST_API int toist_sparse_clear(float* g0, uint8_t* touched0, int64_t numel0, float* g1, uint8_t* touched1, int64_t numel1, int chunk,
                    void* stream);

/* ------------------------------------------------------------------------------------------------
 * Set-criterion losses for all decoder layers at once.  Replaces SetCriterion.loss_labels / loss_boxes
 * / loss_cardinality (/root/reference/models/mdetr.py:488-518, 805-825, 783-803) given the device-
 * resident assignment of toist_matcher (same src_idx/tgt_idx/match_off/tgt_off).
 *   num_boxes  device f32[1] (already all-reduced / clamped, mdetr.py:997-1001)
 *   fwd: losses [L,4] f32 += (loss_ce, loss_bbox, loss_giou, cardinality_error) -- caller zeroes it
 *   match_status  optional int32[L*B] written by toist_matcher: a non-zero entry (NaN / -inf cost block, where SciPy raises
 *                 ValueError at /root/reference/models/matcher.py:85) poisons that layer's four losses with NaN, so the
 *                 caller's finite-loss guard (/root/reference/engine.py:82-85) trips without a host sync per call
 *   bwd: upstream [L,4] = d(total)/d(loss); dlogits [L,B,Q,K], dboxes [L,B,Q,4] are fully written
 */
TOIST_API int toist_criterion_fwd(const float* logits, const float* boxes, const float* tgt_boxes, const float* pos_map,
                        const int32_t* tgt_off, const int32_t* match_off, const int64_t* src_idx, const int64_t* tgt_idx,
                        const float* num_boxes, int L, int B, int Q, int K, float eos_coef, float* losses,
                        const int32_t* match_status, void* stream);
TOIST_API int toist_criterion_bwd(const float* logits, const float* boxes, const float* tgt_boxes, const float* pos_map,
                        const int32_t* tgt_off, const int32_t* match_off, const int64_t* src_idx, const int64_t* tgt_idx,
                        const float* num_boxes, int L, int B, int Q, int K, float eos_coef, const float* upstream,
                        float* dlogits, float* dboxes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Contrastive-alignment loss for all decoder layers at once.  Replaces SetCriterion.loss_contrastive_align
 * (/root/reference/models/mdetr.py:601-666) given the device-resident assignment of toist_matcher.
 *   proj_queries [L,B,Q,D] f32, proj_tokens [B,T,D] f32: the L2-normalised projections (mdetr.py:429-433)
 *   tok_mask     uint64 [sum_i T_i, 4]: bit t of row r = token t belongs to a positive span of target r
 *                (what the reference derives on the host from tokens_positive + char_to_token, :614-643; T <= 256 = max_text_len)
 *   fwd: losses [L] f32 += loss_contrastive_align of layer l (caller zeroes);  temperature = --temperature_NCE
 *   bwd: upstream [L]; dproj_queries [L,B,Q,D] fully written; dproj_tokens [B,T,D] += (caller zeroes)
 * toist_l2norm_fwd/bwd: F.normalize(x, p=2, dim=-1) on fp32 rows and its backward (dx from x, dy).
 */
TOIST_API int toist_contrastive_fwd(const float* proj_queries, const float* proj_tokens, const uint64_t* tok_mask, const int32_t* tgt_off,
                          const int32_t* match_off, const int64_t* src_idx, const int64_t* tgt_idx, const float* num_boxes, int L,
                          int B, int Q, int T, int D, float temperature, float* losses, void* stream);
TOIST_API int toist_contrastive_bwd(const float* proj_queries, const float* proj_tokens, const uint64_t* tok_mask, const int32_t* tgt_off,
                          const int32_t* match_off, const int64_t* src_idx, const int64_t* tgt_idx, const float* num_boxes, int L,
                          int B, int Q, int T, int D, float temperature, const float* upstream, float* dproj_queries,
                          float* dproj_tokens, void* stream);
/* the same backward with the token gradient summed over the L layers in layer order (no float atomics: the same sum in every run):
 * workspace = [L][B][T][D] fp32 scratch */
TOIST_API int toist_contrastive_bwd_ws(const float* proj_queries, const float* proj_tokens, const uint64_t* tok_mask, const int32_t* tgt_off,
                          const int32_t* match_off, const int64_t* src_idx, const int64_t* tgt_idx, const float* num_boxes, int L,
                          int B, int Q, int T, int D, float temperature, const float* upstream, float* dproj_queries,
                          float* dproj_tokens, float* workspace, void* stream);
/* toist_contrastive_fwd / _bwd_ws for a replayed graph whose captions are padded to T tokens (mdetr.py:601-666 takes its log-sum-exp over every
 * token column, :646-663, so a padded column would change the loss): live_tokens = one int32 in DEVICE memory, read by the kernel, refilled
 * between replays.  Tl = clamp(*live_tokens, 0, T) columns are live: the launch equals the launch on proj_tokens[:, :Tl] with T = Tl --
 * columns t >= Tl form no logit, enter no log-sum-exp, column term or positive count and give nothing to dproj_queries; their rows of
 * dproj_tokens and of the workspace are written as zeros (dproj_tokens: live rows +=, caller zeroes; dead rows = 0). */
TOIST_API int toist_contrastive_fwd_live(const float* proj_queries, const float* proj_tokens, const uint64_t* tok_mask, const int32_t* tgt_off,
                          const int32_t* match_off, const int64_t* src_idx, const int64_t* tgt_idx, const float* num_boxes, int L,
                          int B, int Q, int T, int D, float temperature, const int32_t* live_tokens, float* losses, void* stream);
TOIST_API int toist_contrastive_bwd_ws_live(const float* proj_queries, const float* proj_tokens, const uint64_t* tok_mask, const int32_t* tgt_off,
                          const int32_t* match_off, const int64_t* src_idx, const int64_t* tgt_idx, const float* num_boxes, int L,
                          int B, int Q, int T, int D, float temperature, const int32_t* live_tokens, const float* upstream,
                          float* dproj_queries, float* dproj_tokens, float* workspace, void* stream);
TOIST_API int toist_l2norm_fwd(const float* x, int rows, int D, float* y, void* stream);
TOIST_API int toist_l2norm_bwd(const float* x, const float* dy, int rows, int D, float* dx, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Segmentation branch (config 3), /root/reference/models/segmentation.py.
 *  attnmap_softmax: per-head softmax over HW of MHAttentionMap.forward (:262-273, `flatten(3)`).  scores [B,Q,H,ld] bf16
 *      (+ key_pad [B,HW] u8) -> probabilities channels-last [B*Q, HW, H] bf16; bwd returns dscores [B*Q,H,ld].
 *  groupnorm: torch.nn.GroupNorm(G, C) (+ReLU) on NHWC bf16 [N,HW,C] (:203-241); stats / bstats are f32 [N,G,2]
 *      scratch owned by the caller; bwd accumulates dgamma/dbeta with atomics (caller zeroes them).
 *  upsample_add: out[bq,Y,X,:] = fpn[bq/Q,Y,X,:] + in[bq,Y/2,X/2,:] (nearest 2x + shared FPN term); bwd = 2x2 sums.
 *  sum_queries: out[b,i] = sum_q in[b,q,i] (backward of the per-query broadcasts).
 *  mask_loss: bilinear (align_corners=False) upsample of pred[pred_row[t]] [h,w] f32 to [TH,TW], sigmoid focal
 *      (alpha, gamma=2) + dice sums against gt[gt_row[t]] u8 [TH,TW] (mdetr.py:827-853, segmentation.py:276-319):
 *      sums[t] += {focal, p*t, p, t}; bwd scatters coef[0]*dfocal + coef[1]*ddice into dpred (f32 atomics).
 *      pred_row[t] < 0 = an unused slot of a fixed-capacity pair table: skipped by both kernels (sums stay 0).
 *      mask_loss_bwd_compact writes pair t's gradient to row t of dpred_rows [T,h,w] instead of row pred_row[t] of a [B*Q,h,w] tensor:
 *      the loss (mdetr.py:827-853 `src_masks = outputs["pred_masks"][src_idx]`) touches the matched maps only, every other map's
 *      gradient is exactly zero, and the mask head's backward (per-map convolutions / GroupNorm(8, C) statistics, segmentation.py:203-241)
 *      then runs on those T maps alone.
 *  upsample_add_rows: upsample_add on a gathered subset of the maps: map i is map rows[i] of the batch (its FPN term: image rows[i] / Q).
 *  groupnorm_fwd with y == NULL computes the statistics only; groupnorm_apply normalises with statistics computed earlier.
 *  mask_stage_fwd: one launch per stage of MaskHeadSmallConv's tail (segmentation.py:223-240): the 3x3 convolution `lay` / `out_lay` whose
 *      INPUT is built on the way in from the previous convolution's raw output src [N,SH,SW,c_in]: gn_in = GroupNorm(8, c_in) + ReLU from
 *      src_stats [N,8,2] ({sum, sum of squares}) / gamma / beta; up = nearest 2x (SH = H/2), with the FPN term of `adapter(fpn) + up2(x)`
 *      taken out of the convolution by linearity: fpn_conv [N/Q,H,W,c_out] bf16 = lay(adapter(fpn)) of the map's image (bias included, the
 *      caller's one small convolution per image) is added in the epilogue.  w [w_rows,3,3,c_in] bf16, bias f32 or NULL.  c_out > 1: out
 *      [N,H,W,c_out] bf16 = raw convolution output, out_stats [N,8,2] its GroupNorm(8, c_out) sums (zeroed here, f32 atomics); c_out == 1
 *      (out_lay): out is f32 [N,H,W].  Shapes: (32,16,gn_in,up), (64,32,up), (16,1,gn_in).
 *  sum_segments: out[b,i] = sum over maps s in [seg[b], seg[b+1]) of in[s,i] -- sum_queries for maps packed image by image (seg on the device).
 */
TOIST_API int toist_attnmap_softmax_fwd(const void* scores, const uint8_t* key_pad, int B, int Q, int H, int HW, int ld, void* out, void* stream);
TOIST_API int toist_attnmap_softmax_bwd(const void* prob, const void* dprob, int BQ, int H, int HW, int ld, void* dscores, void* stream);
TOIST_API int toist_groupnorm_fwd(const void* x, const float* gamma, const float* beta, int N, int HW, int C, int G, float eps, int relu,
                        void* y, float* stats, void* stream);
TOIST_API int toist_groupnorm_apply(const void* x, const float* stats, const float* gamma, const float* beta, int N, int HW, int C, int G, float eps, int relu,
                        void* y, void* stream);
/* y may be NULL when beta is given: the ReLU mask (y > 0) is then re-derived from x, stats, gamma and beta with the forward's arithmetic */
TOIST_API int toist_groupnorm_bwd(const void* dy, const void* y, const void* x, const float* stats, const float* gamma, const float* beta, int N, int HW,
                        int C, int G, float eps, int relu, void* dx, float* dgamma, float* dbeta, float* bstats, void* stream);
TOIST_API int toist_upsample_add(const void* in, const void* fpn, int BQ, int Q, int H, int W, int C, void* out, void* stream);
TOIST_API int toist_upsample_add_rows(const void* in, const void* fpn, const int64_t* rows, int n, int Q, int H, int W, int C, void* out, void* stream);
TOIST_API int toist_upsample_add_bwd(const void* dout, int BQ, int H, int W, int C, void* din, void* stream);
/* The same three for ANY target size (/root/reference/models/segmentation.py:218, 225, 232: `cur_fpn + F.interpolate(x, size=cur_fpn.shape[-2:],
 * mode="nearest")` -- the FPN level's size is 2H x 2W only for image sides that are multiples of 32): out [n, OH, OW, C] = fpn[image] + in[n, src(Y), src(X)]
 * with torch's source index min(floor(dst * (float)in / out), in - 1); rows = NULL (map i is map i, n % Q == 0) or the gathered subset as in
 * toist_upsample_add_rows.  toist_resize_add_bwd: din[n, y, x] = sum of the dout pixels that read it. */
TOIST_API int toist_resize_add(const void* in, const void* fpn, const int64_t* rows, int n, int Q, int H, int W, int OH, int OW, int C, void* out, void* stream);
TOIST_API int toist_resize_add_bwd(const void* dout, int BQ, int H, int W, int OH, int OW, int C, void* din, void* stream);
TOIST_API int toist_sum_queries(const void* in, int B, int Q, int64_t per, void* out, void* stream);
TOIST_API int toist_mask_stage_fwd(const void* src, const float* src_stats, const float* gamma, const float* beta, const void* fpn_conv, const void* w,
                        const float* bias, void* out, float* out_stats, int N, int Q, int H, int W, int c_in, int c_out, int w_rows, int gn_in, int up,
                        float eps, void* stream);
/* The mask head of a task sweep: the maps are those of P (image, caption) PAIRS, Q per pair, and the per-IMAGE terms (fpn / fpn_conv [n_images, ...])
 * belong to image pair_image[map / Q] -- a DEVICE int32 table of N / Q entries, so one captured launch serves any pairing.  Otherwise the arguments,
 * the arithmetic and the results are those of toist_mask_stage_fwd (the two `up` stages (64,32) and (32,16,gn_in); out_lay has no image term) and of
 * toist_resize_add with rows = NULL.  toist_sweep_assemble's rule for a table entry outside [0, n_images): it is never used as an index, that pair's
 * image term counts as zero and *status = max(*status, pair + 1) (int32, atomicMax; the caller zeroes and reads it). */
TOIST_API int toist_mask_stage_fwd_pairs(const void* src, const float* src_stats, const float* gamma, const float* beta, const void* fpn_conv, const void* w,
                        const float* bias, void* out, float* out_stats, int N, int Q, int H, int W, int c_in, int c_out, int w_rows, int gn_in, int up,
                        float eps, const int32_t* pair_image, int n_images, int32_t* status, void* stream);
TOIST_API int toist_resize_add_pairs(const void* in, const void* fpn, const int32_t* pair_image, int n_images, int n, int Q, int H, int W, int OH, int OW,
                        int C, void* out, int32_t* status, void* stream);
TOIST_API int toist_sum_segments(const void* in, const int32_t* seg, int B, int rows, int64_t per, void* out, void* stream);
/* The mask head's BACKWARD over pairs (shared-image training: P pairs of Q maps each, pair p on image pair_image[p], a DEVICE int32 table of P entries).
 * toist_resize_add_rows_pairs: toist_resize_add on a gathered subset (rows int64 [n], n need not be a multiple of Q) whose image is read through the
 * table: out[i, Y, X, :] = fpn[pair_image[rows[i] / Q], Y, X, :] + in[i, src(Y), src(X), :], the arithmetic of toist_resize_add (fp32 add of two bf16
 * values, one rounding; the shift form for exact doublings).  A pair rows[i] / Q outside [0, P) or an image outside [0, n_images) is never used as an
 * index: its image term counts as zero and *status = max(*status, pair + 1) (P + 1 for a negative pair).
 * toist_sum_maps_by_image: in bf16 [rows, per] -> out bf16 [n_images, per]: out[b, :] = the fp32 sum, rounded once, of the maps of every pair p with
 * pair_image[p] == b, in ascending pair order and ascending map order -- no atomics: the same bits every run, whatever the order of the table.  Pair p's
 * maps are [seg[p], seg[p + 1]) clamped to [0, rows) (seg int32 [P + 1] on the device), or [p Q, (p + 1) Q) with seg = NULL.  An image without a pair
 * gets zeros; a table entry outside [0, n_images) is skipped and reported in *status as above.  per % 8 == 0. */
TOIST_API int toist_resize_add_rows_pairs(const void* in, const void* fpn, const int64_t* rows, const int32_t* pair_image, int n_images, int P, int n, int Q,
                        int H, int W, int OH, int OW, int C, void* out, int32_t* status, void* stream);
TOIST_API int toist_sum_maps_by_image(const void* in, const int32_t* seg, const int32_t* pair_image, int P, int Q, int n_images, int rows, int64_t per,
                        void* out, int32_t* status, void* stream);
TOIST_API int toist_mask_loss_fwd(const float* pred, const int32_t* pred_row, const uint8_t* gt, const int32_t* gt_row, int T, int h, int w,
                        int TH, int TW, float alpha, float* sums, const int32_t* valid_hw, void* stream);
TOIST_API int toist_mask_loss_bwd(const float* pred, const int32_t* pred_row, const uint8_t* gt, const int32_t* gt_row, int T, int h, int w,
                        int TH, int TW, float alpha, const float* sums, const float* coef, float* dpred, const int32_t* valid_hw, void* stream);
TOIST_API int toist_mask_loss_bwd_compact(const float* pred, const int32_t* pred_row, const uint8_t* gt, const int32_t* gt_row, int T, int h, int w,
                        int TH, int TW, float alpha, const float* sums, const float* coef, float* dpred_rows, const int32_t* valid_hw, void* stream);
/* valid_hw (all three; NULL = everything): device int32 [4] = {VH, VW, hs, ws} for a batch that sits in the corner of a larger bucket (a captured graph's
 * static shape).  The reference resizes its [hs, ws] prediction to the batch's largest image [VH, VW] (mdetr.py:843) and averages loss_mask over
 * those pixels: prediction rows / columns [0, hs) x [0, ws) are mapped onto target pixels [0, VH) x [0, VW) (align_corners = False grid of that
 * pair of sizes), nothing else takes part, and the caller divides loss_mask by VH * VW.  gt keeps its row stride TW. */

/* ---- optimizer tail: clip_grad_norm_ + AdamW + EMA + bf16 compute-copy refresh in one multi-tensor pass ------------
 * Replaces engine.py:87-101 of the reference (torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm);
 * optimizer.step() with torch.optim.AdamW over the 3 parameter groups of main.py:351-392; update_ema of
 * util/optim.py:9-26).  All tables live in device memory and are owned by the caller; `grads[i]` is the device
 * address of tensor i's fp32 gradient (0 = no gradient this step: the tensor is only EMA-averaged).
 * Work is cut into chunks of toist_opt_chunk_elems() elements: chunks[2*b] = tensor index, chunks[2*b+1] = chunk
 * index inside that tensor.  State (step count, clip coefficient, bias corrections) stays on the device so a
 * captured hipGraph replays the tail unchanged; learning rates are read from `groups` at run time.
 * Guard (opt-in): toist_opt_finish_norm_guarded SKIPS a step whose gradient norm is not finite (NaN / inf gradients, or an fp32
 * sum of squares that overflows: finite gradients of ~1e19 and above) or that a veto word objects to -- device words read at run
 * time through two pointer tables: int32 words veto when non-zero (a kernel's failure status), fp32 words when not finite (the
 * loss).  A skipped step sets state.skipped, does not advance state.step, and every toist_opt_adamw_ema[_blocks] launch that reads
 * that state returns without writing: parameters, moments, averages and bf16 copies stay bit for bit as they were.  The plain
 * toist_opt_finish_norm never skips (it clears state.skipped): a non-finite norm then reaches the parameters, as in torch. */
typedef struct toist_opt_tensor {
    float* p;                 /* fp32 master parameter (or the EMA source for buffers / frozen parameters)            */
    float* m;                 /* exp_avg     (NULL: never updated by the optimizer)                                   */
    float* v;                 /* exp_avg_sq                                                                           */
    float* ema;               /* EMA copy of p, or NULL                                                               */
    uint16_t* w;              /* bf16 compute copy refreshed from the new p, or NULL                                  */
    const float* row_scale;   /* optional: w = bf16(p * row_scale[element / row_len]) (folded FrozenBatchNorm scale)  */
    int64_t numel;
    int32_t row_len;
    int32_t group;            /* index into groups[]                                                                  */
} toist_opt_tensor;           /* 64 bytes */

typedef struct toist_opt_group {
    float lr;
    float weight_decay;
} toist_opt_group;

typedef struct toist_opt_state {
    float clip_coef;          /* min(1, max_norm / (grad_norm + 1e-6)); 1 when max_norm <= 0                          */
    float grad_norm;          /* total 2-norm of all gradients before clipping                                        */
    float bias1;              /* 1 - beta1^step                                                                       */
    float bias2_sqrt;         /* sqrt(1 - beta2^step)                                                                 */
    int32_t step;             /* optimizer steps APPLIED (incremented by toist_opt_finish_norm[_guarded]; not by a skipped step) */
    int32_t skipped;          /* 1: the last finish-norm launch vetoed the step (toist_opt_adamw_ema then returns at once), else 0 */
    int32_t skipped_total;    /* vetoed steps since the state was zeroed                                              */
    int32_t veto_mask;        /* why the last step was vetoed: bit 0 = grad_norm not finite, bit 1+i = integer veto word i
                                 non-zero, bit 9+j = float veto word j not finite; 0 after an applied guarded step   */
} toist_opt_state;            /* 32 bytes */
#define TOIST_OPT_MAX_VETO 8  /* veto words of each kind a guarded finish-norm launch reads                           */

/* ---- attention cores (head dim 32; csrc/attn2.hip; the first-generation toist_attn_fwd / toist_attn_bwd of rounds 1-4 were removed in round 5).  Operands: per-head column
 * slices of [B*S, ld*] bf16 buffers), flash-style only: nothing score-shaped is stored, the key count is unbounded.
 *   toist_attn2_fwd   ctx = dropout(softmax(scale q k^T + key padding)) v; lse (f32 [B*H, Sq, 2]) receives (maximum of the RAW dot
 *                     products of the row, 1 / sum of exp(scale (s - max))).  The keep mask of element (row = bh * Sq + q, key) is the
 *                     16-bit field key & 1 of pair_hash((row * round8(Sk) + key) >> 1) compared with round(drop_p * 65536).
 *   toist_attn2_bwd   key-owning backward: dk / dv are written once; workgroup x of a head owns keys [128 x, 128 x + 128).  With
 *                     toist_attn2_splits(Sk) == 1 dq is written directly; otherwise every split leaves ITS share of dq in
 *                     dq_part (bf16 [splits][B*Sq][H*32], already multiplied by scale) and the consumer adds the shares
 *                     (toist_rowgemm's fold prologue); dq may then be NULL. */
TOIST_API int toist_attn2_splits(int Sk);
TOIST_API int toist_attn2_fwd(const void* q, int ldq, const void* kmat, int ldk, const void* v, int ldv, const uint8_t* key_pad, int B, int H, int Sq,
                    int Sk, int dh, float scale, float drop_p, uint64_t seed, const uint64_t* seed_dev, void* ctx, int ldo, float* lse,
                    void* stream);
TOIST_API int toist_attn2_bwd(const void* q, int ldq, const void* kmat, int ldk, const void* v, int ldv, const void* ctx, int ldo, const void* dctx, int lddo,
                    const float* lse, const uint8_t* key_pad, int B, int H, int Sq, int Sk, int dh, float scale, float drop_p, uint64_t seed,
                    const uint64_t* seed_dev, void* dq, int lddq, void* dk, int lddk, void* dv, int lddv, void* dq_part, void* stream);

/* ---- row-complete transformer sub-layers (d_model = 256; csrc/tlayer.hip).  One launch computes out[m][0..255] for blocks of 16
 * rows over the whole reduction length K and finishes the rows on chip:
 *   TOIST_ROW_LN_FWD  x + dropout(sublayer(x)) followed by LayerNorm -- `norm1(src + dropout1(src2))`, `norm2(src + dropout2(src2))` of
 *                     /root/reference/models/transformer.py:297-303 and norm1 / norm3 / norm4 of :376-407:
 *                       z = bf16(res + dropout(a w^T + bias));  out = LayerNorm(z) gamma + beta;  out2 = bf16(out + add) (optional);
 *                       z, mean, rstd are kept for the backward pass;
 *   TOIST_ROW_LN_BWD  the data gradient a w (+ res + res2: gradients arriving over residual connections) is the gradient w.r.t. a
 *                     LayerNorm OUTPUT; the launch applies the LayerNorm backward (saved z / mean / rstd, gamma) and writes
 *                       out = dz (gradient of the LayerNorm input = of the residual stream), out2 = dropout-masked dz (the gradient
 *                       of the dropout(sublayer) term, same (seed, m * 256 + n) hash as the forward pass; optional),
 *                       partials[2][blocks][256] f32 = per-block sums of g * xhat and g over the block's rows (d gamma / d beta, folded
 *                       by toist_splitk_reduce_batch; blocks = toist_rowgemm_blocks(M)); NULL when gamma is frozen;
 *   TOIST_ROW_PLAIN   out = bf16(a w (+ bias) + res + res2).
 * w is the nn.Linear parameter's bf16 copy read in place: TOIST_B_ROWK = [256][K] rows (forward: y = a w^T), TOIST_B_KROW = [K][256]
 * rows (data gradient: da = dy w).  Fold prologue (fold_parts > 1): columns [0, fold_cols) of every A row are the f32 sum of fold_parts
 * bf16 slabs (slab s, row m, column c at fold + s * fold_stride + m * fold_cols + c) -- the key-split partial dQ of toist_attn2_bwd --
 * rounded once and WRITTEN BACK to a (the weight-gradient GEMM reads the folded rows later).
 * All pointers 16-byte aligned, leading dimensions multiples of 8 elements, K a multiple of 128 (<= 4096).  The caller owns every
 * buffer; nothing is allocated, nothing synchronises. */
enum { TOIST_ROW_PLAIN = 0, TOIST_ROW_LN_FWD = 1, TOIST_ROW_LN_BWD = 2 };

typedef struct toist_rowgemm_desc {
    int32_t M, K;             /* rows, reduction length; the output is [M, 256] */
    int32_t b_kind;           /* TOIST_B_ROWK or TOIST_B_KROW */
    int32_t epi;              /* TOIST_ROW_* */
    const void* a;            /* bf16 [M, K], row stride lda (written when folding) */
    const void* w;            /* bf16 weights, row stride ldw */
    int32_t lda, ldw;
    const void* fold;         /* bf16 slabs of the fold prologue, or NULL */
    int64_t fold_stride;      /* elements between slabs */
    int32_t fold_parts, fold_cols;
    const float* bias;        /* f32 [256] or NULL */
    const void* res;          /* bf16 [M, 256], row stride ldr, or NULL */
    const void* res2;         /* bf16 [M, 256], row stride ldr2, or NULL */
    int32_t ldr, ldr2;
    float drop_p;             /* LN_FWD: dropout of (a w^T + bias);  LN_BWD: the mask of out2 */
    float eps;                /* LN_FWD */
    uint64_t drop_seed;
    const uint64_t* drop_seed_dev;   /* optional device word added to drop_seed (graph replay) */
    const float* gamma;       /* f32 [256] */
    const float* beta;        /* f32 [256] (LN_FWD) */
    void* z;                  /* bf16 [M, 256] contiguous: LN_FWD output (optional), LN_BWD input */
    float* mean;              /* f32 [M]: LN_FWD output (optional), LN_BWD input */
    float* rstd;
    void* out;                /* bf16 [M, 256], row stride ldo */
    int32_t ldo, reserved;
    const void* add;          /* LN_FWD: bf16 [M, 256] contiguous constant added into out2 */
    void* out2;               /* bf16 [M, 256] contiguous (see above), or NULL */
    float* partials;          /* LN_BWD: f32 [2][blocks][256], or NULL */
} toist_rowgemm_desc;

TOIST_API int toist_rowgemm_blocks(int M);
TOIST_API int toist_rowgemm(const toist_rowgemm_desc* d, void* stream);

/* ---- XCD-resident decoder stack, forward (/root/reference/models/transformer.py:225-267 TransformerDecoder.forward, :362-408
 * TransformerDecoderLayer.forward_post): ALL L post-norm decoder layers of d_model 256 / 8 heads / dim_feedforward 2048 in ONE launch.
 * Images are independent from the first decoder layer to the last, and an MI355X has 8 XCDs of 32 CUs with one L2 each: the launch is
 * 256 workgroups of 512 threads (one per CU); every workgroup reads its XCC id from the hardware register, takes a ticket on that XCD's
 * counter, and the 32 workgroups that read the same id form the group of image b = xcc (+ 8, + 16 ... for B > 8).  A group exchanges
 * activations only through its own L2 (plain stores, `s_waitcnt vmcnt(0)`, an L2-scope atomic arrival counter polled by one lane, sc1
 * loads that bypass the reader's L1): 0.84 us per synchronisation point (profiles/r05_xcd_barrier.txt), four per layer:
 *   P1  q | k | v = [x + query_pos | x] W_in^T + b_in             column tiles over the 32 CUs                      -> barrier
 *   A   a CU owns 4 query rows: self-attention of its rows (wave = head), out_proj + dropout + residual + norm1, the cross-attention
 *       query projection, cross-attention into the pre-projected memory K / V (wave = head, flash over 128-key blocks), out_proj +
 *       dropout + residual + norm3 -- all inside the workgroup                                                     -> barrier
 *   P6  a CU owns 64 of the 2048 hidden units: ReLU(y3 W1^T + b1) with dropout, and ITS partial sum of linear2    -> barrier
 *   P7  the row owners add the 32 partials, bias, dropout, residual, norm4 (and y4 + query_pos for the next layer) -> barrier
 * Every tensor the existing backward launches read (csrc/attn2.hip toist_attn2_bwd, csrc/tlayer.hip toist_rowgemm LN_BWD, the grouped
 * weight gradients) is written with the layouts, (maximum, 1 / sum) statistics and dropout hashes of the per-op forward kernels, so
 * the backward pass is unchanged.  Limits: Q <= 128, S <= 512, L <= 8, the device must expose 8 XCDs x 32 CUs.
 * ctl: 1024 uint32 of caller scratch, zeroed once by the caller; the launch function re-zeroes words 0 .. 1022 (a memset node under
 * capture).  ctl[1023] is sticky: != 0 = a bounded spin expired in some launch (a group was not co-resident) and that launch's
 * results are invalid.  Such a launch also overwrites every layer output (y4) of the affected images with NaN (the backward launch: their
 * `sink` rows), so the failure reaches the losses / the gradient norm even if nobody reads the status word. */
enum { TOIST_XDEC_MAX_LAYERS = 8, TOIST_XDEC_CTL_WORDS = 1024 };

typedef struct toist_xdec_layer {
    const void* w_in;  const float* b_in;      /* self_attn.in_proj_weight bf16 [768, 256] / bias f32 [768] */
    const void* w_os;  const float* b_os;      /* self_attn.out_proj */
    const float* g1;   const float* be1;       /* norm1 */
    const void* w_q;   const float* b_q;       /* cross_attn_image.in_proj rows 0 .. 255 (the query projection) */
    const void* w_oc;  const float* b_oc;      /* cross_attn_image.out_proj */
    const float* g3;   const float* be3;       /* norm3 */
    const void* w1;    const float* b1;        /* linear1 bf16 [2048, 256] */
    const void* w2;    const float* b2;        /* linear2 bf16 [256, 2048] */
    const float* g4;   const float* be4;       /* norm4 */
    uint64_t seed[6];                          /* dropout seeds: self-attention, norm1 branch, cross-attention, norm3 branch, hidden, norm4 branch */
} toist_xdec_layer;

typedef struct toist_xdec_desc {
    int32_t B, Q, S, L;
    const void* x0;            /* bf16 [B*Q, 256]: tgt entering layer 0 (zeros in the reference) */
    const void* qpos;          /* bf16 [B*Q, 256]: query_pos broadcast over the batch */
    const void* xe0;           /* bf16 [B*Q, 256]: x0 + query_pos, the rows layer 0's q | k projections read (later layers keep y4 + query_pos themselves: y4e).
                                * With x0 = 0 (the reference) pass qpos itself. */
    const void* kv;            /* bf16 [B*S, ldkv]: memory K (with pos) / V projections of layer l at columns l*512 / l*512 + 256 */
    int32_t ldkv;
    int32_t ff;                /* dim_feedforward of linear1 / linear2: the launch is compiled for 2048, anything else is refused (TOIST_EINVAL) */
    int32_t test_absent;       /* 0.  Failure-path tests only: that many workgroups per XCD leave at once, as if they were not co-resident */
    int32_t reserved;
    const uint8_t* key_pad;    /* [B, S] 1 = padding, or NULL */
    float drop_p, eps;
    const uint64_t* seed_dev;  /* optional device word added to every seed (graph replay) */
    /* stacked per-layer outputs, layer l at + l * B*Q * width elements */
    void* qkv;                 /* bf16 [L][B*Q][768] */
    void* ctx_s;               /* bf16 [L][B*Q][256] self-attention context */
    float* lse_s;              /* f32  [L][B*8][Q][2] */
    void* z1; void* y1; void* y1e; float* mean1; float* rstd1;          /* norm1: pre-norm sum, output, output + query_pos */
    void* qc;                  /* bf16 [L][B*Q][256] cross-attention queries */
    void* ctx_c;               /* bf16 [L][B*Q][256] */
    float* lse_c;              /* f32  [L][B*8][Q][2] */
    void* z3; void* y3; float* mean3; float* rstd3;                      /* norm3 */
    void* h;                   /* bf16 [L][B*Q][2048] dropout(relu(linear1)) */
    void* z4; void* y4; void* y4e; float* mean4; float* rstd4;          /* norm4: y4 = the layer output (tgt_stack), y4e = y4 + query_pos */
    void* part;                /* bf16 [B][32][128][256] scratch: linear2 partial sums */
    uint32_t* ctl;             /* TOIST_XDEC_CTL_WORDS words of scratch */
    uint64_t* prof;            /* diagnostics, normally NULL: [256 workgroups][L][16] device-clock stamps (100 MHz) at the phase boundaries of image 0 .. 7 */
    toist_xdec_layer layer[TOIST_XDEC_MAX_LAYERS];
} toist_xdec_desc;

TOIST_API int toist_xdec_supported(int B, int Q, int S, int L);      /* 1 when toist_xdec_fwd takes the shape on the current device */
TOIST_API int toist_xdec_fwd(const toist_xdec_desc* d, void* stream);

/* ---- XCD-resident decoder stack, backward: the data-gradient chain of ALL L decoder layers in one launch, consuming what toist_xdec_fwd saved
 * (same grouping: one image per XCD, 32 workgroups of 512 threads, XCD-local barriers; six per layer):
 *   R0  row owners: norm4 backward of their 4 rows (gradient of the layer output = next layer's input gradient + the shared final norm's share)
 *   H   CU = 64 hidden units: dh = (dzd4 W2) masked by h > 0, and ITS partial sum of dh W1
 *   C   row owners: fold the 32 partials + residual gradient, norm3 backward, gradient of the cross-attention context (x W_oc)
 *   D   CU = (head, key split): cross-attention backward (the body of toist_attn2_bwd: dk / dv of the memory written once, dq shares)
 *   E   row owners: fold dq, x W_q + residual gradient, norm1 backward, gradient of the self-attention context (x W_os)
 *   F   CU = head: self-attention backward (dq | dk | dv of the layer's q | k | v)
 *   G   row owners: [dq | dk | dv] W_in + residual gradient + the final norm's share of the layer below = the next R0's input
 * Weight gradients are NOT formed here: every operand they need (dzd4, dh, dzd3, dq, dzd1, dq | dk | dv) is left in the output tensors for the
 * grouped weight-gradient launches, and the LayerNorm parameter gradients leave as per-row-block partial sums (ln_part) for
 * toist_splitk_reduce_batch.  Limits as toist_xdec_fwd. */
typedef struct toist_xdec_bwd_layer {
    const void* w_in;          /* bf16 weights, read in place as k-major operands */
    const void* w_os;
    const void* w_q;
    const void* w_oc;
    const void* w1;
    const void* w2;
    const float* g1;           /* LayerNorm gammas */
    const float* g3;
    const float* g4;
    uint64_t seed[6];          /* the forward's seeds */
} toist_xdec_bwd_layer;

typedef struct toist_xdec_bwd_desc {
    int32_t B, Q, S, L;
    const void* kv;            /* as toist_xdec_desc */
    int32_t ldkv, ldsink, lddkv;
    int32_t ff;                /* as toist_xdec_desc: must be 2048 */
    int32_t test_absent;       /* as toist_xdec_desc: 0 outside failure-path tests */
    int32_t reserved;
    const uint8_t* key_pad;
    float drop_p, reserved2;
    const uint64_t* seed_dev;
    /* saved by the forward launch (stacked per layer) */
    const void* qkv; const void* ctx_s; const float* lse_s; const void* z1; const float* mean1; const float* rstd1;
    const void* qc; const void* ctx_c; const float* lse_c; const void* z3; const float* mean3; const float* rstd3;
    const void* h; const void* z4; const float* mean4; const float* rstd4;
    const void* g_out;         /* bf16 [L][B*Q][256]: gradient of the shared final norm w.r.t. every layer's output */
    /* outputs */
    void* gb4;                 /* bf16 [L][B*Q][256]: (dropout-masked) gradient of norm4's input = dy of linear2 */
    void* dh;                  /* bf16 [L][B*Q][2048]: gradient of linear1's output */
    void* go3;                 /* bf16 [L][B*Q][256]: dy of cross_attn out_proj */
    void* go1;                 /* bf16 [L][B*Q][256]: dy of self_attn out_proj */
    void* sink;                /* bf16 [B*Q][ldsink]: per layer l at columns l*1024: [dq_s | dk_s | dv_s | dq_c] */
    void* dkv;                 /* bf16 [B*S][lddkv]: dk / dv of the memory projections, layer l at columns l*512 / l*512 + 256 */
    float* ln_part;            /* f32 [L][3][2][B*ceil(Q/4)][256]: (sum v*xhat, sum v) per row block for norm1 / norm3 / norm4 */
    /* scratch */
    void* dctx;                /* bf16 [2][B*Q][256] */
    void* part;                /* bf16 [B][32][128][256] */
    void* dq_part;             /* bf16 [4][B*Q][256] */
    uint32_t* ctl;
    uint64_t* prof;
    toist_xdec_bwd_layer layer[TOIST_XDEC_MAX_LAYERS];
} toist_xdec_bwd_desc;

TOIST_API int toist_xdec_bwd(const toist_xdec_bwd_desc* d, void* stream);

/* ---- masked row scatter (the nearest-replacement memory-bank update, /root/reference/models/mdetr.py:98-103, when the pair table has a fixed
 * capacity and the live slots are only known on the device: hipGraph replay of the distillation step).  dst[dst_row[i]] = src[src_row[i]] (rows of d
 * floats) for every i < m with src_row[i] >= 0 and dst_row[i] >= 0; live destinations must be distinct. */
TOIST_API int toist_scatter_rows_f32(const float* src, const int64_t* src_row, float* dst, const int64_t* dst_row, int m, int d, void* stream);

/* ---- k-means of the distillation step on the device (models/kmeans.py:21-96 as mdetr.py:213-234 calls it).  One workgroup per
 * distinct task of the batch: group g covers samples members[group_off[g] .. group_off[g+1]) (batch order), all of task
 * group_task[g]; for each sample: Lloyd iterations over banks[task] ([N, D] f32, stride bank_stride elements) from
 * centers[task] ([K, D] f32, stride centers_stride, updated IN PLACE) until (sum_k |shift_k|)^2 < tol (or max_iter), then
 * pick[sample] = index of the centre nearest to features[sample] ([*, D] f32) and chosen_center[sample] = that centre.
 * No host synchronisation; iters (optional) receives the iteration count per sample. */
TOIST_API int toist_kmeans(const float* banks, int64_t bank_stride, float* centers, int64_t centers_stride, const int32_t* group_task,
                 const int32_t* group_off, const int32_t* members, int n_groups, const float* features, int N, int D, int K, float tol,
                 int max_iter, int32_t* pick, float* chosen_center, int32_t* iters, void* stream);

/* ---- toist_kmeans with a start decided on the device (models/kmeans.py:8-18, `initialize`, and the `full_label == 0` test of kmeans.py:55-58):
 * the same Lloyd body.  full_label f32 [T] is the criterion's buffer, init_rows i32 [*, K] holds, per SAMPLE, the bank rows the host drew with
 * np.random.choice(N, K, replace=False) or -1.  Before a member's iterations: full_label[task] == 0 and init_rows[sample][0] >= 0 -> the centres are
 * those K rows of banks[task] (every member restarts from its own rows; same-task members stay in batch order); full_label[task] != 0 and a negative
 * row -> toist_kmeans' behaviour; the two disagree (or a row lies outside [0, N)) -> toist_kmeans' behaviour and bit 0 is OR-ed into *status (i32,
 * never cleared here).  Nothing in the launch arguments depends on the batch or on the fill state: the launch can be captured. */
TOIST_API int toist_kmeans_init(const float* banks, int64_t bank_stride, float* centers, int64_t centers_stride, const int32_t* group_task,
                 const int32_t* group_off, const int32_t* members, int n_groups, const float* features, int N, int D, int K, float tol,
                 int max_iter, int32_t* pick, float* chosen_center, int32_t* iters, const float* full_label, const int32_t* init_rows,
                 int32_t* status, void* stream);

/* ---- the prototype choice of a task sweep in one launch (ClusterCriterion.infer_choice, models/mdetr.py:282-312, over the P (image, caption) pairs
 * of toist_sweep_assemble; replaces its per-sample feature mean :240-260, memory_cluster :213-234 and the img_memory_mod clone + row writes :300-310).
 *   memory     bf16 [P, S, D], S = HW + L : the encoder output, read only          memory_mod bf16 [P, S, D] : holds a copy of memory on entry
 *   pair_caption i32 [P], live i32 [1]    : device tables; the pairs p >= *live are padding and are never looked at
 *   W_sth f32 [T, L], sub_sth u8 [T, L], cap_task i32 [T] : per CAPTION -- mean weights and marks of the tokens of the word 'something', task index
 *   group_task i32 [T]                    : the distinct tasks of the captions, one per slot, -1 (or anything outside [0, n_tasks)) = unused slot
 *   banks f32 [n_tasks, N, D] (stride bank_stride), centers f32 [n_tasks, K, D] (stride centers_stride, updated IN PLACE)
 * One 1024-thread workgroup per slot walks p = 0 .. *live-1 in ascending order and serves the pairs with cap_task[pair_caption[p]] == its task:
 *   features[p, d] = sum over l ascending of W_sth[c, l] * float(memory[p, HW + l, d]) -- fp32, every product formed and rounded, no contraction;
 *   toist_kmeans' iterations from the centres the task's previous pair left (tol, max_iter) and its nearest-centre pick; centers[task] stored back;
 *   memory_mod[p, HW + l, :] = bf16(centre[pick]) (round to nearest even) for every l with sub_sth[c, l].  Nothing else of memory_mod is written.
 * pair_caption[p] outside [0, T) is never used as an index: the pair is skipped and *status = max(*status, p + 1) (toist_sweep_assemble's word and
 * rule).  pick i32 [P], features f32 [P, D], iters i32 [P]: optional (NULL), written for served pairs only.  Limits: toist_kmeans', and L <= 256. */
TOIST_API int toist_sweep_prototypes(const void* memory, void* memory_mod, const int32_t* pair_caption, const int32_t* live, const float* W_sth,
                 const uint8_t* sub_sth, const int32_t* cap_task, const int32_t* group_task, const float* banks, int64_t bank_stride,
                 float* centers, int64_t centers_stride, int P, int HW, int L, int T, int n_tasks, int N, int D, int K, float tol, int max_iter,
                 int32_t* status, int32_t* pick, float* features, int32_t* iters, void* stream);

/* ---- FIFO update of the memory banks with its bookkeeping on the device (mdetr.py:85-97; update_count / full_label: mdetr.py:90-92).  Group g =
 * the n = group_off[g+1] - group_off[g] samples members[group_off[g] ..) of task t = group_task[g] (n_groups slots, n_groups <= B <= N), rows f32
 * [B, D] the new features by sample.  With label = full_label[t] as the launch finds it:
 *   label == 0 or fifo_when_full:  banks[t][:N-n] = banks[t][n:], banks[t][N-n:] = the group's rows in batch order, lsap_rows[g] = 0; and when
 *                                  label == 0: full_label[t] = 1 if update_count[t] > N (looked at BEFORE the add), then update_count[t] += n;
 *   otherwise:                     the bank stays, lsap_rows[g] = n (the nearest-replacement LSAP behind this launch takes the group);
 *   an unused slot (n == 0):       lsap_rows[g] = 0.
 * One workgroup owns a task's bank and counters; the overlapping move is ordered inside it (loads of a chunk, barrier, stores).  No host value in
 * the launch arguments: the launch can be captured. */
TOIST_API int toist_bank_fifo(float* banks, int64_t bank_stride, float* update_count, float* full_label, const int32_t* group_task,
                 const int32_t* group_off, const int32_t* members, int n_groups, const float* rows, int T, int B, int N, int D,
                 int fifo_when_full, int32_t* lsap_rows, void* stream);

/* ---- whole-head self-attention for short sequences (S <= 64 keys, head dim <= 64, % 8 == 0): the text encoder's attention
 * (RoBERTa over a 16-token caption: transformer.py:129-130 via transformers.RobertaSelfAttention) as ONE launch each way instead of
 * batched 16 x 16 GEMMs + softmax kernels.  q / k / v / ctx / gradients are per-head column slices of [B*S, ld*] bf16 buffers
 * (row b*S + s, feature h*dh + e); bq / bk / bv (optional, f32 [H*dh]) are the projection biases, added on load so the packed
 * q | k | v projection needs no epilogue vector; key_pad [B, S] u8 (1 = padding) or NULL; stats f32 [B*H, S, 2] = (row maximum,
 * 1 / row sum) written by fwd, read by bwd, which re-forms the probabilities and the dropout mask ((seed + *seed_dev, element)). */
TOIST_API int toist_attn_small_fwd(const void* q, int ldq, const void* kmat, int ldk, const void* v, int ldv, const uint8_t* key_pad, int B, int H, int S,
                         int dh, float scale, float drop_p, uint64_t seed, const uint64_t* seed_dev, void* ctx, int ldo, float* stats,
                         const float* bq, const float* bk, const float* bv, void* stream);
TOIST_API int toist_attn_small_bwd(const void* q, int ldq, const void* kmat, int ldk, const void* v, int ldv, const uint8_t* key_pad, int B, int H, int S,
                         int dh, float scale, float drop_p, uint64_t seed, const uint64_t* seed_dev, const float* stats, const void* dctx,
                         int lddo, void* dq, int lddq, void* dk, int lddk, void* dv, int lddv, const float* bq, const float* bk,
                         const float* bv, void* stream);

/* ---- 3x3 / stride 1 / pad 1 convolution with <= 32 channels on either side (mask-head stages at 160x160,
 * segmentation.py:176-241 lay5 / out_lay; HBM-bound): NHWC bf16 in / out, weights [w_co][3][3][w_ci] bf16.
 * dgrad = 0: out[p, co] = shift[co] + sum x[p + tap, ci] w[co, tap, ci] (+ res);  c_src = w_ci, c_out = w_co.
 * dgrad = 1: out[p, ci] = sum dy[p - tap, co] w[co, tap, ci] (+ res);             c_src = w_co, c_out = w_ci. */
TOIST_API int toist_conv3x3_small(int dgrad, const void* src, const void* w, const float* shift, const void* res, void* out, int n_img, int H, int W,
                        int c_src, int c_out, int w_co, int w_ci, void* stream);

/* weight gradient of the same convolutions: every one of toist_wgrad3x3_small_blocks() workgroups writes an fp32 partial
 * [c_out][9 * c_in] to ws; fold them with toist_splitk_reduce_batch (splits = blocks, M = c_out, N = 9 * c_in). */
TOIST_API int toist_wgrad3x3_small_blocks(void);
TOIST_API int toist_wgrad3x3_small(const void* dy, const void* x, float* ws, int n_img, int H, int W, int c_in, int c_out, void* stream);

/* ---- batched linear sum assignment on caller-supplied cost matrices ---------------------------------------------
 * scipy.optimize.linear_sum_assignment for the reference's other call sites (mdetr.py:100 memory-bank replacement on
 * an L1 cdist, mdetr.py:539 softkd matcher): problem p is the row-major fp32 matrix [rows[p], cols[p]] at
 * cost + offset[p]; min(rows, cols) pairs are written at row_idx / col_idx + out_off[p], rows ascending (SciPy's
 * order).  status[p]: 0 ok, 1 NaN or -inf in the matrix (SciPy: ValueError), 2 infeasible. */
TOIST_API int toist_lsap(const float* cost, const int64_t* offset, const int32_t* rows, const int32_t* cols, int ld /* row stride, 0 = cols[p] */,
               int n, int max_rows, int max_cols,
               int64_t max_cells /* max over problems of rows*cols: sizes the LDS */, const int64_t* out_off, int64_t* row_idx, int64_t* col_idx, int32_t* status, void* stream);

/* ---- deferred split-K reductions ------------------------------------------------------------------------
 * toist_gemm_bf16 with flags bit1 (TOIST_GEMM_DEFER_REDUCE) writes the k-slice partials to `workspace` and returns
 * without launching the reduction; the caller later folds up to many such GEMMs with ONE launch per 48 descriptors:
 *   out[m][n] (+)= alpha * rscale[m] * sum_s ws[s][m][n].
 * toist_gemm_effective_split tells how many slices the kernel really wrote (k-slices that would own no k-tile are
 * dropped).  `descs` is a HOST array (copied into the kernel arguments); nothing is kept after the call returns. */
#define TOIST_GEMM_DEFER_REDUCE 2
/* flags bit2: split_k > 1 with the COMPLETE epilogue.  The k-slices store raw f32 partial tiles to `workspace` ([k-slice][M][N]) as
 * for any split, and a second kernel adds them in slice order and applies scale / shift / dropout / residual / activation / the
 * output type exactly as the un-split GEMM would -- for nn.Linear GEMMs with few output tiles and a deep reduction (128 tokens,
 * K = 3072: 24 tiles on 256 CUs).  batch = 1, no group, no row map; N %% 4 == 0. */
#define TOIST_GEMM_SPLIT_EPILOGUE 4
/* flags bit 15: with split_k > 1 and no group, a_colsum is a [split][M] fp32 buffer that receives each k-slice's column sums (plain stores,
 * no atomics); the caller folds the slices in order (toist_splitk_reduce_batch with M = 1) -- a bias gradient that is the same in every run */
#define TOIST_GEMM_COLSUM_SLICES 32768
/* tile code toist_gemm_bf16 would run this descriptor on: the dispatcher's pick for `tile` = 0, for a forced `tile` its low byte -- or
 * 137 / 138 where a weight-gradient kernel replaces 129 / 130 / 134.  Answered for descriptors toist_gemm_bf16 would refuse, too. */
TOIST_API int toist_gemm_pick_tile(const toist_gemm* desc);
typedef struct toist_reduce_desc {
    const float* ws;          /* [splits][M][N] fp32 partials                */
    float* out;               /* [M][ldc] fp32                               */
    const float* rscale;      /* optional per-row scale [M]                  */
    int32_t splits, M, N, ldc;
    float alpha;
    int32_t accumulate;       /* 1: out += ..., 0: out = ...                 */
} toist_reduce_desc;          /* 48 bytes */
TOIST_API int toist_gemm_effective_split(const toist_gemm* desc);
TOIST_API int toist_splitk_reduce_batch(const toist_reduce_desc* descs, int n, void* stream);

/* ---- two chained 1x1 convolutions of a ResNet stage in one row-local launch (csrc/gemm.hip conv_pair_kernel): conv3 of bottleneck i and
 * conv1 of bottleneck i + 1 (torchvision Bottleneck as reached through /root/reference/models/backbone.py:75), or their data gradients
 * in the opposite order.  A workgroup owns 64 rows, finishes and stores them 4C wide, and multiplies the same rows again:
 *   dgrad = 0:  mid[M][4C] = relu(a[M][C] w_first^T + shift_mid + res),  w_first  bf16 [4C][C];   out[M][C] = relu(mid w_second^T + shift_out),  w_second bf16 [C][4C]
 *   dgrad = 1:  mid[M][4C] = (a[M][C] w_first + res) where aux_mid > 0,  w_first  bf16 [C][4C];   out[M][C] = (mid w_second) where aux_out > 0,  w_second bf16 [4C][C]
 * Both results are, bit for bit, what the two toist_gemm_bf16 calls they replace write for the same M (mid is rounded to bf16 before the
 * second product reads it).  C = 256 only; weights contiguous; every pointer 16-byte aligned, every leading dimension a multiple of 8
 * and at least the row's width; res is required; aux_mid / aux_out are required with dgrad = 1 and must be NULL with dgrad = 0; shift_mid
 * [4C] / shift_out [C] f32 are optional with dgrad = 0 and must be NULL with dgrad = 1. */
typedef struct toist_conv_pair {
    int32_t M, C;             /* rows; channels of a / out (mid has 4C) */
    int32_t dgrad;            /* 0 = forward pair, 1 = data-gradient pair */
    int32_t lda;
    const void* a;
    const void* w_first;
    const void* w_second;
    const float* shift_mid;
    const float* shift_out;
    const void* res;          /* bf16 [M][4C], row stride ldr */
    const void* aux_mid;      /* bf16 [M][4C], row stride ldaux_mid */
    const void* aux_out;      /* bf16 [M][C], row stride ldaux_out */
    void* mid;                /* bf16 [M][4C], row stride ldmid */
    void* out;                /* bf16 [M][C], row stride ldout */
    int32_t ldr, ldaux_mid, ldaux_out, ldmid, ldout, reserved;
} toist_conv_pair;            /* 120 bytes */
TOIST_API int toist_conv_pair_bf16(const toist_conv_pair* desc, void* stream);

TOIST_API int toist_opt_chunk_elems(void);
TOIST_API int toist_opt_sqnorm(const toist_opt_tensor* table, const int64_t* grads, const int32_t* chunks, int n_chunks, float* partial, void* stream);
TOIST_API int toist_opt_finish_norm(const float* partial, int n_chunks, float max_norm, float beta1, float beta2, toist_opt_state* state, void* stream);
/* veto_i32 / veto_f32: DEVICE tables of n_veto_i32 / n_veto_f32 (each 0 .. TOIST_OPT_MAX_VETO) device addresses; NULL only with a count of 0 */
TOIST_API int toist_opt_finish_norm_guarded(const float* partial, int n_chunks, float max_norm, float beta1, float beta2, toist_opt_state* state,
                        const int32_t* const* veto_i32, int n_veto_i32, const float* const* veto_f32, int n_veto_f32, void* stream);
TOIST_API int toist_opt_adamw_ema(const toist_opt_tensor* table, const int64_t* grads, const int32_t* chunks, int n_chunks,
                        const toist_opt_group* groups, const toist_opt_state* state, float beta1, float beta2, float eps,
                        float ema_decay, void* stream);
/* the same update issued by at most max_blocks workgroups (0 = one per chunk): a slim launch that shares the chip with other work -- the
 * late parameter groups of toist_amd.optim, updated beside the next forward pass */
TOIST_API int toist_opt_adamw_ema_blocks(const toist_opt_tensor* table, const int64_t* grads, const int32_t* chunks, int n_chunks,
                               const toist_opt_group* groups, const toist_opt_state* state, float beta1, float beta2, float eps,
                               float ema_decay, int max_blocks, void* stream);
/* The same two launches for tables that hold row-sparse gradients (toist_embed_bwd_sparse).  touched, hot: device tables parallel to grads, one
 * device address per tensor; chunk c of tensor i is chunk c of its toist_opt_chunk_elems() cut.
 *   touched[i]  0 = a dense gradient; else the gradient's `touched` bytes (owned by whoever writes the gradient): a clear byte means the chunk
 *               of the gradient is +0 throughout
 *   hot[i]      0 = tensor i always takes the dense path; else bytes owned by the optimizer: a clear byte means m and v of the chunk are +0
 *               throughout.  The update sets a chunk's byte whenever its gradient is dense or touched, and never clears one.
 * sqnorm stores +0 for an untouched chunk without loading it (what the loads would have summed to).  adamw_ema takes the COLD path on a chunk
 * that is neither touched nor hot: it loads p and ema only, runs the same arithmetic on zeros for g, m, v, stores p, ema and w, and stores m, v
 * (setting the hot byte) only where a result is not the bit pattern +0 -- a NaN clip coefficient or a non-finite lr poisons them as the dense
 * path does.  Every byte written equals what toist_opt_sqnorm / toist_opt_adamw_ema_blocks write.  touched = NULL (sqnorm) or touched = hot =
 * NULL (adamw_ema): exactly those entry points.  A skipped step (state.skipped) changes no hot byte either. */
TOIST_API int toist_opt_sqnorm_sparse(const toist_opt_tensor* table, const int64_t* grads, const int64_t* touched, const int32_t* chunks,
                               int n_chunks, float* partial, void* stream);
TOIST_API int toist_opt_adamw_ema_sparse(const toist_opt_tensor* table, const int64_t* grads, const int64_t* touched, const int64_t* hot,
                               const int32_t* chunks, int n_chunks, const toist_opt_group* groups, const toist_opt_state* state,
                               float beta1, float beta2, float eps, float ema_decay, int max_blocks, void* stream);

/* ---- evaluation masks (replaces PostProcessSegm's dense resizes, models/postprocessors.py:73-109, and what
 * datasets/coco_eval.py:307-332 asks of pycocotools: mask_util.encode, and maskUtils.iou / area inside COCOeval).
 * A binary mask [h, w] is a column-major bit plane: uint64 bits[mask][x][yw], yw < ceil(h/64), bit b of word yw = pixel
 * (y = 64*yw + b, x), bits beyond h zero -- RLE's pixel order (index x*h + y).  n <= 65535 masks per call.
 *   resize_pack : src [n, h0, w0] fp32 mask logits -> bilinear (align_corners false) to [max_h, max_w], its
 *                 [crop_h, crop_w] corner -> bilinear to [h, w], sigmoid(v) > threshold, packed
 *   pack/unpack : dense [n, h, w] bytes (non-zero = foreground; unpack writes 0/1)
 *   area        : foreground pixels per mask
 *   iou         : iou[d, g] (row-major double) = i / (iscrowd[g] ? area_dt[d] : area_dt[d] + area_gt[g] - i), 0 when i = 0
 *   rle_count   : column_transitions[m, x] = value changes inside column x, counted against the preceding pixel in RLE
 *                 order (the last pixel of column x-1; 0 before the first pixel)
 *   rle_emit    : positions[column_offset[m, x] ...] = pixel indices of those changes, ascending (column_offset = an
 *                 exclusive prefix sum of column_transitions over the flattened [n, w] array)
 *   rle_counts  : mask m owns positions[first_position[m] .. first_position[m+1]) and writes its
 *                 (transitions + 1) run lengths, zeros first, to counts[first_run[m] ...]  (= rleEncode's cnts) */
TOIST_API int toist_mask_resize_pack(const float* src, int n, int h0, int w0, int max_h, int max_w, int crop_h, int crop_w, int h, int w,
                           float threshold, uint64_t* bits, void* stream);
/* resize_pack for a whole batch in one launch that takes every size from the device (the batched form of PostProcessSegm's loop over the images,
 * models/postprocessors.py:86-107; nothing is read from the host, so the launch can sit in a captured hipGraph): src [batch, queries, h0, w0] fp32,
 * one first-resize size [max_h, max_w] for all images, table int64 [batch, 4] = (crop_h, crop_w, h, w) per image.  Image i writes its `queries`
 * planes [queries, w_i, ceil(h_i/64)] densely from word i * capacity_words of `bits`; the words behind them are left untouched.  The grid covers
 * [cap_h, cap_w]; capacity_words >= queries * cap_w * ceil(cap_h/64).  A table row that does not fit (h_i > cap_h, w_i > cap_w, crop outside
 * [max_h, max_w]) writes nothing: the caller checks its sizes on the host before the launch. */
TOIST_API int toist_mask_resize_pack_batch(const float* src, int batch, int queries, int h0, int w0, int max_h, int max_w, const int64_t* table,
                                 int cap_h, int cap_w, long long capacity_words, float threshold, uint64_t* bits, void* stream);
TOIST_API int toist_mask_pack(const uint8_t* dense, int n, int h, int w, uint64_t* bits, void* stream);
TOIST_API int toist_mask_unpack(const uint64_t* bits, int n, int h, int w, uint8_t* dense, void* stream);
TOIST_API int toist_mask_area(const uint64_t* bits, int n, int h, int w, uint32_t* area, void* stream);
TOIST_API int toist_mask_iou(const uint64_t* dt, int n_dt, const uint64_t* gt, int n_gt, const uint8_t* iscrowd, const uint32_t* area_dt,
                   const uint32_t* area_gt, int h, int w, double* iou, void* stream);
TOIST_API int toist_mask_rle_count(const uint64_t* bits, int n, int h, int w, int32_t* column_transitions, void* stream);
TOIST_API int toist_mask_rle_emit(const uint64_t* bits, int n, int h, int w, const int64_t* column_offset, uint32_t* positions, void* stream);
TOIST_API int toist_mask_rle_counts(const uint32_t* positions, const int64_t* first_position, const int64_t* first_run, int n, int h, int w,
                          uint32_t* counts, void* stream);

/* PostProcess for a whole batch in one launch (models/postprocessors.py:19-55): per (image, query) row
 *   scores [B, Q] f32        = 1 - softmax(pred_logits [B, Q, C])[-1], fp32 with the row maximum subtracted
 *   boxes  [B, Q, 4] f32     = pred_boxes (cx, cy, w, h) as (x0, y0, x1, y1), scaled by the image's (w, h, w, h)
 *   scores_refexp [B, Q] f32 = scores * sigmoid(pred_isfinal [B, Q])        (both NULL without the referring-expression head)
 * orig_sizes = DEVICE int64 [B, 2] rows (h, w).  *_bf16 != 0: that input holds bfloat16, else fp32.  The labels are the constant 1 (host side). */
TOIST_API int toist_postprocess(const void* pred_logits, int logits_bf16, const void* pred_boxes, int boxes_bf16, const void* pred_isfinal, int isfinal_bf16,
                      const int64_t* orig_sizes, int B, int Q, int C, float* scores, float* boxes, float* scores_refexp, void* stream);

/* COCOeval.evaluateImg over a batch of images (pycocotools cocoeval.py; reached from datasets/coco_eval.py:368-399).  Image i owns
 * detections [dt_offset[i], dt_offset[i+1]) (score-descending, already cut to maxDets[-1]), ground truth [gt_offset[i], gt_offset[i+1])
 * and the row-major [D_i, G_i] block of `iou` at iou_offset[i].  For every area range a = [lo, hi] and IoU threshold t:
 *   dt_match [A*T*dt_offset[i] + (a*T + t)*D_i + d] = ground-truth index matched by detection d (within the image), or -1
 *   dt_ignore[same index]                          = matched an ignored ground truth, or unmatched with its area outside the range
 *   gt_range_ignore[A*gt_offset[i] + a*G_i + g]    = gt_ignore[g] or its area outside the range
 * gt_taken (A*T bytes per ground truth) is scratch.  Offsets tables have n_images + 1 entries. */
TOIST_API int toist_coco_match(const double* iou, const int64_t* iou_offset, const double* dt_area, const int64_t* dt_offset, const double* gt_area,
                     const uint8_t* gt_ignore, const uint8_t* gt_crowd, const int64_t* gt_offset, int n_images, const double* area_ranges,
                     int n_ranges, const double* iou_thresholds, int n_thresholds, int32_t* dt_match, uint8_t* dt_ignore,
                     uint8_t* gt_range_ignore, uint8_t* gt_taken, void* stream);

/* The box side of COCOeval for a whole batch of PostProcess rows in one launch (csrc/evalbox.hip; datasets/coco_eval.py:291-305 convert_to_xywh, and
 * what pycocotools' computeIoU asks of maskApi.c bbIou): the piece between toist_postprocess and toist_coco_match.  Nothing is read from the host, so
 * the launch can sit in a captured hipGraph.  Row r < R owns scores [Q] f32 and boxes [Q, 4] f32 (x0, y0, x1, y1) -- toist_postprocess's outputs, read in
 * place -- and names its ground truth by row_slot[r] (int32), a slot of the STAGED ground truth of a whole evaluation: slot s owns entries
 * [slot_off[s], slot_off[s + 1]) of gt_xywh f64 [n_gt, 4] (x, y, w, h), gt_area f64 [n_gt] and gt_crowd u8 [n_gt]; slot_off = int64 [n_slots + 1].
 * With G = the size of the row's slot and D = min(Q, max_det) the row writes
 *   order    int32 [R, D]: the query index of its d-th kept detection -- stable, score-descending on the scores as doubles: NaN first (in index
 *                          order), ties (-0.0 equals 0.0) to the lower index, i.e. torch.sort(descending=True, stable=True)
 *   dt_score f64 [R, D]  : that query's score;  dt_area f64 [R, D]: (double)(x1 - x0) * (double)(y1 - y0), the differences formed in fp32
 *   iou      f64 [D, G] row-major at iou_off[r]: bbIou in double on (x0, y0, x1 - x0, y1 - y0) widened: da = dw * dh, ga = gw * gh,
 *                          w = min(dw + dx, gw + gx) - max(dx, gx), h likewise, i = w * h, u = gt_crowd ? da : da + ga - i; i / u where w > 0 and h > 0, else 0
 *   out_gt_area f64, out_gt_crowd u8 [G] at gt_off[r]: the slot's entries, contiguous per row as toist_coco_match reads them
 * iou_off / gt_off = DEVICE int64 [R + 1], built by the host per batch (exclusive prefix sums of D * G and G).  Every element of every row's extents
 * is written and nothing else.  The caller checks the tables on the host before the launch (slots in range, offsets that agree with the slot sizes);
 * the kernel never uses an out-of-range row_slot entry as an index: such a row, a row whose extents disagree with its slot, and a row whose extents
 * leave iou_cap / gt_cap (the element capacities of iou and of out_gt_area / out_gt_crowd) write order, dt_score and dt_area only.
 * Q <= TOIST_COCO_BOXES_MAX_Q (the scores of a row sit in LDS as doubles), checked on the host. */
#define TOIST_COCO_BOXES_MAX_Q 1024
TOIST_API int toist_coco_boxes(const float* scores, const float* boxes, int R, int Q, int max_det, const int32_t* row_slot, const int64_t* slot_off,
                     int n_slots, const double* gt_xywh, const double* gt_area, const uint8_t* gt_crowd, long long n_gt, const int64_t* iou_off,
                     const int64_t* gt_off, long long iou_cap, long long gt_cap, int32_t* order, double* dt_score, double* dt_area, double* iou,
                     double* out_gt_area, uint8_t* out_gt_crowd, void* stream);

/* The mask side of COCOeval for a whole batch of rows in one launch (csrc/evalrows.hip; datasets/coco_eval.py:307-332, and what pycocotools' computeIoU
 * asks of maskApi.c rleIou): the piece between toist_mask_resize_pack_batch / toist_coco_boxes and a second toist_coco_match.  Nothing is read from the
 * host, nothing is allocated and nothing synchronises, so the launch can sit in a captured hipGraph.  Row r < R owns Q column-major bit planes
 * [w_r][ceil(h_r / 64)] (the layout of csrc/evalmask.hip) from word r * capacity_words of `bits`, plane q at + q * w_r * ceil(h_r / 64) -- the buffer
 * toist_mask_resize_pack_batch fills; the words behind a row's Q planes are not the row's and are never read.  row_hw = int64 [R, 2] = (h, w) per row.
 * order int32 [R, D] = toist_coco_boxes' output: the query index of the row's d-th kept detection, so "segm" ranks as "bbox" does.  The row names its
 * ground truth by row_slot[r], a slot of the STAGED ground truth (slot_off int64 [n_slots + 1] as for toist_coco_boxes): entry n of the staged tables
 * owns the plane at word gt_plane_off[n] of gt_bits (gt_words words in all; gt_plane_off = int64 [n_gt + 1]), its popcount gt_parea[n] (u32 -- NOT the
 * annotation's "area") and its crowd flag gt_crowd[n]; slot_hw int32 [n_slots, 2] = the (h, w) of a slot's planes.  With G = the size of the row's slot:
 *   dt_area f64 [R, D]  : popcount of plane order[r, d]
 *   iou     f64 [D, G] row-major at iou_off[r]: i = popcount(dt & gt); 0.0 when i == 0, else (double)i / u with
 *                         u = gt_crowd ? (double)area_d : (double)area_d + (double)area_g - (double)i  -- toist_mask_iou's arithmetic, exact in any order
 * iou_off = DEVICE int64 [R + 1] (exclusive prefix sums of D * G), iou_cap = the element capacity of `iou`.  Every element of every row's extents is
 * written and nothing else.  The caller checks the tables on the host (coco_eval.mask_row_tables); the kernel never uses an unchecked value as an
 * index.  A row is BAD when h or w is not positive, Q * w * ceil(h / 64) exceeds capacity_words, its slot lies outside [0, n_slots), G > 0 and
 * slot_hw differs from (h, w), its extents disagree with the slot or leave iou_cap, a plane offset leaves gt_words, or an order entry lies outside
 * [0, Q): such a row writes dt_area only (0 for an entry whose plane it could not read) and no IoU, and reads nothing out of range.
 * Refused on the host before any launch: null tables, negative extents, D > Q, R > 65535.  R == 0 returns 0.
 * TOIST_COCO_MASKS_CHUNK_WORDS: the words of a detection plane one workgroup holds in LDS at a time (a plane is streamed from HBM once). */
#define TOIST_COCO_MASKS_CHUNK_WORDS 4096
TOIST_API int toist_coco_masks(const uint64_t* bits, long long capacity_words, const int64_t* row_hw, int R, int Q, int D, const int32_t* order,
                     const int32_t* row_slot, const int64_t* slot_off, int n_slots, const uint64_t* gt_bits, long long gt_words,
                     const int64_t* gt_plane_off, const int32_t* slot_hw, const uint32_t* gt_parea, const uint8_t* gt_crowd, long long n_gt,
                     const int64_t* iou_off, long long iou_cap, double* dt_area, double* iou, void* stream);

/* ---- image preparation on the device (replaces the host pipeline between the decoded uint8 image and the model's input: datasets/tdod.py:301-335,
 * datasets/transforms.py:18-59 crop, 62-80 hflip, 83-138 resize = PIL Image.resize(BILINEAR), 244-273 ToTensor / Normalize, and the padding + mask of
 * util/misc.py:185-209 NestedTensor.from_tensor_list).  One launch per batch; every size comes from the device, so the launch can sit in a captured
 * hipGraph.  `desc` = int32 [batch_cap, TOIST_PREP_DESC_WORDS], one row per image:
 *    0 src_off (bytes from `src`)   1 src_h   2 src_w   3 src_stride (bytes per row; uint8 HWC RGB)      4 flip (horizontal, applied first)
 *    5 crop_y  6 crop_x  7 crop_h  8 crop_w   (in the coordinates of the flipped source; the whole image when there is no crop)
 *    9 out_h  10 out_w  11 ksize_h  12 ksize_v   (`_h` = the horizontal pass crop_w -> out_w, `_v` = the vertical pass crop_h -> out_h)
 *   13 bounds_h  14 coef_h  15 bounds_v  16 coef_v   (int32 word offsets into `arena`)      17 dst_off (bytes from `dst_u8`)      18, 19 reserved
 * bounds = (first tap, tap count) per output index; coef = ksize int32 coefficients per output index with 22 fractional bits (Pillow's 8-bit
 * resampler: out = clip((2^21 + sum_j pixel[first + j] * k_j) >> 22, 0, 255), horizontal pass first, its uint8 result the vertical pass's input).
 * The grid covers [batch_cap, cap_h, cap_w].  A row with out_h = 0 is an empty slot; a row that does not fit the capacities (src_bytes, arena_words,
 * dst_bytes, cap_h, cap_w) is treated as one: the caller checks its sizes on the host before the launch.  Exactly one output mode:
 *   final        (out != NULL): out fp32 [batch_cap, 3, cap_h, cap_w] = lut[c][pixel] inside (out_h, out_w), 0 outside; mask bytes [batch_cap, cap_h,
 *                cap_w] = 0 inside, 1 outside.  The WHOLE capacity is written.  lut = fp32 [3, 256] = (v / 255 - mean[c]) / std[c].  cap_w % 4 == 0.
 *   intermediate (dst_u8 != NULL): image i as uint8 HWC [out_h, out_w, 3] at dst_u8 + dst_off; nothing else is written.  dst_u8 may be another part
 *                of the buffer `src` points into, as long as no image's output overlaps any image's source. */
#define TOIST_PREP_DESC_WORDS 20
TOIST_API int toist_image_prep(const uint8_t* src, long long src_bytes, const int32_t* desc, const int32_t* arena, long long arena_words, const float* lut,
                     int batch_cap, int cap_h, int cap_w, float* out, uint8_t* mask, uint8_t* dst_u8, long long dst_bytes, void* stream);

/* ---- target masks on the device (replaces what the host does to a target's masks: datasets/transforms.py:62-80 hflip, 118-138 resize =
 * F.interpolate(mode="nearest"), 18-59 crop, and the zero padding of util/misc.py:185-209).  Flip, nearest resize and crop are index maps: the host
 * composes an image's plan into one table of source rows and one of source columns; the launch gathers single bits of the ORIGINAL-size masks into
 * the bytes the mask losses read.  One launch per batch; every size comes from the device, so the launch can sit in a captured hipGraph.
 * `src` = the source masks, one bit per pixel: pixel x of a row is bit (x & 31) of 32-bit word (x >> 5) (numpy packbits, bitorder "little"), rows padded
 * to whole words, every mask 4-byte aligned.  `desc` = int32 [slots, TOIST_TMASK_DESC_WORDS], one row per slot:
 *    0 src_off (bytes from `src`, a multiple of 4)   1 src_h   2 src_w   3 src_stride_words (32-bit words per source row)
 *    4 out_h   5 out_w   (the prepared mask)      6 tab_y   7 tab_x   (int32 word offsets into `arena`)
 * tab_y[out_h] = the source row of every output row, tab_x[out_w] = the source column of every output column (the flip folded in); the targets of
 * an image share one pair.  An entry outside the source reads as 0.
 * dst = uint8 [slots, cap_h, cap_w], values 0 / 1.  The grid covers it.  A row with out_h = 0 is a DEAD slot: nothing of it is written.  Any other
 * slot is written completely: the gathered bit inside (out_h, out_w), 0 outside.  A row that does not fit the capacities (src_bytes, arena_words, cap_h,
 * cap_w) gives an all-zero slot: the caller checks its sizes on the host before the launch.  Any cap_w; 16-byte stores where a row's address allows. */
#define TOIST_TMASK_DESC_WORDS 8
TOIST_API int toist_target_masks(const uint8_t* src, long long src_bytes, const int32_t* desc, const int32_t* arena, long long arena_words, int slots,
                     int cap_h, int cap_w, uint8_t* dst, void* stream);

/* ---- polygon annotations on the device (replaces the host's rasteriser of an object's polygons: datasets/tdod.py:133-147 convert_coco_poly_to_mask =
 * pycocotools frPyObjects + decode + any(dim=2), i.e. maskApi.c rleFrPoly per polygon and the union per object).  The masks EQUAL the host's
 * (toist_amd/coco_eval.py: polygon_to_mask) bit for bit: the same fp64 operations in the same order, no fused multiply-add.  One launch per batch;
 * every size comes from the device, so the launch can sit in a captured hipGraph.  Three tables of int32 words:
 *   desc  [slots, TOIST_POLY_DESC_WORDS], one row per object slot:
 *      0 dst_off (bytes from `dst`, a multiple of 4; packed mode)   1 h   2 w   3 stride_words (32-bit words per packed row, >= ceil(w / 32))
 *      4 poly_first   5 poly_count   (records of `polys`)      6, 7 reserved
 *   polys [poly_cap, TOIST_POLY_REC_WORDS]: first vertex, vertex count of one polygon
 *   verts [vert_cap, 2]: x, y on rleFrPoly's 5x grid, int(5.0 * c + .5) computed by the host in float64 (the device never sees the coordinates)
 * The grid covers [slots, ceil(cap_w / TOIST_POLY_STRIP)]: a workgroup owns TOIST_POLY_STRIP columns of one object and holds them for up to
 * TOIST_POLY_MAX_ROWS rows in LDS; cap_h <= TOIST_POLY_MAX_ROWS.  A row with h = 0 is a DEAD slot: nothing of it is written.  A row that does not fit
 * the capacities (cap_h, cap_w, poly_cap, vert_cap, dst_bytes, the stride the grid covers) writes nothing either: the caller checks its sizes -- and
 * the trace steps of the batch, sum over the edges of max(|dx|, |dy|) on the grid, which is the launch's work -- on the host before the launch.
 *   TOIST_POLY_PACKED: the object's h rows of stride_words words at dst + dst_off, pixel x of a row = bit (x & 31) of little-endian word (x >> 5)
 *                      (the source format of toist_target_masks).  EVERY word of every row is written, pad bits as zeros; nothing else is.
 *   TOIST_POLY_DENSE : dst = uint8 [slots, cap_h, cap_w], values 0 / 1; the live h x w region of a slot is written completely, the rest is left alone. */
#define TOIST_POLY_DESC_WORDS 8
#define TOIST_POLY_REC_WORDS 2
#define TOIST_POLY_STRIP 64
#define TOIST_POLY_MAX_ROWS 2048
#define TOIST_POLY_PACKED 0
#define TOIST_POLY_DENSE 1
TOIST_API int toist_polygon_masks(const int32_t* desc, int slots, const int32_t* polys, int poly_cap, const int32_t* verts, int vert_cap, int cap_h,
                     int cap_w, uint8_t* dst, long long dst_bytes, int mode, void* stream);

/* ---- task sweep: T captions over B images as P (image, caption) pairs (replaces the three torch.cat of Transformer.encode_native,
 * toist_amd/transformer.py:559-565 = models/transformer.py:143-148 of the reference, for a batch whose rows are PAIRS: the image rows of pair p come
 * from image pair_image[p], the caption rows from caption pair_caption[p]).  One launch; the tables are DEVICE int32 [P], so a captured launch serves
 * any pairing.  With S = HW + L, all bf16 arrays 16-byte aligned, D % 8 == 0:
 *   img_tok, img_pos bf16 [B, HW, D], img_pad bytes [B, HW]; txt_tok bf16 [T, L, D], txt_pad bytes [T, L]
 *   tokens  bf16 [P, S, D] : rows 0 .. HW-1 = the pair's image rows, rows HW .. S-1 = its caption rows
 *   pos     bf16 [P, S, D] : rows 0 .. HW-1 = the pair's img_pos rows, rows HW .. S-1 = 0 (what PositionEmbeddingSine.tokens(mask, tail=L) writes)
 *   key_pad bytes [P, S]   : img_pad row | txt_pad row
 * A pure copy: EVERY output byte is written, every element is bit-equal to its source.  A table entry outside [0, B) / [0, T) is never used as an
 * index: that pair's tokens, pos and key_pad are zeros and *status = max(*status, p + 1) (int32, atomicMax; the caller zeroes and reads it). */
TOIST_API int toist_sweep_assemble(const void* img_tok, const void* img_pos, const uint8_t* img_pad, int B, int HW, const void* txt_tok,
                     const uint8_t* txt_pad, int T, int L, const int32_t* pair_image, const int32_t* pair_caption, int P, int D, void* tokens,
                     void* pos, uint8_t* key_pad, int32_t* status, void* stream);

/* The gradient of toist_sweep_assemble with respect to its token inputs, one launch (the shared-image training step, MDETR.encode_pairs):
 *   d_seq bf16 [P, S, D]  ->  d_img bf16 [B, HW, D], d_txt bf16 [T, L, D]
 *   d_img[i, s, :] = bf16( sum over p ascending with pair_image[p]   == i of float(d_seq[p, s,      :]) )
 *   d_txt[t, l, :] = bf16( sum over p ascending with pair_caption[p] == t of float(d_seq[p, HW + l, :]) )
 * One fp32 accumulator per element, pairs added in ascending order, ONE round-to-nearest-even at the end; no atomics: bit-reproducible.  EVERY
 * element of an output is written (no pair: zeros; P == 0: all zeros; no memset before the launch).  The tables are read from the device on every
 * launch; a pair with an entry outside [0, B) / [0, T) is never used as an index and adds to NEITHER output.  d_img or d_txt may be NULL (frozen
 * backbone / frozen text side): that half is skipped.  Same extent rules as the forward: D % 8 == 0, 16-byte aligned arrays, P*S < 2^31. */
TOIST_API int toist_sweep_assemble_bwd(const void* d_seq, const int32_t* pair_image, const int32_t* pair_caption, int P, int B, int HW, int T, int L,
                     int D, void* d_img, void* d_txt, void* stream);

/* Rows gathered by a pair table, one launch: dst[p, :] = src[pair_image[p], :] for p < P, rows of row_bytes bytes of ANY count and alignment (the
 * per-image key-padding bytes and lay1 terms that the mask head of a sweep needs per pair).  src [n_images, row_bytes], dst [P, row_bytes] bytes,
 * pair_image DEVICE int32 [P].  A pure copy: EVERY output byte is written.  An entry outside [0, n_images) is never used as an index: that row is
 * zeros and *status = max(*status, p + 1) (int32, atomicMax). */
TOIST_API int toist_sweep_gather(const void* src, const int32_t* pair_image, int n_images, int P, long long row_bytes, void* dst, int32_t* status,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TOIST_HIP_H */
