/*
 * reid_hip.h - C ABI of the MI355X (gfx950) re-ID embedding-and-matching engine.
 *
 * The reference (SuperbTUM/real-time-ReID-tracking) is pure Python and has no FFI
 * of its own; the entry points below are what a binding for its DeepSORT hot
 * path needs.  Each one cites the reference interface it
 * replaces.  INTEGRATION.md shows the ctypes stub a maintainer adds on the
 * reference side.
 *
 * Conventions
 *   - every function returns 0 (REID_OK) or a negative reid_status; the message
 *     for the calling thread is available from reid_last_error().
 *   - "host" entry points take plain host pointers, stage through library-owned
 *     device buffers and return after the result is in the caller's memory.
 *   - "_dev" entry points take device pointers (hipMalloc / torch.Tensor.data_ptr()),
 *     enqueue on the context's stream and return without synchronising.
 *   - outputs are caller-allocated; the library never frees caller memory.
 *   - one context per (process, device); a context is not thread-safe (the
 *     reference's caller is single-threaded: feature_extractor.py:48-53).
 *   - layouts: crops are NHWC uint8 (the DeepSORT caller's HxWx3 arrays);
 *     float images are NCHW fp32 (torch convention of the plugin surface);
 *     matrices are row-major fp32.
 */
#ifndef REID_HIP_H
#define REID_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct reid_ctx reid_ctx;

enum reid_status {
    REID_OK = 0,
    REID_ERR_ARG = -1,     /* bad argument (null pointer, bad size, unknown metric) */
    REID_ERR_HIP = -2,     /* a HIP runtime call failed */
    REID_ERR_STATE = -3,   /* e.g. embed before weights were loaded */
    REID_ERR_NOMEM = -4
};

/* distance definitions (metric argument) */
enum reid_metric {
    REID_METRIC_L2 = 0,        /* sqrt(clamp(|x|^2+|y|^2-2x.y, 1e-12))   reid/losses/utils.py:21-35 euclidean_dist */
    REID_METRIC_L2SQR = 1,     /* |x|^2+|y|^2-2x.y                        faiss METRIC_L2, reid/faiss_utils.py:56-118 */
    REID_METRIC_COS_HALF = 2,  /* (1 - x.y/(|x||y|))/2                    reid/losses/utils.py:12-18 cosine_dist */
    REID_METRIC_COS = 3,       /* 1 - x.y/(|x||y|)                        DeepSORT nn_matching cosine (MAX_DIST, deep_sort.yaml:3) */
    REID_METRIC_DOT = 4        /* x.y (similarity)                        reid/evaluate.py:58 score = gf @ q */
};

/* kernel classes for reid_profile_get() */
enum reid_kernel_kind {
    REID_K_CONV_GEMM = 0,   /* implicit-GEMM convolutions (the dominant kernel of the embed path) */
    REID_K_DIST_GEMM = 1,   /* N x M distance-matrix GEMM */
    REID_K_ELEMENTWISE = 2, /* norm / SE / pool / combine kernels */
    REID_K_SELECT = 3,      /* argmin / top-k / rank counting */
    REID_K_COUNT = 4
};

/* ---- runtime ---------------------------------------------------------------------------- */
const char* reid_last_error(void);
int reid_device_count(int* n);
/* one context per process and device; replaces `self.device` / `.to(device)` of feature_extractor.py:17,22 */
int reid_ctx_create(int device, reid_ctx** out);
int reid_ctx_destroy(reid_ctx* ctx);
/* run on an existing HIP stream (e.g. torch.cuda.current_stream().cuda_stream); NULL = the context's own stream */
int reid_ctx_set_stream(reid_ctx* ctx, void* hip_stream);
/* run on the HIP null (legacy default) stream - torch's default stream; its handle 0 means "own stream" to reid_ctx_set_stream */
int reid_ctx_set_null_stream(reid_ctx* ctx);
int reid_ctx_sync(reid_ctx* ctx);
/* hipDeviceSynchronize on the context's device: every stream, not only the context's (the timing bracket of bench.py; replaces
 * the torch.cuda.synchronize() a torch host would call around track_yolov5.py:178-253's loop) */
int reid_device_sync(reid_ctx* ctx);
/* The context's sticky fault word.  Kernels raise it when (a) in mode 2 an activation outside f16's range (or a NaN) reaches a
 * site that splits operands into [xh | xl'], or (b) in any mode a non-finite embedding leaves the neck - a checkpoint that
 * load_pretrained_weights (modification_tracking/reid_model_factory.py:158-210) accepted but this arithmetic cannot run.  While it
 * is set, every embed / frame entry point, reid_ctx_sync and reid_device_sync return REID_ERR_STATE (the synchronising embed
 * calls report a fault raised by their own work); reid_ctx_clear_fault drains the stream and resets it. */
int reid_ctx_clear_fault(reid_ctx* ctx);
/* crops per pass through the network, 1..4096; default 1024 (the measured-best size: a pass of 1024 crops fills every launch of the
 * network with whole rounds of tiles; activation working set = crops in the pass * 3.2 MB).  Swin passes are capped at 1024 images. */
int reid_ctx_set_chunk(reid_ctx* ctx, int crops_per_pass);
/* arithmetic of the convolution GEMMs:
 *   0 = exact fp32 (v_mfma_f32_32x32x2_f32) - the reference's arithmetic, the default;
 *   1 = fp16 storage / fp32 accumulate (activations and weights live in HBM as f16; north_star's 1e-3 cosine tolerance);
 *   2 = "fp32-class": fp32 storage, every convolution (and every Linear / convolution of the Swin trunk) as three
 *       v_mfma_f32_32x32x16_f16 per multiply on hi/lo-split operands (x = xh + xl, xh = f16(x), xl' = f16((x - xh) 2^11)) with fp32 accumulation - 22-bit operands, the
 *       dropped xl.wl term at 2^-22; held to mode 0's parity thresholds (tests/test_gpu_parity.py).  Operands must lie inside
 *       f16's range: |activation| < 65504, |weight| 2^11 < 65504 (any trained ResNet18-IBN-SE by a wide margin).  ENFORCED: mode 2
 *       is refused (REID_ERR_ARG naming the tensor) when the loaded checkpoint has a convolution / Linear weight outside the
 *       range, and so is loading such a checkpoint into a context already in mode 2; an activation outside the range raises the
 *       context's fault word (reid_ctx_clear_fault below). */
int reid_ctx_set_precision(reid_ctx* ctx, int mode);
/* The shared context of a process may hold the weights of BOTH backbones.  reid_ctx_set_precision(2) refuses when either loaded
 * checkpoint is outside the range; a host object that owns one of them asks here whether ITS checkpoint is the reason: arch 0 =
 * ResNet18-IBN-SE family, 1 = Swin; REID_OK when that checkpoint can run in `mode` (or none is loaded), REID_ERR_ARG + the
 * tensor's name otherwise.  reid_ctx_fault_peek: the sticky fault word without draining the stream or starting work (bit 0 range,
 * bit 1 non-finite embedding, bit 2 split-K rendezvous) - lets a caller tell a fault that predates its call from one it raised.
 * (No reference counterpart: the reference has one arithmetic, modification_deepsort/feature_extractor.py:15-29.) */
int reid_ctx_precision_ok(reid_ctx* ctx, int arch, int mode);
int reid_ctx_fault_peek(reid_ctx* ctx, int* bits);
/* optional side information of the NEXT embed call(s): one index per image, consumed in order by the passes that follow (n images
 * in total; n = 0 clears).  ResNet18-IBN-SE: the camera of every crop - SERse18_IBN.forward(x, cam) adds cam_factor *
 * cam_bias[cam] to the BNNeck output before the classifier (reid/backbones/SERes18_IBN.py:269-270); Swin: the view of every
 * image - SwinTransformer.forward(img, view_index) adds side_info_coeff * side_info_embedding[view] to the SFE output
 * (reid/backbones/swin_transformer.py:301-302).  The weight blob must carry the table (cam.bias + cam.factor / sfe.side +
 * sfe.side_coeff); an index outside it, or more images than indices, is REID_ERR_ARG. */
int reid_ctx_set_side_index(reid_ctx* ctx, const int32_t* index, int n);

/* device memory for hosts without torch */
int reid_malloc(reid_ctx* ctx, size_t bytes, void** dptr);
int reid_free(reid_ctx* ctx, void* dptr);
int reid_memcpy_h2d(reid_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int reid_memcpy_d2h(reid_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
/* pinned host memory: uploads from it are asynchronous DMAs (a copy from pageable memory blocks the caller until the
 * stream has drained) - where a tracker packs the crops it hands to reid_frame_submit */
int reid_host_alloc(reid_ctx* ctx, size_t bytes, void** out);
int reid_host_free(reid_ctx* ctx, void* p);

/* HIP-event timing on the context's stream (bench.py) */
int reid_timer_start(reid_ctx* ctx);
int reid_timer_stop(reid_ctx* ctx, float* elapsed_ms);      /* records, synchronises, returns elapsed */
/* per-kernel-class timing: when enabled every launch of the class is bracketed by HIP events */
int reid_profile_enable(reid_ctx* ctx, int on);
int reid_profile_reset(reid_ctx* ctx);
int reid_profile_get(reid_ctx* ctx, int kind, double* total_ms, long long* launches, double* flops, double* bytes);

/* ---- weights ----------------------------------------------------------------------------- */
/* Packed ResNet18-IBN-SE weights (reid_amd.weights.pack_seres18): one fp32 blob plus a text manifest of
 * "name offset count" lines.  Replaces torch.load + load_state_dict(strict=False), feature_extractor.py:18-19,
 * and load_pretrained_weights, modification_tracking/reid_model_factory.py:158-210. */
int reid_seres18_load(reid_ctx* ctx, const float* blob, size_t n_floats, const char* manifest);
int reid_seres18_dims(reid_ctx* ctx, int* embed_dim, int* num_class);

/* ---- embedding: Extractor.__call__, feature_extractor.py:48-53; SERse18_IBN.forward, SERes18_IBN.py:250-276 */
/* n crops already at 128x256: uint8[n][256][128][3] -> emb fp32[n][512] (BNNeck output), logits fp32[n][num_class] or NULL */
int reid_embed_u8(reid_ctx* ctx, const uint8_t* crops_nhwc, int n, float* emb, float* logits);
int reid_embed_u8_dev(reid_ctx* ctx, const uint8_t* d_crops_nhwc, int n, float* d_emb, float* d_logits);
/* crops of arbitrary size (feature_extractor.py:31-46 _preprocess: /255, bilinear resize to 128x256, (x-0.5)/0.5):
 * packed = concatenated HxWx3 uint8 images, offsets[i] = byte offset of crop i, hw[2i],hw[2i+1] = its height,width */
int reid_embed_ragged_u8(reid_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n,
                         float* emb, float* logits);
/* crops as windows frame[y1:y2, x1:x2] of ONE uint8 HxWx3 frame (what DeepSort._get_features slices before calling the
 * Extractor): the frame is uploaded once and each window is resized on the device.  boxes_xyxy int32[n][4], inside the
 * frame and non-empty (an empty slice fails in the reference's cv2.resize as well). */
int reid_embed_frame_u8(reid_ctx* ctx, const uint8_t* frame_hwc, int fh, int fw, const int32_t* boxes_xyxy, int n,
                        float* emb, float* logits);
/* reid_embed_frame_u8 at out_h x out_w: DeepSort._get_features' windows ([external] deep_sort.py) through Extractor._preprocess of an
 * extractor built at another size (feature_extractor.py:31-46).  Size, mean_std6 and refusals as reid_embed_ragged_u8_hw: (256, 128) is
 * reid_embed_frame_u8 (every architecture and mode, mean_std6 NULL or 0.5 / 0.5); any other size (sides 32 .. 512) runs seres18_ibn (with reid_ctx_set_hw_siblings 1 also cares18_ibn, with reid_ctx_set_hw_ema 1 also emares18_ibn) under the
 * reid_ctx_set_hw_precision rule, opened by the fused resize + stem + max-pool kernel of libreid_hip_anysize_front.so, which must lie
 * beside this library like libreid_hip_anysize.so (REID_ERR_STATE naming the missing file, before anything is queued).  The embeddings
 * are those of reid_embed_ragged_u8_hw on the same pixels, bit for bit. */
int reid_embed_frame_u8_hw(reid_ctx* ctx, const uint8_t* frame_hwc, int fh, int fw, const int32_t* boxes_xyxy, int n, int out_h, int out_w,
                           const float* mean_std6, float* emb, float* logits);
/* normalised float images, fp32[n][3][256][128] NCHW: the model(im_batch) call of the plugin surface
 * (modification_tracking/models/__init__.py:93-121 returned object) */
int reid_embed_f32_nchw(reid_ctx* ctx, const float* x, int n, float* emb, float* logits);
int reid_embed_f32_nchw_dev(reid_ctx* ctx, const float* d_x, int n, float* d_emb, float* d_logits);
/* intermediate activation of the last embed call, for stage-level parity tests:
 * stage 0 = stem conv+BN [n][128][64][64], 1 = maxpool [n][64][32][64], 2..9 = SE blocks 11..42 (NHWC), 10 = GeM [n][512].
 * Only valid when n <= chunk and after reid_ctx_set_debug_keep(ctx, 1).  Copies up to max_floats and returns the stage's element count in *count. */
int reid_ctx_set_debug_keep(reid_ctx* ctx, int on);   /* tests only: give every stage its own buffer; 1 also splits the
                                                        * fp16 stem into conv + pool kernels so that stage 0 exists,
                                                        * 2 keeps the production (fused) kernels: stage 0 is not written */
int reid_debug_stage(reid_ctx* ctx, int stage, float* out_host, size_t max_floats, size_t* count);
/* the same for the Swin backbone: stage 0 = ShadowFeatureExtraction output [n][H/4][W/4][96], 1..4 = the four stage outputs (NHWC),
 * 5 = GeM_1D output [n][96]; valid after a reid_swin_embed_* call that ran as one pass (n <= min(chunk, 1024)) */
int reid_debug_swin_stage(reid_ctx* ctx, int stage, float* out_host, size_t max_floats, size_t* count);

/* ---- Swin-T backbone (reference: reid/backbones/swin_transformer.py:339-427, swin_t :508-513; versions "v1" and "v2") ----
 * Packed weights from reid_amd.weights.pack_swin.  The manifest says which version the blob holds: the entry `swin.version` (one
 * float, 1 or 2; absent = 1).  v1 blocks (pre-norm, q.k / sqrt(32) + a 13x13 position table: `.pos`) or v2 blocks (:140-149,205-209,
 * 238-246: post-norm, cosine attention times a scale per head, plus a position bias per head - `.scale` [heads] already clamped and
 * exponentiated, `.bias` [heads][49][49] = meta_mlp evaluated by the packer).  reid_swin_load reads it; the embed calls, the mode-2
 * weight-range refusal and reid_ctx_precision_ok(ctx, 1, mode) serve both versions.  Input: normalised float images fp32[n][3][h][w] NCHW with h, w multiples
 * of 224 (the reference rejects 128x256); output: 96-d BatchNorm'd embedding (x_norm, :421) and logits. */
int reid_swin_load(reid_ctx* ctx, const float* blob, size_t n_floats, const char* manifest);
int reid_swin_dims(reid_ctx* ctx, int* embed_dim, int* num_class);
int reid_swin_embed_f32_nchw(reid_ctx* ctx, const float* x, int n, int h, int w, float* emb, float* logits);
int reid_swin_embed_f32_nchw_dev(reid_ctx* ctx, const float* d_x, int n, int h, int w, float* d_emb, float* d_logits);
/* The same model fed the way a tracker feeds it - the reference registers swin_transformer as a tracker ReID model
 * (modification_tracking/models/__init__.py:80, reid_model_factory.py:9) and its Extractor hands over uint8 crops of any size
 * (feature_extractor.py:31-53).  ragged: crops as for reid_embed_ragged_u8; frame: windows of one frame as for reid_embed_frame_u8
 * (DeepSort._get_features).  Each crop is resized (bilinear, the taps of the ResNet entry points) to out_h x out_w - multiples of 224;
 * the reference uses 224x224 and 448x224 - and normalised as (x / 255 - mean[c]) / std[c], mean_std6 = mean[3] then std[3] (std > 0),
 * NULL = ImageNet's 0.485, 0.456, 0.406 / 0.229, 0.224, 0.225 (reid/data_transforms.py:64).  Resize, normalisation and the stem's first
 * convolution are one kernel of libreid_hip_swin_crops.so, which must lie beside this library (REID_ERR_STATE naming it otherwise); the
 * result is bit-identical to reid_swin_embed_f32_nchw on the same crops preprocessed in fp32 on the host.  emb fp32[n][96], logits
 * fp32[n][num_class] or NULL.  Passes of min(chunk, the Swin pass cap) crops; with several, reid_swin_embed_ragged_u8 moves pass k + 1's
 * crops up and pass k - 1's embeddings down under pass k's kernels.  reid_ctx_set_side_index applies as to the float entries. */
int reid_swin_embed_ragged_u8(reid_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n, int out_h, int out_w,
                              const float* mean_std6, float* emb, float* logits);
int reid_swin_embed_frame_u8(reid_ctx* ctx, const uint8_t* frame_hwc, int fh, int fw, const int32_t* boxes_xyxy, int n, int out_h, int out_w,
                             const float* mean_std6, float* emb, float* logits);
/* The evaluation script's retrieval descriptor for this backbone - reid/image_reid_inference.py offers --backbone swin_v1 | swin_v2
 * beside seres18 | cares18 (:145-152, :202-208) and runs the Swin at 448x224 with ImageNet normalisation (data_transforms.py:78-84).
 * In eval mode SwinTransformer.forward returns (logits, x_norm) (swin_transformer.py:422-423; SERes18 returns (x_norm, logits)), and
 * inference_efficient concatenates normalize(first) | normalize(second), so a Swin row is [normalize(logits) (num_class) |
 * normalize(x_norm) (96)], the logits part FIRST: out fp32[n][num_class + 96].  flip_tta == 0: that row of the plain view, not
 * renormalised (as reid_descriptor_*); flip_tta != 0: normalize((d(x) + d(hflip x)) / 2) (:252-253).  normalize is F.normalize,
 * v / max(||v||, 1e-12).  The loaded v1 or v2 weights, every precision; h, w / out_h, out_w multiples of 224; passes of min(chunk, the
 * Swin pass cap) images.  With --sie the script passes an image's camera index as the view_index of both views (inference_efficient
 * :117-120, model(img, cam.repeat(2))): pending side indices (reid_ctx_set_side_index, n of them) apply to the plain AND the mirrored
 * view of the same image at every pass size, and nothing is left pending afterwards, also on error.
 * The mirrored view is never materialised: the stem reads the source with reversed columns, and one kernel runs the classifier of both
 * views in exact fp32, the four norms, the average and the renormalisation - the logits never reach memory.  In precisions 1 and 2 the
 * descriptor's logits therefore come from exact-fp32 arithmetic on x_norm, while the logits reid_swin_embed_* returns come from that
 * mode's GEMM.  These kernels are libreid_hip_swin_eval.so, which must lie beside this library.
 * ragged_u8: crops, out_h, out_w and mean_std6 as reid_swin_embed_ragged_u8; the mirror is taken AFTER the resize, the order of the
 * reference's transforms (Resize -> flip -> ToTensor -> Normalize); bit-identical to reid_swin_descriptor_f32_nchw on the same crops
 * resized and normalised in fp32 on the host.
 * Refused before anything is queued: no Swin weights, a blob without classifier, or a missing side library (REID_ERR_STATE, the latter
 * naming the file); a bad size or mean_std6, a side-index count other than n or an index outside the table, or more than 4096 classes
 * (the descriptor kernel's limit: both views' logits are held on chip) (REID_ERR_ARG).  n == 0 returns REID_OK. */
int reid_swin_descriptor_f32_nchw(reid_ctx* ctx, const float* x, int n, int h, int w, int flip_tta, float* out);
int reid_swin_descriptor_f32_nchw_dev(reid_ctx* ctx, const float* d_x, int n, int h, int w, int flip_tta, float* d_out);
int reid_swin_descriptor_ragged_u8(reid_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n, int out_h,
                                   int out_w, const float* mean_std6, int flip_tta, float* out);

/* ---- matching ----------------------------------------------------------------------------- */
/* out[m][n] = metric(x[m][d], y[n][d])        reid/losses/utils.py:12-35, reid/evaluate.py:58
 * Non-finite operands propagate as in the reference: every metric gives NaN where numpy / torch give NaN, REID_METRIC_L2 included (its
 * clamp(min=1e-12) keeps NaN); an all-zero row is 0 / 0 = NaN under the cosine metrics; REID_METRIC_DOT gives +-inf where the sum does. */
int reid_distmat(reid_ctx* ctx, const float* x, int m, const float* y, int n, int d, int metric, float* out);
int reid_distmat_dev(reid_ctx* ctx, const float* d_x, int m, const float* d_y, int n, int d, int metric, float* d_out);
/* The same matrix (reid/losses/utils.py:12-35, reid/evaluate.py:58) with the dot product in the fp32-class arithmetic on the f16 matrix
 * pipe (csrc/distmat_x3.hip in libreid_hip_distmat_x3.so, which must lie beside this library - without the file these
 * two calls are REID_ERR_STATE naming it and nothing else is affected).  Entry points of their own: no setting changes reid_distmat* or
 * anything built on it.
 * Arithmetic: xh = f16_rn(x), xl' = f16_rn((x - xh) 2^11), yh = f16_rn(y), yq = f16(yh 2^11), yl' = f16_rn((y - yh) 2^11) (f16 subnormals
 * kept); per 32 columns three f16 products into one fp32 accumulator in the order xh.yq, xl'.yh, xh.yl'; x.y = 2^-11 of it.  The squared
 * norms and the metric formulas are those of reid_distmat*: only the dot product differs.  K is never split: out[i][j] has the same bits
 * whatever m, n or its position.  The dot product carries the three roundings of the split (about 2^-21 sum_k |x_k y_k|, against 2^-24
 * per term of exact fp32) - an fp32-class value, NOT the bits of reid_distmat, and no rank (arg-min, top-k, CMC) is promised to agree
 * with the exact entry where two distances lie closer than both entries' errors.
 * Domain: |x| < 65504 and |y| 2^11 < 65504 (|y| < 31.98), every operand finite.  A value outside it raises the context's sticky fault
 * word (bit 0 of reid_ctx_fault_peek): reid_distmat_x3 returns REID_ERR_STATE and its output is invalid; reid_distmat_x3_dev is
 * asynchronous, there the next synchronising call (reid_ctx_sync) or the next entry reports it; it stays until reid_ctx_clear_fault, as
 * in mode 2.  L2 and L2SQR are symmetric: the caller may put the larger-ranged set on the x side and read the transpose.
 * Arguments as reid_distmat*: m == 0 or n == 0 returns REID_OK, a bad metric REID_ERR_ARG.  Profiling kind REID_K_DIST_GEMM. */
int reid_distmat_x3(reid_ctx* ctx, const float* x, int m, const float* y, int n, int d, int metric, float* out);
int reid_distmat_x3_dev(reid_ctx* ctx, const float* d_x, int m, const float* d_y, int n, int d, int metric, float* d_out);
/* per-row minimum of the distance matrix; ties -> lowest column index.  From 2048 rows of y on the selection runs in the
 * epilogue of the distance GEMM (csrc/dist_select.hip) and the m x n matrix is never written; smaller problems go through a
 * scratch matrix of a few MB.  evaluate.py:58-63 (the top-1 of `score`).
 * Distances that are NaN - one rule for reid_argmin_rows* and reid_knn*, whichever path a shape takes: a NaN distance, of either sign bit,
 * is NOT a candidate.  A row without any non-NaN distance answers idx = -1, val = NaN.  +inf and -inf are ordinary values (-inf is the
 * smallest); ties go to the lowest column. */
int reid_argmin_rows(reid_ctx* ctx, const float* x, int m, const float* y, int n, int d, int metric,
                     int32_t* idx, float* val);
int reid_argmin_rows_dev(reid_ctx* ctx, const float* d_x, int m, const float* d_y, int n, int d, int metric,
                         int32_t* d_idx, float* d_val);
/* brute-force squared-L2 k-NN: D fp32[nq][k] ascending, I int32[nq][k]; ties -> lowest index.  k <= 64 and nb >= 2048: fused
 * distance + selection (no nq x nb matrix), otherwise distance matrix tiles + a top-k pass.
 * A NaN distance is not a candidate (the rule at reid_argmin_rows): a row with fewer than k non-NaN distances - k > nb, or NaN in the
 * operands - is padded with (I = -1, D = +inf).  reid_rerank_jaccard skips such an index (csrc/rerank.hip checks 0 <= index < n).
 * The rule holds on every path, the wide one of large searches (csrc/knn_wide.hip) included: when a squared row norm is NaN or +inf - a
 * non-finite component, or finite ones whose square overflows fp32 - that path answers the whole call from exact fp32 distances (slow,
 * and the fused search's bits); no reid_knn* path raises the context's fault word.
 * search_raw_array_pytorch / IndexFlatL2.search, reid/faiss_utils.py:56-139 */
int reid_knn(reid_ctx* ctx, const float* xq, int nq, const float* xb, int nb, int d, int k, float* D, int32_t* I);
int reid_knn_dev(reid_ctx* ctx, const float* d_xq, int nq, const float* d_xb, int nb, int d, int k,
                 float* d_D, int32_t* d_I);
/* The per-row minimum (evaluate.py:58-63, the top-1 of `score`) with the CANDIDATES from the fp32-class arithmetic of reid_distmat_x3 on
 * the f16 matrix pipe and the ANSWER in exact fp32 (csrc/select_x3.hip in libreid_hip_select_x3.so, which must lie beside this library -
 * without the file these calls are REID_ERR_STATE naming it and nothing else is affected).  Contract: inside the domain idx and val are
 * the bits of reid_argmin_rows* - whatever m, n or the row's position, under all five metrics, ties to the lowest column.  The x3 kernel
 * keeps per row and column tile the keys below a per-row threshold (no m x n matrix is written), the best 32 are recomputed in exact
 * fp32 in the exact entry's summation order, and a row is answered from them only when its minimum lies strictly below what any other
 * column can reach (the threshold minus a bound on the difference of the two arithmetics); every other row is recomputed from all n
 * columns in exact fp32.  No row is answered approximately.
 * Domain: that of reid_distmat_x3 - finite operands, |x| < 65504, |y| < 31.98.  A value outside it raises the context's sticky fault word
 * (bit 0): the host entry returns REID_ERR_STATE and its output is invalid, the _dev entry reports it at the next synchronising call.
 * The NaN rule of reid_argmin_rows* is not claimed.  m == 0 or n == 0 returns REID_OK; a bad metric is REID_ERR_ARG before anything is
 * queued.  val / d_val may be NULL.  Entry points of their own: no setting changes reid_argmin_rows* or anything built on it. */
int reid_argmin_rows_x3(reid_ctx* ctx, const float* x, int m, const float* y, int n, int d, int metric, int32_t* idx, float* val);
int reid_argmin_rows_x3_dev(reid_ctx* ctx, const float* d_x, int m, const float* d_y, int n, int d, int metric, int32_t* d_idx,
                            float* d_val);
/* Brute-force squared-L2 k-NN (search_raw_array_pytorch / IndexFlatL2.search, reid/faiss_utils.py:56-139) the same way: candidates from
 * the fp32-class arithmetic, D and I the bits of reid_knn* inside the domain above, whatever nq, nb or the row's position; ties to the
 * lowest index; a row with nb < k is padded with (I = -1, D = +inf) as reid_knn pads.  1 <= k <= 24, anything else is REID_ERR_ARG before
 * anything is queued; nq == 0 or nb == 0 returns REID_OK.  Library, domain and fault reporting as reid_argmin_rows_x3*. */
int reid_knn_x3(reid_ctx* ctx, const float* xq, int nq, const float* xb, int nb, int d, int k, float* D, int32_t* I);
int reid_knn_x3_dev(reid_ctx* ctx, const float* d_xq, int nq, const float* d_xb, int nb, int d, int k, float* d_D, int32_t* d_I);
/* k-reciprocal Jaccard re-ranking, compute_jaccard_distance reid/faiss_utils.py:147-244: x fp32[n][d] L2-normalised rows,
 * rank int32[n][k1] neighbour lists or NULL (then reid_knn supplies them, self included), out fp32[n][n].
 * 1 <= k1 <= 64, k1 <= n, k2 >= 1 (k2 == 1 skips the local query expansion, as in the reference). */
int reid_rerank_jaccard(reid_ctx* ctx, const float* x, int n, int d, int k1, int k2, const int32_t* rank, float* out_nn);
int reid_rerank_jaccard_dev(reid_ctx* ctx, const float* d_x, int n, int d, int k1, int k2, const int32_t* d_rank,
                            float* d_out_nn);
/* DIoU of one tlwh box against m candidates, fp64, bit-exact with numpy   modification_deepsort/iou_matching.py:5-47 */
int reid_diou(reid_ctx* ctx, const double* box4, const double* cand_m4, int m, double* out_m);
/* cost[t][m] = 1 - DIoU(tracks[t], dets[m])   ([external] deep_sort iou_cost loop over iou()) */
int reid_diou_cost(reid_ctx* ctx, const double* tracks_t4, int t, const double* dets_m4, int m, double* out_tm);
/* ---- evaluation-script post-processing --------------------------------------------------- */
/* retrieval descriptor of reid/image_reid_inference.py:112-123,252-253: cat(normalize(emb), normalize(logits)) per image,
 * with flip_tta != 0 averaged with the horizontally mirrored image and renormalised.  x: fp32 [n][3][256][128] already
 * normalised by the caller's transform; out: fp32 [n][512 + num_class] (reid_seres18_dims). */
int reid_descriptor_f32_nchw(reid_ctx* ctx, const float* x, int n, int flip_tta, float* out);
int reid_descriptor_f32_nchw_dev(reid_ctx* ctx, const float* d_x, int n, int flip_tta, float* d_out);
/* The same descriptors from uint8 images as the dataset stores them: the evaluation script's own transform runs on the device.
 * reid/data_transforms.py:56-127 is transforms.Resize((H, W)) on an RGB PIL image - Pillow's 8-bit Image.resize((W, H), BILINEAR): two
 * passes of 22-bit fixed-point arithmetic with the support widened by the scale when an axis shrinks, the horizontal pass first into a
 * uint8 image, the vertical pass on that rounded image - then ToTensor and Normalize(mean, std); the mirrored view flips the resized
 * image (:130-209).  Integer arithmetic has one answer, so the resized image equals Pillow's byte for byte, and the normalised float is a
 * lookup in a [3][256] table (v / 255 - mean) / std built on the host in fp32 with two true divisions, the bits of torch's.
 * packed / offsets / hw: n RGB HWC images as reid_embed_ragged_u8 takes crops (image i is hw[2i] x hw[2i + 1] pixels at byte offsets[i] of
 * packed; images may share bytes and lie in any order); mean_std6 = mean[3] | std[3], NULL = ImageNet.  Host in, host out, passes
 * pipelined as the other host entries.
 *   reid_descriptor_images_u8       seres18 / cares18 / emares18: Resize((256, 128)); out fp32 [n][512 + num_class], in every precision
 *                                   bit-identical to reid_descriptor_f32_nchw on the same images preprocessed on the host (flip_tta: the
 *                                   resized image mirrored).  n pending side indices (the camera of each image) serve both views of
 *                                   an image, as the script's model(img, cam.repeat(2)): what that entry computes when it is given the
 *                                   indices twice; another count is REID_ERR_ARG.
 *   reid_swin_descriptor_images_u8  Swin v1 / v2: out_h, out_w multiples of 224 (the script: 448x224, or 224x224 for VeRi); out fp32
 *                                   [n][num_class + 96], bit-identical to reid_swin_descriptor_f32_nchw likewise; n pending side indices
 *                                   serve both views of an image.  Refusals as reid_swin_descriptor_ragged_u8.
 * Limits: 1 <= h, w <= 4096 per source image (pil_resize_max_side() of the side library; the int32 accumulator and the coefficient
 * tables are sized for it).  Workspace beyond the float entry's: per pass of p images the uint8 intermediates, sum of h_i * out_w * 3
 * bytes (at most p * 4096 * out_w * 3), the pass's fp32 images, p * 3 * out_h * out_w * 4 bytes, and the call's coefficient tables, at
 * most (2 * in + 5 * out) * 4 bytes per distinct (in, out) pair of an axis.  A larger source is REID_ERR_ARG naming the limit, an image
 * without pixels REID_ERR_ARG, both before anything is queued; n == 0 returns REID_OK; nothing pending stays pending.
 * The kernels are libreid_hip_pil_resize.so, which must lie beside this library (REID_ERR_STATE naming it otherwise). */
int reid_descriptor_images_u8(reid_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n, const float* mean_std6,
                              int flip_tta, float* out);
int reid_swin_descriptor_images_u8(reid_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n, int out_h, int out_w,
                                   const float* mean_std6, int flip_tta, float* out);
/* ---- ResNet18-IBN-SE at any input size ---------------------------------------------------- */
/* The network is fully convolutional with a GeM neck, and the evaluation script runs the ResNet family on VeRi at
 * Resize((224, int(ratio * 224))), ratio = the mean width / height of the dataset's images (reid/data_transforms.py:121,
 * reid/image_reid_inference.py:169-180) - a width such as 251 or 268; the tracker plug-in carries DeepSORT's (64, 128) beside (128, 256)
 * (modification_deepsort/feature_extractor.py:23-24).  The entries below are the entries of the same name without _hw with the input
 * size h x w (out_h x out_w: the size the uint8 sources are resized to) as arguments, each 32 .. 512, odd values allowed.
 *   (256, 128)   is handed to the existing entry: the same code path, the same bits, every architecture and precision mode.
 *   other sizes  a second forward, generic in H and W, for seres18_ibn weights in precision mode 0 (exact fp32): the convolutions on the
 *                generic implicit-GEMM kernel, InstanceNorm / SE / GeM for any number of pixels from libreid_hip_anysize.so, which must
 *                lie beside this library (REID_ERR_STATE naming it otherwise).  Another architecture or precision mode is REID_ERR_ARG
 *                naming both - nothing falls back (cares18_ibn runs with reid_ctx_set_hw_siblings 1, emares18_ibn with reid_ctx_set_hw_ema 1, below).  A pass is chunk * 256 * 128 / (h * w) images, clamped to 1 .. 4096, so it needs no
 *                more workspace than a pass of the 256 x 128 forward; results do not depend on the pass size.  Pending side indices
 *                (camera bias) apply as in the entries without _hw; reid_debug_stage reads the taps of the last pass, each
 *                [n][Ho][Wo][C] of its own map size.
 * reid_embed_ragged_u8_hw: the cv2-style bilinear resize of reid_embed_ragged_u8 to out_h x out_w, then (v - mean[c]) / std[c];
 * mean_std6 = mean[3] | std[3], NULL = 0.5 / 0.5 (the tracker's Normalize; at (256, 128) the only one).
 * reid_descriptor_images_u8_hw: Pillow's Resize((out_h, out_w)) as reid_descriptor_images_u8, bit-identical to
 * reid_descriptor_f32_nchw_hw on the same images preprocessed on the host; the mirrored view is read with reversed columns by the
 * layout kernel in front of the stem, no flipped copy of the batch is made.
 * Refused before anything is queued: a side outside 32 .. 512 (REID_ERR_ARG).
 *
 * reid_ctx_set_hw_precision(ctx, v): the arithmetic of that second forward, a setting of its own because the forward has kernels of its own.
 *   -1 (default)  the rule above: another size needs the context in mode 0.
 *    0            other sizes run exact fp32 whatever the context's mode.
 *    2            other sizes run fp32-class (the arithmetic of mode 2: hi/lo-split f16 operands on the matrix pipe, one fp32 accumulator,
 *                 fp32 storage) whatever the context's mode: the 3x3 and 1x1 convolutions of the trunk on any_conv_x3_kernel from
 *                 libreid_hip_anysize_x3.so, which must lie beside this library (REID_ERR_STATE naming it otherwise, on the first call at
 *                 another size); the 7x7 stem, the classifier, the max-pool and the tails stay exact fp32.  The activations are split in the
 *                 kernel's loader and a value outside f16's range raises REID_FAULT bit 0 as in mode 2.  A loaded ResNet checkpoint outside
 *                 the split range (|w| 2^11 >= 65504) makes the call fail with REID_ERR_ARG naming the tensor, as reid_ctx_set_precision(2)
 *                 does, and so does loading one while v == 2.
 *   Any other value is REID_ERR_ARG.  (256, 128) is not affected by v, and cares18_ibn / emares18_ibn stay refused at other sizes (cares18_ibn:
 *   unless reid_ctx_set_hw_siblings below is 1, emares18_ibn: unless reid_ctx_set_hw_ema below is 1, and then under this rule too). */
int reid_ctx_set_hw_precision(reid_ctx* ctx, int v);
/* reid_ctx_set_hw_siblings(ctx, on): CARes18-IBN at input sizes other than 256 x 128, a setting of its own because the refusal above is
 * what callers of the default see.
 *   0 (default)  as above: at another size every reid_*_hw entry refuses a loaded cares18_ibn / emares18_ibn, status and message unchanged.
 *   1            a loaded cares18_ibn runs at another size through the any-size forward with the TripletAttention block tail of
 *                libreid_hip_anysize_ca.so (csrc/anysize_ca.h: fp64 statistics, exact-fp32 gates and combine), which must lie beside this
 *                library (REID_ERR_STATE naming it otherwise, before anything is queued and before a frame slot is touched).  The size
 *                range (32 .. 512 per side), the reid_ctx_set_hw_precision rule (-1 needs mode 0, 0 exact fp32, 2 fp32-class convolutions
 *                with exact-fp32 stem and tails), the pass sizes and the side indices are those of seres18_ibn; every reid_*_hw entry,
 *                the _shift entries, reid_embed_frame_u8_hw and reid_frame_submit_hw follow.  emares18_ibn stays REID_ERR_ARG (its tail
 *                keeps a channel group's slab in LDS, which bounds the map): the message names it and says that only cares18_ibn has an
 *                any-size tail (emares18_ibn has a setting of its own, reid_ctx_set_hw_ema below).
 *   Any other value is REID_ERR_ARG.  (256, 128) is never affected. */
int reid_ctx_set_hw_siblings(reid_ctx* ctx, int on);
/* reid_ctx_set_hw_ema(ctx, on): EMARes18-IBN at input sizes other than 256 x 128, a setting of its own because the two refusals above are
 * what callers of the defaults see.
 *   0 (default)  as above: at another size every reid_*_hw entry refuses a loaded emares18_ibn, status and message unchanged (the message
 *                under reid_ctx_set_hw_siblings 1 included).
 *   1            a loaded emares18_ibn runs at another size through the any-size forward with the EMA block tail of
 *                libreid_hip_anysize_ema.so (csrc/anysize_ema.h: no slab in LDS, fp64 sums in a fixed order, fp32 convolutions and gates),
 *                whatever reid_ctx_set_hw_siblings is.  The library must lie beside this one (REID_ERR_STATE naming it otherwise, before
 *                anything is queued and before a frame slot is touched).  The size range (32 .. 512 per side), the
 *                reid_ctx_set_hw_precision rule (-1 needs mode 0, 0 exact fp32, 2 fp32-class convolutions with exact-fp32 stem and
 *                tails), the pass sizes and the side indices are those of seres18_ibn; every reid_*_hw entry, the _shift entries,
 *                reid_embed_frame_u8_hw and reid_frame_submit_hw follow.  cares18_ibn is not affected: it still needs
 *                reid_ctx_set_hw_siblings 1.
 *   Any other value is REID_ERR_ARG and changes nothing.  (256, 128) is never affected. */
int reid_ctx_set_hw_ema(reid_ctx* ctx, int on);
/* reid_ctx_set_hw_f16(ctx, on): ResNet18-IBN-SE at input sizes other than 256 x 128 in the fp16-storage arithmetic (f16 activations and
 * weights, fp32 accumulation on the matrix pipe, fp32 or wider statistics, gates, GeM and neck), a setting of its own because
 * reid_ctx_set_hw_precision refuses 1 and callers of that refusal keep it.
 *   0 (default)  as above: reid_ctx_set_hw_precision and the context's mode decide, every status and message unchanged.
 *   1            a loaded seres18_ibn runs at another size (32 .. 512 per side, odd sizes allowed) through the kernels of
 *                libreid_hip_anysize_f16.so (csrc/anysize_f16.h: stem on the matrix pipe, max-pool, implicit-GEMM trunk convolutions, IBN
 *                finish, SE tail, GeM + neck), whatever the context's mode and whatever reid_ctx_set_hw_precision is set to; the stored
 *                hw_precision keeps its value (its checkpoint rules too) and governs again once this setting is back at 0.  The library
 *                must lie beside this one (REID_ERR_STATE naming it otherwise, before anything is queued and before a frame slot is
 *                touched).  A loaded cares18_ibn / emares18_ibn at another size is REID_ERR_ARG whatever reid_ctx_set_hw_siblings /
 *                reid_ctx_set_hw_ema are: the message names the architecture and says that the fp16-storage any-size forward serves
 *                seres18_ibn only.  The size range, the pass sizes and the side indices are unchanged; every reid_*_hw entry, the _shift
 *                entries, reid_embed_frame_u8_hw and reid_frame_submit_hw follow (the frame entries through resize + normalise and the
 *                f16 stem: libreid_hip_anysize_front.so is not needed).  The camera bias and the classifier stay fp32;
 *                reid_debug_stage returns the f16 taps widened to fp32, each at its own map size.
 *   Any other value is REID_ERR_ARG and changes nothing.  (256, 128) is never affected. */
int reid_ctx_set_hw_f16(reid_ctx* ctx, int on);
/* reid_ctx_set_hw_sib_f16(ctx, on): CARes18-IBN (reid/backbones/CARes18.py) and EMARes18-IBN (reid/backbones/EMA_Res18.py) at input sizes
 * other than 256 x 128 in the fp16-storage arithmetic, a setting of its own because reid_ctx_set_hw_f16 1 refuses a loaded sibling and
 * callers of that refusal keep it.
 *   0 (default)  as above: every status, message and bit unchanged, the refusal of a sibling under reid_ctx_set_hw_f16 1 included.
 *   1            a loaded cares18_ibn / emares18_ibn runs at another size (32 .. 512 per side) in fp16 storage with fp32 accumulation: stem,
 *                max-pool, convolutions, IBN finish and GeM + neck of libreid_hip_anysize_f16.so, the TripletAttention / EMA block tail of
 *                libreid_hip_anysize_sib_f16.so (csrc/anysize_sib_f16.h: fp64 statistics in a fixed order, fp32 gates, one f16 rounding at
 *                the store) - whatever the context's mode, reid_ctx_set_hw_precision, reid_ctx_set_hw_siblings, reid_ctx_set_hw_ema and
 *                reid_ctx_set_hw_f16 are; those keep their values and govern again once this setting is back at 0.
 *                libreid_hip_anysize.so, libreid_hip_anysize_f16.so and libreid_hip_anysize_sib_f16.so must lie beside this library
 *                (REID_ERR_STATE naming the missing one otherwise, before anything is queued and before a frame slot is touched).  The size
 *                range, the pass sizes and the side indices are those of seres18_ibn; every reid_*_hw entry, the _shift entries,
 *                reid_embed_frame_u8_hw and reid_frame_submit_hw follow (the frame entries through resize + normalise and the f16 stem).
 *                A loaded seres18_ibn is not affected.
 *   Any other value is REID_ERR_ARG and changes nothing.  (256, 128) is never affected. */
int reid_ctx_set_hw_sib_f16(reid_ctx* ctx, int on);
int reid_embed_f32_nchw_hw(reid_ctx* ctx, const float* x, int n, int h, int w, float* emb, float* logits);
int reid_embed_f32_nchw_hw_dev(reid_ctx* ctx, const float* d_x, int n, int h, int w, float* d_emb, float* d_logits);
int reid_embed_ragged_u8_hw(reid_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n, int out_h, int out_w,
                            const float* mean_std6, float* emb, float* logits);
int reid_descriptor_f32_nchw_hw(reid_ctx* ctx, const float* x, int n, int h, int w, int flip_tta, float* out);
int reid_descriptor_f32_nchw_hw_dev(reid_ctx* ctx, const float* d_x, int n, int h, int w, int flip_tta, float* d_out);
int reid_descriptor_images_u8_hw(reid_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n, int out_h,
                                 int out_w, const float* mean_std6, int flip_tta, float* out);
/* ---- the evaluation chain's shifted mirrored view and attribute distance --------------------- */
/* For --backbone seres18 / cares18 the script's second view is get_inference_transforms_flipped(..., strong_inference=True)
 * (reid/image_reid_inference.py:179-181, reid/data_transforms.py:130-191): Resize -> RandomHorizontalFlip(p=1) -> Pad(10) ->
 * RandomCrop((H, W)) -> ToTensor -> Normalize - the mirrored image shifted by up to +-pad pixels on each axis over a black border, which
 * Normalize turns into (0 - mean) / std.  The entries below are reid_descriptor_f32_nchw_hw* / reid_descriptor_images_u8_hw with
 * flip_tta = 1 and that second view: with (top, left) = shift_tl[2 i], shift_tl[2 i + 1] of image i (a HOST int32 [n][2], in the _dev
 * entry too; RandomCrop.get_params' (i, j)),
 *     sy = oy + top - pad;  sx = ox + left - pad;   view[c][oy][ox] = (0 <= sy < h && 0 <= sx < w) ? x[c][sy][w - 1 - sx] : fill3[c],
 * exactly crop(pad(mirror(x))); (top, left) == (pad, pad) is the plain mirror and then the bits of flip_tta = 1.  Size, architecture,
 * precision, hw_precision, pending side indices (they serve both views), pass sizes and every refusal are those of the entries without
 * _shift: (256, 128) runs every architecture in every mode, another size seres18_ibn (and, with reid_ctx_set_hw_siblings 1,
 * cares18_ibn, with reid_ctx_set_hw_ema 1 emares18_ibn) under the hw_precision rule.  The view is pure data
 * movement (shift_mirror_nchw_kernel of libreid_hip_eval_links.so, which must lie beside this library - without the file these calls are
 * REID_ERR_STATE naming it, before anything is queued, and nothing else is affected): at 256 x 128 it writes the workspace the plain
 * mirror is written to, at another size a shifted copy of the pass on which the any-size forward runs unmirrored.
 * reid_descriptor_images_u8_shift pads with the normalisation table's entry for pixel value 0 per channel, (0 / 255 - mean) / std in the
 * table's own arithmetic: Pad(fill=0) on the 8-bit image followed by ToTensor + Normalize.
 * REID_ERR_ARG before anything is queued: fill3 == NULL (float entries), pad outside 0 .. 32, a shift outside [0, 2 pad] (the message
 * names the image index). */
int reid_descriptor_f32_nchw_shift(reid_ctx* ctx, const float* x, int n, int h, int w, const int32_t* shift_tl, int pad, const float* fill3,
                                   float* out);
int reid_descriptor_f32_nchw_shift_dev(reid_ctx* ctx, const float* d_x, int n, int h, int w, const int32_t* shift_tl, int pad,
                                       const float* fill3, float* d_out);
int reid_descriptor_images_u8_shift(reid_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n, int out_h,
                                    int out_w, const float* mean_std6, const int32_t* shift_tl, int pad, float* out);
/* For --dataset market1501 the script adds get_attribute_dist(labels, path) to the Jaccard matrix before DBSCAN
 * (reid/image_reid_inference.py:276-289, reid/tricks/additional_market_attributes.py:11-38): euclidean_dist (reid/losses/utils.py:21-35)
 * of the normalised 30-wide attribute rows with themselves.  In place on inout fp32 [n][n], a fp32 [n][d], 1 <= d <= 32:
 *     inout[i][j] += sqrt(max(s_i + s_j - 2 a_i.a_j, 1e-12)),   s_i the squared norm of row i in fp32,
 * one read and one write of the matrix and no second matrix (dist_add_l2_kernel of libreid_hip_eval_links.so; without the file
 * REID_ERR_STATE naming it).  The dot product and the norms are ascending-k fp32 FMA chains and s_i + s_j one fp32 add, so the term is
 * symmetric bit for bit.  n == 0 is REID_OK, d outside 1 .. 32 REID_ERR_ARG; a NaN in a propagates, as in reid_distmat (the clamp keeps
 * it).  d_inout must be 16-byte aligned. */
int reid_distmat_add_l2(reid_ctx* ctx, const float* a, int n, int d, float* inout);
int reid_distmat_add_l2_dev(reid_ctx* ctx, const float* d_a, int n, int d, float* d_inout);
/* diminish_camera_bias, reid/inference_utils.py:5-15, in place on x fp32 [n][d]: per camera id c (cams is a host int32[n],
 * ids >= 0) rows X_c <- normalize_rows((X_c - mean X_c) inverse(X_c^T X_c + n_c*la*I)^T).  The inverse is a Newton-Schulz
 * iteration of fp32 GEMMs that stops when the residual reaches the fp32 noise floor (iters = upper bound, <= 0: 40); behind a
 * finished inverse X the projected rows Y = C X (C the centred rows) take two rounds of residual correction Y <- Y + (C - Y A) X,
 * which removes the kappa^2 eps cancellation of C X alone.  An iteration cut short by `iters` is projected as it stands.
 * la > 0 (anything else, NaN included, is REID_ERR_ARG).  Supported range: condition number kappa of X_c^T X_c + n_c*la*I up to
 * 3e4 - any la, row scale or camera size that stays below it -, where every element is within 8x the error of the reference's own
 * arithmetic (fp32 LAPACK inverse) of the float64 result (tests/test_gpu_postproc.py; measured 0.7x - 3.3x).  Above 3e4 fp32
 * LAPACK itself is off by 1e-2 and nothing is promised.  A camera with a single row is 0 / 0 = NaN, as in the reference. */
int reid_cam_debias(reid_ctx* ctx, float* x, const int32_t* cams, int n, int d, float la, int iters);
int reid_cam_debias_dev(reid_ctx* ctx, float* d_x, const int32_t* cams, int n, int d, float la, int iters);
/* smooth_tracklets, reid/inference_utils.py:18-27, in place on x fp32 [n][d]: every row with valid[i] != 0 (valid NULL = all)
 * becomes keep * row + (1 - keep) * mean of the valid rows that share its sequence id (keep = 0.1 in the reference).
 * seqs / valid are host arrays. */
int reid_smooth_tracklets(reid_ctx* ctx, float* x, const int32_t* seqs, const uint8_t* valid, int n, int d, float keep);
int reid_smooth_tracklets_dev(reid_ctx* ctx, float* d_x, const int32_t* seqs, const uint8_t* valid, int n, int d, float keep);
/* ---- DeepSORT appearance metric with the feature bank on the device ---------------------------
 * [external] deep_sort/sort/nn_matching.py NearestNeighborDistanceMetric (the per-frame consumer of Extractor.__call__;
 * MAX_DIST / NN_BUDGET from modification_deepsort/deep_sort.yaml:3,9).  A bank holds, per track slot, the last `budget`
 * d-dimensional features in HBM; the caller maps track ids to slots 0..max_tracks-1. */
typedef struct reid_bank reid_bank;
int reid_bank_create(reid_ctx* ctx, int max_tracks, int budget, int d, reid_bank** out);
int reid_bank_destroy(reid_bank* bank);   /* before reid_ctx_destroy of its context */
/* partial_fit: row i of feats[n][d] is appended to track slots[i], in call order (oldest samples fall out of the ring) */
int reid_bank_update(reid_ctx* ctx, reid_bank* bank, const float* feats, const int32_t* slots, int n);
int reid_bank_update_dev(reid_ctx* ctx, reid_bank* bank, const float* d_feats, const int32_t* slots, int n);
/* forget tracks (targets missing from active_targets) so their slots can be reused */
int reid_bank_clear(reid_ctx* ctx, reid_bank* bank, const int32_t* slots, int n);
/* samples currently held for a slot (<= budget) */
int reid_bank_count(reid_bank* bank, int slot, int* out);
/* distance(): cost[t][m] = min over the samples of track slots[t] of metric(sample, dets[m]); metric REID_METRIC_COS
 * (_nn_cosine_distance) or REID_METRIC_L2SQR (_nn_euclidean_distance).  max_dist >= 0 also applies
 * linear_assignment.min_cost_matching's gate: cost > max_dist -> max_dist + 1e-5.  slots is a host array. */
int reid_bank_cost(reid_ctx* ctx, reid_bank* bank, const int32_t* slots, int t, const float* dets, int m, int metric,
                   float max_dist, float* out_tm);
int reid_bank_cost_dev(reid_ctx* ctx, reid_bank* bank, const int32_t* slots, int t, const float* d_dets, int m, int metric,
                       float max_dist, float* d_out_tm);
/* ---- one DeepSORT frame as asynchronous stages with a single wait ------------------------------
 * [external] deep_sort.py DeepSort.update: _get_features (Extractor.__call__, feature_extractor.py:48-53) -> Tracker.update
 * -> metric.distance + iou_cost -> metric.partial_fit.  `slot` (0 / 1) names one of two frame slots that own their crops,
 * embeddings and result staging: call cost(f), submit(f+1), fetch(f), <assign on the host>, update(f) and the device
 * embeds frame f+1 while the host assigns frame f.
 * submit (asynchronous): crops as for reid_embed_ragged_u8; `packed` must stay untouched until the slot's reid_frame_fetch
 *   returns (offsets / hw are copied).  m == 0 is allowed.
 * cost (asynchronous): appearance cost as reid_bank_cost over track slots[t] (bank NULL: skipped), DIoU cost as
 *   reid_diou_cost over tlwh boxes tracks_t4[t] / dets_m4[m] (NULL: skipped), embeddings when want_emb != 0.  The full
 *   t x m matrices serve every subset the matching cascade asks for.
 * fetch (waits for the slot's cost stage only): emb fp32[m][d], cost_tm fp32[t][m], iou_tm fp64[t][m]; NULL = not wanted.
 * update (asynchronous): partial_fit with row rows[i] of the slot's embeddings appended to track slots[i].
 * A slot remembers the width d of its embeddings - 512 after reid_frame_submit, the loaded Swin's embed_dim (96) after
 * reid_frame_submit_swin - and cost / fetch / update work at that width: a bank of another width is REID_ERR_ARG naming both. */
int reid_frame_submit(reid_ctx* ctx, int slot, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int m);
/* submit for the reference's swin_transformer tracker model (modification_tracking/models/__init__.py:80, reid_model_factory.py:9; the
 * frame's crops as Extractor.__call__ gets them from DeepSort._get_features, feature_extractor.py:31-53): as reid_frame_submit -
 * asynchronous, the same slot state, uploads and stream order - with the forward of reid_swin_embed_ragged_u8 on the loaded v1 / v2
 * weights in the context's precision, in passes of min(chunk, the Swin pass cap) crops.  out_h, out_w (multiples of 224) and mean_std6
 * (NULL = ImageNet) as there; mean_std6 is read before the call returns.  reid_ctx_set_side_index applies as to the other Swin entries.
 * The slot's cost stage then runs bank_cost96_kernel of libreid_hip_bank96.so, which must lie beside this library like
 * libreid_hip_swin_crops.so.  Refused before anything is queued or the slot is touched: no Swin weights or a missing side library
 * (REID_ERR_STATE, naming the file), a bad size or mean_std6 (REID_ERR_ARG). */
int reid_frame_submit_swin(reid_ctx* ctx, int slot, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int m, int out_h,
                           int out_w, const float* mean_std6);
/* submit for a tracker whose Extractor resizes to another crop size than 256 x 128 (feature_extractor.py:31-46 with `size=`; DeepSORT's
 * own 128 x 64, the evaluation script's VeRi geometry, image_reid_inference.py:169-180): as reid_frame_submit - asynchronous, the same
 * slot state, uploads and stream order, 512-wide embeddings - with the forward of reid_embed_ragged_u8_hw in passes of the same size,
 * opened by the fused front end of libreid_hip_anysize_front.so.  out_h, out_w, mean_std6 (read before the call returns) and every
 * refusal as reid_embed_frame_u8_hw; (256, 128) is reid_frame_submit.  Refused before anything is queued or the slot is touched. */
int reid_frame_submit_hw(reid_ctx* ctx, int slot, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int m, int out_h, int out_w,
                         const float* mean_std6);
int reid_frame_cost(reid_ctx* ctx, int slot, reid_bank* bank, const int32_t* slots, int t, int metric, float max_dist,
                    const double* tracks_t4, const double* dets_m4, int want_emb);
int reid_frame_fetch(reid_ctx* ctx, int slot, float* emb, float* cost_tm, double* iou_tm);
/* K camera streams batched into ONE pass per frame time (track_yolov5.py:178-253 runs one such loop per video; a frame of ~30
 * crops leaves most of the chip idle, K cameras' frames in one forward do not): submit the cameras' crops one camera after the
 * other (m_counts[g] crops of camera g, sum = the slot's m), then this cost stage in place of reid_frame_cost - camera g's
 * t_counts[g] tracks (slots / tracks_t4: the groups' concatenations, on banks[g]) against ITS detections only.  reid_frame_fetch
 * then returns, in cost_tm / iou_tm, the groups' t_g x m_g blocks one after the other; reid_frame_update takes slot-wide rows. */
int reid_frame_cost_groups(reid_ctx* ctx, int slot, int groups, reid_bank* const* banks, const int32_t* t_counts,
                           const int32_t* m_counts, const int32_t* slots, int metric, float max_dist, const double* tracks_t4,
                           const double* dets_m4, int want_emb);
/* multi-GPU frames (every rank embeds its round-robin share of the frame's crops): between submit and
 * cost, gather the ranks' embeddings into the slot as equal blocks of per = ceil(n / world) rows - one ncclAllGather; the slot
 * then holds world * per rows (row r * per + i = detection r + i * world; rows past a rank's share are padding) on every rank.
 * Asynchronous; without a communicator (reid_comm_init) a no-op.  For slots of reid_frame_submit (512-wide rows): REID_ERR_ARG after
 * reid_frame_submit_swin. */
int reid_frame_gather(reid_ctx* ctx, int slot, int per);
int reid_frame_update(reid_ctx* ctx, int slot, reid_bank* bank, const int32_t* rows, const int32_t* slots, int n);
/* Look-ahead streams (a video file / detection dump whose detections are known F frames ahead: F frames' crops are submitted as one
 * slot, their cost / update stages follow frame by frame): on != 0 moves the cost and update stages of THIS context's frame pipeline
 * to a stream of their own, ordered against the forwards by events, so that a group's serial cost -> assign -> update chain runs
 * beside the next group's forward.  While it is on, the context's banks must be driven through reid_frame_cost* / reid_frame_update
 * only.  Synchronises the context.  ([external] deep_sort.py DeepSort.update is strictly frame by frame: no counterpart.) */
int reid_frame_match_stream(reid_ctx* ctx, int on);
/* retrieval evaluation, reid/evaluate.py:33-105: for every query the ranks of its good gallery items among
 * non-junk items (descending similarity gf@q).  cmc_sum int32[ng] = sum over valid queries of the CMC step,
 * ap double[nq], valid int32[nq] (0 when the query has no good item).  Order: np.argsort(score, kind="stable")[::-1] (NaN
 * first, equal scores by higher gallery index first).  REID_ERR_ARG for a query with more than 2048 good items, and for a query
 * labelled -1 while gallery items labelled -1 lie in other cameras. */
int reid_rank_eval(reid_ctx* ctx, const float* qf, const int64_t* ql, const int64_t* qc, int nq,
                   const float* gf, const int64_t* gl, const int64_t* gc, int ng, int d,
                   int32_t* cmc_sum, double* ap, int32_t* valid);
/* the same with the features already on the device (labels and results stay host arrays; synchronises) */
int reid_rank_eval_dev(reid_ctx* ctx, const float* d_qf, const int64_t* ql, const int64_t* qc, int nq,
                       const float* d_gf, const int64_t* gl, const int64_t* gc, int ng, int d,
                       int32_t* cmc_sum, double* ap, int32_t* valid);

/* ---- multi-GPU exchange: one process per GPU, collectives directly on librccl (RCCL over xGMI) -----
 * The path shards with ONE exchange step: crops are split contiguous-by-index, every rank embeds its shard, one all-gather of
 * the [n_local][512] fp32 embeddings follows, each rank computes its row block of the distance matrix.  A fixed gallery is
 * sharded by rows - the reference's own faiss.IndexShards pattern (reid/faiss_utils.py:121-135: shard, search, merge).
 * Rank 0 creates the id, the host distributes its 128 bytes (any channel: a TCP store, MPI, a file), every rank calls
 * reid_comm_init.  Without a communicator (or world == 1) every collective below degrades to the local copy. */
#define REID_COMM_ID_BYTES 128
int reid_comm_unique_id(void* id128);                                        /* ncclGetUniqueId */
int reid_comm_init(reid_ctx* ctx, int rank, int world, const void* id128);   /* ncclCommInitRank on the context's device */
int reid_comm_info(reid_ctx* ctx, int* rank, int* world);
int reid_comm_destroy(reid_ctx* ctx);
/* d_recv[r * bytes ..] = rank r's d_send (bytes per rank equal on all ranks); enqueued on the context's stream, no sync */
int reid_allgather_dev(reid_ctx* ctx, const void* d_send, void* d_recv, size_t bytes_per_rank);
/* ragged row blocks: rank r contributes n_local rows of row_bytes; d_out = all rows in rank order, counts_host[world] (may be
 * NULL) the per-rank row counts, *n_total their sum.  Synchronises the stream once (the counts are needed on the host). */
int reid_allgather_rows_dev(reid_ctx* ctx, const void* d_local, int n_local, size_t row_bytes, void* d_out,
                            int32_t* counts_host, int* n_total);
/* small host-side reduction over the ranks, op 0 = sum, 1 = max, count <= 64; also the job's barrier.  Synchronises. */
int reid_allreduce_f64(reid_ctx* ctx, double* inout_host, int count, int op);
/* squared-L2 k-NN over a gallery whose ROWS are sharded across the ranks (index_init_gpu's IndexShards, faiss_utils.py:121-135):
 * d_xq [nq][d] identical on every rank, d_xb_local [nb_local][d] this rank's rows, index_base their first global row.
 * Same (d_D, d_I) on every rank, equal to a single-process reid_knn_dev over the whole gallery (ties -> lowest global row). */
int reid_knn_gallery_sharded_dev(reid_ctx* ctx, const float* d_xq, int nq, const float* d_xb_local, int nb_local,
                                 int index_base, int d, int k, float* d_D, int32_t* d_I);

/* ---- single operators (unit tests and reuse by other backbones) --------------------------- */
/* NHWC convolution, weights [Cout][R][S][Cin], optional per-channel scale/shift, residual (same shape as out), ReLU.  In mode 2
 * weights with |w| 2^11 >= 65504 are refused (REID_ERR_ARG); the context's fault status is returned after the call. */
int reid_conv2d_nhwc(reid_ctx* ctx, const float* x, int n, int h, int w, int cin, const float* wgt, int cout, int r,
                     int s, int stride, int pad, const float* scale, const float* shift, const float* residual,
                     int relu, float* out);
/* C[m][n] = A[m][k] . B[n][k]^T (+ bias[n]) */
int reid_gemm_nt(reid_ctx* ctx, const float* a, int m, const float* b, int n, int k, const float* bias, float* c);

#ifdef __cplusplus
}
#endif
#endif /* REID_HIP_H */
