/* Experiment and correctness-harness entry points of libreid_hip_debug.so (built from csrc/debug.hip + csrc/microbench.hip,
 * linked on top of libreid_hip.so).  NOT part of the drop-in C ABI of include/reid_hip.h: nothing the reference's callers
 * would bind lives here.  Used by the tools/ scripts (kernel A/B timing, feed / MFMA-shape microbenchmarks) and by one parity test
 * of the layer-1 fp16 convolution kernel.  All functions return a reid_hip.h status code. */
#pragma once
#include "reid_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Experiment switches of a context, by the name of the reid_ctx field (csrc/reid_internal.h: f16_cfg, split_pair, split_terms,
 * swin_two_linear, swin_attn_mfma, swin_attn_split, swin_fold, swin_stop, knn_wide, knn_wide_min, select_two_pass, f32_conv, ...).
 * They select kernels, arithmetic forms and summation orders; the product library gives them fixed defaults and reads none of them
 * from the environment.  The setter drains the context's stream first.  Unknown name / value: REID_ERR_ARG. */
int reid_debug_set_switch(reid_ctx* ctx, const char* name, long long value);
int reid_debug_get_switch(reid_ctx* ctx, const char* name, long long* value);
/* Times `iters` launches of one fp16-storage implicit-GEMM convolution (SERes18_IBN.py:120-128 shapes) on random device
 * data; cfg = BN*1000 + BK*10 + NST, 2000000 / 2000001 = LDS-halo kernel without / with loader waves. */
int reid_debug_conv_f16(reid_ctx* ctx, int n, int h, int w, int cin, int cout, int r, int stride, int pad, int cfg, int iters,
                        float* ms_per_launch);
/* Times one fp32-class 3x3 stride-1 convolution (SPLIT build of the LDS-halo kernel) on random device data; ablate != 0 switches
 * phases of its main loop off (1 weight DMA, 2 halo DMA, 4 MFMAs, 8 fragment reads, 16 barriers): timing experiments, wrong results. */
int reid_debug_conv_split(reid_ctx* ctx, int n, int h, int w, int c, int cout, int ablate, int iters, float* ms_per_launch);
/* The same for the exact-fp32 convolutions.  flags: 1 fused input affine + ReLU, 2 BN epilogue, 4 residual + ReLU,
 * 8 statistics; variant 0 = gemm_f32_kernel<A_IM2COL>, 1 = conv_f32.hip. */
int reid_debug_conv_f32(reid_ctx* ctx, int n, int h, int w, int cin, int cout, int r, int stride, int pad, int flags,
                        int variant, int iters, float* ms_per_launch);
/* Correctness harness of conv3x3_c64_f16.hip: fp32 host operands are rounded to f16, one launch, fp32 results back. */
int reid_debug_conv_c64(reid_ctx* ctx, int n, const float* x, const float* w_krsc, const float* scale, const float* shift,
                        const float* residual, int relu, float* out, float* stats);
/* Times one dense fp16 GEMM C[m][n] = A[m][k] . B[n][k]^T; diag_host: optional [64*8*4] per-wave cycle sums. */
int reid_debug_gemm_f16(reid_ctx* ctx, int m, int n, int k, int cfg, int iters, float* ms_per_launch,
                        unsigned long long* diag_host);
/* Times one Swin Linear layer [m][k] x [n][k]^T on random device data: mode bit 0 = fp16-storage GEMM (else exact fp32),
 * bits 1-2 = epilogue (0 bias, 1 bias + erf-GELU, 2 bias + fp32 residual into the fp32 stream). */
int reid_debug_linear(reid_ctx* ctx, int m, int n, int k, int mode, int iters, float* ms_per_launch);
/* One Swin Linear layer on host operands through the f16 linear build (correctness harness: identical input rows must give
 * bit-identical output rows wherever they sit in a tile).  mode 1 = fp16 storage, 2 = fp32-class (split operands); flags bit 0 =
 * erf-GELU, bit 1 = f16 output through the LDS-staged epilogue (mode 2: [yh | yl'], returned as yh + yl' / 2^11), else fp32
 * output (+ res) through the buffer-store epilogue. */
int reid_debug_linear_rows(reid_ctx* ctx, const float* x, const float* w, const float* bias, const float* res, int m, int n, int k,
                           int mode, int flags, float* out);
/* One convolution of the ResNet trunk through the launcher the forward uses (correctness harness, tests/test_gpu_conv.py): x fp32 NHWC
 * [n][h][w][cin], wgt [cout][r][r][cin]; out = relu_from-on ReLU (if relu) of conv * scale + shift (+ residual), fp32 [m][cout] with
 * m = n ho wo.  The context's precision and switches pick the kernel.  pack_from >= 0 asks for the [yh | yl'] f16 store of the
 * columns from pack_from on (raw f16 bits, [m][2 cout]; the fp32 output of those columns is then not written); *packed_written says
 * whether the launch made it.  want_stats: per-128-row column sums [m / 128][cout][2] (sum, sum of squares) of the output.
 * a_scale / a_shift [n][cin] (+ a_relu): the exact-fp32 loader's input affine.  Every output the launch leaves alone reads as NaN
 * (0xffff).  Drops the split weights cached for its weight buffer first; returns the context's fault status. */
int reid_debug_conv_layer(reid_ctx* ctx, const float* x, int n, int h, int w, int cin, const float* wgt, int cout, int r, int stride,
                          int pad, const float* scale, const float* shift, const float* residual, int relu, int relu_from, int pack_from,
                          int want_stats, const float* a_scale, const float* a_shift, int a_relu, float* out, uint16_t* packed,
                          float* stats, int* packed_written);
/* One convolution of the fp16-storage trunk through conv_gemm16(A16_IM2COL, ...), the call the forward makes (correctness harness,
 * tests/test_gpu_conv_f16.py).  Operands are raw f16 bits, so the caller owns the exact values: x [n][h][w][cin], wgt [cout][r][r][cin],
 * residual [m][cout] (may be null), m = n ho wo; scale / shift fp32 [cout] (both or neither).  out = ReLU (if relu) of conv * scale + shift
 * (+ residual) as raw f16 bits [m][cout]; want_stats: per-128-row column sums [m / 128][cout][2] (sum, sum of squares) of the fp32 values
 * before the f16 rounding.  The context's switches (f16_halo, f16_cfg, f16_split_k, ...) pick the kernel as in the forward; the context
 * must hold a loaded ResNet checkpoint (its zero page).  Every output the launch leaves alone reads as NaN (0xffff).  Arguments the
 * launchers refuse (m % 128, cin % 32, cout % 64 != 0) return REID_ERR_ARG with nothing launched; else the context's fault status.
 * *form names the launch that was made (reid_ctx::conv_form, written by the launchers on the host; 0 = none):
 *   launch_gemm_f16 (implicit GEMM):   the tile configuration BN * 1000 + BK * 10 + NST: 64642, 64323, 128323, 128642, 256324, 256642;
 *   launch_conv3x3_f16 (LDS halo):     BN * 10 + split K: 641, 642, 644 (64-wide tiles), 1281 (128-wide; 1282 .. 1284 with f16_wide_splitk);
 *   launch_conv3x3_c64_f16:            1 plain, 2 with the fused SE tail. */
int reid_debug_conv_layer_f16(reid_ctx* ctx, const uint16_t* x, int n, int h, int w, int cin, const uint16_t* wgt, int cout, int r, int stride,
                              int pad, const float* scale, const float* shift, const uint16_t* residual, int relu, int want_stats,
                              uint16_t* out, float* stats, int* form);
/* launch_conv3x3_c64_f16 (layer 1: 3x3, 64 -> 64 channels on 64 x 32 maps) on raw f16 bits: x / residual (may be null) / out [n][64][32][64],
 * w_folded [64][576] with the BN scale already folded in (f16(w * scale), what scale_rows_f16_kernel makes), shift fp32 [64] (may be null).
 * se_w1 / se_w2t fp32 [8][64] set: conv2 with the fused SE tail, out = relu(gate y + residual), y = relu(conv + shift + residual) (needs
 * shift and residual).  Both null: the plain launch on the same operands; stats (may be null) [n][64][2] then holds the per-image sums.
 * Unwritten outputs read as NaN (0xffff); returns the context's fault status; *form (may be null) as above. */
int reid_debug_conv_c64_se(reid_ctx* ctx, int n, const uint16_t* x, const uint16_t* w_folded, const float* shift, const uint16_t* residual,
                           int relu, const float* se_w1, const float* se_w2t, uint16_t* out, float* stats, int* form);
/* The kernels that finish a residual block and the neck (correctness harness, tests/test_gpu_tail.py), each through the launcher the
 * forward calls, on host operands.  stats [n][tiles][c][2] (per-group sum, sum of squares), activations NHWC [n][hw][c]; f16 operands
 * and results are raw f16 bits.  Every output the launch leaves alone reads as NaN (0xffff); each call returns the context's fault status.
 * norm_finish: IBN finish of conv1, channels [0, half) InstanceNorm (in_gamma / in_beta [half]), [half, c) BatchNorm (bn_scale /
 * bn_shift [c - half]).  form 0 norm_finalize -> a_scale / a_shift [n][c]; 1 in_apply on fp32 x -> out; 2 / 3 in_apply_pack with in_only
 * 0 / 1 -> out16 [n hw][2c] ([xh | xl']) and out (x after the launch); 4 norm_apply_f16 on f16 x -> out16; 5 norm_finalize +
 * affine_relu_f16 -> out16, a_scale, a_shift. */
int reid_debug_norm_finish(reid_ctx* ctx, int form, int n, int hw, int c, int half, int tiles, const void* x, const float* stats,
                           const float* in_gamma, const float* in_beta, const float* bn_scale, const float* bn_shift, float* out,
                           uint16_t* out16, float* a_scale, float* a_shift);
/* se_tail: SE gate + combine, out = relu(sigmoid(w2t^T relu(w1 pooled)) y + shortcut), w1 / w2t [mid][c].  form 0 se_finalize +
 * se_combine -> out, gate [n][c]; 1-3 launch_se_tail's rule, 4-6 se_tail_kernel<false>, 7-9 se_tail_kernel<true>, each with fp32 out
 * only / packed [n hw][2c] out16 only / both; 10 se_tail_f16 and 11 se_finalize + se_combine_f16 on f16 y / shortcut -> out16 (and
 * gate for 11). */
int reid_debug_se_tail(reid_ctx* ctx, int form, int n, int hw, int c, int mid, int tiles, const float* stats, const float* w1,
                       const float* w2t, const void* y, const void* shortcut, float* out, uint16_t* out16, float* gate);
/* The exact-fp32 attention tails of the sibling backbones (csrc/attention_f32.hip) through the forward's launchers, on host operands:
 * arch 1 TripletAttention (prm [3][100]), arch 2 EMA (prm of c / 32 channels per group), out = relu(tail(y) + shortcut), NHWC [n][h][w][c].
 * The yardstick tests/test_gpu_siblings_f16.py measures the f16 tails of libreid_hip_siblings_f16.so against. */
int reid_debug_sibling_tail(reid_ctx* ctx, int arch, int n, int h, int w, int c, const float* prm, const float* y, const float* shortcut,
                            float* out);
/* gem_neck: GeM (exponent p) + BNNeck, emb = gem * scale + shift, on fp32 x (f16 = 0) or f16 x (f16 = 1); gem_out may be null. */
int reid_debug_gem_neck(reid_ctx* ctx, int f16, int n, int hw, int c, float p, const void* x, const float* scale, const float* shift,
                        float* gem_out, float* emb);
/* The kernels of libreid_hip_anysize.so (csrc/anysize.h: the block tails of ResNet18-IBN-SE for any number of pixels hw) through the
 * launchers the any-size forward calls, on host operands; NHWC fp32, c = 64 .. 512 a power of two.  Every output has ONE guard pixel
 * (c floats) behind its last row, set to 0xff bytes before the launch as the outputs are: out [n hw c + c], gate / gem_out / emb [n c + c].
 *   any_norm     x -> out in place: channels < half InstanceNorm2d(affine) over the image's hw pixels + ReLU; channels >= half
 *                relu(x * bn_scale + bn_shift), or left as they are when bn_scale is NULL (half % 32 == 0).
 *   any_se_tail  out = relu(sigmoid(w2t^T relu(w1 mean_hw(y))) y + shortcut), w1 / w2t [mid][c]; gate may be null.
 *   any_gem      GeM (exponent p, clamp 1e-6) + BNNeck, emb = gem * scale + shift; gem_out may be null.
 * The switch "anysize_force" (reid_debug_set_switch) sends 256 x 128 through the any-size forward in the reid_*_hw entries. */
int reid_debug_any_norm(reid_ctx* ctx, int n, int hw, int c, int half, const float* x, const float* in_gamma, const float* in_beta,
                        const float* bn_scale, const float* bn_shift, float* out);
int reid_debug_any_se_tail(reid_ctx* ctx, int n, int hw, int c, int mid, const float* w1, const float* w2t, const float* y,
                           const float* shortcut, float* out, float* gate);
int reid_debug_any_gem(reid_ctx* ctx, int n, int hw, int c, float p, const float* x, const float* scale, const float* shift, float* gem_out,
                       float* emb);
/* The TripletAttention block tail of libreid_hip_anysize_ca.so (csrc/anysize_ca.h; tests/test_gpu_anysize_ca.py) through the launcher the
 * any-size forward calls for cares18_ibn, on host operands: y, shortcut NHWC fp32 [n][h][w][c], prm [3 gates: cw, hc, hw][100] = conv weight
 * [2][7][7], folded BN scale, shift; 2 <= h, w <= 128, c in {64, 128, 256, 512} (anything else REID_ERR_ARG).
 *   out = relu(1/3 * ((y s_hw[h, w] + y s_cw[c, w]) + y s_hc[h, c]) + shortcut),  out [n h w c + c] with ONE guard pixel behind the last.
 * maps / gates (may be NULL), per = h w + c w + h c floats per image, in the layout of csrc/anysize_ca.h:
 *   maps  [n][2 per]      hw [2][h][w] | cw [2][c][w] | hc [2][h][c], channel 0 = unbiased std, channel 1 = mean
 *   gates [n per + c]     hw [h][w] | cw [w][c] (transposed) | hc [h][c] per image, then ONE guard of c floats
 * out and the workspace are set to 0xff bytes before the launch: an element the kernels leave alone reads as NaN.
 * The switch "any_ca" (reid_debug_set_switch) picks the tail of the any-size trunk for cares18_ibn: 1 (default) = this library, 0 =
 * launch_ta_tail of csrc/attention_f32.hip, for A/B timing of whole passes in one process.
 * Returns the context's fault status. */
int reid_debug_any_ca_tail(reid_ctx* ctx, int n, int h, int w, int c, const float* prm, const float* y, const float* shortcut, float* out,
                           float* maps, float* gates);
/* The EMA block tail of libreid_hip_anysize_ema.so (csrc/anysize_ema.h; tests/test_gpu_anysize_ema.py) through the launcher the any-size
 * forward calls for emares18_ibn, on host operands: y, shortcut NHWC fp32 [n][h][w][c], prm (cg = c / 32) = conv1x1 w [cg][cg], b [cg] |
 * conv3x3 w [cg][cg][3][3], b [cg] | GroupNorm weight [cg], bias [cg]; 2 <= h, w <= 128, c in {64, 128, 256, 512} (anything else
 * REID_ERR_ARG).
 *   out = relu(y * sigmoid(weights[h, w]) + shortcut),  out [n h w c + c] with ONE guard pixel behind the last.
 * sig / small (may be NULL), in the layout of csrc/anysize_ema.h:
 *   sig   [n][h + w][c]      rows [0, h) the sigmoid of the 1x1 convolution of the row means, rows [h, h + w) that of the column means
 *   small [n 4 c + c]        mu | rstd | s1 = softmax(agp(x1)) | s2 = softmax(agp(x2)), [4][c] per image, then ONE guard of c floats
 * out and the workspace are set to 0xff bytes before the launch: an element the kernels leave alone reads as NaN.
 * The switch "any_ema" (reid_debug_set_switch) picks the tail of the any-size trunk for emares18_ibn: 1 (default) = this library, 0 =
 * launch_ema_tail of csrc/attention_f32.hip (REID_ERR_ARG where the group's slab does not fit LDS), for A/B timing of whole passes in one
 * process.  Returns the context's fault status. */
int reid_debug_any_ema_tail(reid_ctx* ctx, int n, int h, int w, int c, const float* prm, const float* y, const float* shortcut, float* out,
                            float* sig, float* small);
/* One trunk convolution of the any-size forward (tests/test_gpu_anysize_x3.py) through the launcher the forward calls, on host operands:
 * x [n][h][w][cin], wgt [cout][r][r][cin], out [n ho wo cout + cout] with ONE guard row (cout floats) behind the last pixel, preset to 0xff
 * bytes with the rest.  r = 3 with pad 1 or r = 1 with pad 0, stride 1 or 2, cin % 32 == 0, cout % 64 == 0.  out = acc * scale + shift (both
 * or neither NULL), + residual [n ho wo cout] (may be NULL), ReLU from column relu_from on when relu != 0.
 *   hw_precision 2   any_conv_x3_kernel of libreid_hip_anysize_x3.so (fp32-class: activations split in the loader, the cached split of wgt
 *                    dropped first); form_out (may be NULL) = the tile form launched, 1 = 128 x 64, 2 = 128 x 128.
 *   hw_precision 0   the exact-fp32 GEMM the forward uses at reid_ctx_set_hw_precision 0 / -1, for A/B; form_out = 0.
 * Returns the context's fault status (REID_ERR_STATE when the loader met a value outside f16's range). */
int reid_debug_any_conv(reid_ctx* ctx, int hw_precision, const float* x, int n, int h, int w, int cin, const float* wgt, int cout, int r,
                        int stride, int pad, const float* scale, const float* shift, const float* residual, int relu, int relu_from, float* out,
                        int* form_out);
/* The kernels of libreid_hip_anysize_f16.so (csrc/anysize_f16.h; tests/test_gpu_anysize_f16.py) through the launchers the any-size forward
 * calls under reid_ctx_set_hw_f16 1, on host operands.  f16 operands and results are handed over as their bits (uint16_t), NHWC.  Every
 * output has ONE guard row behind its last pixel, preset to 0xff bytes with the rest (NaN in f16 and in fp32).
 *   any_conv_f16     x [n][h][w][cin], wgt [cout][r][r][cin], out [n ho wo cout + cout]; geometry, epilogue and NULL rules of
 *                    reid_debug_any_conv, residual f16; form_out (may be NULL) = the tile form launched, 1 = 128 x 64, 2 = 128 x 128.
 *   any_stem_f16     x fp32 [n][h][w][3], w16 [64][192] (k = r 24 + s 3 + c, zero padded): conv 7x7 s2 p3 + BN -> stem_out
 *                    [n H1 W1 64 + 64], then MaxPool(3, 2, 1) of that map -> pool_out [n H2 W2 64 + 64].
 *   any_norm_f16     x -> out [n hw c + c] in place: channels < half InstanceNorm2d(affine) over the image's hw pixels + ReLU, the rest untouched.
 *   any_se_tail_f16  out = relu(sigmoid(w2t^T relu(w1 mean_hw(y))) y + shortcut); alias != 0: the launch writes into y's buffer; gate
 *                    [n c + c] fp32 may be NULL.
 *   any_gem_f16      GeM (exponent p, clamp 1e-6) + BNNeck on f16 x, gem_out (may be NULL) / emb fp32 [n c + c]. */
int reid_debug_any_conv_f16(reid_ctx* ctx, const uint16_t* x, int n, int h, int w, int cin, const uint16_t* wgt, int cout, int r, int stride,
                            int pad, const float* scale, const float* shift, const uint16_t* residual, int relu, int relu_from, uint16_t* out,
                            int* form_out);
int reid_debug_any_stem_f16(reid_ctx* ctx, const float* x, int n, int h, int w, const uint16_t* w16, const float* scale, const float* shift,
                            uint16_t* stem_out, uint16_t* pool_out);
int reid_debug_any_norm_f16(reid_ctx* ctx, int n, int hw, int c, int half, const uint16_t* x, const float* in_gamma, const float* in_beta,
                            uint16_t* out);
int reid_debug_any_se_tail_f16(reid_ctx* ctx, int n, int hw, int c, int mid, const float* w1, const float* w2t, const uint16_t* y,
                               const uint16_t* shortcut, int alias, uint16_t* out, float* gate);
int reid_debug_any_gem_f16(reid_ctx* ctx, int n, int hw, int c, float p, const uint16_t* x, const float* scale, const float* shift,
                           float* gem_out, float* emb);
/* The TripletAttention and EMA block tails of libreid_hip_anysize_sib_f16.so (csrc/anysize_sib_f16.h; tests/test_gpu_anysize_sib_f16.py)
 * through the launchers the any-size forward calls under reid_ctx_set_hw_sib_f16 1, on host operands: reid_debug_any_ca_tail /
 * reid_debug_any_ema_tail above with y, shortcut and out handed over as f16 bits (uint16_t), NHWC [n][h][w][c]; prm and the shape range are
 * theirs (anything else REID_ERR_ARG, out untouched).  out [n h w c + c] carries ONE guard pixel behind the last, preset to 0xff bytes
 * (NaN in f16) with the rest.  maps / gates and sig / small (may be NULL) are the fp32 workspace statistics, returned with the sizes, the
 * layouts and the guard the fp32 harnesses return them with.  Returns the context's fault status. */
int reid_debug_any_ca_tail_f16(reid_ctx* ctx, int n, int h, int w, int c, const float* prm, const uint16_t* y, const uint16_t* shortcut,
                               uint16_t* out, float* maps, float* gates);
int reid_debug_any_ema_tail_f16(reid_ctx* ctx, int n, int h, int w, int c, const float* prm, const uint16_t* y, const uint16_t* shortcut,
                                uint16_t* out, float* sig, float* small);
/* The front end of the any-size forward from uint8 windows (tests/test_gpu_anysize_front.py) through the launcher reid_frame_submit_hw and
 * reid_embed_frame_u8_hw call, on host operands: src [src_bytes] holds n windows, window i hw[2i] x hw[2i + 1] pixels at byte offsets[i],
 * its rows one after the other (pitch 0) or `pitch` pixels apart (windows of one frame); every window must lie inside src.  They are
 * resized to out_h x out_w (cv2-style bilinear), normalised with mean_std6 (NULL = 0.5 / 0.5), convolved with stem_w [64][192]
 * (k = r * 24 + s * 3 + c, zero padded), scaled by scale / shift [64] and max-pooled (3, 2, 1).
 *   fused 1   any_front_kernel of libreid_hip_anysize_front.so, one launch
 *   fused 0   any_resize_norm_kernel, the generic GEMM's stem and maxpool3s2_kernel, as the other reid_*_hw entries run
 * out [n H2 W2 64 + W2 64]: the pooled map NHWC and ONE guard pixel row (W2 * 64 floats) behind it, preset to 0xff bytes with the rest.
 * The switch "any_front" (reid_debug_set_switch) picks the front end of the two entries: 1 = the kernel, 0 = the three launches, 2 (default) =
 * the kernel for passes of at most 65 536 stem pixels (n H1 W1), where it measured faster, the three launches above.
 * Returns the context's fault status. */
int reid_debug_any_front(reid_ctx* ctx, int fused, const uint8_t* src, int64_t src_bytes, const int64_t* offsets, const int32_t* hw, int n,
                         int pitch, int out_h, int out_w, const float* mean_std6, const float* stem_w, const float* scale, const float* shift,
                         float* out);
/* gem_neck of the last block's tail in one launch (launch_gem_neck_tail; tests/test_gpu_tail_stream.py): GeM + BNNeck of
 * relu(gate y + shortcut) with se_tail's gate, fp32 operands as in se_tail; equals se_tail form 4 followed by gem_neck bit for bit. */
int reid_debug_gem_neck_fused(reid_ctx* ctx, int n, int hw, int c, int mid, int tiles, float p, const float* stats, const float* w1,
                              const float* w2t, const float* y, const float* shortcut, const float* scale, const float* shift,
                              float* gem_out, float* emb);
/* The front end of a ResNet pass (correctness harness, tests/test_gpu_frontend.py), each through the launcher the forward calls, on host
 * operands.  Every output the launch leaves alone reads as NaN (0xffff); each call returns the context's fault status.
 * stem: conv 7x7 stride 2 pad 3 (3 -> 64) * scale + shift, no ReLU, + MaxPool(3, 2, 1).  x [n][256][128][3], uint8 crops (is_u8, normalised
 * (2v - 255) / 255 by the loaders) or fp32; w [64][7][7][3], packed here to stem.w [64][8][24] and its two f16 forms as reid_seres18_load does.
 * form 0 launch_stem_f32 unpooled -> out [n][128][64][64]; 1 launch_stem_f32 pooled -> out [n][64][32][64]; 2 launch_stem_split -> out and
 * out16 [n 64 32][xh 64 | xl' 64]; 3 launch_stem_pool_f16 straight from uint8 -> out16 [n][64][32][64]; 4 prep_*_pad_f16 +
 * launch_stem_pool_f16 -> out16; 5 prep_*_pad_f16 + conv_gemm16(A16_STEM) + launch_maxpool3s2_f16 -> out16; 6 conv_gemm(A_STEM_U8 /
 * A_STEM_F32) + launch_maxpool3s2 -> out.  f16 results are raw bits.  The launchers keep the strip / tile count they choose to themselves:
 * the test restates the two rules. */
int reid_debug_stem(reid_ctx* ctx, int form, int is_u8, const void* x, int n, const float* w, const float* scale, const float* shift,
                    float* out, uint16_t* out16);
/* resize_norm: n uint8 windows of hw[i] = (h, w) pixels at byte offsets[i] of `packed`, rows `pitch` pixels apart (0: the window's own
 * width), bilinear to 256 x 128 and normalised -> out [n][256][128][3] fp32. */
int reid_debug_resize_norm(reid_ctx* ctx, const uint8_t* packed, const long long* offsets, const int* hw, int n, int pitch, float* out);
/* swin_crop_front: the one kernel of libreid_hip_swin_crops.so (csrc/swin_crops.hip; tests/test_gpu_swin_crops.py) through the launcher the
 * Swin crops entry points call: windows as for resize_norm, bilinear to out_h x out_w (multiples of 224), (v - mean) / std with mean_std6 =
 * mean[3], std[3], then ShadowFeatureExtraction's first convolution (2x2 stride 2, 3 -> 12, c1_w [12][(kh, kw, c)], c1_b [12]) ->
 * out [n][out_h / 2][out_w / 2][12] fp32.  swin_conv1: the stem of the float entry points (sfe_conv1_kernel) alone, x fp32 NCHW
 * [n][3][h][w] -> out [n][h / 2][w / 2][12]. */
int reid_debug_swin_crop_front(reid_ctx* ctx, const uint8_t* packed, const long long* offsets, const int* hw, int n, int pitch, int out_h,
                               int out_w, const float* mean_std6, const float* c1_w, const float* c1_b, float* out);
int reid_debug_swin_conv1(reid_ctx* ctx, const float* x, int n, int h, int w, const float* c1_w, const float* c1_b, float* out);
/* The three kernels of libreid_hip_swin_eval.so (csrc/swin_eval.hip; tests/test_gpu_swin_eval.py), each through the launcher the Swin
 * descriptor entry points call, on host operands.  swin_conv1_mirror / swin_crop_front_mirror: the arguments of swin_conv1 /
 * swin_crop_front, the result of the horizontally mirrored (resized) image.  swin_descriptor: e1, e2 (NULL: one view) [n][96] and cls_w
 * [num_class][96] -> rows [0, n) x columns [0, num_class + 96) of out [out_rows][ld] (out_rows >= n, ld >= num_class + 96); everything
 * else of out reads NaN afterwards. */
int reid_debug_swin_conv1_mirror(reid_ctx* ctx, const float* x, int n, int h, int w, const float* c1_w, const float* c1_b, float* out);
int reid_debug_swin_crop_front_mirror(reid_ctx* ctx, const uint8_t* packed, const long long* offsets, const int* hw, int n, int pitch, int out_h,
                                      int out_w, const float* mean_std6, const float* c1_w, const float* c1_b, float* out);
int reid_debug_swin_descriptor(reid_ctx* ctx, const float* e1, const float* e2, const float* cls_w, int n, int num_class, int out_rows, int ld,
                               float* out);
/* The two kernels of libreid_hip_pil_resize.so (csrc/pil_resize.hip; tests/test_gpu_pil_resize.py) through the launcher the *_images_u8
 * entry points call, one launch of all n images: packed / offsets / hw as reid_descriptor_images_u8, out_h and out_w from 1 to 1024,
 * mean_std6 NULL = ImageNet -> u8_out [n][out_h][out_w][3], Pillow's Image.resize((out_w, out_h), BILINEAR) (may be NULL), and f32_out
 * [n][3][out_h][out_w], ToTensor + Normalize of it.  A float the launch leaves alone reads NaN.  Returns the fault status. */
int reid_debug_pil_resize(reid_ctx* ctx, const uint8_t* packed, const long long* offsets, const int* hw, int n, int out_h, int out_w,
                          const float* mean_std6, uint8_t* u8_out, float* f32_out);
/* maxpool: MaxPool(3, 2, 1) of x NHWC [n][h][w][c] -> out [n][(h - 1) / 2 + 1][(w - 1) / 2 + 1][c], fp32 (f16 = 0) or raw f16 bits. */
int reid_debug_maxpool(reid_ctx* ctx, int f16, const void* x, int n, int h, int w, int c, void* out);
/* The two kernels of the Swin "v2" blocks alone (csrc/swin_v2.hip; correctness harnesses, tests/test_gpu_swin_v2.py), each through the
 * launcher the forward calls, on host operands; f16 results are raw f16 bits; each call returns the context's fault status.
 * window_attn_cos: cosine window attention of n maps of h x w tokens (multiples of 7), qkv fp32 [n h w][3 heads 32] (q | k | v, head-major),
 * bias [heads][49 queries][49 keys], scale [heads] (already clamped and exponentiated).  mode 0: fp32 in -> out fp32 [tokens][heads 32];
 * mode 2: fp32 in -> out16 [tokens][2 heads 32] = [oh | ol'] (ol' = f16((o - oh) 2^11)); mode 1: qkv rounded to f16 -> out16 [tokens][heads 32]. */
int reid_debug_window_attn_cos(reid_ctx* ctx, int mode, const float* qkv, int n, int h, int w, int heads, int shifted, const float* bias,
                               const float* scale, float* out, uint16_t* out16);
/* post_norm: out = x + (LayerNorm(y) g + b) over t rows of c channels (eps 1e-5), x / y / out fp32 [t][c]; side 0: out only, 1: out16 = f16
 * copy of out [t][c], 2: out16 = [oh | ol'] [t][2c].  in_place != 0: the launch writes out over its own x. */
int reid_debug_post_norm(reid_ctx* ctx, int side, const float* x, const float* y, int t, int c, const float* g, const float* b, int in_place,
                         float* out, uint16_t* out16);
/* The kernels of the Swin v1 forward that are not GEMMs, and its geometric convolutions (csrc/swin.hip; correctness harnesses,
 * tests/test_gpu_swin_kernels.py), each through the function the forward calls, on host operands.  f16 results are raw f16 bits; every
 * output the launch leaves alone reads as NaN (0xffff); each call returns the context's fault status.
 * window_attn: window attention of n maps of h x w tokens (multiples of 7) through launch_window_attn, with the context put into the precision
 * and switches that reach one kernel for the call: form 0 window_attn_kernel<float> -> out fp32 [tokens][heads 32]; 1 the same kernel's packed
 * store -> out16 [tokens][2 heads 32] = [oh | ol'] (ol' = f16((o - oh) 2^11)); 2 window_attn_kernel<f16> and 3 window_attn_mfma_f16_kernel ->
 * out16 [tokens][heads 32], qkv rounded to f16 on the device into rows of the forward's stride (3 heads 32 rounded up to 64, the padding NaN);
 * 4 window_attn_mfma_split_kernel -> out16 as form 1; 5 window_attn_mfma_f32_kernel -> out.  qkv fp32 [n h w][3 heads 32] (q | k | v,
 * head-major), pos169 the block's [13][13] relative-position table (expanded to [key 64][query 64] by the function reid_swin_load uses). */
int reid_debug_window_attn(reid_ctx* ctx, int form, const float* qkv, int n, int h, int w, int heads, int shifted, const float* pos169,
                           float* out, uint16_t* out16);
/* layernorm: (x - mean) / sqrt(var + 1e-5) g + b over t rows of c channels (c <= 768, a multiple of 4).  form 0 launch_layernorm<float> ->
 * out [t][c]; 1 launch_layernorm<f16> -> out16 [t][c]; 2 launch_layernorm_packed -> out16 [t][2c] = [yh | yl']. */
int reid_debug_layernorm(reid_ctx* ctx, int form, const float* x, int t, int c, const float* g, const float* b, float* out, uint16_t* out16);
/* ln_linear: LayerNorm 1 + to_qkv of the fp32-class mode in one kernel (csrc/two_linear_f16.hip, launch_ln_linear; the context is in
 * precision 2 for the call): out [t][n] = LayerNorm(x [t][c]; ln_g, ln_b) . w [n][c]^T + bias (bias may be null).  Drops the tile image
 * cached for its weight buffer first. */
int reid_debug_ln_linear(reid_ctx* ctx, const float* x, const float* ln_g, const float* ln_b, const float* w, const float* bias, int t, int c,
                         int n, float* out);
/* swin_linear: one Linear layer, y = act(x [m][k] . w [n][k]^T + bias) + res, through linear() / linear16() of csrc/swin.hip - the
 * functions every Linear of the Swin trunk and the classifier go through - so a case sees the forward's dispatch, padding and epilogue
 * (tests/test_gpu_linear.py).  bias [n] and res [m][n] may be null.  The context is put into `precision` for the call and its switches
 * (f32_conv, lin_x3, f16_lin_256, f16_cfg) pick the kernel.  Operands are prepared as the forward prepares them: precision 0 fp32 as
 * given; 1 x and w rounded to f16 on the device, w padded with zero rows to a multiple of 64; 2 x packed to [xh | xl'] and the weight
 * image [wh 2^11 | wh | wl'] built and cached by linear() itself (dropped again before the call returns) - unless flags bit 2 leaves x in
 * fp32, the classifier's call, which stays on the exact kernel.  flags: bit 0 erf-GELU; bit 1 the residual aliases the output (the rows
 * of the output buffer hold res when the launch starts, and res32 == out: fc2 and post_proj run so); bit 2 as above.
 * out_form 0: fp32 rows of ldc floats into `out`; 1 (precision 1, no res): f16 rows of ldc halves into `out16`; 2 (precision 2, packed x,
 * no res): rows [yh | yl'] of 2 n halves into `out16` as the two raw f16 planes (y = yh + yl' 2^-11 is left to the caller).  ldc >= n in
 * precision 1 (the qkv row stride of the fp16-storage mode), ldc == n otherwise.
 * The output comes back WITH its guard: `front` elements (64 floats / 128 halves), then m + 8 rows of ld = ldc (2 n for form 2) elements;
 * every byte the launch leaves alone is 0xff.  out / out16 hold front + (m + 8) ld elements.
 * *form = reid_ctx::conv_form of the launch, written by the launchers on the host (0: none was made):
 *   gemm_f32_dma_kernel<64>   5064320 (<128>: 5128320, K-tiles of 16: 5128160);   gemm_f32_kernel<.., 64 | 128>   6064000 | 6128000;
 *   gemm_f16_kernel LIN builds   64323, 128323, 256642, 256324;   lin_x3_kernel<128>   7128000.
 * REID_ERR_ARG with nothing queued for m <= 0, k % 32 != 0 with f16 operands (k % 4 != 0 with fp32 ones), a null output pointer of the
 * chosen form, a form the precision does not have; else what the launcher returns, else the context's fault status. */
int reid_debug_swin_linear(reid_ctx* ctx, const float* x, const float* w, const float* bias, const float* res, int m, int n, int k,
                           int precision, int flags, int out_form, int ldc, float* out, uint16_t* out16, int* form);
/* swin_sfe: ShadowFeatureExtraction after its first convolution (sfe_norm_kernel + sfe_conv2_fc_kernel with the forward's grids).  c1
 * [n][h1][w1][12]; in_g / in_b [6] InstanceNorm affine of channels 0-5, bn_s / bn_t [6] folded BatchNorm of channels 6-11; c2_w [48][(kh, kw,
 * c) 48], c2_b [48], fc_w [96][48], fc_b [96] -> ab [n][24] (12 scales, 12 shifts) and tok [n][h1 / 2][w1 / 2][96]. */
int reid_debug_swin_sfe(reid_ctx* ctx, const float* c1, int n, int h1, int w1, const float* in_g, const float* in_b, const float* bn_s,
                        const float* bn_t, const float* c2_w, const float* c2_b, const float* fc_w, const float* fc_b, float* ab, float* tok);
/* swin_tail: LayerNorm(96, eps 1e-6; g, b) per token -> GeM_1D (exponent p; p == 3 takes the cube branch) over ntok tokens -> BatchNorm1d
 * (swin_tail_partial_kernel + swin_tail_final_kernel with the forward's grids).  x [n][ntok][96] -> gem [n][96], emb = gem bn_s + bn_t. */
int reid_debug_swin_tail(reid_ctx* ctx, const float* x, int n, int ntok, const float* g, const float* b, float p, const float* bn_s,
                         const float* bn_t, float* gem, float* emb);
/* swin_merge / swin_fuse: the geometric convolutions of the trunk on the weights THIS CONTEXT HAS LOADED (reid_swin_load: Unfold-order and
 * parity repacking, f16 rows, split forms) and in its precision, through the functions the forward calls.  merge: patch merging in front of
 * `stage` (2 .. 4), x [n][h][w][48 2^(stage - 1)] -> out fp32 [n][h / 2][w / 2][96 2^(stage - 1)].  fuse: the top-down fusion, sfe / x1
 * [n][h1][w1][96], x2 .. x4 the later stage outputs (half the tokens, twice the channels each) -> a0 = x4 + Conv8x8s8(sfe)
 * [n][h1 / 8][w1 / 8][768], f3 = x3 + ConvT(a0), f2 = x2 + ConvT(f3) (fp32; precision 1: raw f16 bits) and f1 = x1 + ConvT(f2) fp32. */
int reid_debug_swin_merge(reid_ctx* ctx, int stage, const float* x, int n, int h, int w, float* out);
int reid_debug_swin_fuse(reid_ctx* ctx, const float* sfe, const float* x1, const float* x2, const float* x3, const float* x4, int n, int h1,
                         int w1, void* a0, void* f3, void* f2, float* f1);
/* bank_cost96: the cost stage of the frame pipeline for a 96-wide bank (NearestNeighborDistanceMetric.distance, [external]
 * deep_sort/sort/nn_matching.py, for the swin_transformer tracker model) through the launch reid_frame_cost makes: bank_cost96_kernel of
 * libreid_hip_bank96.so, or bank_cost_kernel with the `bank_fast` switch at 0.  slots [t] (host) of a bank with d = 96, dets [m][96] ->
 * out [t][m]; metric REID_METRIC_COS / REID_METRIC_L2SQR, gate < 0 raw, else cost > gate -> gate + 1e-5. */
int reid_debug_bank_cost96(reid_ctx* ctx, reid_bank* bank, const int32_t* slots, int t, const float* dets_host, int m, int metric, float gate,
                           float* out_host);
/* Timing experiments on that kernel (WRONG results while set): bit 0 = no weight refills after the first two steps, bit 1 = no block
 * barriers.  0 restores the product behaviour. */
int reid_debug_two_linear_ablate(reid_ctx* ctx, int bits);
/* The fused pair of linears of the fp32-class mode (csrc/two_linear_f16.hip) alone: out = res + w2 . act(w1 . x + b1) + b2, x / res /
 * out [m][c], w1 [hid][c], w2 [c][hid], all fp32 on the host; act 1 = erf-GELU.  iters > 1: the launch repeated, mean time in *ms.
 * ln_g / ln_b [c] (or both null): the first linear reads LayerNorm(x) (eps 1e-5), made in the kernel's prologue. */
int reid_debug_two_linear(reid_ctx* ctx, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                          const float* res, int m, int c, int hid, int act, int iters, float* out, float* ms, const float* ln_g,
                          const float* ln_b);
/* two_linear_form: the same pair as a test harness (tests/test_gpu_two_linear.py): ONE launch through launch_split_pack (packed builds)
 * and launch_two_linear, the functions the forward calls, in the context's own precision (2, or the launcher refuses) and switches
 * (swin_two_linear).  Operands as above.  flags: bit 0 erf-GELU; bit 1 the LN build - x stays fp32 and LayerNorm(ln_g, ln_b; both
 * required, and both null without the bit) runs in the kernel's prologue; bit 2 the forward's aliasing - LN build: ONE device buffer is
 * x32, res and out (the MLP's call; res must be null, the residual is x); packed build: the output rows hold res when the launch starts
 * and res == out.  Without bit 2 x, res and out are three buffers.
 * The output comes back WITH its guard, by the conventions of reid_debug_swin_linear: 64 floats, then m + 8 rows of c floats; every
 * byte the launch leaves alone is 0xff.  out holds 64 + (m + 8) c floats.  The tile images cached for the harness's weight buffers are
 * dropped before and after the launch.
 * Returns REID_ERR_ARG from launch_two_linear's own check (two_linear_supported: precision 2, swin_two_linear, c 96 or 192, hid a
 * multiple of 32 up to 4 c) with the untouched output copied back; else the context's fault status - REID_ERR_STATE when the launch
 * raised the range guard of the hidden split (|h| >= 65504 or NaN) or of the normalised input, the output still copied back. */
int reid_debug_two_linear_form(reid_ctx* ctx, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                               const float* res, int m, int c, int hid, int flags, const float* ln_g, const float* ln_b, float* out);
/* Experiment switch of the fused distance + selection kernel: 0 product behaviour, 1 / 2 skip phases (INCOMPLETE results: timing
 * only), 4 print candidate-list statistics. */
int reid_debug_select_exp(reid_ctx* ctx, int mode);
/* Test switch of the large k-NN path (candidates on the f16 matrix pipe + exact fp32 refinement): enable = 0 -> fused fp32 search
 * for every size; force > 0 -> rows whose index is a multiple of it take the exact-row fallback. */
int reid_debug_knn_wide(reid_ctx* ctx, int enable, int force);
/* knn_wide_eligible (csrc/knn_wide.hip): 1 when reid_knn_dev sends this shape through the large k-NN path under the context's switches. */
int reid_debug_knn_wide_eligible(reid_ctx* ctx, int nq, int nb, int d, int k);
/* The large k-NN path itself on host operands xq [nq][d], xb [nb][d], 1 <= k <= 24, whatever reid_debug_knn_wide_eligible says: rows
 * zero-padded to a multiple of 64 floats and squared norms as reid_knn_dev makes them, then knn_wide_dev.  D / I are [nq + 1][k]: the
 * device outputs carry one guard row preset to 0xff bytes, which is returned with them.  tile_rows > 0 (a multiple of 256) replaces the
 * rule that bounds the scratch matrix to 1 GiB by query tiles, for this call only.  For a call of ONE tile the stages come back too
 * (each pointer may be NULL; with several tiles they must be):
 *   mat   fp32 [nq][ceil256(nb)]  the candidate matrix sx sy (|y|^2 - 2 x.y) as selection and proof read it (padding columns: whatever the GEMM left);
 *   keys  uint64 [nq][32]         the 32 smallest of each row, (order-preserving key of the value << 32) | column, ascending, ~0 = none;
 *   flags int32 [nq]              rows sent through the exact-row fallback (forced, more than 1024 survivors, proof failed);
 *   sc    fp32 [4]                sx, sy, sx sy, max |y|^2;
 * nflagged: the rows the fallback kernel recomputed, counted on the device.  Waits for the stream. */
int reid_debug_knn_wide_run(reid_ctx* ctx, const float* xq, int nq, const float* xb, int nb, int d, int k, int tile_rows, float* D,
                            int32_t* I, float* mat, unsigned long long* keys, int32_t* flags, float* sc, int32_t* nflagged);
/* reid_argmin_rows_x3_dev (k = 1, any metric) / reid_knn_x3_dev (metric = REID_METRIC_L2SQR) through the launcher those entries call, on
 * device operands (d_D [m][k] may be NULL, d_I [m][k]), with the test hook and the statistics they do not expose:
 * force_fallback_every = f > 0 sends every row whose index is a multiple of f through the exact-row kernel (the hook reid_debug_knn_wide
 * has); stats = {rows proven, rows recomputed by the exact-row kernel, tile form (1 = 128 x 64, 2 = 128 x 128), candidates per row KK}.
 * Waits for the stream. */
int reid_debug_select_x3(reid_ctx* ctx, const float* d_x, int m, const float* d_y, int n, int d, int metric, int k, float* d_D,
                         int32_t* d_I, int force_fallback_every, int32_t* stats);
/* Switches the s_memtime stamps of the loader-wave conv kernel on / off (out_host [64*8*5] when disabling). */
int reid_debug_conv_diag(reid_ctx* ctx, int enable, unsigned long long* out_host);
/* Bare MFMA loop with fragments re-read from LDS (shape 32 = 32x32x16 f16, 16 = 16x16x32 f16). */
int reid_debug_mfma_shape(reid_ctx* ctx, int shape, int iters, int blocks, float* tflops);
/* Registers-only MFMA loop (no LDS, no memory; 512 blocks x 4 waves): what the matrix pipe of THIS device sustains.  shape 32 =
 * v_mfma_f32_32x32x16_f16, 16 = v_mfma_f32_16x16x32_f16; zero != 0: all-zero operands (the chip holds its clock); else random. */
int reid_debug_mfma_bare(reid_ctx* ctx, int shape, int zero, int iters, float* tflops);
/* Operand-feed microbenchmark: rows of `rowb` bytes at `stride` from a `footprint`-byte buffer, LDS-DMA or register loads. */
int reid_debug_feed(reid_ctx* ctx, int mode, size_t footprint, int rowb, size_t stride, int iters, int inflight,
                    float* gbs_per_cu, float* tbs_chip);
/* The device k-way merge of reid_knn_gallery_sharded_dev run on host lists [world][nq][kk] (tests with virtual shards). */
int reid_debug_knn_merge(reid_ctx* ctx, const float* Dall, const int32_t* Iall, int world, int nq, int kk, int k, float* D,
                         int32_t* I);
/* Loop-back communicator: `world` contexts of this process on one device become ranks 0..world-1 of a job, one host thread
 * each; every collective of csrc/comm.hip then runs with world > 1 on a one-GPU box (host rendezvous + device copies, no
 * RCCL).  reid_comm_destroy / reid_ctx_destroy detach a rank. */
int reid_debug_comm_loopback(reid_ctx** ctxs, int world);
/* What a wave that stages data can issue beside the other wave's back-to-back v_mfma_f32_32x32x2_f32 (microbench.hip). */
int reid_debug_coissue(reid_ctx* ctx, int mode, int iters, int roles, double* cyc_mfma_wave, double* cyc_other_wave);
/* The two kernels of the 256 x 128 descriptor entries (csrc/postproc.hip; tests/test_gpu_postproc.py), each through the launcher
 * descriptor_dev calls, on host operands.  Every output carries ONE guard row behind its last row, preset to 0xff bytes with the rest (what
 * the launch leaves alone reads as NaN); each call returns the context's fault status.
 *   descriptor  e1 / e2 [n][de], l1 / l2 [n][dl] -> out [(n + 1)(de + dl)]: row = cat(e1 / max(|e1|, 1e-12), l1 / max(|l1|, 1e-12)); with a
 *               second view (e2 and l2, both or neither NULL) the mean of the two views' rows, divided by max(its norm, 1e-12).  A single
 *               view is not renormalised.
 *   flip_w      x [rows][w] -> y [(rows + 1) w]: every row with its columns reversed. */
int reid_debug_descriptor(reid_ctx* ctx, const float* e1, const float* l1, const float* e2, const float* l2, int n, int de, int dl,
                          float* out);
int reid_debug_flip_w(reid_ctx* ctx, const float* x, long long rows, int w, float* y);
/* The two kernels of libreid_hip_eval_links.so (csrc/eval_links.hip; tests/test_gpu_eval_links.py), each through the launcher the entries
 * call, on host operands; guards preset to 0xff bytes with the rest; each call returns the context's fault status.
 *   shift_mirror  x [m][3][h][w], shift_tl int32 [m][2], fill3 -> y [m 3 h w + w]: crop(pad(mirror(x))) and ONE guard row of w floats behind
 *                 it (reid_descriptor_f32_nchw_shift).
 *   dist_add_l2   a [n][d], inout [n n + n]: the matrix, updated in place as reid_distmat_add_l2 does, and ONE guard row of n floats
 *                 behind it, which the call presets itself (what the caller put there is ignored). */
int reid_debug_shift_mirror(reid_ctx* ctx, const float* x, int m, int h, int w, const int32_t* shift_tl, int pad, const float* fill3,
                            float* y);
int reid_debug_dist_add_l2(reid_ctx* ctx, const float* a, int n, int d, float* inout);

#ifdef __cplusplus
}
#endif
