// libreid_hip_anysize_f16.so (anysize_f16.hip): ResNet18-IBN-SE at an input size other than 256 x 128 in fp16 storage with fp32
// accumulation - what the any-size forward launches when reid_ctx_set_hw_f16 is 1.  Activations are NHWC f16 with 16-byte aligned rows
// (c % 32 == 0), convolution weights f16 [cout][r r][cin] (the layout of the fp16-storage mode), statistics, gates and the embedding fp32
// or wider.  Every kernel rounds to f16 once, at its store.  libreid_hip.so does not link it: api.hip opens it from its own directory with
// dlopen on the first reid_*_hw call at another size under that setting; without the file that call is REID_ERR_STATE naming it.  The
// callers (api.hip, debug.hip) check the arguments; every pointer is a device pointer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// out[m][co] = f16( relu?( (sum_k x.w)[m][co] * scale[co] + shift[co] (+ residual[m][co]) ) ), m = (image, oy, ox) of n Ho Wo output pixels,
// k = (tap, channel) with padding taps read as zero, summed in fp32 on v_mfma_f32_16x16x32_f16.  r = 3 (pad 1) or 1 (pad 0), stride 1 or 2,
// cin % 32 == 0, cout % 64 == 0.  ReLU (relu != 0) from column relu_from on.  scale / shift NULL: 1 / 0.  No launch splits K: an output
// element is summed in one fixed order whatever tile it falls into and whatever n is.
// form_out (may be NULL): the tile form launched, ANYSIZE_F16_FORM_*; it depends on the geometry only, never on n.
hipError_t anysize_f16_conv(hipStream_t stream, const _Float16* x, int n, int h, int w, int cin, const _Float16* w16, int cout, int r, int stride,
                            int pad, const float* scale, const float* shift, const _Float16* residual, int relu, int relu_from, _Float16* out,
                            int* form_out);
// Stem: conv 7x7 stride 2 pad 3 + folded BN, no ReLU.  x fp32 NHWC [n][h][w][3], rounded to f16 by the loader; w16 [64][192] f16 with
// k = r 24 + s 3 + c, zero padded (the f16 image of the packed fp32 stem weights); out f16 [n][H1][W1][64], H1 = (h - 1) / 2 + 1.
hipError_t anysize_f16_stem(hipStream_t stream, const float* x, int n, int h, int w, const _Float16* w16, const float* scale, const float* shift,
                            _Float16* out);
// MaxPool2d(3, 2, 1) on f16 NHWC [n][h][w][c] -> [n][(h - 1) / 2 + 1][(w - 1) / 2 + 1][c]; taps outside the map are skipped (odd h, w too).
hipError_t anysize_f16_maxpool(hipStream_t stream, const _Float16* x, int n, int h, int w, int c, _Float16* out);
// IBN finish in place: channels [0, half) of x [n][hw][c]: InstanceNorm2d(affine, eps 1e-5, biased variance) over the image's hw pixels,
// then ReLU.  Channels [half, c) are not touched (the producing convolution's epilogue finished them).  half % 32 == 0.
hipError_t anysize_f16_norm(hipStream_t stream, _Float16* x, int n, int hw, int c, int half, const float* in_gamma, const float* in_beta);
// SEBlock + combine: pooled [n][c] fp32 (workspace) = mean of y over hw; gate = sigmoid(W2 relu(W1 pooled)), w1 [mid][c], w2t [mid][c],
// mid <= 64; out = f16(relu(gate * y + shortcut)).  gate_out [n][c] may be NULL.  out may be y.
hipError_t anysize_f16_se_tail(hipStream_t stream, const _Float16* y, const _Float16* shortcut, int n, int hw, int c, int mid, const float* w1,
                               const float* w2t, float* pooled, _Float16* out, float* gate_out);
// GeM + BNNeck: g = (mean over hw of clamp(x, 1e-6)^p)^(1/p), emb = g * scale + shift, both fp32.  p [1] on the device.  gem_out may be NULL.
hipError_t anysize_f16_gem(hipStream_t stream, const _Float16* x, int n, int hw, int c, const float* p, const float* scale, const float* shift,
                           float* gem_out, float* emb);
}
enum { ANYSIZE_F16_FORM_128x64 = 1, ANYSIZE_F16_FORM_128x128 = 2 };
