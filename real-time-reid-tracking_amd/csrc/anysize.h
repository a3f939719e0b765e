// libreid_hip_anysize.so (anysize.hip): what the ResNet18-IBN-SE forward launches between its convolutions when the input is not
// 256 x 128 - the memory-bound kernels of a block for ANY hw = Ho * Wo (the product library's count tiles of 128 pixels).  libreid_hip.so
// does not link it: api.hip opens it from its own directory with dlopen on the first reid_*_hw call at another size, so every other caller
// needs what it needed before.  Such a call without this library is REID_ERR_STATE naming the file.  The callers (api.hip, debug.hip) check
// the arguments; everything here is a device pointer, activations are NHWC fp32 with 16-byte aligned rows (c % 32 == 0).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// IBN finish in place (SERes18_IBN.py:88-93): x [n][hw][c]; channels [0, half): InstanceNorm2d(affine, eps 1e-5, biased variance) over the
// image's hw pixels, then ReLU; channels [half, c): relu(x * bn_scale[ch - half] + bn_shift[ch - half]) when bn_scale is not NULL, untouched
// when it is (the producing convolution's epilogue finished them).  half % 32 == 0, 32 <= half <= c <= 512.
hipError_t anysize_norm(hipStream_t stream, float* x, int n, int hw, int c, int half, const float* in_gamma, const float* in_beta,
                        const float* bn_scale, const float* bn_shift);
// SEBlock + combine (SERes18_IBN.py:32-41, :123-128): pooled [n][c] (workspace) = mean of y over hw; gate = sigmoid(W2 relu(W1 pooled)),
// w1 [mid][c], w2t [mid][c] (fc2 transposed), mid <= 64; out = relu(gate * y + shortcut).  gate_out [n][c] may be NULL.  out may be y.
hipError_t anysize_se_tail(hipStream_t stream, const float* y, const float* shortcut, int n, int hw, int c, int mid, const float* w1,
                           const float* w2t, float* pooled, float* out, float* gate_out);
// GeM (attention_pooling.py:58-60) + BNNeck: g = (mean over hw of clamp(x, 1e-6)^p)^(1/p), emb = g * scale + shift.  p [1] on the device.
// gem_out [n][c] may be NULL.
hipError_t anysize_gem(hipStream_t stream, const float* x, int n, int hw, int c, const float* p, const float* scale, const float* shift,
                       float* gem_out, float* emb);
// fp32 NCHW [n][3][h][w] -> NHWC [n][h][w][3]; mirror != 0: output column ox from input column w - 1 - ox (the flipped view of the flip-TTA
// descriptor without a mirrored copy of the NCHW batch).
hipError_t anysize_nchw_to_nhwc3(hipStream_t stream, const float* x, int n, int h, int w, int mirror, float* out);
// Extractor._preprocess (feature_extractor.py:31-46) to H x W with a caller's Normalize: u8 / 255 -> cv2 INTER_LINEAR -> (v - mean[c]) / std[c],
// NHWC out.  The taps and the roundings of resize_norm_kernel (elementwise.hip); mean = std = 0.5 gives its bits.
hipError_t anysize_resize_norm(hipStream_t stream, const uint8_t* packed, const long long* offsets, const int* hw, int n, int H, int W,
                               int pitch, const float* mean_std6_host, float* out);
}
