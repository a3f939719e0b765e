// Front end of the Swin uint8 entry points: uint8 crops (packed one after the other, or windows of one frame) -> the output of
// ShadowFeatureExtraction's first convolution (swin_transformer.py:297), in ONE kernel.  The two-step path writes the resized, normalised
// fp32 image (602 KB per 224 x 224 crop) on the host, uploads it and reads it back in sfe_conv1_kernel (swin.hip); here the four resized
// pixels under a 2x2 stride-2 tap live in the thread's registers and the fp32 image never exists.
//
// The arithmetic is the two-step path's, rounding for rounding, so that the embeddings are the same bits:
//   resize     resize_norm_kernel's (elementwise.hip): u8 / 255, half-pixel centres, clamp to the window's border, horizontal then
//              vertical lerp, every * and + rounded on its own (numpy's arithmetic; tests/swin_crops_ref.py);
//   normalise  (v - mean[c]) / std[c]: a true subtraction and a true division (reid/data_transforms.py:64 Normalize);
//   convolve   sfe_conv1_kernel's loop: acc = bias[co]; acc += wgt[co * 12 + k] * in[k], k = (kh, kw, c), under this file's default
//              contraction - as in swin.hip, the compiler fuses each step into one FMA.
// `#pragma clang fp contract(off)` is lexical (see the comment above lin_tap in elementwise.hip): it sits in the two functions that hold
// the resize / normalise arithmetic and not in the kernel body, whose only arithmetic is the convolution.
//
// Built as a library of its own, libreid_hip_swin_crops.so (swin_crops.h): libreid_hip.so, its dependencies and its kernel list
// (tests/golden/kernels.json) stay what they were; this library's kernel is held to tests/golden/kernels_swin_crops.json.
#include "swin_crops.h"
#include "swin_crop_taps.h"   // MeanStd, crop_tap, crop_pixel
#include <math.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

// One thread per output pixel of c1 (grid-stride): its 2x2 input pixels are resized pixels (2 oy + kh, 2 ox + kw) of window img.  Reads
// stay inside the window: rows sy, sy1 in [0, h - 1], columns sx, sx1 in [0, w - 1] (crop_tap clamps), i.e. bytes
// [offsets[img], offsets[img] + ((h - 1) pitch + w) 3) of src, which the callers check against the buffer.  12 outputs = three 16-byte
// stores; consecutive threads write consecutive 48-byte pixels.
__global__ __launch_bounds__(256) void swin_crop_front_kernel(const uint8_t* __restrict__ src, const long long* __restrict__ offsets,
                                                              const int* __restrict__ hw, int n, int H, int W, int pitch, MeanStd ms,
                                                              const float* __restrict__ wgt, const float* __restrict__ bias,
                                                              float* __restrict__ out) {
    const int ho = H / 2, wo = W / 2;
    const long long total = (long long)n * ho * wo;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int ox = (int)(i % wo);
        const long long t = i / wo;
        const int oy = (int)(t % ho);
        const int img = (int)(t / ho);
        const int h = hw[2 * img], w = hw[2 * img + 1];
        const uint8_t* base = src + offsets[img];
        const long long ps = (long long)(pitch ? pitch : w) * 3;   // bytes per source row
        int sx[2], sx1[2], sy[2], sy1[2];
        float fx[2], fy[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            crop_tap(2 * ox + k, W, w, sx[k], fx[k]);
            crop_tap(2 * oy + k, H, h, sy[k], fy[k]);
            sx1[k] = min(sx[k] + 1, w - 1);
            sy1[k] = min(sy[k] + 1, h - 1);
        }
        float in[12];  // (kh, kw, c)
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int kw = 0; kw < 2; ++kw)
                crop_pixel(base + sy[kh] * ps, base + sy1[kh] * ps, sx[kw], sx1[kw], fx[kw], fy[kh], ms, in + (kh * 2 + kw) * 3);
        float o[12];
#pragma unroll
        for (int co = 0; co < 12; ++co) {
            float acc = bias[co];
#pragma unroll
            for (int k = 0; k < 12; ++k) acc += wgt[co * 12 + k] * in[k];
            o[co] = acc;
        }
        f32x4* dst = (f32x4*)(out + i * 12);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const f32x4 v = {o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]};
            dst[q] = v;
        }
    }
}

}  // namespace

extern "C" hipError_t swin_crops_front(hipStream_t stream, const uint8_t* src, const long long* offsets, const int* hw, int n, int H, int W,
                                       int pitch, const float* mean_std6, const float* c1_w, const float* c1_b, float* c1_out) {
    if (!src || !offsets || !hw || !mean_std6 || !c1_w || !c1_b || !c1_out || n < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || pitch < 0 ||
        ((uintptr_t)c1_out & 15))
        return hipErrorInvalidValue;
    MeanStd ms;
    for (int c = 0; c < 3; ++c) {
        ms.mean[c] = mean_std6[c];
        ms.std[c] = mean_std6[3 + c];
    }
    const long long total = (long long)n * (H / 2) * (W / 2);
    long long g = (total + 255) / 256;
    if (g > 4096) g = 4096;   // 256 CUs x 16 blocks; the loop strides over the rest
    hipLaunchKernelGGL(swin_crop_front_kernel, dim3((unsigned)g), dim3(256), 0, stream, src, offsets, hw, n, H, W, pitch, ms, c1_w, c1_b,
                       c1_out);
    return hipGetLastError();
}
