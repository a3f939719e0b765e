// Device arithmetic of the Swin uint8 front ends, shared by swin_crop_front_kernel (swin_crops.hip) and its mirrored form
// swin_crop_front_mirror_kernel (swin_eval.hip): one definition, so the two kernels round every tap and every pixel alike.
// `#pragma clang fp contract(off)` is lexical: it sits in the two functions below and travels with them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

namespace {

struct MeanStd {
    float mean[3], std[3];
};

// resize_norm_kernel's tap (elementwise.hip lin_tap), restated: source index s and weight f of destination index d, dst <- src pixels
__device__ __forceinline__ void crop_tap(int d, int dst, int src, int& s, float& f) {
#pragma clang fp contract(off)
    const double scale = (double)src / (double)dst;
    float fx = (float)(((double)d + 0.5) * scale - 0.5);
    int sx = (int)floorf(fx);
    fx = fx - (float)sx;
    if (sx < 0) { sx = 0; fx = 0.f; }
    if (sx >= src - 1) { sx = src - 1; fx = 0.f; }
    s = sx;
    f = fx;
}

// one resized, normalised pixel (3 channels) from its four taps; row0 / row1 = the two source rows, x0 / x1 = the two columns (pixels)
__device__ __forceinline__ void crop_pixel(const uint8_t* __restrict__ row0, const uint8_t* __restrict__ row1, int x0, int x1, float fx,
                                           float fy, const MeanStd& ms, float* __restrict__ v3) {
#pragma clang fp contract(off)
    const float gx = 1.0f - fx, gy = 1.0f - fy;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float p00 = (float)row0[x0 * 3 + c] / 255.0f;
        const float p01 = (float)row0[x1 * 3 + c] / 255.0f;
        const float p10 = (float)row1[x0 * 3 + c] / 255.0f;
        const float p11 = (float)row1[x1 * 3 + c] / 255.0f;
        const float r0 = p00 * gx + p01 * fx;
        const float r1 = p10 * gx + p11 * fx;
        const float v = r0 * gy + r1 * fy;
        v3[c] = (v - ms.mean[c]) / ms.std[c];
    }
}

}  // namespace
