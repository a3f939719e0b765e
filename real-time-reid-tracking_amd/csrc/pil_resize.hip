// Pillow's 8-bit bilinear resize, bit for bit, and ToTensor + Normalize as a table lookup: the evaluation script's transform
// (reid/data_transforms.py:56-127, transforms.Resize((H, W)) on an RGB PIL image -> ToTensor -> Normalize) for the *_images_u8 entries.
//
// Resample.c makes two passes over an 8-bit image, the horizontal one first into a uint8 image, the vertical one on that ROUNDED image;
// each output value is clip8(((1 << 21) + sum_x in[xmin + x] * k[x]) >> 22) with an int32 accumulator and 22-bit fixed-point coefficients
// that depend on (in_size, out_size) alone.  The coefficients are computed on the host in double (pil_resize_coeffs below, Pillow's
// precompute_coeffs and normalize_coeffs_8bpc restated), once per distinct (in, out) pair of a call; the kernels do integer arithmetic
// only, so there is nothing to round differently.  A pass whose size does not change gets k = {1 << 22, 0} from the same rules and
// copies its input.
//
// Two launches with the uint8 intermediate [h][out_w][3] in HBM rather than one fused launch with a band of it in LDS: see DESIGN.md
// section 4.  One thread per output pixel (all three channels), the grid's y dimension walks the images.
//
// Built as a library of its own, libreid_hip_pil_resize.so (pil_resize.h): libreid_hip.so, its dependencies and its kernel list
// (tests/golden/kernels.json) stay what they were; this library's kernels are held to tests/golden/kernels_pil_resize.json.
#include "pil_resize.h"
#include <math.h>

namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;   // Resample.c PRECISION_BITS
constexpr int kMaxSide = 4096;               // 255 * (sum of |k| <= 2^22 + ksize / 2) stays far inside int32 for any ksize this allows
constexpr int kMaxOut = 1024;

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> kPrecisionBits;     // arithmetic shift, as Pillow's clip8
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// src image [h][w][3] -> mid image [h][out_w][3].  Reads: columns xmin .. xmin + xmax - 1 <= w - 1 of row y < h (pil_resize_coeffs
// guarantees xmin + xmax <= in_size); writes: pixel p < h * out_w of the image's own intermediate.
__global__ __launch_bounds__(256) void pil_resize_h_kernel(const uint8_t* __restrict__ src, const long long* __restrict__ offsets,
                                                           const int* __restrict__ hw, int n, int out_w, const int32_t* __restrict__ tables,
                                                           const PilImage* __restrict__ images, uint8_t* __restrict__ mid) {
    for (int img = blockIdx.y; img < n; img += gridDim.y) {
        const int h = hw[2 * img], w = hw[2 * img + 1];
        const PilImage it = images[img];
        const int32_t* bnd = tables + it.h_tab;
        const int32_t* kk = bnd + 2 * out_w;
        const uint8_t* s = src + offsets[img];
        uint8_t* d = mid + it.mid;
        const int total = h * out_w;
        for (int p = blockIdx.x * 256 + threadIdx.x; p < total; p += gridDim.x * 256) {
            const int y = p / out_w, xx = p - y * out_w;
            const int xmin = bnd[2 * xx], xmax = bnd[2 * xx + 1];
            const uint8_t* r = s + ((long long)y * w + xmin) * 3;
            const int32_t* k = kk + xx * it.h_ksize;
            int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
            for (int x = 0; x < xmax; ++x) {
                const int kv = k[x];
                a0 += (int)r[3 * x] * kv;
                a1 += (int)r[3 * x + 1] * kv;
                a2 += (int)r[3 * x + 2] * kv;
            }
            uint8_t* o = d + (long long)p * 3;
            o[0] = (uint8_t)clip8(a0);
            o[1] = (uint8_t)clip8(a1);
            o[2] = (uint8_t)clip8(a2);
        }
    }
}

// mid image [h][out_w][3] -> u8_out [out_h][out_w][3] (optional) and f32_out [3][out_h][out_w] = table[c][value].  Reads: rows
// ymin .. ymin + ymax - 1 <= h - 1 of the intermediate; writes: pixel p < out_h * out_w of image img < n.
__global__ __launch_bounds__(256) void pil_resize_v_kernel(const uint8_t* __restrict__ mid, int n, int out_h, int out_w,
                                                           const int32_t* __restrict__ tables, const PilImage* __restrict__ images,
                                                           const float* __restrict__ table, uint8_t* __restrict__ u8_out,
                                                           float* __restrict__ f32_out) {
    __shared__ float lut[768];
    for (int i = threadIdx.x; i < 768; i += 256) lut[i] = table[i];
    __syncthreads();
    const int total = out_h * out_w;
    const long long row = (long long)out_w * 3;
    for (int img = blockIdx.y; img < n; img += gridDim.y) {
        const PilImage it = images[img];
        const int32_t* bnd = tables + it.v_tab;
        const int32_t* kk = bnd + 2 * out_h;
        const uint8_t* m = mid + it.mid;
        for (int p = blockIdx.x * 256 + threadIdx.x; p < total; p += gridDim.x * 256) {
            const int yy = p / out_w, xx = p - yy * out_w;
            const int ymin = bnd[2 * yy], ymax = bnd[2 * yy + 1];
            const uint8_t* r = m + (long long)ymin * row + xx * 3;
            const int32_t* k = kk + yy * it.v_ksize;
            int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
            for (int y = 0; y < ymax; ++y) {
                const int kv = k[y];
                a0 += (int)r[0] * kv;
                a1 += (int)r[1] * kv;
                a2 += (int)r[2] * kv;
                r += row;
            }
            const int v0 = clip8(a0), v1 = clip8(a1), v2 = clip8(a2);
            if (u8_out) {
                uint8_t* o = u8_out + ((long long)img * total + p) * 3;
                o[0] = (uint8_t)v0;
                o[1] = (uint8_t)v1;
                o[2] = (uint8_t)v2;
            }
            float* f = f32_out + (long long)img * 3 * total + p;
            f[0] = lut[v0];
            f[total] = lut[256 + v1];
            f[2 * (long long)total] = lut[512 + v2];
        }
    }
}

}  // namespace

extern "C" int pil_resize_max_side(void) { return kMaxSide; }
extern "C" int pil_resize_max_out(void) { return kMaxOut; }

// Resample.c precompute_coeffs (bilinear_filter, support 1.0) + normalize_coeffs_8bpc.  Every operation below is the double operation
// Pillow's C performs, in its order; a fused multiply-add would round (xx + 0.5) * scale - support differently.
extern "C" int pil_resize_coeffs(int in_size, int out_size, int32_t* k, int32_t* bounds, int* ksize_out) {
#pragma clang fp contract(off)
    if (in_size < 1 || out_size < 1 || !ksize_out) return -1;
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    *ksize_out = ksize;
    if (!k && !bounds) return 0;
    if (!k || !bounds) return -1;
    const double ss = 1.0 / filterscale;
    double w[2 * kMaxSide + 3];
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        if (xmax > ksize) return -1;   // cannot happen: xmax <= 2 * support + 1
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            double a = (x + xmin - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            const double v = a < 1.0 ? 1.0 - a : 0.0;
            w[x] = v;
            ww += v;
        }
        int32_t* kx = k + (size_t)xx * ksize;
        for (int x = 0; x < xmax; ++x) {
            double v = w[x];
            if (ww != 0.0) v /= ww;
            kx[x] = v < 0 ? (int)(-0.5 + v * (1 << kPrecisionBits)) : (int)(0.5 + v * (1 << kPrecisionBits));
        }
        for (int x = xmax; x < ksize; ++x) kx[x] = 0;
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    return 0;
}

extern "C" void pil_resize_norm_table(const float* mean_std6, float* table) {
#pragma clang fp contract(off)
    for (int c = 0; c < 3; ++c)
        for (int v = 0; v < 256; ++v) {
            const float t = (float)v / 255.0f;
            const float u = t - mean_std6[c];
            table[c * 256 + v] = u / mean_std6[3 + c];
        }
}

extern "C" hipError_t pil_resize_launch(hipStream_t stream, const uint8_t* src, const long long* offsets, const int* hw, int n, int max_h,
                                        int out_h, int out_w, const int32_t* tables, const PilImage* images, const float* table, uint8_t* mid,
                                        uint8_t* u8_out, float* f32_out) {
    if (!src || !offsets || !hw || !tables || !images || !table || !mid || !f32_out || n < 1 || max_h < 1 || max_h > kMaxSide || out_h < 1 ||
        out_h > kMaxOut || out_w < 1 || out_w > kMaxOut)
        return hipErrorInvalidValue;
    const int gy = n < 32768 ? n : 32768;
    const long long hp = ((long long)max_h * out_w + 255) / 256, vp = ((long long)out_h * out_w + 255) / 256;
    hipLaunchKernelGGL(pil_resize_h_kernel, dim3((unsigned)(hp < 1024 ? hp : 1024), gy), dim3(256), 0, stream, src, offsets, hw, n, out_w, tables,
                       images, mid);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pil_resize_v_kernel, dim3((unsigned)(vp < 1024 ? vp : 1024), gy), dim3(256), 0, stream, (const uint8_t*)mid, n, out_h, out_w,
                       tables, images, table, u8_out, f32_out);
    return hipGetLastError();
}
