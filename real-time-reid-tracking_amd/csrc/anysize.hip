// libreid_hip_anysize.so: the block tails of ResNet18-IBN-SE for any map size (anysize.h).
//
// Without the 128-pixel tiles of the 256 x 128 forward no convolution epilogue can hand per-image column sums on (a tile of the generic
// GEMM crosses image borders), so the three reductions over an image's pixels - InstanceNorm statistics, the SE average pool, GeM - are
// passes of their own here, and they share ONE structure: grid (c / 32, images), 256 threads = 8 channel quads x 32 pixel groups.  A lane
// reads 16 bytes, the 8 lanes of a pixel one 128-byte line, a wave 8 pixels per trip with four trips in flight.  A thread adds its pixels
// pg, pg + 32, ... in fp64 (a product of two floats is exact there, so sum and sum of squares carry no cancellation into mean and
// variance), the 8 pixel groups of a wave are combined with three shuffles, the four waves through LDS in a fixed order: the result does
// not depend on the launch, and hw below 64 or odd only leaves lanes without pixels.
#include "anysize.h"
#include <math.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int QUADS = 8;     // 32 channels per block
constexpr int PGS = 32;      // pixel groups

// v[k] of every thread -> the block's total for that thread's channel quad, k = 0 .. K - 1.  red: K * 32 doubles.  Ends with a barrier.
template <int K>
__device__ __forceinline__ void quad_totals(double (&v)[K], double* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, quad = threadIdx.x & (QUADS - 1);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        v[k] += __shfl_xor(v[k], 8);
        v[k] += __shfl_xor(v[k], 16);
        v[k] += __shfl_xor(v[k], 32);
    }
    if (lane < QUADS) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[(wave * QUADS + lane) * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k)
        v[k] = ((red[(0 * QUADS + quad) * K + k] + red[(1 * QUADS + quad) * K + k]) + red[(2 * QUADS + quad) * K + k]) +
               red[(3 * QUADS + quad) * K + k];
    __syncthreads();
}

// the pixels pg, pg + 32, ... of one image's channel quad through f(v), four loads in flight
template <class F>
__device__ __forceinline__ void walk_pixels(const float* __restrict__ xi, int hw, int c, int pg, F f) {
    int px = pg;
    for (; px + 3 * PGS < hw; px += 4 * PGS) {
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *(const f32x4*)(xi + (long long)(px + PGS * u) * c);
#pragma unroll
        for (int u = 0; u < 4; ++u) f(v[u]);
    }
    for (; px < hw; px += PGS) f(*(const f32x4*)(xi + (long long)px * c));
}

__global__ __launch_bounds__(256) void any_norm_kernel(float* __restrict__ x, int hw, int c, int half, const float* __restrict__ in_gamma,
                                                       const float* __restrict__ in_beta, const float* __restrict__ bn_scale,
                                                       const float* __restrict__ bn_shift) {
    __shared__ double red[8 * 32];
    const int img = blockIdx.y, c0 = blockIdx.x * 32;
    const int quad = threadIdx.x & (QUADS - 1), pg = threadIdx.x >> 3;
    const int ch = c0 + quad * 4;
    float* xi = x + (long long)img * hw * c + ch;
    f32x4 a, b;
    if (c0 < half) {   // block-uniform
        double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        walk_pixels(xi, hw, c, pg, [&](const f32x4 v) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = (double)v[e];
                s[e] += d;
                s[4 + e] += d * d;
            }
        });
        quad_totals<8>(s, red);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double mean = s[e] / hw;
            double var = s[4 + e] / hw - mean * mean;
            if (var < 0.0) var = 0.0;
            const double inv = 1.0 / sqrt(var + 1e-5);
            a[e] = (float)(inv * (double)in_gamma[ch + e]);
            b[e] = (float)((double)in_beta[ch + e] - mean * inv * (double)in_gamma[ch + e]);
        }
    } else {
        a = *(const f32x4*)(bn_scale + ch - half);
        b = *(const f32x4*)(bn_shift + ch - half);
    }
    for (int px = pg; px < hw; px += PGS) {
        f32x4* ptr = (f32x4*)(xi + (long long)px * c);
        f32x4 v = *ptr;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(__builtin_fmaf(v[e], a[e], b[e]), 0.f);
        *ptr = v;
    }
}

__global__ __launch_bounds__(256) void any_pool_kernel(const float* __restrict__ y, int hw, int c, float* __restrict__ pooled) {
    __shared__ double red[4 * 32];
    const int img = blockIdx.y;
    const int quad = threadIdx.x & (QUADS - 1), pg = threadIdx.x >> 3;
    const int ch = blockIdx.x * 32 + quad * 4;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    walk_pixels(y + (long long)img * hw * c + ch, hw, c, pg, [&](const f32x4 v) {
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] += (double)v[e];
    });
    quad_totals<4>(s, red);
    if (pg == 0) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (float)(s[e] / hw);
        *(f32x4*)(pooled + (long long)img * c + ch) = o;
    }
}

__device__ __forceinline__ float wave_total(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// grid (slices, images): every block forms its image's gate (a few thousand multiply-adds), then streams rows [blockIdx.x * rows, + rows)
__global__ __launch_bounds__(256) void any_se_tail_kernel(const float* __restrict__ pooled_g, int c, int mid, int hw, int rows,
                                                          const float* __restrict__ w1, const float* __restrict__ w2t,
                                                          const float* __restrict__ y, const float* __restrict__ sc, float* __restrict__ out,
                                                          float* __restrict__ gate_out) {
    __shared__ __attribute__((aligned(16))) float pooled[512];
    __shared__ float hid[64];
    __shared__ __attribute__((aligned(16))) float gate[512];
    const int img = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int ch = tid; ch < c; ch += 256) pooled[ch] = pooled_g[(long long)img * c + ch];
    __syncthreads();
    for (int m = wave; m < mid; m += 4) {   // wave-uniform
        float acc = 0.f;
        for (int ch = lane; ch < c; ch += 64) acc = __builtin_fmaf(w1[(long long)m * c + ch], pooled[ch], acc);
        acc = wave_total(acc);
        if (lane == 0) hid[m] = fmaxf(acc, 0.f);
    }
    __syncthreads();
    for (int ch = tid; ch < c; ch += 256) {
        float acc = 0.f;
        for (int m = 0; m < mid; ++m) acc = __builtin_fmaf(w2t[(long long)m * c + ch], hid[m], acc);
        const float g = 1.0f / (1.0f + expf(-acc));
        gate[ch] = g;
        if (gate_out && blockIdx.x == 0) gate_out[(long long)img * c + ch] = g;
    }
    __syncthreads();
    const int c4n = c >> 2;
    const int r0 = blockIdx.x * rows;
    const int nrows = min(rows, hw - r0);
    if (nrows <= 0) return;
    const long long base = ((long long)img * hw + r0) * c;
    const int total4 = nrows * c4n;
    const int cc = tid % c4n;   // 256 % c4n == 0 (c = 64 .. 512 in powers of two): a thread keeps its channel quad
    const f32x4 g = *(const f32x4*)&gate[cc * 4];
    auto finish = [&](const f32x4 yy, const f32x4 rr, long long off) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaxf(__builtin_fmaf(g[e], yy[e], rr[e]), 0.f);
        *(f32x4*)(out + off) = o;
    };
    int i = tid;
    for (; i + 3 * 256 < total4; i += 4 * 256) {
        f32x4 yy[4], rr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            yy[u] = *(const f32x4*)(y + base + (long long)(i + u * 256) * 4);
            rr[u] = *(const f32x4*)(sc + base + (long long)(i + u * 256) * 4);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) finish(yy[u], rr[u], base + (long long)(i + u * 256) * 4);
    }
    for (; i < total4; i += 256) {
        const long long off = base + (long long)i * 4;
        finish(*(const f32x4*)(y + off), *(const f32x4*)(sc + off), off);
    }
}

// x^p for a trained p as gem_neck_kernel (elementwise.hip) forms it: exp2(p log2 x) on the transcendental unit, the exponent raised by 64
// where the result would be subnormal
__global__ __launch_bounds__(256) void any_gem_kernel(const float* __restrict__ x, int hw, int c, const float* __restrict__ p_ptr,
                                                      const float* __restrict__ scale, const float* __restrict__ shift,
                                                      float* __restrict__ gem_out, float* __restrict__ emb) {
    __shared__ double red[4 * 32];
    const int img = blockIdx.y;
    const int quad = threadIdx.x & (QUADS - 1), pg = threadIdx.x >> 3;
    const int ch = blockIdx.x * 32 + quad * 4;
    const float p = p_ptr[0];
    const bool cube = p == 3.0f;
    auto powp = [&](float f) {
        const float e = p * __builtin_amdgcn_logf(f);
        return e < -126.f ? __builtin_amdgcn_exp2f(e + 64.f) * 0x1p-64f : __builtin_amdgcn_exp2f(e);
    };
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    walk_pixels(x + (long long)img * hw * c + ch, hw, c, pg, [&](const f32x4 v) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float f = fmaxf(v[e], 1e-6f);
            s[e] += (double)(cube ? f * f * f : powp(f));
        }
    });
    quad_totals<4>(s, red);
    if (pg == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float m = (float)(s[e] / hw);
            const float g = cube ? cbrtf(m) : powf(m, 1.0f / p);
            if (gem_out) gem_out[(long long)img * c + ch + e] = g;
            emb[(long long)img * c + ch + e] = __builtin_fmaf(g, scale[ch + e], shift[ch + e]);
        }
    }
}

__global__ void any_nchw_to_nhwc3_kernel(const float* __restrict__ x, long long npix, int h, int w, int mirror, float* __restrict__ out) {
    const int hw = h * w;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < npix; i += (long long)gridDim.x * blockDim.x) {
        const long long img = i / hw;
        const int p = (int)(i - img * hw);
        const int oy = p / w, ox = p - oy * w;
        const float* src = x + img * 3 * hw + (long long)oy * w + (mirror ? w - 1 - ox : ox);
        float* dst = out + i * 3;
        dst[0] = src[0];
        dst[1] = src[hw];
        dst[2] = src[2 * hw];
    }
}

struct MeanStd { float v[6]; };

__device__ __forceinline__ void lin_tap(int d, int dst, int src, int& s, float& f) {
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

__global__ void any_resize_norm_kernel(const uint8_t* __restrict__ packed, const long long* __restrict__ offsets, const int* __restrict__ hw,
                                       int n, int H, int W, int pitch, MeanStd ms, float* __restrict__ out) {
#pragma clang fp contract(off)
    const long long total = (long long)n * H * W;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int img = (int)(i / (H * W));
        const int rem = (int)(i - (long long)img * H * W);
        const int dy = rem / W, dx = rem - dy * W;
        const int h = hw[2 * img], w = hw[2 * img + 1];
        const uint8_t* src = packed + offsets[img];
        const long long ps = pitch ? pitch : w;
        int sx, sy;
        float fx, fy;
        lin_tap(dx, W, w, sx, fx);
        lin_tap(dy, H, h, sy, fy);
        const int sx1 = min(sx + 1, w - 1), sy1 = min(sy + 1, h - 1);
        const float gx = 1.0f - fx, gy = 1.0f - fy;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float p00 = (float)src[(sy * ps + sx) * 3 + ch] / 255.0f;
            const float p01 = (float)src[(sy * ps + sx1) * 3 + ch] / 255.0f;
            const float p10 = (float)src[(sy1 * ps + sx) * 3 + ch] / 255.0f;
            const float p11 = (float)src[(sy1 * ps + sx1) * 3 + ch] / 255.0f;
            const float r0 = p00 * gx + p01 * fx;
            const float r1 = p10 * gx + p11 * fx;
            const float v = r0 * gy + r1 * fy;
            out[i * 3 + ch] = (v - ms.v[ch]) / ms.v[3 + ch];
        }
    }
}

inline int grid_for(long long work) {
    const long long g = (work + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

inline bool shape_ok(int n, int hw, int c) { return n >= 1 && n <= 65535 && hw >= 1 && c >= 64 && c <= 512 && (c & (c - 1)) == 0; }

}  // namespace

extern "C" hipError_t anysize_norm(hipStream_t stream, float* x, int n, int hw, int c, int half, const float* in_gamma, const float* in_beta,
                                   const float* bn_scale, const float* bn_shift) {
    if (!x || !shape_ok(n, hw, c) || half < 32 || half > c || half % 32 || !in_gamma || !in_beta || (bn_scale == nullptr) != (bn_shift == nullptr))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(any_norm_kernel, dim3((bn_scale ? c : half) / 32, n), dim3(256), 0, stream, x, hw, c, half, in_gamma, in_beta, bn_scale,
                       bn_shift);
    return hipGetLastError();
}

extern "C" hipError_t anysize_se_tail(hipStream_t stream, const float* y, const float* shortcut, int n, int hw, int c, int mid, const float* w1,
                                      const float* w2t, float* pooled, float* out, float* gate_out) {
    if (!y || !shortcut || !w1 || !w2t || !pooled || !out || !shape_ok(n, hw, c) || mid < 1 || mid > 64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(any_pool_kernel, dim3(c / 32, n), dim3(256), 0, stream, y, hw, c, pooled);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // ~8192 16-byte chunks per block: the gate (2 mid c multiply-adds and as many weights from L2) stays a small part of a block's work
    long long slices = ((long long)hw * (c / 4) + 8191) / 8192;
    if (slices > hw) slices = hw;
    if (slices > 65535) slices = 65535;
    const int rows = (int)((hw + slices - 1) / slices);
    hipLaunchKernelGGL(any_se_tail_kernel, dim3((hw + rows - 1) / rows, n), dim3(256), 0, stream, pooled, c, mid, hw, rows, w1, w2t, y, shortcut,
                       out, gate_out);
    return hipGetLastError();
}

extern "C" hipError_t anysize_gem(hipStream_t stream, const float* x, int n, int hw, int c, const float* p, const float* scale,
                                  const float* shift, float* gem_out, float* emb) {
    if (!x || !p || !scale || !shift || !emb || !shape_ok(n, hw, c)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(any_gem_kernel, dim3(c / 32, n), dim3(256), 0, stream, x, hw, c, p, scale, shift, gem_out, emb);
    return hipGetLastError();
}

extern "C" hipError_t anysize_nchw_to_nhwc3(hipStream_t stream, const float* x, int n, int h, int w, int mirror, float* out) {
    if (!x || !out || n < 1 || h < 1 || w < 1) return hipErrorInvalidValue;
    const long long npix = (long long)n * h * w;
    hipLaunchKernelGGL(any_nchw_to_nhwc3_kernel, dim3(grid_for(npix)), dim3(256), 0, stream, x, npix, h, w, mirror, out);
    return hipGetLastError();
}

extern "C" hipError_t anysize_resize_norm(hipStream_t stream, const uint8_t* packed, const long long* offsets, const int* hw, int n, int H, int W,
                                          int pitch, const float* mean_std6_host, float* out) {
    if (!packed || !offsets || !hw || !out || !mean_std6_host || n < 1 || H < 1 || W < 1 || pitch < 0) return hipErrorInvalidValue;
    MeanStd ms;
    for (int i = 0; i < 6; ++i) ms.v[i] = mean_std6_host[i];
    hipLaunchKernelGGL(any_resize_norm_kernel, dim3(grid_for((long long)n * H * W)), dim3(256), 0, stream, packed, offsets, hw, n, H, W, pitch,
                       ms, out);
    return hipGetLastError();
}
