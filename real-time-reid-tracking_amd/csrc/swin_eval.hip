// The Swin side of the evaluation script (reid/image_reid_inference.py with --backbone swin_v1 | swin_v2, :145-152, :202-208): what
// reid_swin_descriptor_* launch beyond the forward of reid_swin_embed_*.
//
//   inference_efficient (:112-123)   model(cat(img, flip(img))) -> cat(normalize(first output), normalize(second output)) per view
//   swin_transformer.py:422-423      eval mode returns (logits, x_norm): the first output is the LOGITS, so a Swin descriptor is
//                                    [normalize(logits) (num_class) | normalize(x_norm) (96)] - SERes18 returns (x_norm, logits)
//   :252-253, :267-268               descriptor = normalize((plain + mirrored) / 2)
//
// Two stems for the mirrored view, which read the source with reversed columns instead of making a mirrored copy of it (1.2 GB per 1024
// images at 448 x 224) - a saving of memory and of one launch, not of time - and the descriptor kernel, which runs the classifier of both
// views itself so that the logits never reach HBM.
//
// The stems repeat the arithmetic of the kernels they mirror, rounding for rounding: sfe_conv1_kernel's loop (swin.hip) and
// swin_crop_front_kernel's (swin_crops.hip; the taps and the pixel arithmetic are the shared functions of swin_crop_taps.h), under this
// file's default contraction, as there: acc = bias[co]; acc += wgt[co * 12 + k] * in[k], one FMA per step.
//
// Built as a library of its own, libreid_hip_swin_eval.so (swin_eval.h): libreid_hip.so, its dependencies and its kernel list
// (tests/golden/kernels.json) stay what they were; this library's kernels are held to tests/golden/kernels_swin_eval.json.
#include "swin_eval.h"
#include "swin_crop_taps.h"   // MeanStd, crop_tap, crop_pixel
#include <math.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kMaxClasses = 4096;
constexpr int kDim = 96;   // x_norm of the Swin-T (embed_dim)

// ---- ShadowFeatureExtraction's first convolution (swin_transformer.py:297) of the mirrored image: sfe_conv1_kernel with input column
// w - 1 - (2 ox + kw) where that kernel reads 2 ox + kw.  Reads stay inside image img: rows 2 oy + kh < h, columns in [0, w - 1].
__global__ void sfe_conv1_mirror_kernel(const float* __restrict__ x, int n, int h, int w, const float* __restrict__ wgt,
                                        const float* __restrict__ bias, float* __restrict__ out) {
    const int ho = h / 2, wo = w / 2;
    const long long total = (long long)n * ho * wo;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int ox = (int)(i % wo);
        const long long t = i / wo;
        const int oy = (int)(t % ho);
        const int img = (int)(t / ho);
        float in[12];  // (kh, kw, c)
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int kw = 0; kw < 2; ++kw)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    in[(kh * 2 + kw) * 3 + c] = x[(((long long)img * 3 + c) * h + 2 * oy + kh) * w + (w - 1 - (2 * ox + kw))];
        float* o = out + i * 12;
#pragma unroll
        for (int co = 0; co < 12; ++co) {
            float acc = bias[co];
#pragma unroll
            for (int k = 0; k < 12; ++k) acc += wgt[co * 12 + k] * in[k];
            o[co] = acc;
        }
    }
}

// ---- swin_crop_front_kernel (swin_crops.hip) with the resized image mirrored: output pixel (oy, ox) takes resized pixels
// (2 oy + kh, W - 1 - (2 ox + kw)).  Reads stay inside the window, as there: crop_tap clamps rows to [0, h - 1] and columns to [0, w - 1].
__global__ __launch_bounds__(256) void swin_crop_front_mirror_kernel(const uint8_t* __restrict__ src, const long long* __restrict__ offsets,
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
            crop_tap(W - 1 - (2 * ox + k), W, w, sx[k], fx[k]);
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

// ---- the descriptor
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sum over the block's 256 threads of up to four values at once: wavefront shuffles, then the four waves' partials through LDS, added
// in a fixed order.  `part` holds 16 floats no other phase of the kernel touches.
template <int N>
__device__ __forceinline__ void block_sums(float (&v)[N], float* part) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = wave_sum(v[i]);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int i = 0; i < N; ++i) part[(threadIdx.x >> 6) * N + i] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = (part[i] + part[N + i]) + (part[2 * N + i] + part[3 * N + i]);
}

__device__ __forceinline__ float dot4(const f32x4 w, const f32x4 x, float acc) {
    acc = fmaf(w.x, x.x, acc);
    acc = fmaf(w.y, x.y, acc);
    acc = fmaf(w.z, x.z, acc);
    return fmaf(w.w, x.w, acc);
}

// One block (256 threads) per image.  LDS, all of it dynamic (16-byte aligned base): se [2][96] the two views' x_norm, two partial-sum
// areas of 16 floats, then lg [views][ncp] the logits, ncp = num_class rounded up to 4 - 896 + views * ncp * 4 bytes, 33664 at the limit.
//   1  thread t computes logits t, t + 256, ...: one pass over the weight row in 16-byte loads serves both views (x_norm comes from LDS
//      as broadcast reads); k runs 0 .. 95 in order, one FMA per step, so a logit does not depend on the launch's shape;
//   2  the four norms (both views' logits and x_norm) in one block reduction;
//   3  element k of the row: its normalised value, averaged over the views; with two views it goes back to LDS and its square into the
//      last norm, then the row is written once.  A single view is already the concatenation of two unit vectors: the reference does not
//      renormalise it (inference_efficient), and neither does descriptor_kernel (postproc.hip).
// Rows are `ld` floats apart; only columns [0, num_class + 96) of row blockIdx.x are written.
__global__ __launch_bounds__(256) void swin_descriptor_kernel(const float* __restrict__ e1, const float* __restrict__ e2,
                                                              const float* __restrict__ cls_w, int nc, long long ld, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* se = (float*)smem;        // [2][96]
    float* part = se + 2 * kDim;     // [16] + [16]
    float* lg = part + 32;           // [views][ncp]
    const int r = blockIdx.x, tid = threadIdx.x;
    const bool two = e2 != nullptr;
    const int ncp = (nc + 3) & ~3;
    if (tid < kDim) se[tid] = e1[(long long)r * kDim + tid];
    else if (tid >= 128 && tid < 128 + kDim) se[kDim + tid - 128] = two ? e2[(long long)r * kDim + tid - 128] : 0.f;
    __syncthreads();

    float s[4] = {0.f, 0.f, 0.f, 0.f};   // squares: logits 1, logits 2, x_norm 1, x_norm 2
    const f32x4* x1 = (const f32x4*)se;
    const f32x4* x2 = (const f32x4*)(se + kDim);
    for (int k = tid; k < nc; k += 256) {
        const f32x4* wr = (const f32x4*)(cls_w + (long long)k * kDim);
        float a1 = 0.f, a2 = 0.f;
        if (two) {
#pragma unroll
            for (int j = 0; j < kDim / 4; ++j) {
                const f32x4 w = wr[j];
                a1 = dot4(w, x1[j], a1);
                a2 = dot4(w, x2[j], a2);
            }
            lg[ncp + k] = a2;
        } else {
#pragma unroll
            for (int j = 0; j < kDim / 4; ++j) a1 = dot4(wr[j], x1[j], a1);
        }
        lg[k] = a1;
        s[0] = fmaf(a1, a1, s[0]);
        s[1] = fmaf(a2, a2, s[1]);
    }
    if (tid < kDim) s[2] = se[tid] * se[tid];
    else if (tid >= 128 && tid < 128 + kDim) s[3] = se[kDim + tid - 128] * se[kDim + tid - 128];
    block_sums(s, part);
    const float nl1 = fmaxf(sqrtf(s[0]), 1e-12f), nl2 = fmaxf(sqrtf(s[1]), 1e-12f);
    const float ne1 = fmaxf(sqrtf(s[2]), 1e-12f), ne2 = fmaxf(sqrtf(s[3]), 1e-12f);

    const int d = nc + kDim;
    float* o = out + (long long)r * ld;
    if (!two) {
        for (int k = tid; k < d; k += 256) o[k] = k < nc ? lg[k] / nl1 : se[k - nc] / ne1;
        return;
    }
    // each thread reads and rewrites its own elements of lg / se: no barrier between the phases beyond the reductions' own
    float acc[1] = {0.f};
    for (int k = tid; k < d; k += 256) {
        float* p = k < nc ? lg + k : se + (k - nc);
        const float v = k < nc ? p[0] / nl1 : p[0] / ne1;
        const float u = k < nc ? p[ncp] / nl2 : p[kDim] / ne2;
        const float m = (v + u) / 2.0f;
        p[0] = m;
        acc[0] = fmaf(m, m, acc[0]);
    }
    block_sums(acc, part + 16);
    const float nrm = fmaxf(sqrtf(acc[0]), 1e-12f);
    for (int k = tid; k < d; k += 256) o[k] = (k < nc ? lg[k] : se[k - nc]) / nrm;
}

inline unsigned grid_for(long long work) {
    long long g = (work + 255) / 256;
    return (unsigned)(g > 4096 ? 4096 : g);   // 256 CUs x 16 blocks; the loops stride over the rest
}

}  // namespace

extern "C" int swin_eval_max_classes(void) { return kMaxClasses; }

extern "C" hipError_t swin_eval_conv1_mirror(hipStream_t stream, const float* x, int n, int h, int w, const float* c1_w, const float* c1_b,
                                             float* c1_out) {
    if (!x || !c1_w || !c1_b || !c1_out || n < 1 || h < 2 || w < 2 || (h & 1) || (w & 1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sfe_conv1_mirror_kernel, dim3(grid_for((long long)n * (h / 2) * (w / 2))), dim3(256), 0, stream, x, n, h, w, c1_w, c1_b,
                       c1_out);
    return hipGetLastError();
}

extern "C" hipError_t swin_eval_crop_front_mirror(hipStream_t stream, const uint8_t* src, const long long* offsets, const int* hw, int n, int H,
                                                  int W, int pitch, const float* mean_std6, const float* c1_w, const float* c1_b,
                                                  float* c1_out) {
    if (!src || !offsets || !hw || !mean_std6 || !c1_w || !c1_b || !c1_out || n < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || pitch < 0 ||
        ((uintptr_t)c1_out & 15))
        return hipErrorInvalidValue;
    MeanStd ms;
    for (int c = 0; c < 3; ++c) {
        ms.mean[c] = mean_std6[c];
        ms.std[c] = mean_std6[3 + c];
    }
    hipLaunchKernelGGL(swin_crop_front_mirror_kernel, dim3(grid_for((long long)n * (H / 2) * (W / 2))), dim3(256), 0, stream, src, offsets, hw,
                       n, H, W, pitch, ms, c1_w, c1_b, c1_out);
    return hipGetLastError();
}

extern "C" hipError_t swin_eval_descriptor(hipStream_t stream, const float* e1, const float* e2, const float* cls_w, int n, int num_class,
                                           long long ld, float* out) {
    if (!e1 || !cls_w || !out || n < 1 || num_class < 1 || num_class > kMaxClasses || ld < (long long)num_class + kDim ||
        (((uintptr_t)e1 | (uintptr_t)e2 | (uintptr_t)cls_w) & 15))
        return hipErrorInvalidValue;
    const int ncp = (num_class + 3) & ~3;
    const size_t lds = (size_t)(2 * kDim + 32 + (e2 ? 2 : 1) * ncp) * sizeof(float);
    hipLaunchKernelGGL(swin_descriptor_kernel, dim3((unsigned)n), dim3(256), lds, stream, e1, e2, cls_w, num_class, ld, out);
    return hipGetLastError();
}
