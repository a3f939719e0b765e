// Attention tails of the sibling backbones for the fp16-storage mode (precision 1): f16 NHWC activations [img][h][w][c], fp32 (fp64
// where sums could cancel) arithmetic inside, one rounding to f16 at the end.  The arithmetic and the parameter layouts are those of
// attention_f32.hip; the launch shapes are not.
//   * CARes18_IBN: out = relu(TripletAttention(y) + shortcut)   (triplet_attention.py:46-101, CARes18.py:150-157)
//   * EMARes18_IBN: out = relu(EMA(y) + shortcut)               (EMA_Res18.py:10-38,79-86)
// Built as a library of its own, libreid_hip_siblings_f16.so, which api.hip opens the first time a sibling checkpoint runs in mode 1
// (siblings_f16.h): libreid_hip.so, its dependencies and its kernel list (tests/golden/kernels.json) stay what they were; this
// library's kernels are held to tests/golden/kernels_siblings_f16.json the same way.
//
// TripletAttention, three launches:
//   ta_stats: grid (images, row slices).  A block copies its R rows (R W C = 32768 elements, 64 KB: 16 / 16 / 16 / 8 rows of the four
//     layers, so 4 / 2 / 1 / 2 slices) into LDS with 16-byte loads - the only time y's bytes leave HBM for the statistics - and
//     takes all three ZPool reductions from there.  Over C (per pixel): from the registers of the copy, eight channels per lane,
//     xor shuffles across the C/8 lanes of a pixel.  Over W (per row and channel): complete inside the slice.  Over H (per column
//     and channel): a slice leaves (sum, M2 about its own mean) per (w, c); the gate kernel merges the slices (Chan et al.), every
//     term of which is non-negative.  All sums are fp64 (the inputs are f16: products and sums are exact to 2^-53), rounded once.
//   ta_gate: grid (images, 3 planes): the plane's (std, mean) maps into LDS, conv 7x7 + BN + sigmoid in fp32, as ta_gate_kernel.
//     The (c, w) gate is written as [w][c], so the apply pass reads every gate along c.
//   ta_apply: eight channels per lane: y and the shortcut read once (16 bytes each), out written once, rounded by cvt_f16_rn.
// The slicing depends on the geometry alone, so an image's result does not depend on the batch or on its place in it.
//
// EMA: one block per (image, channel group) with the group's slab in LDS as fp32, as ema_tail_kernel; a lane loads the cg channels
// of a pixel as one vector (4 - 32 bytes, at a stride of C halves: one instruction per pixel instead of cg, but a wave's load still
// touches 64 cache lines, which the 32 group blocks of an image share in L2 - with one block per (image, group) the reads cannot be
// contiguous across lanes), the parameters sit in LDS, the row means are shuffle reductions (a lane per element
// instead of a lane per row, which read LDS with a stride of W floats).  x1, x2, the GroupNorm statistics and both softmaxes are fp32.
#include "siblings_f16.h"
#include "lin_math.h"   // cvt_f16_rn
#include <math.h>
#include <atomic>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16;
typedef f16 half2v __attribute__((ext_vector_type(2)));
typedef f16 half8 __attribute__((ext_vector_type(8)));

namespace {

const int TA_SLICE_ELEMS = 32768;   // f16 elements of a row slice: 64 KB of LDS, two blocks per CU

inline int ta_rows(int H, int W, int C) {
    const int r = TA_SLICE_ELEMS / (W * C);
    return r < H ? r : H;
}
// per-image workspace, in floats: maps_hw [2][H][W] | maps_hc [2][H][C] | cw partials [S][W][C][2] | gates [H][W] | [W][C] | [H][C]
struct TaWs {
    long long hc, part, gates, per;
};
__host__ __device__ inline TaWs ta_ws(int H, int W, int C, int S) {
    TaWs o;
    o.hc = 2LL * H * W;
    o.part = o.hc + 2LL * H * C;
    o.gates = o.part + 2LL * S * W * C;
    o.per = o.gates + (long long)H * W + (long long)W * C + (long long)H * C;
    return o;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of (kernel, device): set once per pair, not per launch (a tracking frame
// is eight tails).  slot = the kernel; the bit of a device is raised after its call succeeded, so a racing thread at worst repeats it.
inline hipError_t lds_limit_once(int slot, const void* fn, int bytes) {
    static std::atomic<unsigned long long> done[6];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (dev < 64 && (done[slot].load(std::memory_order_acquire) & bit)) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && dev < 64) done[slot].fetch_or(bit, std::memory_order_release);
    return e;
}

__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// (unbiased std, mean) of n values from their sum and sum of squares (fp64), as torch.std / torch.mean
__device__ __forceinline__ void put_std_mean(float* dst, long long plane, long long idx, double s1, double s2, int n) {
    const double mean = s1 / n;
    double var = (s2 - n * mean * mean) / (n - 1);
    if (var < 0.0) var = 0.0;
    dst[idx] = (float)sqrt(var);
    dst[plane + idx] = (float)mean;
}

__global__ __launch_bounds__(512) void ta_stats_f16_kernel(const f16* __restrict__ y, int H, int W, int C, int R, float* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    half8* slab8 = (half8*)smem;                      // [R][W][C] f16
    const half2v* slab2 = (const half2v*)smem;
    const int img = blockIdx.x, slice = blockIdx.y, S = gridDim.y, tid = threadIdx.x;
    const TaWs o = ta_ws(H, W, C, S);
    float* wsi = ws + img * o.per;
    const int G = C >> 3;                             // lanes per pixel (a power of two <= 64)
    const int items = R * W * G;
    const half8* src = (const half8*)(y + ((long long)img * H + (long long)slice * R) * W * C);
    for (int base = 0; base < items; base += 512) {   // copy + ZPool over C
        const int i = base + tid;
        const bool live = i < items;
        half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (live) {
            v = src[i];
            slab8[i] = v;
        }
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const double d = (double)(float)v[e];
            s1 += d;
            s2 = fma(d, d, s2);
        }
        for (int x = G >> 1; x > 0; x >>= 1) {
            s1 += __shfl_xor(s1, x);
            s2 += __shfl_xor(s2, x);
        }
        if (live && (i & (G - 1)) == 0) put_std_mean(wsi, (long long)H * W, (long long)slice * R * W + i / G, s1, s2, C);
    }
    __syncthreads();
    const int C2 = C >> 1;
    for (int t = tid; t < R * C2; t += 512) {         // ZPool over W: (h, channel pair)
        const int h = t / C2, cp = t - h * C2;
        double a1 = 0.0, a2 = 0.0, b1 = 0.0, b2 = 0.0;
        for (int w = 0; w < W; ++w) {
            const half2v v = slab2[(h * W + w) * C2 + cp];
            const double d0 = (double)(float)v[0], d1 = (double)(float)v[1];
            a1 += d0; a2 = fma(d0, d0, a2);
            b1 += d1; b2 = fma(d1, d1, b2);
        }
        const long long idx = (long long)(slice * R + h) * C + 2 * cp;
        put_std_mean(wsi + o.hc, (long long)H * C, idx, a1, a2, W);
        put_std_mean(wsi + o.hc, (long long)H * C, idx + 1, b1, b2, W);
    }
    float2* part = (float2*)(wsi + o.part) + (long long)slice * W * C;
    for (int t = tid; t < W * C2; t += 512) {         // ZPool over H, this slice's share: (w, channel pair)
        const int w = t / C2, cp = t - w * C2;
        double a1 = 0.0, a2 = 0.0, b1 = 0.0, b2 = 0.0;
        for (int h = 0; h < R; ++h) {
            const half2v v = slab2[(h * W + w) * C2 + cp];
            const double d0 = (double)(float)v[0], d1 = (double)(float)v[1];
            a1 += d0; a2 = fma(d0, d0, a2);
            b1 += d1; b2 = fma(d1, d1, b2);
        }
        const double ma = a2 - a1 * a1 / R, mb = b2 - b1 * b1 / R;   // M2 about the slice's mean (fp64: exact to 2^-53 of a2)
        part[w * C + 2 * cp] = make_float2((float)a1, (float)(ma > 0.0 ? ma : 0.0));
        part[w * C + 2 * cp + 1] = make_float2((float)b1, (float)(mb > 0.0 ? mb : 0.0));
    }
}

// gate = sigmoid(BN(conv7x7(std, mean))) on one of the three planes of an image.  grid (images, 3): 0 = (H, W), 1 = (C, W), 2 = (H, C).
__global__ __launch_bounds__(256) void ta_gate_f16_kernel(int H, int W, int C, int R, int S, const float* __restrict__ wts,
                                                          float* __restrict__ ws) {
    extern __shared__ float m[];                      // [2][P][Qp]
    __shared__ float wk[100];
    const int img = blockIdx.x, part = blockIdx.y, tid = threadIdx.x;
    const TaWs o = ta_ws(H, W, C, S);
    float* wsi = ws + img * o.per;
    const int hw = H * W;
    int P, Q, Qp, gsel;
    long long goff;
    if (part == 0) { P = H; Q = W; Qp = Q; gsel = 2; goff = 0; }
    else if (part == 1) { P = C; Q = W; Qp = Q + 1; gsel = 0; goff = hw; }          // lanes run along c = P here: odd row stride
    else { P = H; Q = C; Qp = Q; gsel = 1; goff = hw + (long long)W * C; }
    if (tid < 100) wk[tid] = wts[gsel * 100 + tid];
    const int plane = P * Qp, outs = P * Q;
    if (part == 1) {                                  // merge the row slices: mean, then M2 = sum M2_k + R (mean_k - mean)^2
        const float2* pp = (const float2*)(wsi + o.part);
        for (int i = tid; i < outs; i += 256) {       // i = w C + c
            const int w = i / C, c = i - w * C;
            double tot = 0.0;
            for (int k = 0; k < S; ++k) tot += (double)pp[(long long)k * W * C + i].x;
            const double mean = tot / H;
            double m2 = 0.0;
            for (int k = 0; k < S; ++k) {
                const float2 v = pp[(long long)k * W * C + i];
                const double d = (double)v.x / R - mean;
                m2 += (double)v.y + R * d * d;
            }
            m[c * Qp + w] = (float)sqrt(m2 / (H - 1));
            m[plane + c * Qp + w] = (float)mean;
        }
    } else {
        const float* src = wsi + (part == 0 ? 0 : o.hc);
        for (int i = tid; i < 2 * outs; i += 256) m[i] = src[i];
    }
    __syncthreads();
    float* g = wsi + o.gates + goff;
    for (int i = tid; i < outs; i += 256) {
        int pr, qc;
        if (part == 1) { qc = i / P; pr = i - qc * P; }
        else { pr = i / Q; qc = i - pr * Q; }
        float acc = 0.f;
        for (int ch = 0; ch < 2; ++ch)
            for (int r = 0; r < 7; ++r) {
                const int pp = pr + r - 3;
                if ((unsigned)pp >= (unsigned)P) continue;
                for (int s = 0; s < 7; ++s) {
                    const int qq = qc + s - 3;
                    if ((unsigned)qq >= (unsigned)Q) continue;
                    acc += wk[ch * 49 + r * 7 + s] * m[ch * plane + pp * Qp + qq];
                }
            }
        acc = acc * wk[98] + wk[99];
        g[i] = 1.0f / (1.0f + expf(-acc));            // part 1: i = w C + c, the [w][c] form
    }
}

__global__ __launch_bounds__(256) void ta_apply_f16_kernel(const f16* __restrict__ y, const f16* __restrict__ sc, long long chunks, int H,
                                                           int W, int C, int S, const float* __restrict__ ws, f16* __restrict__ out) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= chunks) return;
    const TaWs o = ta_ws(H, W, C, S);
    const int G = C >> 3, hw = H * W;
    const int c8 = (int)(i % G) * 8;
    const long long pix = i / G;
    const int p = (int)(pix % hw);
    const long long img = pix / hw;
    const int h = p / W, w = p - h * W;
    const float* g = ws + img * o.per + o.gates;
    const float ghw = g[p];
    const float* gcw = g + hw + (long long)w * C + c8;
    const float* ghc = g + hw + (long long)W * C + (long long)h * C + c8;
    const f32x4 cw0 = *(const f32x4*)gcw, cw1 = *(const f32x4*)(gcw + 4), hc0 = *(const f32x4*)ghc, hc1 = *(const f32x4*)(ghc + 4);
    const half8 vy = *(const half8*)(y + i * 8), vs = *(const half8*)(sc + i * 8);
    half8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float v = (float)vy[e];
        const float a = v * ghw, b = v * (e < 4 ? cw0[e & 3] : cw1[e & 3]), d = v * (e < 4 ? hc0[e & 3] : hc1[e & 3]);
        const float t = 0.3333333333333333f * ((a + b) + d);
        r[e] = cvt_f16_rn(fmaxf(t + (float)vs[e], 0.f));
    }
    *(half8*)(out + i * 8) = r;
}

// ---- EMA + residual + ReLU.  LDS (floats): gx | x1 | x2 [CG][hw] each, cat | sig [CG][H + W], small [6 CG], the parameters.
template <int CG>
__global__ __launch_bounds__(256) void ema_tail_f16_kernel(const f16* __restrict__ y, const f16* __restrict__ sc, int H, int W, int C,
                                                           const float* __restrict__ prm, f16* __restrict__ out) {
    typedef f16 hvec __attribute__((ext_vector_type(CG)));
    constexpr int PN = CG * CG * 10 + 4 * CG;
    extern __shared__ float sm[];
    const int hw = H * W, HW2 = H + W;
    float* gx = sm;
    float* x1 = gx + CG * hw;
    float* x2 = x1 + CG * hw;
    float* cat = x2 + CG * hw;
    float* sig = cat + CG * HW2;
    float* small = sig + CG * HW2;     // mu, rstd, agp(x1), agp(x2), softmax(agp(x1)), softmax(agp(x2))
    float* pw = small + 6 * CG;
    const float* w1 = pw;
    const float* b1 = w1 + CG * CG;
    const float* w3 = b1 + CG;
    const float* b3 = w3 + CG * CG * 9;
    const float* gw = b3 + CG;
    const float* gb = gw + CG;
    const int img = blockIdx.x >> 5, grp = blockIdx.x & 31;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long base = (long long)img * hw * C + grp * CG;
    for (int i = tid; i < PN; i += 256) pw[i] = prm[i];
    for (int p = tid; p < hw; p += 256) {
        const hvec v = *(const hvec*)(y + base + (long long)p * C);
#pragma unroll
        for (int c = 0; c < CG; ++c) gx[c * hw + p] = (float)v[c];
    }
    __syncthreads();
    for (int b0 = 0; b0 < CG * hw; b0 += 256) {          // pool_h: mean over w, the W lanes of a row add with xor shuffles
        const int i = b0 + tid;
        float s = i < CG * hw ? gx[i] : 0.f;
        for (int x = W >> 1; x > 0; x >>= 1) s += __shfl_xor(s, x);
        if (i < CG * hw && (i & (W - 1)) == 0) {
            const int c = i / hw, h = (i - c * hw) / W;
            cat[c * HW2 + h] = s / (float)W;
        }
    }
    for (int i = tid; i < CG * W; i += 256) {             // pool_w: mean over h
        const int c = i / W, w = i - c * W;
        float s = 0.f;
        for (int h = 0; h < H; ++h) s += gx[c * hw + h * W + w];
        cat[c * HW2 + H + w] = s / (float)H;
    }
    __syncthreads();
    for (int i = tid; i < CG * HW2; i += 256) {           // conv1x1 over the channels of the group, then sigmoid
        const int co = i / HW2, j = i - co * HW2;
        float acc = b1[co];
#pragma unroll
        for (int ci = 0; ci < CG; ++ci) acc += w1[co * CG + ci] * cat[ci * HW2 + j];
        sig[i] = 1.0f / (1.0f + expf(-acc));
    }
    __syncthreads();
    for (int i = tid; i < CG * hw; i += 256) {            // gated slab (before GroupNorm) and the 3x3 conv of the raw slab
        const int c = i / hw, p = i - c * hw;
        const int h = p / W, w = p - h * W;
        x1[i] = gx[i] * sig[c * HW2 + h] * sig[c * HW2 + H + w];
        float acc = b3[c];
        for (int ci = 0; ci < CG; ++ci)
            for (int r = 0; r < 3; ++r) {
                const int hh = h + r - 1;
                if ((unsigned)hh >= (unsigned)H) continue;
                for (int s = 0; s < 3; ++s) {
                    const int ww = w + s - 1;
                    if ((unsigned)ww >= (unsigned)W) continue;
                    acc += w3[((c * CG + ci) * 3 + r) * 3 + s] * gx[ci * hw + hh * W + ww];
                }
            }
        x2[i] = acc;
    }
    __syncthreads();
    for (int c = wave; c < CG; c += 4) {                  // GroupNorm statistics (one group per channel, biased variance, eps 1e-5): two passes
        float s = 0.f;
        for (int p = lane; p < hw; p += 64) s += x1[c * hw + p];
        const float mu = wave_sum_f(s) / (float)hw;
        float q = 0.f;
        for (int p = lane; p < hw; p += 64) { const float d = x1[c * hw + p] - mu; q += d * d; }
        const float var = wave_sum_f(q) / (float)hw;
        float s2 = 0.f;
        for (int p = lane; p < hw; p += 64) s2 += x2[c * hw + p];
        s2 = wave_sum_f(s2) / (float)hw;
        if (lane == 0) {
            small[c] = mu;
            small[CG + c] = 1.0f / sqrtf(var + 1e-5f);
            small[3 * CG + c] = s2;                       // agp(x2)
        }
    }
    __syncthreads();
    for (int i = tid; i < CG * hw; i += 256) {
        const int c = i / hw;
        x1[i] = (x1[i] - small[c]) * small[CG + c] * gw[c] + gb[c];
    }
    __syncthreads();
    for (int c = wave; c < CG; c += 4) {                  // agp(x1)
        float s = 0.f;
        for (int p = lane; p < hw; p += 64) s += x1[c * hw + p];
        s = wave_sum_f(s) / (float)hw;
        if (lane == 0) small[2 * CG + c] = s;
    }
    __syncthreads();
    if (tid < 2) {                                         // softmax over the group's channels of agp(x1) / agp(x2)
        const float* a = small + (2 + tid) * CG;
        float* o = small + (4 + tid) * CG;
        float mx = -INFINITY;
        for (int c = 0; c < CG; ++c) mx = fmaxf(mx, a[c]);
        float den = 0.f;
        for (int c = 0; c < CG; ++c) { o[c] = expf(a[c] - mx); den += o[c]; }
        for (int c = 0; c < CG; ++c) o[c] /= den;
    }
    __syncthreads();
    for (int p = tid; p < hw; p += 256) {                  // weights = x11 . x2 + x21 . x1 -> out = relu(gx * sigmoid(weights) + shortcut)
        float wa = 0.f, wb = 0.f;
#pragma unroll
        for (int c = 0; c < CG; ++c) {
            wa += small[4 * CG + c] * x2[c * hw + p];
            wb += small[5 * CG + c] * x1[c * hw + p];
        }
        const float g = 1.0f / (1.0f + expf(-(wa + wb)));
        const long long o = base + (long long)p * C;
        const hvec s = *(const hvec*)(sc + o);
        hvec r;
#pragma unroll
        for (int c = 0; c < CG; ++c) r[c] = cvt_f16_rn(fmaxf(gx[c * hw + p] * g + (float)s[c], 0.f));
        *(hvec*)(out + o) = r;
    }
}

inline bool ta_shape_ok(int n, int H, int W, int C) {
    if (n < 0 || H < 2 || W < 2 || C < 8 || C > 512 || (C & (C - 1)) != 0) return false;   // C / 8 lanes per pixel: a power of two <= 64
    if ((long long)W * C > TA_SLICE_ELEMS || ((long long)H * W) % 4 != 0) return false;
    return H % ta_rows(H, W, C) == 0;
}

template <int CG>
hipError_t ema_launch(hipStream_t stream, const f16* y, const f16* sc, int n, int H, int W, int C, const float* prm, f16* out) {
    const size_t lds = ((size_t)3 * CG * H * W + (size_t)2 * CG * (H + W) + 6 * CG + CG * CG * 10 + 4 * CG) * 4;
    if (lds > 150 * 1024) return hipErrorInvalidValue;
    const hipError_t e = lds_limit_once(CG == 2 ? 2 : CG == 4 ? 3 : CG == 8 ? 4 : 5, (const void*)ema_tail_f16_kernel<CG>, 150 * 1024);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ema_tail_f16_kernel<CG>, dim3((unsigned)n * 32), dim3(256), lds, stream, y, sc, H, W, C, prm, out);
    return hipGetLastError();
}

}  // namespace

extern "C" size_t siblings_f16_ta_workspace_bytes(int n, int H, int W, int C) {
    if (!ta_shape_ok(n, H, W, C)) return 0;
    return (size_t)n * (size_t)ta_ws(H, W, C, H / ta_rows(H, W, C)).per * 4;
}

extern "C" hipError_t siblings_f16_ta_tail(hipStream_t stream, const _Float16* y, const _Float16* sc, int n, int H, int W, int C,
                                           const float* wts, void* workspace, _Float16* out) {
    if (!ta_shape_ok(n, H, W, C) || !y || !sc || !wts || !workspace || !out) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const int R = ta_rows(H, W, C), S = H / R;
    float* ws = (float*)workspace;
    const size_t slab = (size_t)R * W * C * 2;
    const int pq = H * W > C * (W + 1) ? H * W : C * (W + 1);   // the (c, w) plane has rows of W + 1
    const size_t gate_lds = (size_t)2 * (pq > H * C ? pq : H * C) * 4;
    if (gate_lds > 128 * 1024) return hipErrorInvalidValue;
    hipError_t e = lds_limit_once(0, (const void*)ta_stats_f16_kernel, 64 * 1024);
    if (e == hipSuccess) e = lds_limit_once(1, (const void*)ta_gate_f16_kernel, 128 * 1024);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ta_stats_f16_kernel, dim3(n, S), dim3(512), slab, stream, y, H, W, C, R, ws);
    hipLaunchKernelGGL(ta_gate_f16_kernel, dim3(n, 3), dim3(256), gate_lds, stream, H, W, C, R, S, wts, ws);
    const long long chunks = (long long)n * H * W * (C / 8);
    hipLaunchKernelGGL(ta_apply_f16_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, stream, y, sc, chunks, H, W, C, S,
                       (const float*)ws, out);
    return hipGetLastError();
}

extern "C" size_t siblings_f16_ema_workspace_bytes(int, int, int, int) { return 0; }

extern "C" hipError_t siblings_f16_ema_tail(hipStream_t stream, const _Float16* y, const _Float16* sc, int n, int H, int W, int C,
                                            const float* prm, _Float16* out) {
    if (n < 0 || H < 1 || !(W == 8 || W == 16 || W == 32 || W == 64) || !y || !sc || !prm || !out) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    switch (C) {
        case 64: return ema_launch<2>(stream, y, sc, n, H, W, C, prm, out);
        case 128: return ema_launch<4>(stream, y, sc, n, H, W, C, prm, out);
        case 256: return ema_launch<8>(stream, y, sc, n, H, W, C, prm, out);
        case 512: return ema_launch<16>(stream, y, sc, n, H, W, C, prm, out);
        default: return hipErrorInvalidValue;
    }
}
