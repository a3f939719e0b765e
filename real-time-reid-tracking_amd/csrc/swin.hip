// Swin-T (reference: reid/backbones/swin_transformer.py, versions "v1" and "v2") on the device: token layout [image][y][x][C] fp32.
// Every Linear / patch-merge / 8x8 conv / ConvTranspose is a launch of the f32 MFMA GEMM (gemm_f32.hip) with fused
// bias / GELU / residual epilogues; this file holds the kernels that are not GEMMs (stem, LayerNorm, window attention,
// LN + GeM_1D + BN tail) and the launch sequence.  The two kernels only v2 blocks launch are in swin_v2.hip (libreid_hip_swin_v2.so, opened when v2 weights are loaded).
// What the descriptor entries (reid_swin_descriptor_*) launch beyond the forward is in swin_eval.hip (libreid_hip_swin_eval.so).
//
// Cyclic shift: LayerNorm and every Linear are per-token, so the roll(-3,-3) ... roll(+3,+3) pair of a shifted block
// (swin_transformer.py:193-194,230-231) is folded into the attention kernel's indexing alone: window position (y', x')
// reads and writes token ((y'+3) % H, (x'+3) % W).
#include "reid_internal.h"
#include "swin_v2.h"
#include "swin_crops.h"
#include "swin_eval.h"
#include "pil_launch.h"
#include <mutex>
#include <math.h>
#include <string.h>
#include <sstream>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16;
typedef f16 half4 __attribute__((ext_vector_type(4)));

namespace {

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- ShadowFeatureExtraction part 1 (swin_transformer.py:297): conv2x2 s2 (3 -> 12, bias), NCHW in, NHWC12 out
__global__ void sfe_conv1_kernel(const float* __restrict__ x, int n, int h, int w, const float* __restrict__ wgt,
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
                    in[(kh * 2 + kw) * 3 + c] = x[(((long long)img * 3 + c) * h + 2 * oy + kh) * w + 2 * ox + kw];
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

// ---- MixedNorm statistics (swin_transformer.py:42-54): per image, channels 0..5 InstanceNorm (biased var, eps 1e-5),
// channels 6..11 eval BatchNorm (folded on the host) -> per-(image, channel) affine
__global__ __launch_bounds__(256) void sfe_norm_kernel(const float* __restrict__ y, int hw, const float* __restrict__ in_g,
                                                       const float* __restrict__ in_b, const float* __restrict__ bn_s,
                                                       const float* __restrict__ bn_t, float* __restrict__ ab) {
    __shared__ double red[4][12];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double s1[6], s2[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) { s1[c] = 0.0; s2[c] = 0.0; }
    const float* yi = y + (long long)img * hw * 12;
    for (int p = tid; p < hw; p += 256) {
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const double v = yi[(long long)p * 12 + c];
            s1[c] += v;
            s2[c] += v * v;
        }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { s1[c] += __shfl_xor(s1[c], o); s2[c] += __shfl_xor(s2[c], o); }
        if (lane == 0) { red[wave][c] = s1[c]; red[wave][6 + c] = s2[c]; }
    }
    __syncthreads();
    if (tid < 12) {
        float a, b;
        if (tid < 6) {
            const double t1 = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
            const double t2 = red[0][6 + tid] + red[1][6 + tid] + red[2][6 + tid] + red[3][6 + tid];
            const double mean = t1 / hw;
            double var = t2 / hw - mean * mean;
            if (var < 0) var = 0;
            const double inv = 1.0 / sqrt(var + 1e-5);
            a = (float)(inv * in_g[tid]);
            b = (float)(in_b[tid] - mean * inv * in_g[tid]);
        } else {
            a = bn_s[tid - 6];
            b = bn_t[tid - 6];
        }
        ab[img * 24 + tid] = a;
        ab[img * 24 + 12 + tid] = b;
    }
}

// ---- ShadowFeatureExtraction part 2 (:297-303): MixedNorm + ReLU -> conv2x2 s2 (12 -> 48, bias) -> ReLU -> Linear(48 -> 96)
// one thread per token; weights in LDS
__global__ __launch_bounds__(256, 3) void sfe_conv2_fc_kernel(const float* __restrict__ y, const float* __restrict__ ab, int n,
                                                           int h1, int w1, const float* __restrict__ w2,
                                                           const float* __restrict__ b2, const float* __restrict__ wf,
                                                           const float* __restrict__ bf, float* __restrict__ tok) {
    __shared__ float sw2[48 * 48], swf[96 * 48], sb2[48], sbf[96];
    for (int i = threadIdx.x; i < 48 * 48; i += 256) sw2[i] = w2[i];
    for (int i = threadIdx.x; i < 96 * 48; i += 256) swf[i] = wf[i];
    if (threadIdx.x < 48) sb2[threadIdx.x] = b2[threadIdx.x];
    if (threadIdx.x < 96) sbf[threadIdx.x] = bf[threadIdx.x];
    __syncthreads();
    const int ho = h1 / 2, wo = w1 / 2;
    const long long total = (long long)n * ho * wo;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int ox = (int)(i % wo);
        const long long t = i / wo;
        const int oy = (int)(t % ho);
        const int img = (int)(t / ho);
        const float* a = ab + img * 24;
        float in[48];  // (kh, kw, c)
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int kw = 0; kw < 2; ++kw) {
                const float* src = y + (((long long)img * h1 + 2 * oy + kh) * w1 + 2 * ox + kw) * 12;
#pragma unroll
                for (int c = 0; c < 12; ++c) in[(kh * 2 + kw) * 12 + c] = fmaxf(src[c] * a[c] + a[12 + c], 0.f);
            }
        // conv2's 48 outputs are consumed as they are produced: out[j] collects swf[j][k] * mid[k] in the k order of the plain
        // two-loop form (bias first, then k = 0 .. 47), so the sums are the same operations in the same order.  No array is
        // indexed with a run-time value (a `mid[48]` written in a partly unrolled loop lived in scratch: 208 bytes per lane)
        float out[96];
#pragma unroll
        for (int j = 0; j < 96; ++j) out[j] = sbf[j];
#pragma unroll 1
        for (int co = 0; co < 48; ++co) {
            float acc = sb2[co];
#pragma unroll
            for (int k0 = 0; k0 < 48; k0 += 16) {      // (scheduling barriers: hipcc otherwise requests all 144 LDS words of an iteration up front - 264 registers)
#pragma unroll
                for (int k = k0; k < k0 + 16; ++k) acc += sw2[co * 48 + k] * in[k];
                __builtin_amdgcn_sched_barrier(0);
            }
            const float m = fmaxf(acc, 0.f);
#pragma unroll
            for (int j0 = 0; j0 < 96; j0 += 16) {
#pragma unroll
                for (int j = j0; j < j0 + 16; ++j) out[j] += swf[j * 48 + co] * m;
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        float* o = tok + i * 96;
#pragma unroll
        for (int j = 0; j < 96; j += 4) *(f32x4*)(o + j) = f32x4{out[j], out[j + 1], out[j + 2], out[j + 3]};
    }
}

// ---- LayerNorm over the channel dimension, one wave per token (C <= 768)
template <typename OUT>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, long long ntok, int c, float eps,
                                                        const float* __restrict__ g, const float* __restrict__ b,
                                                        OUT* __restrict__ out) {
    const long long tok = blockIdx.x * 4LL + (threadIdx.x >> 6);
    if (tok >= ntok) return;
    const int lane = threadIdx.x & 63;
    const float* xi = x + tok * c;
    float v[12];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        const int ch = lane + 64 * j;
        v[j] = ch < c ? xi[ch] : 0.f;
        s += v[j];
    }
    const float mean = wsum(s) / c;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        const int ch = lane + 64 * j;
        const float d = ch < c ? v[j] - mean : 0.f;
        q += d * d;
    }
    const float rstd = 1.0f / sqrtf(wsum(q) / c + eps);
    OUT* oi = out + tok * c;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        const int ch = lane + 64 * j;
        if (ch < c) oi[ch] = (OUT)((v[j] - mean) * rstd * g[ch] + b[ch]);
    }
}

// ---- WindowAttention v1 (swin_transformer.py:191-232): one wave per (image, window, head); lane = query token (49 of
// 64 lanes active), K and V of the window/head in LDS (read as broadcasts), softmax in registers.
// qkv: [tokens][3C] (q | k | v, head-major inside each), out: [tokens][C].
__device__ __forceinline__ f32x4 ld4(const float* p) { return *(const f32x4*)p; }
__device__ __forceinline__ f32x4 ld4(const f16* p) {
    const half4 h = *(const half4*)p;
    f32x4 r = {(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
    return r;
}
__device__ __forceinline__ void st4(float* p, f32x4 v) { *(f32x4*)p = v; }
__device__ __forceinline__ void st4(f16* p, f32x4 v) {
    half4 h = {(f16)v.x, (f16)v.y, (f16)v.z, (f16)v.w};
    *(half4*)p = h;
}
// T = float (exact mode) or f16 (fp16-storage mode: qkv comes from / the result goes to the f16 GEMMs); ldq = row stride of qkv
// packed != nullptr (T = float, precision 2): the result goes out as [oh | ol'] f16 [tokens][2C] for the fp32-class to_out linear
template <typename T>
__global__ __launch_bounds__(256) void window_attn_kernel(const T* __restrict__ qkv, int ldq, int n_img, int H, int W, int heads,
                                                          int shifted, const float* __restrict__ pos, T* __restrict__ out,
                                                          f16* __restrict__ packed = nullptr, int* __restrict__ fault = nullptr) {
    __shared__ float kv[4][2][49 * 32];
    __shared__ float spos[169];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < 169; i += 256) spos[i] = pos[i];
    const int nwh = H / 7, nww = W / 7;
    const long long task = blockIdx.x * 4LL + wave;
    const long long ntask = (long long)n_img * nwh * nww * heads;
    const bool live = task < ntask;
    const int C = heads * 32;
    int head = 0, wx = 0, wy = 0, img = 0;
    if (live) {
        head = (int)(task % heads);
        long long t = task / heads;
        wx = (int)(t % nww);
        t /= nww;
        wy = (int)(t % nwh);
        img = (int)(t / nwh);
    }
    const int sh = shifted ? 3 : 0;
    const int iy = lane / 7, ix = lane - iy * 7;
    const bool act = live && lane < 49;
    long long tok = 0;
    if (act) {
        const int y = (wy * 7 + iy + sh) % H, x = (wx * 7 + ix + sh) % W;
        tok = ((long long)img * H + y) * W + x;
    }
    float q[32];
    if (act) {
        const T* base = qkv + tok * ldq + head * 32;
#pragma unroll
        for (int d = 0; d < 32; d += 4) {
            const f32x4 a = ld4(base + d);
            q[d] = a.x; q[d + 1] = a.y; q[d + 2] = a.z; q[d + 3] = a.w;
        }
    }
    if (live) {
        // K and V of the window: the wave fills the 49 x 32 images slot by slot (slot = four channels; eight consecutive lanes = the
        // 128 bytes of one token's head slice, consecutive lanes = consecutive LDS addresses).  A lane writing its OWN token's row
        // (stride 128 B) was a 25-way bank conflict on every ds_write_b128 (PMC, round 5: conflict cycles = 1.05 x the LDS busy
        // cycles of this kernel) and eight 16-byte pieces of 49 different lines per load instruction.  Same values, same places;
        // worth 1.2 % of the kernel (689.6 -> 681.1 us per launch, same box): its time is the 3 136 FMAs + 784 broadcast reads per lane.
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            const int slot = lane + 64 * i;
            if (slot < 49 * 8) {
                const int j = slot >> 3, d = (slot & 7) * 4;
                const int jy = j / 7, jx = j - jy * 7;
                const int y = (wy * 7 + jy + sh) % H, x = (wx * 7 + jx + sh) % W;
                const T* base = qkv + (((long long)img * H + y) * W + x) * ldq + head * 32 + d;
                *(f32x4*)&kv[wave][0][slot * 4] = ld4(base + C);
                *(f32x4*)&kv[wave][1][slot * 4] = ld4(base + 2 * C);
            }
        }
    }
    __syncthreads();
    if (!act) return;
    const bool last_row = shifted && wy == nwh - 1, last_col = shifted && wx == nww - 1;
    float s[49];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 49; ++j) {
        const float* kj = &kv[wave][0][j * 32];
        float acc = 0.f;
#pragma unroll
        for (int d = 0; d < 32; ++d) acc += q[d] * kj[d];
        const int jy = j / 7, jx = j - jy * 7;
        acc = acc * 0.17677669529663687f + spos[(jy - iy + 6) * 13 + (jx - ix + 6)];   // 32^-0.5, relative position bias
        // masks of the last window row / column of a shifted block (create_mask, :95-108)
        if (last_row && ((iy >= 4) != (jy >= 4))) acc = -INFINITY;
        if (last_col && ((ix >= 4) != (jx >= 4))) acc = -INFINITY;
        s[j] = acc;
        mx = fmaxf(mx, acc);
    }
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < 49; ++j) {
        s[j] = expf(s[j] - mx);
        den += s[j];
    }
    const float inv = 1.0f / den;
    float o[32];
#pragma unroll
    for (int d = 0; d < 32; ++d) o[d] = 0.f;
#pragma unroll
    for (int j = 0; j < 49; ++j) {
        const float pj = s[j] * inv;
        const float* vj = &kv[wave][1][j * 32];
#pragma unroll
        for (int d = 0; d < 32; ++d) o[d] += pj * vj[d];
    }
    if (packed) {
        f16* ph = packed + tok * 2 * C + head * 32;
        unsigned vm = 0u;   // range guard (reid_ctx.fault)
#pragma unroll
        for (int d = 0; d < 32; ++d) vm = range_acc(vm, o[d]);
        range_raise(fault, vm);
#pragma unroll
        for (int d = 0; d < 32; d += 4) {
            half4 hi = {(f16)o[d], (f16)o[d + 1], (f16)o[d + 2], (f16)o[d + 3]};
            half4 lo = {(f16)((o[d] - (float)hi[0]) * 2048.0f), (f16)((o[d + 1] - (float)hi[1]) * 2048.0f),
                        (f16)((o[d + 2] - (float)hi[2]) * 2048.0f), (f16)((o[d + 3] - (float)hi[3]) * 2048.0f)};
            *(half4*)(ph + d) = hi;
            *(half4*)(ph + C + d) = lo;
        }
        return;
    }
    T* dst = out + tok * C + head * 32;
#pragma unroll
    for (int d = 0; d < 32; d += 4) {
        f32x4 v = {o[d], o[d + 1], o[d + 2], o[d + 3]};
        st4(dst + d, v);
    }
}


// ---- LayerNorm over the channel dimension, 16-byte accesses: LPT lanes per token (32 for C = 96: two tokens per wave; 64
// otherwise), a lane owns the 4-channel chunks sub + LPT * j.  Two-pass (mean, then centred sum of squares) in registers.
// PACK (OUT = f16, precision 2): the normalised token goes out as [yh | yl'] f16 [tokens][2c] (yl' = f16((y - yh) 2^11))
template <typename OUT, int LPT, bool PACK = false>
__global__ __launch_bounds__(256) void layernorm_v4_kernel(const float* __restrict__ x, long long ntok, int c, float eps,
                                                           const float* __restrict__ g, const float* __restrict__ b,
                                                           OUT* __restrict__ out, int* __restrict__ fault = nullptr) {
    constexpr int TPW = 64 / LPT;                  // tokens per wave
    constexpr int MAXJ = LPT == 32 ? 1 : 3;        // chunks per lane: C <= 128 (LPT 32) or C <= 768 (LPT 64)
    const int lane = threadIdx.x & 63, sub = lane & (LPT - 1);
    const long long tok = (blockIdx.x * 4LL + (threadIdx.x >> 6)) * TPW + lane / LPT;
    const bool live = tok < ntok;
    const int nch = c >> 2;
    const float* xi = x + (live ? tok : 0) * c;
    f32x4 v[MAXJ];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        const int ch = sub + LPT * j;
        v[j] = (live && ch < nch) ? *(const f32x4*)(xi + ch * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
    }
#pragma unroll
    for (int o = LPT / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / c;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        if (sub + LPT * j < nch) {
            const f32x4 d = v[j] - mean;
            q += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
        }
    }
#pragma unroll
    for (int o = LPT / 2; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = 1.0f / sqrtf(q / c + eps);
    if (!live) return;
    OUT* oi = out + tok * c * (PACK ? 2 : 1);
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        const int ch = sub + LPT * j;
        if (ch < nch) {
            const f32x4 gg = *(const f32x4*)(g + ch * 4), bb = *(const f32x4*)(b + ch * 4);
            const f32x4 y = (v[j] - mean) * rstd * gg + bb;
            if constexpr (PACK) {
                range_raise(fault, range_acc(range_acc(range_acc(range_acc(0u, y.x), y.y), y.z), y.w));   // range guard (reid_ctx.fault)
                half4 hi = {(f16)y.x, (f16)y.y, (f16)y.z, (f16)y.w};
                half4 lo = {(f16)((y.x - (float)hi[0]) * 2048.0f), (f16)((y.y - (float)hi[1]) * 2048.0f),
                            (f16)((y.z - (float)hi[2]) * 2048.0f), (f16)((y.w - (float)hi[3]) * 2048.0f)};
                *(half4*)(oi + ch * 4) = hi;
                *(half4*)(oi + c + ch * 4) = lo;
            } else {
                st4(oi + ch * 4, y);
            }
        }
    }
}

void launch_layernorm_packed(reid_ctx* ctx, const float* x, long long T, int C, const float* g, const float* b, f16* out) {
    if (C <= 128) hipLaunchKernelGGL((layernorm_v4_kernel<f16, 32, true>), dim3((unsigned)((T + 7) / 8)), dim3(256), 0, ctx->stream, x, T, C, 1e-5f, g, b, out, ctx->fault);
    else hipLaunchKernelGGL((layernorm_v4_kernel<f16, 64, true>), dim3((unsigned)((T + 3) / 4)), dim3(256), 0, ctx->stream, x, T, C, 1e-5f, g, b, out, ctx->fault);
}

template <typename OUT>
void launch_layernorm(reid_ctx* ctx, const float* x, long long T, int C, const float* g, const float* b, OUT* out) {
    if (C <= 128) hipLaunchKernelGGL((layernorm_v4_kernel<OUT, 32>), dim3((unsigned)((T + 7) / 8)), dim3(256), 0, ctx->stream, x, T, C, 1e-5f, g, b, out);
    else hipLaunchKernelGGL((layernorm_v4_kernel<OUT, 64>), dim3((unsigned)((T + 3) / 4)), dim3(256), 0, ctx->stream, x, T, C, 1e-5f, g, b, out);
}

// ---- WindowAttention v1 on the matrix cores (swin_transformer.py:191-232; north_star: "MFMA only on the Swin qk^T / attn.v").
// One wave per (image, window, head); the 49 tokens of a window are padded to 64.
//   S^T[key][query] = K . Q^T      (operands swapped so that a query's scores are lane-local: C layout col = lane & 31)
//   softmax over the keys: 32 scores in the lane's registers + one exchange with lane ^ 32
//   O[query][dim]   = P . V        with the S^T accumulator tile itself as the A operand (cdna_hip_programming.md section 3,
//                                  "An accumulator tile as the next MFMA's operand": X^T . B, k order permuted)
// The relative-position bias (one 13 x 13 table per layer, shared by the heads) is expanded once per block into a
// [key][query] table in LDS, padded keys carry -inf; the masks of the last window row / column of a shifted block
// (create_mask, :95-108) are applied from per-key flags.
typedef f16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
#include "lin_math.h"

__device__ __forceinline__ void build_bias_table(const float* __restrict__ pos, float* sbias, int* kflag, int nthreads) {
    for (int idx = threadIdx.x; idx < 64 * 64; idx += nthreads) {
        const int key = idx >> 6, query = idx & 63;
        float b = 0.f;
        if (key >= 49) b = -INFINITY;
        else if (query < 49) {
            const int jy = key / 7, jx = key - jy * 7, iy = query / 7, ix = query - iy * 7;
            b = pos[(jy - iy + 6) * 13 + (jx - ix + 6)];
        }
        sbias[idx] = b;
    }
    for (int key = threadIdx.x; key < 64; key += nthreads) {
        const int jy = key / 7, jx = key - jy * 7;
        kflag[key] = key < 49 ? ((jy >= 4 ? 1 : 0) | (jx >= 4 ? 2 : 0)) : 0;
    }
}

// scores of one lane: acc[kt][qt][e] = S^T[key = kt*32 + (e&3) + 8*(e>>2) + 4*(lane>>5)][query = qt*32 + (lane&31)]
// -> probabilities (scale, bias, masks, softmax over the 64 keys of each query), in place
// FAST (fp16-storage mode): exp as one v_exp_f32 of the log2e-scaled difference instead of ocml's expf
template <bool FAST>
__device__ __forceinline__ void softmax_scores(f32x16 (&acc)[2][2], const float* sbias, const int* kflag, int lane, bool last_row,
                                               bool last_col) {
    const int li = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int query = qt * 32 + li;
        const int iy = query / 7, ix = query - iy * 7;
        const int qf = (iy >= 4 ? 1 : 0) | (ix >= 4 ? 2 : 0);
        const int msel = (last_row ? 1 : 0) | (last_col ? 2 : 0);
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int key = kt * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                float v = acc[kt][qt][e] * 0.17677669529663687f + sbias[key * 64 + query];   // 32^-0.5
                if (msel && ((kflag[key] ^ qf) & msel)) v = -INFINITY;
                acc[kt][qt][e] = v;
                mx = fmaxf(mx, v);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float den = 0.f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float p = FAST ? __builtin_amdgcn_exp2f((acc[kt][qt][e] - mx) * 1.44269504088896340736f) : expf(acc[kt][qt][e] - mx);
                acc[kt][qt][e] = p;
                den += p;
            }
        den += __shfl_xor(den, 32);
        const float inv = 1.0f / den;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[kt][qt][e] *= inv;
    }
}

// fp16-storage mode: v_mfma_f32_32x32x16_f16, 8 MFMAs for S^T and 8 for P.V per (window, head)
__global__ __launch_bounds__(256) void window_attn_mfma_f16_kernel(const f16* __restrict__ qkv, int ldq, int n_img, int H, int W,
                                                                   int heads, int shifted, const float* __restrict__ bias_tab,
                                                                   f16* __restrict__ out) {
    constexpr int VP = 72;   // V^T row pitch in f16 (144 B)
    constexpr int ZP = 40;   // Z row pitch in f16 (80 B, 16-byte aligned rows)
    __shared__ __attribute__((aligned(16))) float sbias[64 * 64];
    __shared__ int kflag[64];
    __shared__ __attribute__((aligned(16))) f16 wbuf[4][64 * ZP];   // per wave: V^T [32][VP] (4 608 B), later Z [64][ZP] (5 120 B)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int li = lane & 31, lh = lane >> 5;
    // the layer's [key][query] bias table (expanded once at load time: build_bias_table's divisions and gathers cost every
    // block ~15 % of its time) - 16 KB, four 16-byte loads per thread
#pragma unroll
    for (int i = 0; i < 4; ++i)
        *(float4*)(sbias + (threadIdx.x + 256 * i) * 4) = *(const float4*)(bias_tab + (threadIdx.x + 256 * i) * 4);
    if (threadIdx.x < 64) {
        const int key = threadIdx.x, jy = key / 7, jx = key - jy * 7;
        kflag[key] = key < 49 ? ((jy >= 4 ? 1 : 0) | (jx >= 4 ? 2 : 0)) : 0;
    }
    const int nwh = H / 7, nww = W / 7;
    const long long task = blockIdx.x * 4LL + wave;
    const long long ntask = (long long)n_img * nwh * nww * heads;
    const bool live = task < ntask;
    const int C = heads * 32;
    int head = 0, wx = 0, wy = 0, img = 0;
    if (live) {
        head = (int)(task % heads);
        long long t = task / heads;
        wx = (int)(t % nww);
        t /= nww;
        wy = (int)(t % nwh);
        img = (int)(t / nwh);
    }
    const int sh = shifted ? 3 : 0;
    auto token = [&](int idx) -> long long {   // window position idx (< 49) -> token row
        const int iy = idx / 7, ix = idx - iy * 7;
        const int y = (wy * 7 + iy + sh) % H, x = (wx * 7 + ix + sh) % W;
        return ((long long)img * H + y) * W + x;
    };
    f16* vt = wbuf[wave];
    // V^T of this (window, head): lane = token, 32 dims -> vt[dim][token]; padded tokens are zero rows
    // all three operands are requested before the first one is consumed (the V^T transposition used to wait for V alone, the
    // Q / K loads for the transposition)
    half8 v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = half8{0, 0, 0, 0, 0, 0, 0, 0};
    if (live && lane < 49) {
        const f16* base = qkv + token(lane) * ldq + 2 * C + head * 32;
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = *(const half8*)(base + c * 8);
    }
    // Q / K fragments: lane (li, lh) holds dims 8*lh .. +7 (k-step 0) and 16 + 8*lh .. (k-step 1) of tokens li and 32 + li
    half8 qf[2][2], kf[2][2];
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
        const int idx = t2 * 32 + li;
        const bool ok = live && idx < 49;
        const f16* base = ok ? qkv + token(idx) * ldq + head * 32 + 8 * lh : qkv;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            qf[t2][s2] = ok ? *(const half8*)(base + s2 * 16) : half8{0, 0, 0, 0, 0, 0, 0, 0};
            kf[t2][s2] = ok ? *(const half8*)(base + C + s2 * 16) : half8{0, 0, 0, 0, 0, 0, 0, 0};
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < 8; ++j) vt[(c * 8 + j) * VP + lane] = v[c][j];
    __syncthreads();   // bias table ready (the wave's own V^T writes are ordered before its reads)
    if (!live) return;
    f32x16 acc[2][2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[kt][qt][e] = 0.f;
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
                acc[kt][qt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[kt][s2], qf[qt][s2], acc[kt][qt], 0, 0, 0);
        }
    softmax_scores<true>(acc, sbias, kflag, lane, shifted && wy == nwh - 1, shifted && wx == nww - 1);
    // O = P . V: A = registers 8*s2 .. 8*s2+7 of the S^T tile as f16 (element j of lane half h is key
    // 16*s2 + 8*(j>>2) + 4*h + (j&3) of the tile), B = V^T[dim = li][those keys]
    f32x16 z[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int e = 0; e < 16; ++e) z[qt][e] = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            const f16* vrow = vt + li * VP + kt * 32 + 16 * s2 + 4 * lh;
            const half4 v0 = *(const half4*)vrow, v1 = *(const half4*)(vrow + 8);
            const half8 vb = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                half8 pa;
#pragma unroll
                for (int j = 0; j < 8; ++j) pa[j] = (f16)acc[kt][qt][8 * s2 + j];
                z[qt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(pa, vb, z[qt], 0, 0, 0);
            }
        }
    // Z[query][dim] (col = dim on the lane, rows in registers) -> LDS -> one 64-byte row per token
    f16* zl = wbuf[wave];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int e = 0; e < 16; ++e) zl[(qt * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh) * ZP + li] = (f16)z[qt][e];
    if (lane < 49) {
        f16* dst = out + token(lane) * C + head * 32;
#pragma unroll
        for (int c = 0; c < 4; ++c) *(half8*)(dst + c * 8) = *(const half8*)(zl + lane * ZP + c * 8);
    }
}

// fp32-class mode (precision 2): the same kernel on fp32 q / k / v split into [hi | lo'] f16 in registers - x.y = xh.yh + (xl'.yh +
// xh.yl') 2^-11 with the leading product and the two corrections in accumulators of their own (no operand carries a 2^11 factor:
// activations are only known to be < 65504) - for S^T and for P.V: 24 + 24 MFMAs per (window, head); exact expf; the result goes
// out as [zh | zl'] f16 [tokens][2C], what the to_out linear reads.
// OPT-IN (REID_SWIN_ATTN_SPLIT=1), not the default: measured end to end (bench.py --workload swin, 1024 images, same box, twice
// each) 14.0 k img/s with this kernel against 14.7 k with the exact-fp32 VALU kernel above.  With 49 tokens and 32 dims per head
// the products are the small part of a window: the hi / lo splits of q, k, v and of the 64 x 64 probabilities, the range guards,
// 64 expf per lane and two LDS transposes are as many VALU instructions (~3.5 k per wave) as the VALU kernel's whole
// arithmetic (~4.2 k), on top of 48 MFMAs.  The exact-fp32 matrix-core form (v_mfma_f32_32x32x2_f32, below) runs at the VALU
// rate and was 5 % slower as well (round 2).
__global__ __launch_bounds__(256) void window_attn_mfma_split_kernel(const float* __restrict__ qkv, int ldq, int n_img, int H, int W,
                                                                     int heads, int shifted, const float* __restrict__ bias_tab,
                                                                     f16* __restrict__ packed, int* __restrict__ fault) {
    constexpr int VP = 72;   // V^T row pitch in f16 (144 B)
    constexpr int ZP = 40;   // Z row pitch in f16 (80 B, 16-byte aligned rows)
    __shared__ __attribute__((aligned(16))) float sbias[64 * 64];
    __shared__ int kflag[64];
    __shared__ __attribute__((aligned(16))) f16 wbuf[4][2][64 * ZP];   // per wave, hi / lo: V^T [32][VP], later Z [64][ZP]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int li = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        *(float4*)(sbias + (threadIdx.x + 256 * i) * 4) = *(const float4*)(bias_tab + (threadIdx.x + 256 * i) * 4);
    if (threadIdx.x < 64) {
        const int key = threadIdx.x, jy = key / 7, jx = key - jy * 7;
        kflag[key] = key < 49 ? ((jy >= 4 ? 1 : 0) | (jx >= 4 ? 2 : 0)) : 0;
    }
    const int nwh = H / 7, nww = W / 7;
    const long long task = blockIdx.x * 4LL + wave;
    const long long ntask = (long long)n_img * nwh * nww * heads;
    const bool live = task < ntask;
    const int C = heads * 32;
    int head = 0, wx = 0, wy = 0, img = 0;
    if (live) {
        head = (int)(task % heads);
        long long t = task / heads;
        wx = (int)(t % nww);
        t /= nww;
        wy = (int)(t % nwh);
        img = (int)(t / nwh);
    }
    const int sh = shifted ? 3 : 0;
    auto token = [&](int idx) -> long long {   // window position idx (< 49) -> token row
        const int iy = idx / 7, ix = idx - iy * 7;
        const int y = (wy * 7 + iy + sh) % H, x = (wx * 7 + ix + sh) % W;
        return ((long long)img * H + y) * W + x;
    };
    auto split8 = [](const f32x4& a, const f32x4& b, half8& hi, half8& lo) {
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            hi[j] = cvt_f16_rn(v[j]);
            lo[j] = cvt_f16_rn((v[j] - (float)hi[j]) * 2048.0f);
        }
    };
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    unsigned vm = 0u;        // range guard (reid_ctx.fault): |q|, |k|, |v|, |z| < 65504
    f16* vth = wbuf[wave][0];
    f16* vtl = wbuf[wave][1];
    // V^T of this (window, head): lane = token, 32 dims -> vt[dim][token], hi and lo; padded tokens are zero rows
    f32x4 vv[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) vv[c] = zero4;
    if (live && lane < 49) {
        const float* base = qkv + token(lane) * ldq + 2 * C + head * 32;
#pragma unroll
        for (int c = 0; c < 8; ++c) vv[c] = *(const f32x4*)(base + c * 4);
    }
    // Q / K fragments: lane (li, lh) holds dims 8*lh .. +7 (k-step 0) and 16 + 8*lh .. (k-step 1) of tokens li and 32 + li
    half8 qh[2][2], ql[2][2], kh[2][2], kl[2][2];
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
        const int idx = t2 * 32 + li;
        const bool ok = live && idx < 49;
        const float* base = ok ? qkv + token(idx) * ldq + head * 32 + 8 * lh : qkv;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            const f32x4 q0 = ok ? *(const f32x4*)(base + s2 * 16) : zero4, q1 = ok ? *(const f32x4*)(base + s2 * 16 + 4) : zero4;
            const f32x4 k0 = ok ? *(const f32x4*)(base + C + s2 * 16) : zero4, k1 = ok ? *(const f32x4*)(base + C + s2 * 16 + 4) : zero4;
            vm = range_acc(range_acc(range_acc(range_acc(vm, q0.x), q0.y), q0.z), q0.w);
            vm = range_acc(range_acc(range_acc(range_acc(vm, q1.x), q1.y), q1.z), q1.w);
            vm = range_acc(range_acc(range_acc(range_acc(vm, k0.x), k0.y), k0.z), k0.w);
            vm = range_acc(range_acc(range_acc(range_acc(vm, k1.x), k1.y), k1.z), k1.w);
            split8(q0, q1, qh[t2][s2], ql[t2][s2]);
            split8(k0, k1, kh[t2][s2], kl[t2][s2]);
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        half8 hi, lo;
        split8(vv[2 * c], vv[2 * c + 1], hi, lo);
        vm = range_acc(range_acc(range_acc(range_acc(vm, vv[2 * c].x), vv[2 * c].y), vv[2 * c].z), vv[2 * c].w);
        vm = range_acc(range_acc(range_acc(range_acc(vm, vv[2 * c + 1].x), vv[2 * c + 1].y), vv[2 * c + 1].z), vv[2 * c + 1].w);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            vth[(c * 8 + j) * VP + lane] = hi[j];
            vtl[(c * 8 + j) * VP + lane] = lo[j];
        }
    }
    __syncthreads();   // bias table ready (the wave's own V^T writes are ordered before its reads)
    if (!live) return;
    f32x16 acc[2][2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            f32x16 corr;
#pragma unroll
            for (int e = 0; e < 16; ++e) { acc[kt][qt][e] = 0.f; corr[e] = 0.f; }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                acc[kt][qt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh[kt][s2], qh[qt][s2], acc[kt][qt], 0, 0, 0);
                corr = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl[kt][s2], qh[qt][s2], corr, 0, 0, 0);
                corr = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh[kt][s2], ql[qt][s2], corr, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[kt][qt][e] = fmaf(corr[e], 1.0f / 2048.0f, acc[kt][qt][e]);
        }
    softmax_scores<false>(acc, sbias, kflag, lane, shifted && wy == nwh - 1, shifted && wx == nww - 1);
    // O = P . V: A = registers 8*s2 .. 8*s2+7 of the S^T tile as [ph | pl'] (element j of lane half h is key
    // 16*s2 + 8*(j>>2) + 4*h + (j&3) of the tile), B = V^T[dim = li][those keys]
    f32x16 z[2], zc[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int e = 0; e < 16; ++e) { z[qt][e] = 0.f; zc[qt][e] = 0.f; }
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            const int voff = li * VP + kt * 32 + 16 * s2 + 4 * lh;
            const half4 h0 = *(const half4*)(vth + voff), h1 = *(const half4*)(vth + voff + 8);
            const half4 l0 = *(const half4*)(vtl + voff), l1 = *(const half4*)(vtl + voff + 8);
            const half8 vbh = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
            const half8 vbl = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                half8 pah, pal;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float pv = acc[kt][qt][8 * s2 + j];
                    pah[j] = cvt_f16_rn(pv);
                    pal[j] = cvt_f16_rn((pv - (float)pah[j]) * 2048.0f);
                }
                z[qt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(pah, vbh, z[qt], 0, 0, 0);
                zc[qt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(pal, vbh, zc[qt], 0, 0, 0);
                zc[qt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(pah, vbl, zc[qt], 0, 0, 0);
            }
        }
    // Z[query][dim] (col = dim on the lane, rows in registers) -> [zh | zl'] -> LDS -> one 64-byte row each per token
    f16* zhl = wbuf[wave][0];
    f16* zll = wbuf[wave][1];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float v = fmaf(zc[qt][e], 1.0f / 2048.0f, z[qt][e]);
            vm = range_acc(vm, v);
            const f16 hv = cvt_f16_rn(v);
            const int o = (qt * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh) * ZP + li;
            zhl[o] = hv;
            zll[o] = cvt_f16_rn((v - (float)hv) * 2048.0f);
        }
    range_raise(fault, vm);
    if (lane < 49) {
        f16* dst = packed + token(lane) * 2 * C + head * 32;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            *(half8*)(dst + c * 8) = *(const half8*)(zhl + lane * ZP + c * 8);
            *(half8*)(dst + C + c * 8) = *(const half8*)(zll + lane * ZP + c * 8);
        }
    }
}

// exact-fp32 mode: v_mfma_f32_32x32x2_f32 (a k-ordered fmaf chain per output), 64 MFMAs for S^T and 64 for P.V.
// Q, K, V rows of the window/head sit in LDS with a 33-float pitch (ds_read_b32 of 32 different rows: conflict-free).
__global__ __launch_bounds__(128) void window_attn_mfma_f32_kernel(const float* __restrict__ qkv, int ldq, int n_img, int H, int W,
                                                                   int heads, int shifted, const float* __restrict__ pos,
                                                                   float* __restrict__ out) {
    constexpr int RP = 33;
    __shared__ float sbias[64 * 64];
    __shared__ int kflag[64];
    __shared__ float rows[2][3][64 * RP];   // per wave: Q, K, V
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int li = lane & 31, lh = lane >> 5;
    build_bias_table(pos, sbias, kflag, 128);
    const int nwh = H / 7, nww = W / 7;
    const long long task = blockIdx.x * 2LL + wave;
    const long long ntask = (long long)n_img * nwh * nww * heads;
    const bool live = task < ntask;
    const int C = heads * 32;
    int head = 0, wx = 0, wy = 0, img = 0;
    if (live) {
        head = (int)(task % heads);
        long long t = task / heads;
        wx = (int)(t % nww);
        t /= nww;
        wy = (int)(t % nwh);
        img = (int)(t / nwh);
    }
    const int sh = shifted ? 3 : 0;
    long long tok = 0;
    const bool act = live && lane < 49;
    if (act) {
        const int iy = lane / 7, ix = lane - iy * 7;
        const int y = (wy * 7 + iy + sh) % H, x = (wx * 7 + ix + sh) % W;
        tok = ((long long)img * H + y) * W + x;
    }
    float* Qs = rows[wave][0];
    float* Ks = rows[wave][1];
    float* Vs = rows[wave][2];
    {
        const float* base = qkv + tok * ldq + head * 32;
#pragma unroll
        for (int d = 0; d < 32; d += 4) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a, c = a;
            if (act) {
                a = *(const f32x4*)(base + d);
                b = *(const f32x4*)(base + C + d);
                c = *(const f32x4*)(base + 2 * C + d);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                Qs[lane * RP + d + e] = a[e];
                Ks[lane * RP + d + e] = b[e];
                Vs[lane * RP + d + e] = c[e];
            }
        }
    }
    __syncthreads();
    if (!live) return;
    f32x16 acc[2][2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[kt][qt][e] = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t) {   // k-step t covers dims 2t, 2t+1 (lane half = k)
        float ka[2], qb[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            ka[u] = Ks[(u * 32 + li) * RP + 2 * t + lh];
            qb[u] = Qs[(u * 32 + li) * RP + 2 * t + lh];
        }
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) acc[kt][qt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[kt], qb[qt], acc[kt][qt], 0, 0, 0);
    }
    softmax_scores<false>(acc, sbias, kflag, lane, shifted && wy == nwh - 1, shifted && wx == nww - 1);
    // O = P . V: register e of an S^T tile is the A operand of one k-step (keys (e&3) + 8*(e>>2) + 4*h of the tile)
    f32x16 z[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int e = 0; e < 16; ++e) z[qt][e] = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float vb = Vs[(kt * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh) * RP + li];
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) z[qt] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[kt][qt][e], vb, z[qt], 0, 0, 0);
        }
    float* zl = Qs;   // Q is dead
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int e = 0; e < 16; ++e) zl[(qt * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh) * RP + li] = z[qt][e];
    if (act) {
        float* dst = out + tok * C + head * 32;
#pragma unroll
        for (int d = 0; d < 32; d += 4) {
            const f32x4 v = {zl[lane * RP + d], zl[lane * RP + d + 1], zl[lane * RP + d + 2], zl[lane * RP + d + 3]};
            *(f32x4*)(dst + d) = v;
        }
    }
}

// ---- tail (:414-420): LayerNorm(96, eps 1e-6) per token -> GeM_1D over the tokens -> BatchNorm1d.
// Stage 1: grid (image, slice): the sum over a slice of the tokens of clamp(LN(x), 1e-6)^p per channel -> part[img][slice][96]
// (one block per image left 3136 tokens to four waves and 7 % of the forward in this kernel).
constexpr int TAIL_SLICES = 16;
__global__ __launch_bounds__(256) void swin_tail_partial_kernel(const float* __restrict__ x, int ntok, const float* __restrict__ g,
                                                                const float* __restrict__ b, const float* __restrict__ p_ptr,
                                                                float* __restrict__ partial) {
    __shared__ float part[4][96];
    const int img = blockIdx.x, slice = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float p = p_ptr[0];
    const float g0 = g[lane], b0 = b[lane];
    const float g1 = lane < 32 ? g[64 + lane] : 0.f, b1 = lane < 32 ? b[64 + lane] : 0.f;
    const int per = (ntok + TAIL_SLICES - 1) / TAIL_SLICES;
    const int t0 = slice * per, t1 = t0 + per < ntok ? t0 + per : ntok;
    float a0 = 0.f, a1 = 0.f;
    // x^p: p = 3 (the initial value of the learnable exponent) is two multiplies, anything else exp2(p log2 x) on the
    // transcendental unit (x >= 1e-6 > 0) - ocml's powf cost this kernel more than its HBM traffic
    const bool cube = p == 3.0f;
    auto pw = [&](float v) { return cube ? v * v * v : __builtin_amdgcn_exp2f(p * __builtin_amdgcn_logf(v)); };
    auto token = [&](float v0, float v1) {
        const float mean = wsum(v0 + v1) / 96.f;
        const float d0 = v0 - mean, d1 = lane < 32 ? v1 - mean : 0.f;
        const float rstd = 1.0f / sqrtf(wsum(d0 * d0 + d1 * d1) / 96.f + 1e-6f);
        // clamp(min = 1e-6) as torch's: a NaN stays a NaN (fmaxf returns the other operand, and a non-finite token left as 1e-6)
        const float y0 = d0 * rstd * g0 + b0, y1 = d1 * rstd * g1 + b1;
        a0 += pw(y0 < 1e-6f ? 1e-6f : y0);
        if (lane < 32) a1 += pw(y1 < 1e-6f ? 1e-6f : y1);
    };
    int t = t0 + wave;
    for (; t + 12 < t1; t += 16) {      // four tokens per wave and trip: their loads are in flight together
        float u0[4], u1[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float* xi = x + ((long long)img * ntok + t + 4 * k) * 96;
            u0[k] = xi[lane];
            u1[k] = lane < 32 ? xi[64 + lane] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) token(u0[k], u1[k]);
    }
    for (; t < t1; t += 4) {
        const float* xi = x + ((long long)img * ntok + t) * 96;
        token(xi[lane], lane < 32 ? xi[64 + lane] : 0.f);
    }
    part[wave][lane] = a0;
    if (lane < 32) part[wave][64 + lane] = a1;
    __syncthreads();
    if (threadIdx.x < 96) {
        const int c = threadIdx.x;
        partial[((long long)img * TAIL_SLICES + slice) * 96 + c] = part[0][c] + part[1][c] + part[2][c] + part[3][c];
    }
}
// Stage 2: mean over the tokens, ^(1/p), BatchNorm1d
__global__ void swin_tail_final_kernel(const float* __restrict__ partial, int n, int ntok, const float* __restrict__ p_ptr,
                                       const float* __restrict__ bn_s, const float* __restrict__ bn_t,
                                       float* __restrict__ gem_out, float* __restrict__ emb, int* __restrict__ fault) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * 96) return;
    const int img = i / 96, c = i - img * 96;
    float s = 0.f;
    for (int k = 0; k < TAIL_SLICES; ++k) s += partial[((long long)img * TAIL_SLICES + k) * 96 + c];
    const float gm = powf(s / (float)ntok, 1.0f / p_ptr[0]);
    if (gem_out) gem_out[i] = gm;
    const float ev = gm * bn_s[c] + bn_t[c];
    emb[i] = ev;
    if (fault && !(fabsf(ev) < INFINITY)) fault[1] = 1;   // a non-finite embedding: the context reports it (reid_ctx.fault)
}

inline int grid_for(long long work, int block) {
    long long g = (work + block - 1) / block;
    return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

// ------------------------------------------------------------------------------------------------ GEMM helpers
// x_packed (precision 2): x already as [xh | xl'] f16 [m][2k]; out_packed: the result as [yh | yl'] f16 [m][2n] instead of fp32 `out`
int linear(reid_ctx* ctx, const float* x, long long m, int k, const float* w, const float* bias, int n, int act,
           const float* residual, float* out, const f16* x_packed = nullptr, f16* out_packed = nullptr) {
    // (only for packed inputs - the block linears of mode 2; the classifier's [n][96] input stays on the exact kernel for every batch
    // size: which arithmetic a layer runs in must not depend on how many images a pass holds)
    if (ctx->precision == 2 && k % 32 == 0 && x_packed) {
        // fp32-class arithmetic on the f16 matrix pipe (reid_ctx_set_precision(ctx, 2); the ResNet convolutions' trick,
        // conv3x3_f16.hip): x -> [xh | xl'] f16, weights [wh 2^11 | wh | wl'] made once, three products per multiply through the
        // f16 linear build with K = 3 k virtual columns, fp32 accumulate, fp32 in / out
        const f16* a16 = x_packed;
        if (!a16) {
            f16* buf;
            REID_TRY(ctx_ws(ctx, "swin.split.a", (size_t)m * 2 * k * 2, (void**)&buf));
            REID_TRY(launch_split_pack(ctx, x, m, k, buf));
            a16 = buf;
        }
        const int npad = (n + 63) / 64 * 64;
        auto it = ctx->split_w.find(w);
        if (it == ctx->split_w.end()) {
            void* w16;
            HIP_TRY(hipMalloc(&w16, (size_t)npad * 3 * k * 2));
            HIP_TRY(hipMemsetAsync(w16, 0, (size_t)npad * 3 * k * 2, ctx->stream));
            REID_TRY(launch_split_weights(ctx, w, n, 1, k, 3, (f16*)w16));
            it = ctx->split_w.emplace(w, w16).first;
        }
        Gemm16Params q;
        memset(&q, 0, sizeof(q));
        q.A = a16; q.lda = 2 * k;
        q.B = (const f16*)it->second; q.ldb = 3 * k;
        q.M = (int)m; q.N = npad; q.K = 3 * k;
        if (out_packed) {   // f16 [m][2n]: the epilogue writes the hi tile, then the low tile n columns further
            q.C = out_packed; q.ldc = 2 * n; q.pack_out = 1;
        } else {
            q.C32 = out; q.ldc = n;
        }
        q.col_shift = bias; q.lin = 1; q.act = act; q.n_real = n; q.res32 = residual;
        q.split_terms = 3; q.a_k = 2 * k; q.acc_scale = 1.0f / 2048.0f;
        if (lin_x3_supported(ctx, q))     // stages 3-4 (N % 128 == 0): 4-wave blocks, two per CU, xh fragments shared by two of the three products
            return launch_lin_x3(ctx, q, REID_K_CONV_GEMM, 2.0 * m * n * k, 4.0 * ((double)m * k + (double)n * k + (double)m * n));
        return launch_gemm_f16(ctx, A16_DENSE, q, REID_K_CONV_GEMM, 2.0 * m * n * k, 4.0 * ((double)m * k + (double)n * k + (double)m * n));
    }
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.A = x; p.lda = k;
    p.B = w; p.ldb = k;
    p.M = (int)m; p.N = n; p.K = k;
    p.C = out; p.ldc = n;
    p.col_shift = bias; p.act = act; p.residual = residual;
    return launch_gemm_f32(ctx, A_DENSE, E_BIAS, p, REID_K_CONV_GEMM, 2.0 * m * n * k, 4.0 * ((double)m * k + (double)n * k + (double)m * n));
}

// fp16-storage linear on the f16 MFMA GEMM: x f16 [m][lda], w f16 [n padded to 64][k]; out = act(x.w^T + bias) (+ res32),
// written as f16 (out16, row stride ldc) or into the fp32 residual stream (out32)
int linear16(reid_ctx* ctx, const f16* x, long long m, int lda, int k, const f16* w, const float* bias, int n, int act,
             const float* res32, f16* out16, float* out32, int ldc) {
    Gemm16Params p;
    memset(&p, 0, sizeof(p));
    p.A = x; p.lda = lda;
    p.B = w; p.ldb = k;
    p.M = (int)m; p.N = (n + 63) / 64 * 64; p.K = k;
    p.C = out16; p.C32 = out32; p.ldc = ldc;
    p.col_shift = bias; p.lin = 1; p.act = act; p.n_real = n; p.res32 = res32;
    return launch_gemm_f16(ctx, A16_DENSE, p, REID_K_CONV_GEMM, 2.0 * m * n * k, 2.0 * ((double)m * k + (double)n * k) + (out32 ? 4.0 : 2.0) * m * n);
}

// fp16-storage convolution (patch merging, alignment conv, ConvTranspose parity) on the f16 MFMA GEMM: im2col gather of an
// NHWC f16 map, weights [Cout padded to 64][R*S*Cin]; out = conv + bias (+ res32 at the output index), f16 or fp32
int conv16(reid_ctx* ctx, const f16* zero_page, const f16* x, int n, int H, int W, int Cin, const f16* w, const float* bias,
           int Cout, int R, int S, int stride, int pad_y, int pad_x, int Ho, int Wo, const float* res32, f16* out16, float* out32,
           int scat_h = 0, int scat_w = 0, int py = 0, int px = 0, long long par_stride = 0) {
    Gemm16Params p;
    memset(&p, 0, sizeof(p));
    p.A = x;
    p.par4 = par_stride != 0; p.par_stride = par_stride;   // all four ConvTranspose parities in one launch (pads / scatter per grid copy)
    p.H = H; p.W = W; p.Cin = Cin; p.R = R; p.S = S; p.stride = stride; p.asym = 1; p.pad_y = pad_y; p.pad_x = pad_x;
    p.Ho = Ho; p.Wo = Wo;
    p.B = w; p.ldb = (long long)R * S * Cin;
    p.M = n * Ho * Wo; p.N = (Cout + 63) / 64 * 64; p.K = R * S * Cin;
    p.C = out16; p.C32 = out32; p.ldc = Cout;
    p.col_shift = bias; p.lin = 1; p.n_real = Cout; p.res32 = res32;
    set_scatter(p, scat_h, scat_w, py, px);
    p.zero_page = zero_page;
    return launch_gemm_f16(ctx, A16_IM2COL, p, REID_K_CONV_GEMM, 2.0 * p.M * Cout * p.K,
                           2.0 * ((double)n * H * W * Cin + (double)Cout * p.K) + (out32 ? 4.0 : 2.0) * p.M * Cout);
}

// generic NHWC conv as implicit GEMM with bias (+residual); scatter for ConvTranspose parities
// precision 2: a convolution of the Swin trunk (patch merging, the 8x8 stride-8 alignment conv, a ConvTranspose as four parity
// convolutions in one launch) in fp32-class arithmetic: x packed to [xh | xl'], weights [wh 2^11 | wh | wl'] per tap made once,
// the f16 im2col linear build over 3 Cin virtual channels, fp32 out.  parities = 4: `w` holds the four parity weight sets.
int conv_split(reid_ctx* ctx, const float* x, int n, int H, int W, int Cin, const float* w, const float* bias, int Cout, int R, int S,
               int stride, int pad_y, int pad_x, int Ho, int Wo, const float* residual, float* out, int scat_h, int scat_w, int py,
               int px, int parities, const f16* zero_page) {
    const long long rows = (long long)n * H * W;
    f16* a16;
    REID_TRY(ctx_ws(ctx, "swin.split.a", (size_t)rows * 2 * Cin * 2, (void**)&a16));
    REID_TRY(launch_split_pack(ctx, x, rows, Cin, a16));
    const int npad = (Cout + 63) / 64 * 64, taps = R * S;
    const size_t per = (size_t)npad * taps * 3 * Cin;
    auto it = ctx->split_w.find(w);
    if (it == ctx->split_w.end()) {
        void* w16;
        HIP_TRY(hipMalloc(&w16, per * parities * 2));
        HIP_TRY(hipMemsetAsync(w16, 0, per * parities * 2, ctx->stream));
        for (int q = 0; q < parities; ++q)
            REID_TRY(launch_split_weights(ctx, w + (size_t)q * Cout * taps * Cin, Cout, taps, Cin, 3, (f16*)w16 + q * per));
        it = ctx->split_w.emplace(w, w16).first;
    }
    Gemm16Params p;
    memset(&p, 0, sizeof(p));
    p.A = a16;
    p.par4 = parities == 4; p.par_stride = (long long)per;
    p.H = H; p.W = W; p.Cin = 3 * Cin; p.R = R; p.S = S; p.stride = stride; p.asym = 1; p.pad_y = pad_y; p.pad_x = pad_x;
    p.Ho = Ho; p.Wo = Wo;
    p.B = (const f16*)it->second; p.ldb = (long long)taps * 3 * Cin;
    p.M = n * Ho * Wo; p.N = npad; p.K = taps * 3 * Cin;
    p.C32 = out; p.ldc = Cout;
    p.col_shift = bias; p.lin = 1; p.n_real = Cout; p.res32 = residual;
    p.split_terms = 3; p.acc_scale = 1.0f / 2048.0f;
    set_scatter(p, scat_h, scat_w, py, px);
    p.zero_page = zero_page;
    return launch_gemm_f16(ctx, A16_IM2COL, p, REID_K_CONV_GEMM, 2.0 * p.M * Cout * taps * Cin * parities,
                           4.0 * ((double)rows * Cin + (double)Cout * taps * Cin * parities + (double)p.M * Cout * parities));
}

int conv_bias(reid_ctx* ctx, const float* x, int n, int H, int W, int Cin, const float* w, const float* bias, int Cout, int R,
              int S, int stride, int pad_y, int pad_x, int Ho, int Wo, const float* residual, float* out, int scat_h = 0,
              int scat_w = 0, int py = 0, int px = 0, const f16* zero_page = nullptr) {
    if (ctx->precision == 2 && zero_page && Cin % 32 == 0)
        return conv_split(ctx, x, n, H, W, Cin, w, bias, Cout, R, S, stride, pad_y, pad_x, Ho, Wo, residual, out, scat_h, scat_w, py, px, 1,
                          zero_page);
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.A = x;
    p.H = H; p.W = W; p.Cin = Cin; p.R = R; p.S = S; p.stride = stride; p.pad_y = pad_y; p.pad_x = pad_x;
    p.Ho = Ho; p.Wo = Wo;
    p.B = w; p.ldb = R * S * Cin;
    p.M = n * Ho * Wo; p.N = Cout; p.K = R * S * Cin;
    p.C = out; p.ldc = Cout;
    p.col_shift = bias; p.residual = residual;
    set_scatter(p, scat_h, scat_w, py, px);
    const double flops = 2.0 * p.M * Cout * p.K;
    const double bytes = 4.0 * ((double)n * H * W * Cin + (double)Cout * p.K + (double)p.M * Cout);
    if (ctx->f32_conv == 1 && conv_f32_general_supported(p)) return launch_conv_f32_general(ctx, p, REID_K_CONV_GEMM, flops, bytes);
    return launch_gemm_f32(ctx, A_IM2COL, E_BIAS, p, REID_K_CONV_GEMM, flops, bytes);
}

// ConvTranspose2d(4, 2, 1) as its four output parities (2x2 stride-1 convs with one-sided padding, scattered to (2j+py, 2i+px));
// wts: four [Cout][4 Cin] matrices.  One launch of 4 x the tile grid on the LDS-DMA kernel, else one launch per parity.
int conv_transpose_parities(reid_ctx* ctx, const float* x, int n, int Hi, int Wi, int ci, const float* wts, const float* bias, int co,
                            const float* residual, float* out, const f16* zero_page = nullptr) {
    if (ctx->precision == 2 && zero_page && ci % 32 == 0)
        return conv_split(ctx, x, n, Hi, Wi, ci, wts, bias, co, 2, 2, 1, 1, 1, Hi, Wi, residual, out, Hi, Wi, 0, 0, 4, zero_page);
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.A = x;
    p.H = Hi; p.W = Wi; p.Cin = ci; p.R = 2; p.S = 2; p.stride = 1; p.pad_y = 1; p.pad_x = 1;
    p.Ho = Hi; p.Wo = Wi;
    p.B = wts; p.ldb = 4 * ci;
    p.M = n * Hi * Wi; p.N = co; p.K = 4 * ci;
    p.C = out; p.ldc = co;
    p.col_shift = bias; p.residual = residual;
    set_scatter(p, Hi, Wi, 0, 0);
    if (ctx->f32_conv == 1 && conv_f32_general_supported(p)) {
        p.par4 = 1;
        p.par_stride = (long long)co * 4 * ci;
        return launch_conv_f32_general(ctx, p, REID_K_CONV_GEMM, 8.0 * p.M * co * p.K,
                                       4.0 * ((double)n * Hi * Wi * ci + 4.0 * co * p.K + 4.0 * p.M * co));
    }
    for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px)
            REID_TRY(conv_bias(ctx, x, n, Hi, Wi, ci, wts + (size_t)(py * 2 + px) * co * 4 * ci, bias, co, 2, 2, 1, 1 - py, 1 - px, Hi, Wi, residual,
                               out, Hi, Wi, py, px));
    return REID_OK;
}

const int kDims[4] = {96, 192, 384, 768}, kLayers[4] = {2, 2, 6, 2}, kHeads[4] = {3, 6, 12, 24};

}  // namespace

// ------------------------------------------------------------------------------------------------ launchers shared with the harnesses
// (reid_internal.h; include/reid_hip_debug.h: each harness of tests/test_gpu_swin_kernels.py goes through the function the forward calls)

// The relative-position bias of one block (pos [13][13]) expanded to the [key 64][query 64] table of the MFMA attention kernels: -inf on
// the padded keys, 0 on the padded queries (same entries as build_bias_table).  Host side: reid_swin_load makes one per block.
void swin_bias_table(const float* pos169, float* tab4096) {
    for (int key = 0; key < 64; ++key)
        for (int query = 0; query < 64; ++query) {
            float b = 0.f;
            if (key >= 49) b = -INFINITY;
            else if (query < 49) b = pos169[(key / 7 - query / 7 + 6) * 13 + (key % 7 - query % 7 + 6)];
            tab4096[key * 64 + query] = b;
        }
}

// Row stride of the qkv buffer the attention kernel of this context's precision reads: the f16 GEMM writes rows padded to its 64-wide tile
int swin_attn_ldq(const reid_ctx* ctx, int C) { return ctx->precision == 1 ? (3 * C + 63) / 64 * 64 : 3 * C; }

// WindowAttention v1 of one block: the context's precision and switches pick the kernel, its grid and which form of the bias it reads.
//   precision 1: qkv f16 [T][ldq] -> out f16 [T][C]; matrix-core kernel (bias_tab) unless swin_attn_mfma == 0 (VALU kernel, pos)
//   precision 2: qkv fp32 [T][3C] -> out f16 [T][2C] = [oh | ol']; VALU kernel (pos) unless swin_attn_split (matrix cores, bias_tab)
//   precision 0: qkv fp32 [T][3C] -> out fp32 [T][C]; VALU kernel unless swin_attn_mfma == 2 (v_mfma_f32_32x32x2_f32), both read pos
int launch_window_attn(reid_ctx* ctx, const void* qkv, int n, int Hs, int Ws, int heads, int shifted, const float* pos, const float* bias_tab,
                       void* out) {
    const int C = heads * 32, ldq = swin_attn_ldq(ctx, C);
    const long long T = (long long)n * Hs * Ws, ntask = (long long)n * (Hs / 7) * (Ws / 7) * heads;
    const dim3 grid4((unsigned)((ntask + 3) / 4));
    prof_begin(ctx, REID_K_ELEMENTWISE, 0, (double)T * C * (ctx->precision == 1 ? 8 : 16));
    if (ctx->precision == 1) {
        if (ctx->swin_attn_mfma)
            hipLaunchKernelGGL(window_attn_mfma_f16_kernel, grid4, dim3(256), 0, ctx->stream, (const f16*)qkv, ldq, n, Hs, Ws, heads, shifted,
                               bias_tab, (f16*)out);
        else
            hipLaunchKernelGGL(window_attn_kernel<f16>, grid4, dim3(256), 0, ctx->stream, (const f16*)qkv, ldq, n, Hs, Ws, heads, shifted, pos,
                               (f16*)out);
    } else if (ctx->precision == 2) {
        if (ctx->swin_attn_split)
            hipLaunchKernelGGL(window_attn_mfma_split_kernel, grid4, dim3(256), 0, ctx->stream, (const float*)qkv, ldq, n, Hs, Ws, heads, shifted,
                               bias_tab, (f16*)out, ctx->fault);
        else
            hipLaunchKernelGGL(window_attn_kernel<float>, grid4, dim3(256), 0, ctx->stream, (const float*)qkv, ldq, n, Hs, Ws, heads, shifted,
                               pos, (float*)nullptr, (f16*)out, ctx->fault);
    } else if (ctx->swin_attn_mfma == 2) {   // fp32 MFMA runs at the fp32 VALU rate: measured 5 % slower than the VALU kernel, kept for A/B
        hipLaunchKernelGGL(window_attn_mfma_f32_kernel, dim3((unsigned)((ntask + 1) / 2)), dim3(128), 0, ctx->stream, (const float*)qkv, ldq, n,
                           Hs, Ws, heads, shifted, pos, (float*)out);
    } else {
        hipLaunchKernelGGL(window_attn_kernel<float>, grid4, dim3(256), 0, ctx->stream, (const float*)qkv, ldq, n, Hs, Ws, heads, shifted, pos,
                           (float*)out);
    }
    prof_end(ctx);
    LAUNCH_CHECK();
    return REID_OK;
}

// LayerNorm (eps 1e-5) of T rows of C channels through the forward's three launchers: form 0 fp32 out, 1 f16 out, 2 [yh | yl'] f16 [T][2C]
int launch_swin_layernorm(reid_ctx* ctx, int form, const float* x, long long T, int C, const float* g, const float* b, void* out) {
    if (form == 0) launch_layernorm<float>(ctx, x, T, C, g, b, (float*)out);
    else if (form == 1) launch_layernorm<f16>(ctx, x, T, C, g, b, (f16*)out);
    else launch_layernorm_packed(ctx, x, T, C, g, b, (f16*)out);
    LAUNCH_CHECK();
    return REID_OK;
}

// ShadowFeatureExtraction after its first convolution: MixedNorm statistics of c1 [n][h1][w1][12] -> ab [n][24], then MixedNorm + ReLU ->
// conv2x2 s2 -> ReLU -> Linear -> tok [n][h1 / 2][w1 / 2][96].  No profiling bracket of its own: the forward runs it inside the stem's.
int launch_sfe_norm_fc(reid_ctx* ctx, const float* c1, int n, int h1, int w1, const float* in_g, const float* in_b, const float* bn_s,
                       const float* bn_t, const float* c2_w, const float* c2_b, const float* fc_w, const float* fc_b, float* ab, float* tok) {
    hipLaunchKernelGGL(sfe_norm_kernel, dim3(n), dim3(256), 0, ctx->stream, c1, h1 * w1, in_g, in_b, bn_s, bn_t, ab);
    hipLaunchKernelGGL(sfe_conv2_fc_kernel, dim3(grid_for((long long)n * (h1 / 2) * (w1 / 2), 256)), dim3(256), 0, ctx->stream, c1, ab, n, h1,
                       w1, c2_w, c2_b, fc_w, fc_b, tok);
    LAUNCH_CHECK();
    return REID_OK;
}

// The tail: LayerNorm(96, eps 1e-6) -> GeM_1D over ntok tokens -> BatchNorm1d, x [n][ntok][96] -> gem [n][96] (may be null), emb [n][96].
// No profiling bracket of its own.
int launch_swin_tail(reid_ctx* ctx, const float* x, int n, int ntok, const float* g, const float* b, const float* p, const float* bn_s,
                     const float* bn_t, float* gem, float* emb) {
    float* tail_part;
    REID_TRY(ctx_ws(ctx, "swin.tailp", (size_t)n * TAIL_SLICES * 96 * 4, (void**)&tail_part));
    hipLaunchKernelGGL(swin_tail_partial_kernel, dim3(n, TAIL_SLICES), dim3(256), 0, ctx->stream, x, ntok, g, b, p, tail_part);
    hipLaunchKernelGGL(swin_tail_final_kernel, dim3((n * 96 + 255) / 256), dim3(256), 0, ctx->stream, tail_part, n, ntok, p, bn_s, bn_t, gem,
                       emb, ctx->fault);
    LAUNCH_CHECK();
    return REID_OK;
}

// libreid_hip_swin_v2.so, opened from the directory this library lies in when the first v2 checkpoint is loaded (or a v2 harness runs):
// a process that never loads v2 weights never opens it.  Missing library or symbol: REID_ERR_STATE naming the file - no other path runs v2.
static struct SwinV2Lib : SideLib {
    SwinV2Lib() : SideLib("libreid_hip_swin_v2.so", "Swin v2 needs") {}
    SIDE_FN(attn, swin_v2_window_attn_cos);
    SIDE_FN(post_norm, swin_v2_post_norm);
} swin_v2;

// libreid_hip_swin_crops.so (swin_crops.h), opened the same way on the first crops call (reid_swin_embed_ragged_u8 / _frame_u8, or their
// harness): a process that only embeds float images never opens it.  Missing library or symbol: REID_ERR_STATE naming the file - there
// is no other path from uint8 crops to the Swin stem.
static struct SwinCropsLib : SideLib {
    SwinCropsLib() : SideLib("libreid_hip_swin_crops.so", "Swin from uint8 crops needs") {}
    SIDE_FN(front, swin_crops_front);
} swin_crops;

// libreid_hip_swin_eval.so (swin_eval.h), opened the same way on the first descriptor call (reid_swin_descriptor_*, or a harness of its
// kernels): a process that only embeds never opens it.  Missing library or symbol: REID_ERR_STATE naming the file - there is no other path
// to a Swin descriptor.
static struct SwinEvalLib : SideLib {
    SwinEvalLib() : SideLib("libreid_hip_swin_eval.so", "Swin descriptors need") {}
    SIDE_FN(conv1_mirror, swin_eval_conv1_mirror);
    SIDE_FN(crop_front_mirror, swin_eval_crop_front_mirror);
    SIDE_FN(max_classes, swin_eval_max_classes);
    SIDE_FN(descriptor, swin_eval_descriptor);
} swin_eval;

// ------------------------------------------------------------------------------------------------ weights
struct SwinBlockW {
    // v2: no pos; bias_t = the block's position-bias table as [head][key 49][query 64] (made at load time from the blob's
    // [head][query][key] .bias), scale = exp(min(logit_scale, ln 100)) per head
    const float *bias_t = nullptr, *scale = nullptr, *bias = nullptr;   // bias: the blob's [head][query][key] table
    const float *ln1_g, *ln1_b, *qkv_w, *pos, *out_w, *out_b, *post_w, *post_b, *ln2_g, *ln2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
};
struct SwinBlockW16 {
    const f16 *qkv, *out, *post, *fc1, *fc2;   // [N padded to a multiple of 64][K], zero rows past N
    // to_out and post_proj (swin_transformer.py:226-231: two Linear layers with nothing in between) folded into one for the
    // fp16-storage mode: W = W_post . W_out (fp32 GEMM at load time), b = W_post . b_out + b_post
    const f16* fold;
    const float* fold_b;
    const float* bias_tab;   // relative-position bias expanded to [key 64][query 64] fp32, -inf on padded keys (window_attn_mfma_f16_kernel)
};
struct SwinWeights {
    bool loaded = false;
    float* blob = nullptr;
    f16* blob16 = nullptr;        // fp16-storage mode: the block linears
    float* fold_bias = nullptr;   // folded biases of the twelve blocks, back to back
    float* bias_tabs = nullptr;   // expanded relative-position bias tables of the twelve blocks (v2: their bias_t tables)
    int version = 1;              // 1 / 2: the manifest's swin.version entry (absent: 1)
    SwinBlockW16 blk16[12];
    const f16 *merge16[4], *img16, *t16[3];   // patch merging, 8x8 alignment conv, ConvTranspose parities (rows padded to 64)
    f16* zero_page = nullptr;
    int num_class = 0;
    const float *c1_w, *c1_b, *in_g, *in_b, *bn_s, *bn_t, *c2_w, *c2_b, *fc_w, *fc_b;
    SwinBlockW blk[12];
    const float *merge_w[4], *merge_b[4];
    const float *img_w, *img_b, *t_w[3], *t_b[3];
    const float *tail_g, *tail_b, *tail_p, *neck_s, *neck_t, *cls_w;
    const float* side = nullptr;   // [views][96] side-information table of the SFE (sfe.side; optional) and its coefficient
    int views = 0;
    float side_coeff = 1.5f;
};

// context -> its Swin weights.  Camera streams load / destroy contexts from several host threads: every access to the map itself
// goes through swin_mutex (std::map nodes are stable, so a SwinWeights found under the lock stays valid until its own context
// is destroyed - which the owner of that context does, not another thread).
static std::mutex& swin_mutex() {
    static std::mutex m;
    return m;
}
static std::map<reid_ctx*, SwinWeights>& swin_registry() {
    static std::map<reid_ctx*, SwinWeights> r;
    return r;
}
static SwinWeights* swin_find(reid_ctx* ctx) {
    std::lock_guard<std::mutex> lk(swin_mutex());
    auto it = swin_registry().find(ctx);
    return it == swin_registry().end() ? nullptr : &it->second;
}

void swin_release(reid_ctx* ctx) {
    // split forms of the old blob's weights (precision 2) are keyed by address: a new blob may reuse the addresses
    for (auto& kv : ctx->split_w) (void)hipFree(kv.second);
    ctx->split_w.clear();
    std::lock_guard<std::mutex> lk(swin_mutex());
    auto& r = swin_registry();
    auto it = r.find(ctx);
    if (it != r.end()) {
        if (it->second.blob) (void)hipFree(it->second.blob);
        if (it->second.blob16) (void)hipFree(it->second.blob16);
        if (it->second.fold_bias) (void)hipFree(it->second.fold_bias);
        if (it->second.bias_tabs) (void)hipFree(it->second.bias_tabs);
        if (it->second.zero_page) (void)hipFree(it->second.zero_page);
        r.erase(it);
    }
}

extern "C" int reid_swin_load(reid_ctx* ctx, const float* blob, size_t n_floats, const char* manifest) {
    ARG_CHECK(ctx && blob && manifest && n_floats > 0);
    CTX_GUARD(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    std::map<std::string, std::pair<size_t, size_t>> tab;
    {
        std::istringstream in(manifest);
        std::string name;
        size_t off, cnt;
        while (in >> name >> off >> cnt) {
            if (off + cnt > n_floats || off % 4 != 0) {
                reid_set_error("swin manifest entry '%s' out of range or not 16-byte aligned", name.c_str());
                return REID_ERR_ARG;
            }
            tab[name] = {off, cnt};
        }
    }
    {   // precision 2 operand range, as in reid_seres18_load: every Linear / convolution weight of the trunk is split
        const float lim = 65504.0f / 2048.0f;
        const std::string bad = split_range_violation(blob, tab, {{".qkv.w", lim}, {".out.w", lim}, {".post.w", lim}, {".fc1.w", lim},
                                                                  {".fc2.w", lim}, {".merge.w", lim}, {"align.img.w", lim},
                                                                  {"align.t0.w", lim}, {"align.t1.w", lim}, {"align.t2.w", lim}});
        if (!bad.empty() && ctx->precision == 2) {
            reid_set_error("reid_swin_load: weight tensor %s cannot be split for the fp32-class arithmetic selected on this context "
                           "(reid_ctx_set_precision 2 needs |w| 2^11 < 65504); load it in mode 0", bad.c_str());
            return REID_ERR_ARG;
        }
        ctx->split_bad_swin = bad;
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    swin_release(ctx);
    SwinWeights w;
    HIP_TRY(hipMalloc((void**)&w.blob, n_floats * sizeof(float)));
    HIP_TRY(hipMemcpy(w.blob, blob, n_floats * sizeof(float), hipMemcpyHostToDevice));
    {
        auto ver = tab.find("swin.version");
        if (ver != tab.end()) {
            const float v = ver->second.second == 1 ? blob[ver->second.first] : 0.f;
            if (v != 1.0f && v != 2.0f) {
                reid_set_error("reid_swin_load: manifest entry 'swin.version' must hold 1 or 2");
                (void)hipFree(w.blob);
                return REID_ERR_ARG;
            }
            w.version = (int)v;
            if (w.version == 2) {   // the v2 kernels' library: absent -> refuse the checkpoint here, not in the middle of a forward
                const int rc = swin_v2.open();
                if (rc != REID_OK) {
                    (void)hipFree(w.blob);
                    return rc;
                }
            }
        }
    }
    bool missing = false;
    std::string first;
    auto get = [&](const std::string& name, size_t expect) -> const float* {
        auto it = tab.find(name);
        if (it == tab.end() || (expect && it->second.second != expect)) {
            if (!missing) first = name;
            missing = true;
            return nullptr;
        }
        return w.blob + it->second.first;
    };
    w.c1_w = get("sfe.conv1.w", 144); w.c1_b = get("sfe.conv1.b", 12);
    w.in_g = get("sfe.in_gamma", 6); w.in_b = get("sfe.in_beta", 6);
    w.bn_s = get("sfe.bn_scale", 6); w.bn_t = get("sfe.bn_shift", 6);
    w.c2_w = get("sfe.conv2.w", 48 * 48); w.c2_b = get("sfe.conv2.b", 48);
    w.fc_w = get("sfe.fc.w", 96 * 48); w.fc_b = get("sfe.fc.b", 96);
    int bi = 0;
    for (int s = 0; s < 4; ++s) {
        const size_t c = kDims[s];
        const std::string st = "s" + std::to_string(s + 1);
        if (s > 0) {
            w.merge_w[s] = get(st + ".merge.w", c * 4 * kDims[s - 1]);
            w.merge_b[s] = get(st + ".merge.b", c);
        }
        for (int j = 0; j < kLayers[s]; ++j, ++bi) {
            const std::string b = st + ".b" + std::to_string(j);
            SwinBlockW& k = w.blk[bi];
            k.ln1_g = get(b + ".ln1.g", c); k.ln1_b = get(b + ".ln1.b", c);
            k.qkv_w = get(b + ".qkv.w", 3 * c * c);
            if (w.version == 2) {
                k.pos = nullptr;
                k.bias = get(b + ".bias", (size_t)kHeads[s] * 49 * 49);
                k.scale = get(b + ".scale", (size_t)kHeads[s]);
            } else {
                k.pos = get(b + ".pos", 169);
            }
            k.out_w = get(b + ".out.w", c * c); k.out_b = get(b + ".out.b", c);
            k.post_w = get(b + ".post.w", c * c); k.post_b = get(b + ".post.b", c);
            k.ln2_g = get(b + ".ln2.g", c); k.ln2_b = get(b + ".ln2.b", c);
            k.fc1_w = get(b + ".fc1.w", 4 * c * c); k.fc1_b = get(b + ".fc1.b", 4 * c);
            k.fc2_w = get(b + ".fc2.w", 4 * c * c); k.fc2_b = get(b + ".fc2.b", c);
        }
    }
    w.img_w = get("align.img.w", 768 * 64 * 96); w.img_b = get("align.img.b", 768);
    for (int t = 0; t < 3; ++t) {   // ConvTranspose 768->384, 384->192, 192->96: four parity GEMMs each
        const size_t ci = kDims[3 - t], co = kDims[2 - t];
        w.t_w[t] = get("align.t" + std::to_string(t) + ".w", 4 * co * 4 * ci);
        w.t_b[t] = get("align.t" + std::to_string(t) + ".b", co);
    }
    w.tail_g = get("tail.ln.g", 96); w.tail_b = get("tail.ln.b", 96); w.tail_p = get("tail.p", 1);
    w.neck_s = get("tail.bn_scale", 96); w.neck_t = get("tail.bn_shift", 96);
    auto cls = tab.find("cls.w");
    if (cls != tab.end() && cls->second.second % 96 == 0) {
        w.cls_w = w.blob + cls->second.first;
        w.num_class = (int)(cls->second.second / 96);
    } else {
        w.cls_w = nullptr;
    }
    // optional: ShadowFeatureExtraction's side-information embedding (swin_transformer.py:285-293, 301-302)
    auto sd = tab.find("sfe.side");
    auto sc = tab.find("sfe.side_coeff");
    if (sd != tab.end() && sc != tab.end() && sd->second.second % 96 == 0 && sc->second.second == 1) {
        w.side = w.blob + sd->second.first;
        w.views = (int)(sd->second.second / 96);
        w.side_coeff = blob[sc->second.first];
    }
    if (missing) {
        reid_set_error("reid_swin_load: manifest entry '%s' missing or of unexpected size", first.c_str());
        (void)hipFree(w.blob);
        return REID_ERR_ARG;
    }
    // fp16 copies of the block linears for reid_ctx_set_precision(ctx, 1): rows padded to a multiple of 64 (the f16 GEMM's
    // narrowest N tile); the padding rows are zero and their output columns are never stored
    {
        auto pad64 = [](size_t n) { return (n + 63) / 64 * 64; };
        size_t total = 0;
        for (int s = 0; s < 4; ++s) {
            const size_t c = kDims[s];
            total += (size_t)kLayers[s] * (pad64(3 * c) * c + 3 * pad64(c) * c + pad64(4 * c) * c + pad64(c) * 4 * c);
            if (s > 0) total += pad64(c) * 4 * kDims[s - 1];
        }
        total += (size_t)768 * 64 * 96;
        for (int t = 0; t < 3; ++t) total += 4 * pad64(kDims[2 - t]) * 4 * kDims[3 - t];
        HIP_TRY(hipMalloc((void**)&w.zero_page, 256));
        HIP_TRY(hipMemsetAsync(w.zero_page, 0, 256, ctx->stream));
        HIP_TRY(hipMalloc((void**)&w.blob16, total * sizeof(f16)));
        HIP_TRY(hipMemsetAsync(w.blob16, 0, total * sizeof(f16), ctx->stream));
        f16* cur = w.blob16;
        auto conv = [&](const float* src, size_t n, size_t k) -> const f16* {
            f16* dst = cur;
            (void)launch_f32_to_f16(ctx, src, n * k, dst);
            cur += pad64(n) * k;
            return dst;
        };
        int b2 = 0;
        size_t nbias = 0;
        for (int s = 0; s < 4; ++s) nbias += (size_t)kLayers[s] * kDims[s];
        HIP_TRY(hipMalloc((void**)&w.fold_bias, nbias * sizeof(float)));
        if (w.version == 2) {   // window_attn_cos_kernel's tables: [head][query][key] of the blob -> [head][key][query padded to 64]
            size_t total_heads = 0;
            for (int s = 0; s < 4; ++s) total_heads += (size_t)kLayers[s] * kHeads[s];
            std::vector<float> tabs(total_heads * 49 * 64, 0.f);
            std::vector<size_t> at(12);
            size_t cur_t = 0;
            int bt = 0;
            for (int s = 0; s < 4; ++s)
                for (int j = 0; j < kLayers[s]; ++j, ++bt) {
                    const float* src = blob + (w.blk[bt].bias - w.blob);   // the host copy of what get() found
                    at[bt] = cur_t;
                    for (int hd = 0; hd < kHeads[s]; ++hd)
                        for (int query = 0; query < 49; ++query)
                            for (int key = 0; key < 49; ++key)
                                tabs[cur_t + ((size_t)hd * 49 + key) * 64 + query] = src[((size_t)hd * 49 + query) * 49 + key];
                    cur_t += (size_t)kHeads[s] * 49 * 64;
                }
            HIP_TRY(hipMalloc((void**)&w.bias_tabs, tabs.size() * sizeof(float)));
            HIP_TRY(hipMemcpy(w.bias_tabs, tabs.data(), tabs.size() * sizeof(float), hipMemcpyHostToDevice));
            for (int i = 0; i < 12; ++i) {
                w.blk[i].bias_t = w.bias_tabs + at[i];
                w.blk16[i].bias_tab = nullptr;
            }
        } else {   // [key][query] bias tables of the MFMA attention kernel (same entries as build_bias_table)
            std::vector<float> tabs((size_t)12 * 4096);
            int bt = 0;
            for (int s = 0; s < 4; ++s)
                for (int j = 0; j < kLayers[s]; ++j, ++bt) {
                    const float* pos = blob + tab["s" + std::to_string(s + 1) + ".b" + std::to_string(j) + ".pos"].first;
                    swin_bias_table(pos, tabs.data() + (size_t)bt * 4096);
                }
            HIP_TRY(hipMalloc((void**)&w.bias_tabs, tabs.size() * sizeof(float)));
            HIP_TRY(hipMemcpy(w.bias_tabs, tabs.data(), tabs.size() * sizeof(float), hipMemcpyHostToDevice));
            for (int i = 0; i < 12; ++i) w.blk16[i].bias_tab = w.bias_tabs + (size_t)i * 4096;
        }
        float *d_t, *d_f;
        REID_TRY(ctx_ws(ctx, "swin.fold.t", (size_t)768 * 768 * 4, (void**)&d_t));
        REID_TRY(ctx_ws(ctx, "swin.fold.f", (size_t)768 * 768 * 4, (void**)&d_f));
        std::vector<float> out_t, bf;
        size_t bias_at = 0;
        for (int s = 0; s < 4; ++s) {
            const size_t c = kDims[s];
            const std::string st = "s" + std::to_string(s + 1);
            for (int j = 0; j < kLayers[s]; ++j, ++b2) {
                const SwinBlockW& k = w.blk[b2];
                SwinBlockW16& h = w.blk16[b2];
                h.qkv = conv(k.qkv_w, 3 * c, c);
                h.out = conv(k.out_w, c, c);
                h.post = conv(k.post_w, c, c);
                h.fc1 = conv(k.fc1_w, 4 * c, c);
                h.fc2 = conv(k.fc2_w, c, 4 * c);
                // fold: y = (x W_out^T + b_out) W_post^T + b_post = x (W_post W_out)^T + (W_post b_out + b_post)
                const std::string b = st + ".b" + std::to_string(j);
                const float* h_out = blob + tab[b + ".out.w"].first;
                const float* h_ob = blob + tab[b + ".out.b"].first;
                const float* h_post = blob + tab[b + ".post.w"].first;
                const float* h_pb = blob + tab[b + ".post.b"].first;
                out_t.resize(c * c);
                bf.resize(c);
                for (size_t r = 0; r < c; ++r)
                    for (size_t q = 0; q < c; ++q) out_t[q * c + r] = h_out[r * c + q];
                for (size_t r = 0; r < c; ++r) {
                    double acc = h_pb[r];
                    for (size_t q = 0; q < c; ++q) acc += (double)h_post[r * c + q] * h_ob[q];
                    bf[r] = (float)acc;
                }
                HIP_TRY(hipMemcpyAsync(d_t, out_t.data(), c * c * 4, hipMemcpyHostToDevice, ctx->stream));
                HIP_TRY(hipMemcpyAsync(w.fold_bias + bias_at, bf.data(), c * 4, hipMemcpyHostToDevice, ctx->stream));
                HIP_TRY(hipStreamSynchronize(ctx->stream));   // the host vectors are reused for the next block
                GemmParams g;
                memset(&g, 0, sizeof(g));
                g.A = k.post_w; g.lda = (long long)c;
                g.B = d_t; g.ldb = (long long)c;
                g.M = (int)c; g.N = (int)c; g.K = (int)c;
                g.C = d_f; g.ldc = (long long)c;
                REID_TRY(launch_gemm_f32(ctx, A_DENSE, E_BIAS, g, REID_K_CONV_GEMM, 0, 0));
                h.fold = conv(d_f, c, c);
                h.fold_b = w.fold_bias + bias_at;
                bias_at += c;
            }
        }
        for (int s = 1; s < 4; ++s) w.merge16[s] = conv(w.merge_w[s], kDims[s], 4 * (size_t)kDims[s - 1]);
        w.img16 = conv(w.img_w, 768, 64 * 96);
        for (int t = 0; t < 3; ++t) {   // four parity matrices [co][4*ci] each, every one padded on its own
            const size_t ci = kDims[3 - t], co = kDims[2 - t];
            w.t16[t] = cur;
            for (int q = 0; q < 4; ++q) (void)conv(w.t_w[t] + (size_t)q * co * 4 * ci, co, 4 * ci);
        }
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    w.loaded = true;
    {
        std::lock_guard<std::mutex> lk(swin_mutex());
        swin_registry()[ctx] = w;
    }
    return REID_OK;
}

extern "C" int reid_swin_dims(reid_ctx* ctx, int* embed_dim, int* num_class) {
    ARG_CHECK(ctx);
    CTX_GUARD(ctx);
    const SwinWeights* sw = swin_find(ctx);
    if (!sw) {
        reid_set_error("no Swin weights loaded");
        return REID_ERR_STATE;
    }
    if (embed_dim) *embed_dim = 96;
    if (num_class) *num_class = sw->num_class;
    return REID_OK;
}

// The two launches of libreid_hip_swin_v2.so (swin_v2.h) with the context's argument checks and profiling slots.
int launch_window_attn_cos(reid_ctx* ctx, int mode, const void* qkv, int ldq, int n_img, int H, int W, int heads, int shifted,
                           const float* bias_t, const float* scale, void* out) {
    if (mode < 0 || mode > 2 || !qkv || !bias_t || !scale || !out || n_img < 1 || heads < 1 || H < 7 || W < 7 || H % 7 || W % 7 ||
        ldq < 3 * heads * 32 || ldq % 4) {
        reid_set_error("launch_window_attn_cos: bad arguments (mode %d, %d x %d tokens, %d heads, ldq %d)", mode, H, W, heads, ldq);
        return REID_ERR_ARG;
    }
    REID_TRY(swin_v2.open());
    prof_begin(ctx, REID_K_ELEMENTWISE, 0, (double)n_img * H * W * heads * 32 * (mode == 1 ? 8 : 16));
    const hipError_t e = swin_v2.attn(ctx->stream, mode, qkv, ldq, n_img, H, W, heads, shifted, bias_t, scale, out, ctx->fault);
    prof_end(ctx);
    HIP_TRY(e);
    return REID_OK;
}

int launch_post_norm(reid_ctx* ctx, int side_mode, const float* x, const float* y, long long T, int C, const float* g, const float* b,
                     float* out, _Float16* side) {
    if (side_mode < 0 || side_mode > 2 || !x || !y || !g || !b || !out || (side_mode && !side) || T < 1 || C < 4 || C > 768 || C % 4) {
        reid_set_error("launch_post_norm: bad arguments (side %d, %lld rows of %d)", side_mode, T, C);
        return REID_ERR_ARG;
    }
    REID_TRY(swin_v2.open());
    prof_begin(ctx, REID_K_ELEMENTWISE, 0, (double)T * C * (12 + 2 * side_mode));
    const hipError_t e = swin_v2.post_norm(ctx->stream, side_mode, x, y, T, C, g, b, out, side, ctx->fault);
    prof_end(ctx);
    HIP_TRY(e);
    return REID_OK;
}

// One block of version "v2" (swin_transformer.py:238-246: Residual(PostNorm(attention)), Residual(PostNorm(feed-forward))):
//   x = x + LN(post_proj(to_out(cos_attn(to_qkv(x)))));   x = x + LN(fc2(gelu(fc1(x))))
// No LayerNorm in front of a linear: to_qkv reads the residual stream itself and fc1 the stream after the first post-norm, so in the
// fp32-class and fp16-storage modes the post-norm kernel also writes the [xh | xl'] pair / the f16 copy the next linear reads (into
// `att`, free by then); `first` = the stream was not written by a post-norm (first block of a stage): one pack / convert pass.
// The reference's two roundings to_out -> post_proj are kept in modes 0 and 2; mode 1 folds them as it does for v1 (swin_fold).
// Buffers as in swin_forward: big = qkv / MLP hidden, att, tmp, lnb = the branch result y (fp32) in every mode.
static int swin_block_v2(reid_ctx* ctx, const SwinBlockW& k, const SwinBlockW16& h, const float* xin, float* xcur, long long T, int n,
                         int Hs, int Ws, int C, int heads, int shifted, bool first, float* lnb, float* big, float* att, float* tmp) {
    if (ctx->precision == 1) {
        f16* x16 = (f16*)att;       // [T][C]: the stream as f16, then the attention output, then the stream again
        f16* big16 = (f16*)big;     // qkv [T][ldq] / MLP hidden [T][4C]
        f16* tmp16 = (f16*)tmp;     // [T][C]
        const int ldq = (3 * C + 63) / 64 * 64;
        if (first) REID_TRY(launch_f32_to_f16(ctx, xin, (size_t)T * C, x16));
        REID_TRY(linear16(ctx, x16, T, C, C, h.qkv, nullptr, 3 * C, 0, nullptr, big16, nullptr, ldq));
        REID_TRY(launch_window_attn_cos(ctx, 1, big16, ldq, n, Hs, Ws, heads, shifted, k.bias_t, k.scale, x16));
        if (ctx->swin_fold) {
            REID_TRY(linear16(ctx, x16, T, C, C, h.fold, h.fold_b, C, 0, nullptr, nullptr, lnb, C));
        } else {
            REID_TRY(linear16(ctx, x16, T, C, C, h.out, k.out_b, C, 0, nullptr, tmp16, nullptr, C));
            REID_TRY(linear16(ctx, tmp16, T, C, C, h.post, k.post_b, C, 0, nullptr, nullptr, lnb, C));
        }
        REID_TRY(launch_post_norm(ctx, 1, xin, lnb, T, C, k.ln1_g, k.ln1_b, xcur, x16));
        REID_TRY(linear16(ctx, x16, T, C, C, h.fc1, k.fc1_b, 4 * C, 1, nullptr, big16, nullptr, 4 * C));
        REID_TRY(linear16(ctx, big16, T, 4 * C, 4 * C, h.fc2, k.fc2_b, C, 0, nullptr, nullptr, lnb, C));
        return launch_post_norm(ctx, 1, xcur, lnb, T, C, k.ln2_g, k.ln2_b, xcur, x16);
    }
    if (ctx->precision == 2) {      // (every pass size: an image's arithmetic must not depend on the batch it comes in)
        f16* x16 = (f16*)att;       // [T][2C]: the stream as [xh | xl'], then the attention output, then the stream again
        f16* big16 = (f16*)big;     // MLP hidden [T][8C] (same bytes as the fp32 [T][4C])
        f16* tmp16 = (f16*)tmp;     // [T][2C]
        if (first) REID_TRY(launch_split_pack(ctx, xin, T, C, x16));
        REID_TRY(linear(ctx, nullptr, T, C, k.qkv_w, nullptr, 3 * C, 0, nullptr, big, x16));
        REID_TRY(launch_window_attn_cos(ctx, 2, big, 3 * C, n, Hs, Ws, heads, shifted, k.bias_t, k.scale, x16));
        REID_TRY(linear(ctx, nullptr, T, C, k.out_w, k.out_b, C, 0, nullptr, nullptr, x16, tmp16));
        REID_TRY(linear(ctx, nullptr, T, C, k.post_w, k.post_b, C, 0, nullptr, lnb, tmp16));
        REID_TRY(launch_post_norm(ctx, 2, xin, lnb, T, C, k.ln1_g, k.ln1_b, xcur, x16));
        REID_TRY(linear(ctx, nullptr, T, C, k.fc1_w, k.fc1_b, 4 * C, 1, nullptr, nullptr, x16, big16));
        REID_TRY(linear(ctx, nullptr, T, 4 * C, k.fc2_w, k.fc2_b, C, 0, nullptr, lnb, big16));
        return launch_post_norm(ctx, 2, xcur, lnb, T, C, k.ln2_g, k.ln2_b, xcur, x16);
    }
    REID_TRY(linear(ctx, xin, T, C, k.qkv_w, nullptr, 3 * C, 0, nullptr, big));
    REID_TRY(launch_window_attn_cos(ctx, 0, big, 3 * C, n, Hs, Ws, heads, shifted, k.bias_t, k.scale, att));
    REID_TRY(linear(ctx, att, T, C, k.out_w, k.out_b, C, 0, nullptr, tmp));
    REID_TRY(linear(ctx, tmp, T, C, k.post_w, k.post_b, C, 0, nullptr, lnb));
    REID_TRY(launch_post_norm(ctx, 0, xin, lnb, T, C, k.ln1_g, k.ln1_b, xcur, nullptr));
    REID_TRY(linear(ctx, xcur, T, C, k.fc1_w, k.fc1_b, 4 * C, 1, nullptr, big));
    REID_TRY(linear(ctx, big, T, 4 * C, k.fc2_w, k.fc2_b, C, 0, nullptr, lnb));
    return launch_post_norm(ctx, 0, xcur, lnb, T, C, k.ln2_g, k.ln2_b, xcur, nullptr);
}

// ------------------------------------------------------------------------------------------------ forward
// The two stems.  Both write ShadowFeatureExtraction's first convolution, c1 [n][h / 2][w / 2][12]; swin_body goes on from there.
// From NCHW: sfe_conv1_kernel on normalised fp32 images [n][3][h][w] on the device.  This launcher, with a profiling bracket of its own,
// serves the harness (reid_debug_swin_conv1); the forward launches the kernel inside the stem's one bracket, as it always has (swin_body).
int launch_sfe_conv1(reid_ctx* ctx, const float* x, int n, int h, int wd, const float* c1_w, const float* c1_b, float* c1) {
    if (!x || !c1_w || !c1_b || !c1 || n < 1 || h < 2 || wd < 2 || (h & 1) || (wd & 1)) {
        reid_set_error("launch_sfe_conv1: bad arguments (%d images of %d x %d)", n, h, wd);
        return REID_ERR_ARG;
    }
    prof_begin(ctx, REID_K_ELEMENTWISE, 0, (double)n * h * wd * (12 + 12));
    hipLaunchKernelGGL(sfe_conv1_kernel, dim3(grid_for((long long)n * (h / 2) * (wd / 2), 256)), dim3(256), 0, ctx->stream, x, n, h,
                       wd, c1_w, c1_b, c1);
    prof_end(ctx);
    LAUNCH_CHECK();
    return REID_OK;
}

// out_h x out_w multiples of 224, mean finite, std finite and positive: the one check of the crops entry points and of the harness
int swin_crops_check(int out_h, int out_w, const float* mean_std6) {
    if (!mean_std6 || out_h <= 0 || out_w <= 0 || out_h % 224 || out_w % 224) {
        reid_set_error("Swin crops: the output size must be multiples of 224 and mean / std given, got %d x %d", out_h, out_w);
        return REID_ERR_ARG;
    }
    for (int c = 0; c < 3; ++c)
        if (!(mean_std6[3 + c] > 0.f) || !std::isfinite(mean_std6[3 + c]) || !std::isfinite(mean_std6[c])) {
            reid_set_error("Swin crops: mean must be finite and std positive (channel %d: mean %g, std %g)", c, mean_std6[c], mean_std6[3 + c]);
            return REID_ERR_ARG;
        }
    return REID_OK;
}

// From uint8 windows: swin_crop_front_kernel (libreid_hip_swin_crops.so) - resize, normalise and the same convolution in one launch.
// d_src / d_off / d_hw on the device (window i: d_hw[2i] x d_hw[2i + 1] pixels at byte d_off[i], rows `pitch` pixels apart, 0 = its own
// width); mean_std6 on the HOST.  The callers have checked that every window lies inside d_src.
int launch_swin_crop_front(reid_ctx* ctx, const uint8_t* d_src, const long long* d_off, const int* d_hw, int n, int h, int wd, int pitch,
                           const float* mean_std6, const float* c1_w, const float* c1_b, float* c1) {
    if (!d_src || !d_off || !d_hw || !mean_std6 || !c1_w || !c1_b || !c1 || n < 1 || h < 224 || wd < 224 || h % 224 || wd % 224 || pitch < 0) {
        reid_set_error("launch_swin_crop_front: bad arguments (%d windows to %d x %d, pitch %d)", n, h, wd, pitch);
        return REID_ERR_ARG;
    }
    REID_TRY(swin_crops.open());
    prof_begin(ctx, REID_K_ELEMENTWISE, 0, (double)n * h * wd * 12);
    const hipError_t e = swin_crops.front(ctx->stream, d_src, d_off, d_hw, n, h, wd, pitch, mean_std6, c1_w, c1_b, c1);
    prof_end(ctx);
    HIP_TRY(e);
    return REID_OK;
}

// The stems of the MIRRORED view and the descriptor (libreid_hip_swin_eval.so, swin_eval.h), through the launchers the descriptor entries
// and the harnesses (reid_debug_swin_conv1_mirror / _crop_front_mirror / _descriptor) share.  Same arguments and checks as the launchers
// of the plain stems above; c1 then goes to swin_body with x == nullptr.
int launch_sfe_conv1_mirror(reid_ctx* ctx, const float* x, int n, int h, int wd, const float* c1_w, const float* c1_b, float* c1) {
    if (!x || !c1_w || !c1_b || !c1 || n < 1 || h < 2 || wd < 2 || (h & 1) || (wd & 1)) {
        reid_set_error("launch_sfe_conv1_mirror: bad arguments (%d images of %d x %d)", n, h, wd);
        return REID_ERR_ARG;
    }
    REID_TRY(swin_eval.open());
    prof_begin(ctx, REID_K_ELEMENTWISE, 0, (double)n * h * wd * (12 + 12));
    const hipError_t e = swin_eval.conv1_mirror(ctx->stream, x, n, h, wd, c1_w, c1_b, c1);
    prof_end(ctx);
    HIP_TRY(e);
    return REID_OK;
}

int launch_swin_crop_front_mirror(reid_ctx* ctx, const uint8_t* d_src, const long long* d_off, const int* d_hw, int n, int h, int wd, int pitch,
                                  const float* mean_std6, const float* c1_w, const float* c1_b, float* c1) {
    if (!d_src || !d_off || !d_hw || !mean_std6 || !c1_w || !c1_b || !c1 || n < 1 || h < 224 || wd < 224 || h % 224 || wd % 224 || pitch < 0) {
        reid_set_error("launch_swin_crop_front_mirror: bad arguments (%d windows to %d x %d, pitch %d)", n, h, wd, pitch);
        return REID_ERR_ARG;
    }
    REID_TRY(swin_eval.open());
    prof_begin(ctx, REID_K_ELEMENTWISE, 0, (double)n * h * wd * 12);
    const hipError_t e = swin_eval.crop_front_mirror(ctx->stream, d_src, d_off, d_hw, n, h, wd, pitch, mean_std6, c1_w, c1_b, c1);
    prof_end(ctx);
    HIP_TRY(e);
    return REID_OK;
}

// e1 / e2 (or nullptr) [n][96], cls_w [num_class][96] -> out rows of num_class + 96 floats, ld floats apart; all on the device
int launch_swin_descriptor(reid_ctx* ctx, const float* e1, const float* e2, const float* cls_w, int n, int num_class, long long ld, float* out) {
    REID_TRY(swin_eval.open());
    if (!e1 || !cls_w || !out || n < 1 || num_class < 1 || ld < (long long)num_class + 96 || (((uintptr_t)e1 | (uintptr_t)e2 | (uintptr_t)cls_w) & 15)) {
        reid_set_error("launch_swin_descriptor: bad arguments (%d rows, %d classes, row pitch %lld; operands 16-byte aligned)", n, num_class, ld);
        return REID_ERR_ARG;
    }
    if (num_class > swin_eval.max_classes()) {
        reid_set_error("Swin descriptor: %d classes, the descriptor kernel holds at most %d (both views' logits stay in LDS)", num_class,
                       swin_eval.max_classes());
        return REID_ERR_ARG;
    }
    prof_begin(ctx, REID_K_ELEMENTWISE, 2.0 * n * num_class * 96 * (e2 ? 2 : 1), (double)n * ((double)num_class * 96 + num_class + 96 * 3) * 4);
    const hipError_t e = swin_eval.descriptor(ctx->stream, e1, e2, cls_w, n, num_class, ld, out);
    prof_end(ctx);
    HIP_TRY(e);
    return REID_OK;
}

static int swin_body(reid_ctx* ctx, const SwinWeights& w, const float* x, float* c1, int n, int h, int wd, float* d_emb, float* d_logits);

static int swin_c1(reid_ctx* ctx, int n, int h, int wd, float** c1) {
    return ctx_ws(ctx, "swin.c1", (size_t)n * (h / 2) * (wd / 2) * 12 * 4, (void**)c1);
}

// x: fp32 NCHW [n][3][h][w] on the device; h, w multiples of 224
static int swin_forward(reid_ctx* ctx, const SwinWeights& w, const float* x, int n, int h, int wd, float* d_emb, float* d_logits) {
    float* c1;
    REID_TRY(swin_c1(ctx, n, h, wd, &c1));
    return swin_body(ctx, w, x, c1, n, h, wd, d_emb, d_logits);
}

// n uint8 windows on the device -> embeddings: the fused stem, then the common body
static int swin_forward_crops(reid_ctx* ctx, const SwinWeights& w, const uint8_t* d_src, const long long* d_off, const int* d_hw, int n,
                              int h, int wd, int pitch, const float* mean_std6, float* d_emb, float* d_logits) {
    float* c1;
    REID_TRY(swin_c1(ctx, n, h, wd, &c1));
    REID_TRY(launch_swin_crop_front(ctx, d_src, d_off, d_hw, n, h, wd, pitch, mean_std6, w.c1_w, w.c1_b, c1));
    return swin_body(ctx, w, nullptr, c1, n, h, wd, d_emb, d_logits);
}

// PatchMerging in front of stage s + 1 (s = 1 .. 3) = conv2x2 s2 with weights repacked to (kh, kw, c) order + bias
// (swin_transformer.py:263-275): prev [n][Hs][Ws][kDims[s - 1]] -> xcur [n][Hs / 2][Ws / 2][kDims[s]], both fp32 (the residual stream);
// scratch: room for an f16 copy of prev (precision 1)
static int swin_merge(reid_ctx* ctx, const SwinWeights& w, int s, const float* prev, int n, int Hs, int Ws, float* scratch, float* xcur) {
    const int C = kDims[s];
    if (ctx->precision == 1) {
        f16* x16 = (f16*)scratch;   // f16 copy of the previous stage's output (the residual stream itself stays fp32)
        REID_TRY(launch_f32_to_f16(ctx, prev, (size_t)n * Hs * Ws * kDims[s - 1], x16));
        return conv16(ctx, w.zero_page, x16, n, Hs, Ws, kDims[s - 1], w.merge16[s], w.merge_b[s], C, 2, 2, 2, 0, 0, Hs / 2, Ws / 2, nullptr, nullptr,
                      xcur);
    }
    return conv_bias(ctx, prev, n, Hs, Ws, kDims[s - 1], w.merge_w[s], w.merge_b[s], C, 2, 2, 2, 0, 0, Hs / 2, Ws / 2, nullptr, xcur, 0, 0, 0, 0,
                     w.zero_page);
}

// top-down fusion (:405-412): a0 = stage4 + Conv8x8s8(sfe); then three ConvTranspose2d(4, 2, 1) + stage outputs -> f3, f2, f1.
// sfe [n][H1][W1][96] and the stage outputs xs[0 .. 3] fp32; a0 [n][H1/8][W1/8][768], f3 [..][384], f2 [..][192] fp32 - precision 1: f16 maps
// in the same buffers, every step adding its fp32 stage output in the epilogue - and f1 [n][H1][W1][96] fp32 in every mode.
// scratch16: room for an f16 copy of sfe (precision 1)
static int swin_fuse(reid_ctx* ctx, const SwinWeights& w, const float* sfe, float* const* xs, int n, int H1, int W1, float* scratch16, float* a0,
                     float* f3, float* f2, float* f1) {
    const int H4 = H1 / 8, W4 = W1 / 8;
    if (ctx->precision == 1) {
        f16* sfe16 = (f16*)scratch16;
        f16* maps16[3] = {(f16*)a0, (f16*)f3, (f16*)f2};   // [n,7,7,768] -> [n,14,14,384] -> [n,28,28,192]
        REID_TRY(launch_f32_to_f16(ctx, sfe, (size_t)n * H1 * W1 * 96, sfe16));
        REID_TRY(conv16(ctx, w.zero_page, sfe16, n, H1, W1, 96, w.img16, w.img_b, 768, 8, 8, 8, 0, 0, H4, W4, xs[3], maps16[0], nullptr));
        int Hi = H4, Wi = W4;
        for (int t = 0; t < 3; ++t) {
            const int ci = kDims[3 - t], co = kDims[2 - t];
            const size_t wstride = (size_t)((co + 63) / 64 * 64) * 4 * ci;
            // the four output parities of the ConvTranspose2d(4, 2, 1) as ONE launch (4 x the tile grid): a parity alone is 147-784
            // blocks, too few for 256 CUs
            REID_TRY(conv16(ctx, w.zero_page, maps16[t], n, Hi, Wi, ci, w.t16[t], w.t_b[t], co, 2, 2, 1, 1, 1, Hi, Wi, xs[2 - t],
                            t < 2 ? maps16[t + 1] : nullptr, t < 2 ? nullptr : f1, Hi, Wi, 0, 0, (long long)wstride));
            Hi *= 2;
            Wi *= 2;
        }
        return REID_OK;
    }
    REID_TRY(conv_bias(ctx, sfe, n, H1, W1, 96, w.img_w, w.img_b, 768, 8, 8, 8, 0, 0, H4, W4, xs[3], a0, 0, 0, 0, 0, w.zero_page));
    const float* fin = a0;
    float* fouts[3] = {f3, f2, f1};
    int Hi = H4, Wi = W4;
    for (int t = 0; t < 3; ++t) {
        const int ci = kDims[3 - t], co = kDims[2 - t];
        REID_TRY(conv_transpose_parities(ctx, fin, n, Hi, Wi, ci, w.t_w[t], w.t_b[t], co, xs[2 - t], fouts[t], w.zero_page));
        fin = fouts[t];
        Hi *= 2;
        Wi *= 2;
    }
    return REID_OK;
}

// The two steps above on the weights this context has loaded (reid_swin_load) and in its precision, on device operands: what
// reid_debug_swin_merge / reid_debug_swin_fuse (libreid_hip_debug.so) run.  stage 2 .. 4: x [n][h][w][kDims[stage - 2]] -> out
// [n][h / 2][w / 2][kDims[stage - 1]]; v1 and v2 checkpoints alike.
int swin_loaded_merge(reid_ctx* ctx, int stage, const float* x, int n, int h, int w, float* scratch, float* out) {
    const SwinWeights* sw = swin_find(ctx);
    if (!sw || !sw->loaded || stage < 2 || stage > 4 || !x || !scratch || !out || n < 1 || h < 2 || w < 2 || (h & 1) || (w & 1)) {
        reid_set_error("swin_loaded_merge: needs loaded Swin weights, stage 2 .. 4 and an even map (stage %d, %d x %d)", stage, h, w);
        return sw && sw->loaded ? REID_ERR_ARG : REID_ERR_STATE;
    }
    return swin_merge(ctx, *sw, stage - 1, x, n, h, w, scratch, out);
}
int swin_loaded_fuse(reid_ctx* ctx, const float* sfe, float* const* xs, int n, int h1, int w1, float* scratch16, float* a0, float* f3, float* f2,
                     float* f1) {
    const SwinWeights* sw = swin_find(ctx);
    if (!sw || !sw->loaded || !sfe || !xs || !scratch16 || !a0 || !f3 || !f2 || !f1 || n < 1 || h1 < 8 || w1 < 8 || h1 % 8 || w1 % 8) {
        reid_set_error("swin_loaded_fuse: needs loaded Swin weights and a stage-1 map whose sides are multiples of 8 (%d x %d)", h1, w1);
        return sw && sw->loaded ? REID_ERR_ARG : REID_ERR_STATE;
    }
    return swin_fuse(ctx, *sw, sfe, xs, n, h1, w1, scratch16, a0, f3, f2, f1);
}
// linear() / linear16() above on device operands prepared as the forward prepares them: what reid_debug_swin_linear
// (libreid_hip_debug.so) runs.  f16_storage != 0: linear16 - x16 f16 [m][k], w f16 [n padded to 64][k], out16 (row stride ldc) or out32.
// Else linear() in the context's precision: x32 fp32 [m][k] or, with x16, the packed [xh | xl'] f16 [m][2k]; w fp32 [n][k]; out32 [m][n]
// or, with out16, the packed [yh | yl'] f16 [m][2n] (ldc is then n).
int swin_linear_for_test(reid_ctx* ctx, int f16_storage, const float* x32, const _Float16* x16, long long m, int k, const void* w,
                         const float* bias, int n, int act, const float* res, float* out32, _Float16* out16, int ldc) {
    if (f16_storage) return linear16(ctx, x16, m, k, k, (const f16*)w, bias, n, act, res, out16, out32, ldc);
    if (ldc != n) {
        reid_set_error("swin_linear_for_test: linear() writes rows of n = %d values (ldc %d)", n, ldc);
        return REID_ERR_ARG;
    }
    return linear(ctx, x32, m, k, (const float*)w, bias, n, act, res, out32, x16, out16);
}

// The common body: from c1 [n][h / 2][w / 2][12] to the embeddings.  x != nullptr (the float entries): c1 is still to be written, by the
// stem from NCHW - sfe_conv1_kernel's launch, first in the stem's one profiling bracket, where it has always been.  x == nullptr (the
// crops entries): the fused stem has filled c1 on this stream.  The side index (reid_ctx_set_side_index) is taken here, so it serves every
// entry point.
static int swin_body(reid_ctx* ctx, const SwinWeights& w, const float* x, float* c1, int n, int h, int wd, float* d_emb, float* d_logits) {
    const int H1 = h / 4, W1 = wd / 4;
    const long long T1 = (long long)n * H1 * W1;   // tokens of stage 1
    float *ab, *sfe, *xs[4], *lnb, *big, *att, *tmp, *f3, *f2, *f1, *gem;
    REID_TRY(ctx_ws(ctx, "swin.ab", (size_t)n * 24 * 4, (void**)&ab));
    REID_TRY(ctx_ws(ctx, "swin.sfe", (size_t)T1 * 96 * 4, (void**)&sfe));
    for (int s = 0; s < 4; ++s) {
        char nm[32];
        snprintf(nm, sizeof(nm), "swin.x%d", s);
        REID_TRY(ctx_ws(ctx, nm, (size_t)T1 * 96 * 4 >> s, (void**)&xs[s]));   // tokens/4, channels*2 per stage
    }
    REID_TRY(ctx_ws(ctx, "swin.ln", (size_t)T1 * 96 * 4, (void**)&lnb));
    REID_TRY(ctx_ws(ctx, "swin.big", (size_t)T1 * 384 * 4, (void**)&big));    // qkv (3C) and MLP hidden (4C)
    REID_TRY(ctx_ws(ctx, "swin.att", (size_t)T1 * 96 * 4, (void**)&att));
    REID_TRY(ctx_ws(ctx, "swin.tmp", (size_t)T1 * 96 * 4, (void**)&tmp));
    REID_TRY(ctx_ws(ctx, "swin.f3", (size_t)T1 * 96 * 4 >> 2, (void**)&f3));   // [n,14,14,384]
    REID_TRY(ctx_ws(ctx, "swin.f2", (size_t)T1 * 96 * 4 >> 1, (void**)&f2));   // [n,28,28,192]
    REID_TRY(ctx_ws(ctx, "swin.f1", (size_t)T1 * 96 * 4, (void**)&f1));        // [n,56,56,96]
    REID_TRY(ctx_ws(ctx, "swin.gem", (size_t)n * 96 * 4, (void**)&gem));

    // stem
    prof_begin(ctx, REID_K_ELEMENTWISE, 0, 0);
    if (x)
        hipLaunchKernelGGL(sfe_conv1_kernel, dim3(grid_for((long long)n * (h / 2) * (wd / 2), 256)), dim3(256), 0, ctx->stream, x, n, h,
                           wd, w.c1_w, w.c1_b, c1);
    const int stem_rc = launch_sfe_norm_fc(ctx, c1, n, h / 2, wd / 2, w.in_g, w.in_b, w.bn_s, w.bn_t, w.c2_w, w.c2_b, w.fc_w, w.fc_b, ab, sfe);
    prof_end(ctx);
    REID_TRY(stem_rc);
    {   // SwinTransformer.forward(img, view_index): + side_info_coeff * side_info_embedding[view] on the SFE output (:301-302)
        const int32_t* d_view;
        REID_TRY(ctx_take_side(ctx, n, w.views, "reid_swin_embed (view index)", &d_view));
        if (d_view) REID_TRY(launch_add_indexed_rows(ctx, sfe, n, (long long)H1 * W1, 96, w.side, d_view, w.side_coeff));
    }

    int bi = 0, Hs = H1, Ws = W1;
    const float* prev = sfe;
    for (int s = 0; s < 4; ++s) {
        const int C = kDims[s], heads = kHeads[s];
        float* xcur = xs[s];
        if (ctx->swin_stop >= 0 && bi * 10 > ctx->swin_stop) {   // diagnostics: leave the scratch buffers as they are
            ctx->swin_last_n = n;
            ctx->swin_last_tok = H1 * W1;
            return REID_OK;
        }
        if (s > 0) {
            REID_TRY(swin_merge(ctx, w, s, prev, n, Hs, Ws, lnb, xcur));
            Hs /= 2;
            Ws /= 2;
        }
        const long long T = (long long)n * Hs * Ws;
        for (int j = 0; j < kLayers[s]; ++j, ++bi) {
            const SwinBlockW& k = w.blk[bi];
            const int shifted = j & 1;
            const int stop = ctx->swin_stop;   // diagnostics: the stage tap then shows the stream right after that point
            if (stop >= 0 && bi * 10 > stop) continue;
            // the first block reads the ShadowFeatureExtraction output (kept for the top-down fusion) and writes stage 1's
            // residual stream; every later block updates that stream in place
            const float* xin = (s == 0 && j == 0) ? sfe : xcur;
            if (w.version == 2) {   // post-norm blocks with cosine attention; REID_SWIN_STOP's phases inside a block are v1's only
                REID_TRY(swin_block_v2(ctx, k, w.blk16[bi], xin, xcur, T, n, Hs, Ws, C, heads, shifted, j == 0, lnb, big, att, tmp));
                continue;
            }
            if (ctx->precision == 1) {
                // fp16-storage mode: the five linears of the block (95 % of its MACs) on the f16 MFMA GEMM with fp32
                // accumulation; LayerNorm, softmax, GELU and the residual stream x stay fp32
                const SwinBlockW16& h = w.blk16[bi];
                f16* ln16 = (f16*)lnb;                 // [T][C]
                f16* big16 = (f16*)big;                // qkv [T][ldq] / MLP hidden [T][4C]
                f16* att16 = (f16*)att;                // [T][C]
                f16* tmp16 = (f16*)tmp;                // [T][C]
                const int ldq = swin_attn_ldq(ctx, C);
                prof_begin(ctx, REID_K_ELEMENTWISE, 0, (double)T * C * 6);
                launch_layernorm<f16>(ctx, xin, T, C, k.ln1_g, k.ln1_b, ln16);
                prof_end(ctx);
                REID_TRY(linear16(ctx, ln16, T, C, C, h.qkv, nullptr, 3 * C, 0, nullptr, big16, nullptr, ldq));
                REID_TRY(launch_window_attn(ctx, big16, n, Hs, Ws, heads, shifted, k.pos, h.bias_tab, att16));
                if (ctx->swin_fold) {   // to_out . post_proj as one Linear (folded at load time)
                    REID_TRY(linear16(ctx, att16, T, C, C, h.fold, h.fold_b, C, 0, xin, nullptr, xcur, C));
                } else {
                    REID_TRY(linear16(ctx, att16, T, C, C, h.out, k.out_b, C, 0, nullptr, tmp16, nullptr, C));
                    REID_TRY(linear16(ctx, tmp16, T, C, C, h.post, k.post_b, C, 0, xin, nullptr, xcur, C));
                }
                if (stop == bi * 10) continue;
                prof_begin(ctx, REID_K_ELEMENTWISE, 0, (double)T * C * 6);
                launch_layernorm<f16>(ctx, xcur, T, C, k.ln2_g, k.ln2_b, ln16);
                prof_end(ctx);
                if (stop == bi * 10 + 2) continue;
                REID_TRY(linear16(ctx, ln16, T, C, C, h.fc1, k.fc1_b, 4 * C, 1, nullptr, big16, nullptr, 4 * C));
                if (stop == bi * 10 + 3) continue;
                REID_TRY(linear16(ctx, big16, T, 4 * C, 4 * C, h.fc2, k.fc2_b, C, 0, xcur, nullptr, xcur, C));
                continue;
            }
            if (ctx->precision == 2) {   // (every pass size: an image's arithmetic must not depend on the batch it comes in)
                // fp32-class mode: the five linears in three-product f16 arithmetic (linear()); LayerNorm, the attention kernel, to_out
                // and fc1 write their results as [yh | yl'] f16 directly, so no linear input goes through a pack pass (the
                // reference's two roundings to_out -> post_proj are kept: no folded matrix in fp32)
                f16* ln16 = (f16*)lnb;      // [T][2C]
                f16* att16 = (f16*)att;     // [T][2C]
                f16* big16 = (f16*)big;     // MLP hidden [T][8C] (same bytes as the fp32 [T][4C])
                if (ln_linear_supported(ctx, T, C, 3 * C)) {   // LayerNorm 1 + to_qkv: the normalised tokens never leave the registers
                    REID_TRY(launch_ln_linear(ctx, xin, k.ln1_g, k.ln1_b, T, C, 3 * C, k.qkv_w, nullptr, big, 3 * C));
                } else {
                    prof_begin(ctx, REID_K_ELEMENTWISE, 0, (double)T * C * 8);
                    launch_layernorm_packed(ctx, xin, T, C, k.ln1_g, k.ln1_b, ln16);
                    prof_end(ctx);
                    REID_TRY(linear(ctx, nullptr, T, C, k.qkv_w, nullptr, 3 * C, 0, nullptr, big, ln16));
                }
                REID_TRY(launch_window_attn(ctx, big, n, Hs, Ws, heads, shifted, k.pos, w.blk16[bi].bias_tab, att16));
                // each pair of linears as ONE launch where the hidden values fit the register file (two_linear_f16.hip): same
                // roundings (the hidden layer is split into [hh | hl'] as the first launch's epilogue did), no [T][C] / [T][4C] trip
                if (two_linear_supported(ctx, T, C, C)) {
                    REID_TRY(launch_two_linear(ctx, att16, T, C, C, k.out_w, k.out_b, k.post_w, k.post_b, 0, xin, xcur));
                } else {
                    REID_TRY(linear(ctx, nullptr, T, C, k.out_w, k.out_b, C, 0, nullptr, nullptr, att16, (f16*)tmp));   // [T][2C] = tmp's bytes
                    REID_TRY(linear(ctx, nullptr, T, C, k.post_w, k.post_b, C, 0, xin, xcur, (const f16*)tmp));
                }
                if (two_linear_supported(ctx, T, C, 4 * C)) {   // LayerNorm 2 in the kernel's prologue: x is read where it is updated
                    REID_TRY(launch_two_linear(ctx, nullptr, T, C, 4 * C, k.fc1_w, k.fc1_b, k.fc2_w, k.fc2_b, 1, xcur, xcur, xcur, k.ln2_g, k.ln2_b));
                } else {
                    prof_begin(ctx, REID_K_ELEMENTWISE, 0, (double)T * C * 8);
                    launch_layernorm_packed(ctx, xcur, T, C, k.ln2_g, k.ln2_b, ln16);
                    prof_end(ctx);
                    REID_TRY(linear(ctx, nullptr, T, C, k.fc1_w, k.fc1_b, 4 * C, 1, nullptr, nullptr, ln16, big16));
                    REID_TRY(linear(ctx, nullptr, T, 4 * C, k.fc2_w, k.fc2_b, C, 0, xcur, xcur, big16));
                }
                continue;
            }
            // x = x + post_proj(to_out(attn(LN(x))))
            prof_begin(ctx, REID_K_ELEMENTWISE, 0, (double)T * C * 8);
            launch_layernorm<float>(ctx, xin, T, C, k.ln1_g, k.ln1_b, lnb);
            prof_end(ctx);
            REID_TRY(linear(ctx, lnb, T, C, k.qkv_w, nullptr, 3 * C, 0, nullptr, big));
            REID_TRY(launch_window_attn(ctx, big, n, Hs, Ws, heads, shifted, k.pos, w.blk16[bi].bias_tab, att));
            REID_TRY(linear(ctx, att, T, C, k.out_w, k.out_b, C, 0, nullptr, tmp));
            REID_TRY(linear(ctx, tmp, T, C, k.post_w, k.post_b, C, 0, xin, xcur));
            // x = x + fc2(gelu(fc1(LN(x))))
            prof_begin(ctx, REID_K_ELEMENTWISE, 0, (double)T * C * 8);
            launch_layernorm<float>(ctx, xcur, T, C, k.ln2_g, k.ln2_b, lnb);
            prof_end(ctx);
            REID_TRY(linear(ctx, lnb, T, C, k.fc1_w, k.fc1_b, 4 * C, 1, nullptr, big));
            REID_TRY(linear(ctx, big, T, 4 * C, k.fc2_w, k.fc2_b, C, 0, xcur, xcur));
        }
        prev = xcur;
    }
    // top-down fusion (:405-412): f = stage4 + Conv8x8s8(sfe); then three ConvTranspose2d(4, 2, 1) + stage outputs
    REID_TRY(swin_fuse(ctx, w, sfe, xs, n, H1, W1, att, tmp, f3, f2, f1));
    prof_begin(ctx, REID_K_ELEMENTWISE, 0, (double)T1 * 96 * 4);
    const int tail_rc = launch_swin_tail(ctx, f1, n, H1 * W1, w.tail_g, w.tail_b, w.tail_p, w.neck_s, w.neck_t, gem, d_emb);
    prof_end(ctx);
    REID_TRY(tail_rc);
    if (d_logits) {
        if (!w.cls_w) {
            reid_set_error("logits requested but the Swin blob has no classifier");
            return REID_ERR_STATE;
        }
        REID_TRY(linear(ctx, d_emb, n, 96, w.cls_w, nullptr, w.num_class, 0, nullptr, d_logits));
    }
    ctx->swin_last_n = n;
    ctx->swin_last_tok = H1 * W1;
    return REID_OK;
}

// Intermediate activations of the last reid_swin_embed_* call (stage-level parity tests): 0 = ShadowFeatureExtraction output
// [n][56][56][96], 1..4 = outputs of the four stages (NHWC fp32 residual streams), 5 = GeM_1D output [n][96].  Valid when the
// call ran as ONE pass (n <= min(chunk, 1024)); the buffers are the forward's own workspaces.
extern "C" int reid_debug_swin_stage(reid_ctx* ctx, int stage, float* out, size_t max_floats, size_t* count) {
    ARG_CHECK(ctx && out && stage >= 0 && stage <= 7);
    CTX_GUARD(ctx);
    static const char* names[8] = {"swin.sfe", "swin.x0", "swin.x1", "swin.x2", "swin.x3", "swin.gem", "swin.ln", "swin.big"};
    auto it = ctx->ws.find(names[stage]);
    if (it == ctx->ws.end() || ctx->swin_last_n <= 0) {
        reid_set_error("reid_debug_swin_stage: no Swin forward has run on this context");
        return REID_ERR_STATE;
    }
    // 6 / 7: the raw LayerNorm-output and qkv / MLP-hidden scratch buffers (diagnostics with REID_SWIN_STOP)
    const size_t per = stage == 5 ? 96 : stage == 6 ? (size_t)ctx->swin_last_tok * 96 : stage == 7 ? (size_t)ctx->swin_last_tok * 384
                                   : ((size_t)ctx->swin_last_tok * 96) >> (stage <= 1 ? 0 : stage - 1);
    const size_t total = per * ctx->swin_last_n;
    if (count) *count = total;
    const size_t ncopy = total < max_floats ? total : max_floats;
    HIP_TRY(hipMemcpyAsync(out, it->second.first, ncopy * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return REID_OK;
}

// images per pass: ~13 MB of fp32 activations per 224x224 image, 13 GB at the cap.  Passes of 1024 instead of 256 images run
// 8 % faster in the fp32-class mode (14.6 -> 15.7 k img/s): the stage 3-4 linears of a 256-image pass are 294-588 tiles for 512
// block slots.  Results are bit-identical for every pass size (tools/swin_chunk_check.py).  REID_SWIN_CHUNK_MAX lowers the cap.
static int swin_pass(const reid_ctx* ctx) { return ctx->chunk < ctx->swin_chunk_cap ? ctx->chunk : ctx->swin_chunk_cap; }

static int swin_loaded(reid_ctx* ctx, const SwinWeights** sw) {
    *sw = swin_find(ctx);
    if (!*sw || !(*sw)->loaded) {
        reid_set_error("reid_swin_embed_*: call reid_swin_load first");
        return REID_ERR_STATE;
    }
    return REID_OK;
}

extern "C" int reid_swin_embed_f32_nchw_dev(reid_ctx* ctx, const float* d_x, int n, int h, int w, float* d_emb, float* d_logits) {
    ARG_CHECK(ctx && d_x && d_emb && n >= 0 && h > 0 && w > 0 && h % 224 == 0 && w % 224 == 0);
    CTX_ENTER(ctx);
    const SwinWeights* sw;
    REID_TRY(swin_loaded(ctx, &sw));
    const size_t img = (size_t)3 * h * w;
    return embed_dev_passes(n, swin_pass(ctx), [&](int i, int m) -> int {
        return swin_forward(ctx, *sw, d_x + (size_t)i * img, m, h, w, d_emb + (size_t)i * 96, d_logits ? d_logits + (size_t)i * sw->num_class : nullptr);
    });
}

extern "C" int reid_swin_embed_f32_nchw(reid_ctx* ctx, const float* x, int n, int h, int w, float* emb, float* logits) {
    ARG_CHECK(ctx && x && emb && n >= 0 && h > 0 && w > 0 && h % 224 == 0 && w % 224 == 0);
    CTX_ENTER(ctx);
    if (n == 0) return REID_OK;
    const SwinWeights* sw;
    REID_TRY(swin_loaded(ctx, &sw));
    const size_t img = (size_t)3 * h * w;
    float* d_in;
    EmbedOut out{emb, logits, 96, sw->num_class};
    REID_TRY(ctx_ws(ctx, "io.in", (size_t)n * img * 4, (void**)&d_in));
    REID_TRY(out.alloc(ctx, "io", n, 0, logits != nullptr));
    return embed_host(
        ctx, n, swin_pass(ctx),
        [&](int i, int m, hipStream_t s) -> int {
            HIP_TRY(hipMemcpyAsync(d_in + (size_t)i * img, x + (size_t)i * img, (size_t)m * img * 4, hipMemcpyHostToDevice, s));
            return REID_OK;
        },
        [&](int i, int m, float* d_emb, float* d_log) -> int { return swin_forward(ctx, *sw, d_in + (size_t)i * img, m, h, w, d_emb, d_log); }, out);
}

// ---- uint8 crops in, embeddings out: the tracker's way of feeding a ReID model (Extractor.__call__, feature_extractor.py:48-53, and
// DeepSort._get_features) for the reference's swin_transformer tracker model (modification_tracking/models/__init__.py:80), with its
// transform for transformer models (reid/data_transforms.py:64: resize to out_h x out_w, ImageNet mean / std)
static const float kImagenetMeanStd[6] = {0.485f, 0.456f, 0.406f, 0.229f, 0.224f, 0.225f};

static int swin_crops_args(int out_h, int out_w, const float** mean_std6) {
    if (!*mean_std6) *mean_std6 = kImagenetMeanStd;
    return swin_crops_check(out_h, out_w, *mean_std6);
}

// the common end of the two crops entries, their arguments checked: fault word, weights, then the windows of `src` in passes
static int swin_embed_windows(reid_ctx* ctx, RaggedSrc& src, int out_h, int out_w, const float* mean_std6, float* emb, float* logits) {
    CTX_ENTER(ctx);
    const SwinWeights* sw;
    REID_TRY(swin_loaded(ctx, &sw));
    if (src.n == 0) return REID_OK;
    EmbedOut out{emb, logits, 96, sw->num_class};
    REID_TRY(src.alloc(ctx, "io"));
    REID_TRY(out.alloc(ctx, "io", src.n, 0, logits != nullptr));
    return embed_host(
        ctx, src.n, swin_pass(ctx), [&](int i, int m, hipStream_t s) -> int { return src.up(i, m, s); },
        [&](int i, int m, float* d_emb, float* d_log) -> int {
            return swin_forward_crops(ctx, *sw, src.d_src, src.d_off + i, src.d_hw + 2 * i, m, out_h, out_w, src.pitch, mean_std6, d_emb, d_log);
        },
        out);
}

// The frame pipeline's Swin submit (reid_frame_submit_swin, bank.hip; contract: reid_internal.h)
int swin_ragged_ready(reid_ctx* ctx, int out_h, int out_w, const float** mean_std6, int* dim_out) {
    REID_TRY(swin_crops_args(out_h, out_w, mean_std6));
    const SwinWeights* sw;
    REID_TRY(swin_loaded(ctx, &sw));
    REID_TRY(swin_crops.open());
    *dim_out = 96;
    return REID_OK;
}

int swin_ragged_enqueue(reid_ctx* ctx, const char* tag, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n, int out_h,
                        int out_w, const float* mean_std6, float** d_emb_out, bool side_copy) {
    const SwinWeights* sw;
    REID_TRY(swin_loaded(ctx, &sw));
    RaggedSrc src{packed, offsets, hw, n};
    EmbedOut out{nullptr, nullptr, 96, sw->num_class};
    REID_TRY(ragged_enqueue_begin(ctx, tag, src, out, false, side_copy));
    REID_TRY(embed_dev_passes(n, swin_pass(ctx), [&](int i, int m) -> int {
        return swin_forward_crops(ctx, *sw, src.d_src, src.d_off + i, src.d_hw + 2 * i, m, out_h, out_w, src.pitch, mean_std6,
                                  out.d_emb + (size_t)i * 96, nullptr);
    }));
    *d_emb_out = out.d_emb;
    return REID_OK;
}

extern "C" int reid_swin_embed_ragged_u8(reid_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n, int out_h,
                                         int out_w, const float* mean_std6, float* emb, float* logits) {
    ARG_CHECK(ctx && packed && offsets && hw && emb && n >= 0);
    REID_TRY(swin_crops_args(out_h, out_w, &mean_std6));
    RaggedSrc src{packed, offsets, hw, n};
    REID_TRY(src.check());
    return swin_embed_windows(ctx, src, out_h, out_w, mean_std6, emb, logits);
}

// Windows frame[y1:y2, x1:x2] of ONE frame, as reid_embed_frame_u8: the frame goes up once, every window is resized straight out of it
// (same taps, clamped to the WINDOW's border: bit-identical to the same pixels handed over as packed crops).
extern "C" int reid_swin_embed_frame_u8(reid_ctx* ctx, const uint8_t* frame, int fh, int fw, const int32_t* boxes_xyxy, int n, int out_h,
                                        int out_w, const float* mean_std6, float* emb, float* logits) {
    ARG_CHECK(ctx && frame && boxes_xyxy && emb && fh >= 1 && fw >= 1 && n >= 0);
    REID_TRY(swin_crops_args(out_h, out_w, &mean_std6));
    RaggedSrc src{};
    REID_TRY(src.frame(frame, fh, fw, boxes_xyxy, n));
    return swin_embed_windows(ctx, src, out_h, out_w, mean_std6, emb, logits);
}

// ------------------------------------------------------------------------------------------------ descriptors
// The evaluation script's retrieval descriptor for a Swin (reid/image_reid_inference.py --backbone swin_v1 | swin_v2, :145-152, :202-208):
// inference_efficient runs model(cat(img, flip(img))) (:112-123, with --sie the camera index of an image as the view_index of BOTH its
// views, :117-120) and SwinTransformer.forward returns (logits, x_norm) in eval mode (swin_transformer.py:422-423), so a row is
// [normalize(logits) | normalize(x_norm)], averaged over the views and renormalised (:252-253).  Per pass: the forward of the plain view,
// the forward of the mirrored view from a stem that reads the source backwards (no mirrored copy), then swin_descriptor_kernel, which
// runs the classifier itself - all three from libreid_hip_swin_eval.so.
namespace {
// whatever side indices are pending when a descriptor entry leaves, on any path, are dropped
struct SidePendingClear {
    reid_ctx* ctx;
    ~SidePendingClear() {
        ctx->side_idx.clear();
        ctx->side_cursor = 0;
    }
};

struct SwinDescPlan {
    const SwinWeights* sw = nullptr;
    std::vector<int32_t> side;   // the call's side indices, one per image (empty: none)
    int nc = 0;
};
}  // namespace

// Everything a descriptor call can be refused for, with nothing queued: weights with a classifier and the side libraries
// (REID_ERR_STATE), the classifier's size and the side indices' count and range (REID_ERR_ARG).  Takes the pending side indices over.
static int swin_descriptor_ready(reid_ctx* ctx, int n, bool crops, SwinDescPlan* p) {
    p->sw = swin_find(ctx);
    if (!p->sw || !p->sw->loaded) {
        reid_set_error("reid_swin_descriptor_*: call reid_swin_load first");
        return REID_ERR_STATE;
    }
    if (!p->sw->cls_w || p->sw->num_class <= 0) {
        reid_set_error("reid_swin_descriptor_*: the loaded weights have no classifier (cls.w), the descriptor needs the logits");
        return REID_ERR_STATE;
    }
    p->nc = p->sw->num_class;
    REID_TRY(swin_eval.open());
    if (crops) REID_TRY(swin_crops.open());
    if (p->nc > swin_eval.max_classes()) {
        reid_set_error("reid_swin_descriptor_*: %d classes, the descriptor kernel holds at most %d (both views' logits stay in LDS)", p->nc,
                       swin_eval.max_classes());
        return REID_ERR_ARG;
    }
    if ((uintptr_t)p->sw->cls_w & 15) {
        reid_set_error("reid_swin_descriptor_*: cls.w must lie 16-byte aligned in the blob (reid_amd.weights.pack_swin places it so)");
        return REID_ERR_ARG;
    }
    if (ctx->side_idx.empty()) return REID_OK;
    const size_t pending = ctx->side_idx.size() - ctx->side_cursor;
    if (p->sw->views <= 0) {
        reid_set_error("reid_swin_descriptor_*: side indices are pending (reid_ctx_set_side_index) but the loaded weights carry no table for them");
        return REID_ERR_STATE;
    }
    if (pending != (size_t)n) {
        reid_set_error("reid_swin_descriptor_*: %d images but %zu side indices are pending", n, pending);
        return REID_ERR_ARG;
    }
    p->side.assign(ctx->side_idx.begin() + ctx->side_cursor, ctx->side_idx.end());
    for (int i = 0; i < n; ++i)
        if (p->side[i] >= p->sw->views) {
            reid_set_error("reid_swin_descriptor_*: side index %d of image %d is outside the table of %d rows", p->side[i], i, p->sw->views);
            return REID_ERR_ARG;
        }
    return REID_OK;
}

// One pass, images [i, i + m) of the call.  view(v, c1, e) queues the forward of view v (0 plain, 1 mirrored) into e [m][96], c1 being the
// pass's first-convolution workspace.  Each view is handed the pass's side indices afresh: swin_body takes them (ctx_take_side) once per
// forward, and the same index serves the plain and the mirrored view of an image.
template <class View>
static int swin_descriptor_pass(reid_ctx* ctx, const SwinDescPlan& p, int i, int m, int h, int wd, int flip_tta, float* e1, float* e2, View view,
                                float* d_out) {
    float* c1;
    REID_TRY(swin_c1(ctx, m, h, wd, &c1));
    for (int v = 0; v < (flip_tta ? 2 : 1); ++v) {
        if (!p.side.empty()) {
            ctx->side_idx.assign(p.side.begin() + i, p.side.begin() + i + m);
            ctx->side_cursor = 0;
        }
        REID_TRY(view(v, c1, v ? e2 : e1));
    }
    return launch_swin_descriptor(ctx, e1, flip_tta ? e2 : nullptr, p.sw->cls_w, m, p.nc, p.nc + 96, d_out);
}

// the two x_norm buffers of a pass
static int swin_descriptor_ws(reid_ctx* ctx, int pass, int flip_tta, float** e1, float** e2) {
    *e2 = nullptr;
    REID_TRY(ctx_ws(ctx, "swd.e1", (size_t)pass * 96 * 4, (void**)e1));
    if (flip_tta) REID_TRY(ctx_ws(ctx, "swd.e2", (size_t)pass * 96 * 4, (void**)e2));
    return REID_OK;
}

// a view of float images: the plain one through swin_body's own stem, the mirrored one through sfe_conv1_mirror_kernel into c1
static int swin_view_f32(reid_ctx* ctx, const SwinWeights& w, int v, const float* d_x, float* c1, int m, int h, int wd, float* e) {
    if (v == 0) return swin_body(ctx, w, d_x, c1, m, h, wd, e, nullptr);
    REID_TRY(launch_sfe_conv1_mirror(ctx, d_x, m, h, wd, w.c1_w, w.c1_b, c1));
    return swin_body(ctx, w, nullptr, c1, m, h, wd, e, nullptr);
}

extern "C" int reid_swin_descriptor_f32_nchw_dev(reid_ctx* ctx, const float* d_x, int n, int h, int w, int flip_tta, float* d_out) {
    ARG_CHECK(ctx);
    SidePendingClear drop{ctx};
    ARG_CHECK(d_x && d_out && n >= 0 && h > 0 && w > 0 && h % 224 == 0 && w % 224 == 0);
    CTX_ENTER(ctx);
    if (n == 0) return REID_OK;
    SwinDescPlan p;
    REID_TRY(swin_descriptor_ready(ctx, n, false, &p));
    const int pass = swin_pass(ctx);
    const size_t img = (size_t)3 * h * w, width = (size_t)p.nc + 96;
    float *e1, *e2;
    REID_TRY(swin_descriptor_ws(ctx, n < pass ? n : pass, flip_tta, &e1, &e2));
    return embed_dev_passes(n, pass, [&](int i, int m) -> int {
        const float* xi = d_x + (size_t)i * img;
        return swin_descriptor_pass(
            ctx, p, i, m, h, w, flip_tta, e1, e2, [&](int v, float* c1, float* e) -> int { return swin_view_f32(ctx, *p.sw, v, xi, c1, m, h, w, e); },
            d_out + (size_t)i * width);
    });
}

extern "C" int reid_swin_descriptor_f32_nchw(reid_ctx* ctx, const float* x, int n, int h, int w, int flip_tta, float* out) {
    ARG_CHECK(ctx);
    SidePendingClear drop{ctx};
    ARG_CHECK(x && out && n >= 0 && h > 0 && w > 0 && h % 224 == 0 && w % 224 == 0);
    CTX_ENTER(ctx);
    if (n == 0) return REID_OK;
    SwinDescPlan p;
    REID_TRY(swin_descriptor_ready(ctx, n, false, &p));
    const int pass = swin_pass(ctx);
    const size_t img = (size_t)3 * h * w;
    float *d_in, *e1, *e2;
    EmbedOut o{out, nullptr, p.nc + 96, 0};
    REID_TRY(ctx_ws(ctx, "io.in", (size_t)n * img * 4, (void**)&d_in));
    REID_TRY(o.alloc(ctx, "swd", n, 0, false));
    REID_TRY(swin_descriptor_ws(ctx, n < pass ? n : pass, flip_tta, &e1, &e2));
    return embed_host(
        ctx, n, pass,
        [&](int i, int m, hipStream_t s) -> int {
            HIP_TRY(hipMemcpyAsync(d_in + (size_t)i * img, x + (size_t)i * img, (size_t)m * img * 4, hipMemcpyHostToDevice, s));
            return REID_OK;
        },
        [&](int i, int m, float* d_row, float*) -> int {
            const float* xi = d_in + (size_t)i * img;
            return swin_descriptor_pass(
                ctx, p, i, m, h, w, flip_tta, e1, e2,
                [&](int v, float* c1, float* e) -> int { return swin_view_f32(ctx, *p.sw, v, xi, c1, m, h, w, e); }, d_row);
        },
        o);
}

// uint8 crops in: the plain view through swin_crop_front_kernel, the mirrored one through swin_crop_front_mirror_kernel, which reverses
// the RESIZED image's columns - Resize -> flip -> ToTensor -> Normalize, the order of the reference's transforms.  Bit-identical to
// reid_swin_descriptor_f32_nchw on the same crops resized and normalised in fp32 on the host.
extern "C" int reid_swin_descriptor_ragged_u8(reid_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n, int out_h,
                                              int out_w, const float* mean_std6, int flip_tta, float* out) {
    ARG_CHECK(ctx);
    SidePendingClear drop{ctx};
    ARG_CHECK(packed && offsets && hw && out && n >= 0);
    REID_TRY(swin_crops_args(out_h, out_w, &mean_std6));
    RaggedSrc src{packed, offsets, hw, n};
    REID_TRY(src.check());
    CTX_ENTER(ctx);
    if (n == 0) return REID_OK;
    SwinDescPlan p;
    REID_TRY(swin_descriptor_ready(ctx, n, true, &p));
    const int pass = swin_pass(ctx);
    float *e1, *e2;
    EmbedOut o{out, nullptr, p.nc + 96, 0};
    REID_TRY(src.alloc(ctx, "io"));
    REID_TRY(o.alloc(ctx, "swd", n, 0, false));
    REID_TRY(swin_descriptor_ws(ctx, n < pass ? n : pass, flip_tta, &e1, &e2));
    return embed_host(
        ctx, n, pass, [&](int i, int m, hipStream_t s) -> int { return src.up(i, m, s); },
        [&](int i, int m, float* d_row, float*) -> int {
            return swin_descriptor_pass(
                ctx, p, i, m, out_h, out_w, flip_tta, e1, e2,
                [&](int v, float* c1, float* e) -> int {
                    REID_TRY((v ? launch_swin_crop_front_mirror : launch_swin_crop_front)(ctx, src.d_src, src.d_off + i, src.d_hw + 2 * i, m, out_h,
                                                                                         out_w, src.pitch, mean_std6, p.sw->c1_w, p.sw->c1_b, c1));
                    return swin_body(ctx, *p.sw, nullptr, c1, m, out_h, out_w, e, nullptr);
                },
                d_row);
        },
        o);
}

// uint8 images of any sizes in: transforms.Resize((out_h, out_w)) as PIL computes it -> ToTensor -> Normalize on the device (PilPlan,
// libreid_hip_pil_resize.so) into the pass's fp32 NCHW workspace, then the two views of reid_swin_descriptor_f32_nchw on it - the same
// kernels on the same values, so the same bits as that entry on the images preprocessed on the host.
extern "C" int reid_swin_descriptor_images_u8(reid_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n, int out_h,
                                              int out_w, const float* mean_std6, int flip_tta, float* out) {
    ARG_CHECK(ctx);
    SidePendingClear drop{ctx};
    ARG_CHECK(packed && offsets && hw && out && n >= 0);
    REID_TRY(swin_crops_args(out_h, out_w, &mean_std6));
    RaggedSrc src{packed, offsets, hw, n};
    REID_TRY(src.check());
    CTX_ENTER(ctx);
    if (n == 0) return REID_OK;
    SwinDescPlan p;
    REID_TRY(swin_descriptor_ready(ctx, n, false, &p));
    const int pass = swin_pass(ctx);
    PilPlan plan;
    REID_TRY(plan.build(src, out_h, out_w, mean_std6, pass));
    float *e1, *e2;
    EmbedOut o{out, nullptr, p.nc + 96, 0};
    REID_TRY(src.alloc(ctx, "io"));
    REID_TRY(o.alloc(ctx, "swd", n, 0, false));
    REID_TRY(plan.alloc(ctx, "io"));
    REID_TRY(swin_descriptor_ws(ctx, n < pass ? n : pass, flip_tta, &e1, &e2));
    return embed_host(
        ctx, n, pass,
        [&](int i, int m, hipStream_t s) -> int {
            REID_TRY(src.up(i, m, s));
            return i == 0 ? plan.up(s) : REID_OK;
        },
        [&](int i, int m, float* d_row, float*) -> int {
            REID_TRY(plan.launch(ctx, src, i, m, nullptr, plan.d_f32));
            return swin_descriptor_pass(
                ctx, p, i, m, out_h, out_w, flip_tta, e1, e2,
                [&](int v, float* c1, float* e) -> int { return swin_view_f32(ctx, *p.sw, v, plan.d_f32, c1, m, out_h, out_w, e); }, d_row);
        },
        o);
}
