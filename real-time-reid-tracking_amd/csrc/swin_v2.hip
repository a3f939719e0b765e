// Swin-T version "v2" blocks (reference: reid/backbones/swin_transformer.py:85-92,140-149,165-209,238-246): the two kernels v2 needs
// beside v1's (swin.hip) - cosine window attention with a scale and a position-bias table per head, and the post-norm
// x + LayerNorm(y).  The launch sequence of a v2 block is in swin.hip (swin_block_v2).
//
// Built as a library of its own, libreid_hip_swin_v2.so, which swin.hip opens on the first v2 checkpoint (swin_v2.h): libreid_hip.so, its
// dependencies and its kernel list (tests/golden/kernels.json) are what they were for every caller that never loads v2 weights; this
// library's kernels are held to tests/golden/kernels_swin_v2.json the same way.
//
// The position bias (meta_mlp over the 49 x 49 log-spaced relative coordinates, :177-189) does not depend on the input: the host
// evaluates it once when it packs the weights (weights.py, swin_v2_bias_table), reid_swin_load transposes it to [head][key][query
// padded to 64], and the attention kernel reads one coalesced 256-byte row per key.
#include "reid_internal.h"   // range_acc / range_raise only
#include "swin_v2.h"
#include <math.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16;
typedef f16 half4 __attribute__((ext_vector_type(4)));

namespace {

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

// ---- WindowAttention v2 (swin_transformer.py:191-232 with :205-209): one wave per (image, window, head), lane = query token (49 of
// 64 lanes active), K and V of the window / head in LDS (read as broadcasts), softmax in registers - window_attn_kernel's frame
// (swin.hip), the cyclic shift folded into the token index the same way.
//   dots[i][j] = (q_i / max(|q_i|, 1e-12)) . (k_j / max(|k_j|, 1e-12)) * scale[head] + bias[head][i][j]   (+ the two shift masks)
// q is normalised in the lane's registers; a K row is normalised while it is staged: the eight lanes that hold the 32 channels of a
// token add their partial sums of squares with three xor shuffles (every one of them ends with the same sum, bit for bit).  True
// divisions, as F.normalize does.  Whatever T is, normalisation, logits and softmax are fp32: with scale up to 100 a logit carries
// 100 times the rounding of its cosine.
// qkv: [tokens][ldq] (q | k | v, head-major inside each), out: [tokens][C].  T = float (exact mode) or f16 (fp16-storage mode).
// packed != nullptr (T = float, precision 2): the result goes out as [oh | ol'] f16 [tokens][2C] for the fp32-class to_out linear.
template <typename T>
__global__ __launch_bounds__(256) void window_attn_cos_kernel(const T* __restrict__ qkv, int ldq, int n_img, int H, int W, int heads,
                                                              int shifted, const float* __restrict__ bias_t,
                                                              const float* __restrict__ scale, T* __restrict__ out,
                                                              f16* __restrict__ packed, int* __restrict__ fault) {
    __shared__ float kv[4][2][49 * 32];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
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
    // the bias row of every key for this lane's query: bias_t[head][key][query], queries padded to 64 (lanes 49 .. 63 read zeros)
    float s[49];
    {
        const float* bt = bias_t + (size_t)head * 49 * 64 + lane;
#pragma unroll
        for (int j = 0; j < 49; ++j) s[j] = bt[j * 64];
    }
    float q[32];
#pragma unroll
    for (int d = 0; d < 32; ++d) q[d] = 0.f;
    if (act) {
        const T* base = qkv + tok * ldq + head * 32;
#pragma unroll
        for (int d = 0; d < 32; d += 4) {
            const f32x4 a = ld4(base + d);
            q[d] = a.x; q[d + 1] = a.y; q[d + 2] = a.z; q[d + 3] = a.w;
        }
        float ss = 0.f;
#pragma unroll
        for (int d = 0; d < 32; ++d) ss += q[d] * q[d];
        const float den = fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
        for (int d = 0; d < 32; ++d) q[d] = q[d] / den;
    }
    // K and V of the window, slot by slot as in window_attn_kernel (slot = four channels; eight consecutive lanes = the 128 bytes of
    // one token's head slice, consecutive lanes = consecutive LDS addresses: coalesced loads, conflict-free ds_write_b128).  The
    // shuffles run on all 64 lanes of every wave, live or not; slots past 49 x 8 carry zeros and store nothing.
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const int slot = lane + 64 * i;
        const bool ok = live && slot < 49 * 8;
        f32x4 kk = {0.f, 0.f, 0.f, 0.f}, vv = kk;
        if (ok) {
            const int j = slot >> 3, d = (slot & 7) * 4;
            const int jy = j / 7, jx = j - jy * 7;
            const int y = (wy * 7 + jy + sh) % H, x = (wx * 7 + jx + sh) % W;
            const T* base = qkv + (((long long)img * H + y) * W + x) * ldq + head * 32 + d;
            kk = ld4(base + C);
            vv = ld4(base + 2 * C);
        }
        float ss = (kk.x * kk.x + kk.y * kk.y) + (kk.z * kk.z + kk.w * kk.w);
        ss += __shfl_xor(ss, 1);
        ss += __shfl_xor(ss, 2);
        ss += __shfl_xor(ss, 4);
        const float den = fmaxf(sqrtf(ss), 1e-12f);
        if (ok) {
            *(f32x4*)&kv[wave][0][slot * 4] = kk / den;
            *(f32x4*)&kv[wave][1][slot * 4] = vv;
        }
    }
    __syncthreads();
    if (!act) return;
    const float sc = scale[head];
    const bool last_row = shifted && wy == nwh - 1, last_col = shifted && wx == nww - 1;
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 49; ++j) {
        const float* kj = &kv[wave][0][j * 32];
        float acc = 0.f;
#pragma unroll
        for (int d = 0; d < 32; ++d) acc += q[d] * kj[d];
        const int jy = j / 7, jx = j - jy * 7;
        acc = acc * sc + s[j];
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

// ---- Post-norm of a v2 block (Residual(PostNorm(..)), swin_transformer.py:66-72,85-92): out = x + (LayerNorm(y) * g + b) over rows
// of C channels, fp32 statistics, two-pass (mean, then centred sum of squares) in registers - layernorm_v4_kernel's frame (swin.hip):
// LPT lanes per token (32 for C = 96: two tokens per wave; 64 otherwise), a lane owns the 4-channel chunks sub + LPT * j, 16-byte
// accesses.  out may be x itself (every element is read and written by the same lane).
// SIDE: what the next linear reads, written here so that no pack pass is needed - 1 = an f16 copy of out [tokens][c] (fp16-storage
// mode), 2 = [oh | ol'] f16 [tokens][2c] with ol' = f16((o - oh) 2^11) and the range guard (fp32-class mode), 0 = nothing.
template <int LPT, int SIDE>
__global__ __launch_bounds__(256) void post_norm_kernel(const float* x, const float* __restrict__ y, long long ntok, int c, float eps,
                                                        const float* __restrict__ g, const float* __restrict__ b, float* out,
                                                        f16* __restrict__ side, int* __restrict__ fault) {
    constexpr int TPW = 64 / LPT;                  // tokens per wave
    constexpr int MAXJ = LPT == 32 ? 1 : 3;        // chunks per lane: C <= 128 (LPT 32) or C <= 768 (LPT 64)
    const int lane = threadIdx.x & 63, sub = lane & (LPT - 1);
    const long long tok = (blockIdx.x * 4LL + (threadIdx.x >> 6)) * TPW + lane / LPT;
    const bool live = tok < ntok;
    const int nch = c >> 2;
    const float* yi = y + (live ? tok : 0) * c;
    f32x4 v[MAXJ];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        const int ch = sub + LPT * j;
        v[j] = (live && ch < nch) ? *(const f32x4*)(yi + ch * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
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
    const float* xi = x + tok * c;
    float* oi = out + tok * c;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        const int ch = sub + LPT * j;
        if (ch < nch) {
            const f32x4 gg = *(const f32x4*)(g + ch * 4), bb = *(const f32x4*)(b + ch * 4);
            const f32x4 ln = (v[j] - mean) * rstd * gg + bb;
            const f32x4 r = *(const f32x4*)(xi + ch * 4) + ln;
            *(f32x4*)(oi + ch * 4) = r;
            if constexpr (SIDE == 1) {
                st4(side + tok * c + ch * 4, r);
            } else if constexpr (SIDE == 2) {
                range_raise(fault, range_acc(range_acc(range_acc(range_acc(0u, r.x), r.y), r.z), r.w));   // range guard (reid_ctx.fault)
                half4 hi = {(f16)r.x, (f16)r.y, (f16)r.z, (f16)r.w};
                half4 lo = {(f16)((r.x - (float)hi[0]) * 2048.0f), (f16)((r.y - (float)hi[1]) * 2048.0f),
                            (f16)((r.z - (float)hi[2]) * 2048.0f), (f16)((r.w - (float)hi[3]) * 2048.0f)};
                f16* si = side + tok * 2 * c;
                *(half4*)(si + ch * 4) = hi;
                *(half4*)(si + c + ch * 4) = lo;
            }
        }
    }
}

}  // namespace

// The two launches, on a stream (swin_v2.h).  No context, nothing of libreid_hip.so: this file is a library of its own.
extern "C" hipError_t swin_v2_window_attn_cos(hipStream_t stream, int mode, const void* qkv, int ldq, int n_img, int H, int W, int heads, int shifted,
                                   const float* bias_t, const float* scale, void* out, int* fault) {
    const long long ntask = (long long)n_img * (H / 7) * (W / 7) * heads;
    const dim3 grid((unsigned)((ntask + 3) / 4)), block(256);
    if (mode == 1)
        hipLaunchKernelGGL(window_attn_cos_kernel<f16>, grid, block, 0, stream, (const f16*)qkv, ldq, n_img, H, W, heads, shifted, bias_t,
                           scale, (f16*)out, (f16*)nullptr, (int*)nullptr);
    else
        hipLaunchKernelGGL(window_attn_cos_kernel<float>, grid, block, 0, stream, (const float*)qkv, ldq, n_img, H, W, heads, shifted,
                           bias_t, scale, mode == 0 ? (float*)out : (float*)nullptr, mode == 2 ? (f16*)out : (f16*)nullptr, fault);
    return hipGetLastError();
}

template <int SIDE>
static void post_norm_launch(hipStream_t stream, const float* x, const float* y, long long T, int C, const float* g, const float* b,
                             float* out, f16* side, int* fault) {
    if (C <= 128)
        hipLaunchKernelGGL((post_norm_kernel<32, SIDE>), dim3((unsigned)((T + 7) / 8)), dim3(256), 0, stream, x, y, T, C, 1e-5f, g, b, out,
                           side, fault);
    else
        hipLaunchKernelGGL((post_norm_kernel<64, SIDE>), dim3((unsigned)((T + 3) / 4)), dim3(256), 0, stream, x, y, T, C, 1e-5f, g, b, out,
                           side, fault);
}

extern "C" hipError_t swin_v2_post_norm(hipStream_t stream, int side_mode, const float* x, const float* y, long long T, int C, const float* g,
                             const float* b, float* out, _Float16* side, int* fault) {
    if (side_mode == 0) post_norm_launch<0>(stream, x, y, T, C, g, b, out, side, fault);
    else if (side_mode == 1) post_norm_launch<1>(stream, x, y, T, C, g, b, out, side, fault);
    else post_norm_launch<2>(stream, x, y, T, C, g, b, out, side, fault);
    return hipGetLastError();
}
