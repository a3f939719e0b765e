// libreid_hip_anysize_ca.so: the TripletAttention tail of CARes18-IBN for any map size (anysize_ca.h).
//
// Three launches.  (1) any_ca_stats_kernel, grid (H + W, images): a block owns ONE line of the image - blocks [0, H) the W pixels of row h,
// blocks [H, H + W) the H pixels of column w - and reduces it per channel in fp64: a row gives the hc plane's (h, :) entries, a column the
// cw plane's (:, w) entries.  The row blocks also reduce each of their pixels over C (the hw plane), across the lanes that share the pixel.
// So y is read twice, every line lives in one block (no partial crosses a block, nothing to combine in a later launch), and an image has
// H + W blocks.  A lane reads 16 bytes along C, the lanes of a pixel one run of C floats, four pixels per lane in flight.  (2)
// any_ca_gate_kernel, one thread per gate element: 98 taps from the maps (L2), affine, sigmoid.  (3) any_ca_apply_kernel, grid (row slabs,
// images) as any_se_tail_kernel: a thread keeps its channel quad, reads y / shortcut / the cw and hc gates 16 bytes at a time, four trips in
// flight.
#include "anysize_ca.h"
#include <math.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

// C4N = C / 4 channel quads.  QL lanes share a pixel (at most one wave's 64: C = 512 gives every lane KQ = 2 quads, QL * 4 floats apart),
// PG = 256 / QL pixel groups walk the line.
template <int C4N>
__global__ __launch_bounds__(256) void any_ca_stats_kernel(const float* __restrict__ y, int H, int W, float* __restrict__ maps) {
    constexpr int KQ = C4N > 64 ? 2 : 1, QL = C4N / KQ, PG = 256 / QL, C = C4N * 4, NK = KQ * 8;
    __shared__ double red[4 * QL * NK];
    const int img = blockIdx.y, tid = threadIdx.x, wave = tid >> 6;
    const int ql = tid & (QL - 1), pg = tid / QL;
    const bool row = (int)blockIdx.x < H;   // block-uniform
    const int line = row ? (int)blockIdx.x : (int)blockIdx.x - H;
    const int L = row ? W : H;
    const long long step = row ? C : (long long)W * C;
    const int hw = H * W;
    const float* base = y + ((long long)img * hw + (row ? line * W : line)) * C + ql * 4;
    float* m = maps + (long long)img * 2 * (hw + C * W + H * C);
    double s[KQ][8];
#pragma unroll
    for (int kq = 0; kq < KQ; ++kq)
#pragma unroll
        for (int k = 0; k < 8; ++k) s[kq][k] = 0.0;
    for (int j0 = 0; j0 < L; j0 += 4 * PG) {   // the same trips for every thread: a pixel group past the line adds zeros
        f32x4 v[4][KQ];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u * PG + pg;
#pragma unroll
            for (int kq = 0; kq < KQ; ++kq) {
                v[u][kq] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (j < L) v[u][kq] = *(const f32x4*)(base + (long long)j * step + kq * QL * 4);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            double p1 = 0.0, p2 = 0.0;
#pragma unroll
            for (int kq = 0; kq < KQ; ++kq)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double d = (double)v[u][kq][e];
                    s[kq][e] += d;
                    s[kq][4 + e] += d * d;
                    p1 += d;
                    p2 += d * d;
                }
            if (row) {   // the pixel over C: its QL lanes are neighbours in one wave
#pragma unroll
                for (int o = QL >> 1; o > 0; o >>= 1) {
                    p1 += __shfl_xor(p1, o);
                    p2 += __shfl_xor(p2, o);
                }
                const int j = j0 + u * PG + pg;
                if (ql == 0 && j < L) {
                    const double mean = p1 / C;
                    double var = (p2 - p1 * mean) / (C - 1);
                    if (var < 0.0) var = 0.0;
                    m[line * W + j] = (float)sqrt(var);
                    m[hw + line * W + j] = (float)mean;
                }
            }
        }
    }
    // the line per channel: the pixel groups of a wave by shuffles, the four waves through LDS in a fixed order
#pragma unroll
    for (int kq = 0; kq < KQ; ++kq)
#pragma unroll
        for (int k = 0; k < 8; ++k) {
#pragma unroll
            for (int o = QL; o < 64; o <<= 1) s[kq][k] += __shfl_xor(s[kq][k], o);
        }
    if ((tid & 63) < QL) {
#pragma unroll
        for (int kq = 0; kq < KQ; ++kq)
#pragma unroll
            for (int k = 0; k < 8; ++k) red[(wave * QL + ql) * NK + kq * 8 + k] = s[kq][k];
    }
    __syncthreads();
    if (tid >= QL) return;
#pragma unroll
    for (int kq = 0; kq < KQ; ++kq) {
        f32x4 sd, mu;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k1 = kq * 8 + e, k2 = k1 + 4;
            const double s1 = ((red[(0 * QL + ql) * NK + k1] + red[(1 * QL + ql) * NK + k1]) + red[(2 * QL + ql) * NK + k1]) +
                              red[(3 * QL + ql) * NK + k1];
            const double s2 = ((red[(0 * QL + ql) * NK + k2] + red[(1 * QL + ql) * NK + k2]) + red[(2 * QL + ql) * NK + k2]) +
                              red[(3 * QL + ql) * NK + k2];
            const double mean = s1 / L;
            double var = (s2 - s1 * mean) / (L - 1);
            if (var < 0.0) var = 0.0;
            sd[e] = (float)sqrt(var);
            mu[e] = (float)mean;
        }
        const int ch = (kq * QL + ql) * 4;
        if (row) {   // hc plane [2][H][C]
            float* dst = m + 2 * hw + 2 * C * W;
            *(f32x4*)(dst + line * C + ch) = sd;
            *(f32x4*)(dst + H * C + line * C + ch) = mu;
        } else {     // cw plane [2][C][W]
            float* dst = m + 2 * hw;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dst[(ch + e) * W + line] = sd[e];
                dst[C * W + (ch + e) * W + line] = mu[e];
            }
        }
    }
}

// grid (ceil(per / 256), images), one thread per gate element.  prm [3: cw, hc, hw][100].
__global__ __launch_bounds__(256) void any_ca_gate_kernel(const float* __restrict__ maps, int H, int W, int C, const float* __restrict__ prm,
                                                          float* __restrict__ gates) {
    __shared__ float wk[300];
    const int img = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < 300; i += 256) wk[i] = prm[i];
    __syncthreads();
    const int hw = H * W, cw = C * W, per = hw + cw + H * C;
    const int i = blockIdx.x * 256 + tid;
    if (i >= per) return;
    int P, Q, pr, qc, moff, gsel;
    if (i < hw) { P = H; Q = W; pr = i / W; qc = i - pr * W; moff = 0; gsel = 2; }                                       // hw [H][W]
    else if (i < hw + cw) { const int k = i - hw; P = C; Q = W; qc = k / C; pr = k - qc * C; moff = 2 * hw; gsel = 0; }   // cw, stored [W][C]
    else { const int k = i - hw - cw; P = H; Q = C; pr = k / C; qc = k - pr * C; moff = 2 * hw + 2 * cw; gsel = 1; }      // hc [H][C]
    const float* m = maps + (long long)img * 2 * per + moff;
    const float* wg = wk + gsel * 100;
    const int plane = P * Q;
    float acc = 0.f;
    for (int ch = 0; ch < 2; ++ch)
        for (int r = 0; r < 7; ++r) {
            const int pp = pr + r - 3;
            if ((unsigned)pp >= (unsigned)P) continue;
            for (int t = 0; t < 7; ++t) {
                const int qq = qc + t - 3;
                if ((unsigned)qq >= (unsigned)Q) continue;
                acc = __builtin_fmaf(wg[ch * 49 + r * 7 + t], m[ch * plane + pp * Q + qq], acc);
            }
        }
    acc = __builtin_fmaf(acc, wg[98], wg[99]);
    gates[(long long)img * per + i] = 1.0f / (1.0f + expf(-acc));
}

// grid (slabs, images): rows [blockIdx.x * rows, + rows) of the image.  256 % (C / 4) == 0: a thread keeps its channel quad.
__global__ __launch_bounds__(256) void any_ca_apply_kernel(const float* __restrict__ y, const float* __restrict__ sc,
                                                           const float* __restrict__ gates, int H, int W, int C, int rows,
                                                           float* __restrict__ out) {
#pragma clang fp contract(off)
    const int img = blockIdx.y, tid = threadIdx.x;
    const int c4n = C >> 2, sh = __builtin_ctz(c4n);
    const int hw = H * W;
    const int h0 = blockIdx.x * rows;
    const int nrows = min(rows, H - h0);
    if (nrows <= 0) return;
    const float* g_hw = gates + (long long)img * (hw + C * W + H * C);
    const float* g_cw = g_hw + hw;        // [W][C]
    const float* g_hc = g_cw + C * W;     // [H][C]
    const int p0 = h0 * W;
    const long long base = ((long long)img * hw + p0) * C;
    const int total4 = nrows * W * c4n;
    const int ch = (tid & (c4n - 1)) * 4;
    auto finish = [&](int i, const f32x4 yy, const f32x4 rr, float ghw, const f32x4 gcw, const f32x4 ghc) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float a = yy[e] * ghw, b = yy[e] * gcw[e], d = yy[e] * ghc[e];
            const float t = 0.3333333333333333f * ((a + b) + d);
            o[e] = fmaxf(t + rr[e], 0.f);
        }
        *(f32x4*)(out + base + (long long)i * 4) = o;
    };
    int i = tid;
    for (; i + 3 * 256 < total4; i += 4 * 256) {
        f32x4 yy[4], rr[4], gcw[4], ghc[4];
        float ghw[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ii = i + u * 256;
            const int p = p0 + (ii >> sh), h = p / W, w = p - h * W;
            yy[u] = *(const f32x4*)(y + base + (long long)ii * 4);
            rr[u] = *(const f32x4*)(sc + base + (long long)ii * 4);
            ghw[u] = g_hw[p];
            gcw[u] = *(const f32x4*)(g_cw + w * C + ch);
            ghc[u] = *(const f32x4*)(g_hc + h * C + ch);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) finish(i + u * 256, yy[u], rr[u], ghw[u], gcw[u], ghc[u]);
    }
    for (; i < total4; i += 256) {
        const int p = p0 + (i >> sh), h = p / W, w = p - h * W;
        finish(i, *(const f32x4*)(y + base + (long long)i * 4), *(const f32x4*)(sc + base + (long long)i * 4), g_hw[p],
               *(const f32x4*)(g_cw + w * C + ch), *(const f32x4*)(g_hc + h * C + ch));
    }
}

inline bool shape_ok(int n, int H, int W, int C) {
    return n >= 1 && n <= 65535 && H >= 2 && H <= 128 && W >= 2 && W <= 128 && (C == 64 || C == 128 || C == 256 || C == 512);
}

}  // namespace

extern "C" size_t anysize_ca_workspace_bytes(int n, int H, int W, int C) {
    if (!shape_ok(n, H, W, C)) return 0;
    return (size_t)n * 3 * ((size_t)H * W + (size_t)C * W + (size_t)H * C) * sizeof(float);
}

extern "C" hipError_t anysize_ca_tail(hipStream_t stream, const float* y, const float* shortcut, int n, int H, int W, int C, const float* prm,
                                      void* ws, float* out) {
    if (!y || !shortcut || !prm || !ws || !out || out == y || out == shortcut || !shape_ok(n, H, W, C)) return hipErrorInvalidValue;
    const int per = H * W + C * W + H * C;
    float* maps = (float*)ws;
    float* gates = maps + (size_t)n * 2 * per;
    const dim3 sgrid(H + W, n);
    switch (C) {
        case 64: hipLaunchKernelGGL(any_ca_stats_kernel<16>, sgrid, dim3(256), 0, stream, y, H, W, maps); break;
        case 128: hipLaunchKernelGGL(any_ca_stats_kernel<32>, sgrid, dim3(256), 0, stream, y, H, W, maps); break;
        case 256: hipLaunchKernelGGL(any_ca_stats_kernel<64>, sgrid, dim3(256), 0, stream, y, H, W, maps); break;
        default: hipLaunchKernelGGL(any_ca_stats_kernel<128>, sgrid, dim3(256), 0, stream, y, H, W, maps); break;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(any_ca_gate_kernel, dim3((per + 255) / 256, n), dim3(256), 0, stream, maps, H, W, C, prm, gates);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    // ~4096 16-byte chunks per block, whole rows: an image's blocks grow with its map, a pass of a few images still has hundreds
    int slabs = (H * W * (C / 4) + 4095) / 4096;
    if (slabs > H) slabs = H;
    const int rows = (H + slabs - 1) / slabs;
    hipLaunchKernelGGL(any_ca_apply_kernel, dim3((H + rows - 1) / rows, n), dim3(256), 0, stream, y, shortcut, gates, H, W, C, rows, out);
    return hipGetLastError();
}
