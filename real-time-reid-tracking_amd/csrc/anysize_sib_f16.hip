// libreid_hip_anysize_sib_f16.so: the TripletAttention and EMA block tails for any map size on f16 maps (anysize_sib_f16.h: arithmetic,
// launches, workspaces).  The kernels are those of anysize_ca.hip and anysize_ema.hip restated for lanes that hold EIGHT channels: a lane
// reads and writes 16 bytes of f16 along C, converts to fp32 at once (exact) and rounds to f16 at its store, nowhere else.
#include "anysize_sib_f16.h"
#include <math.h>

typedef _Float16 f16;
typedef f16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

__device__ __forceinline__ half8 zero8() { return half8{0, 0, 0, 0, 0, 0, 0, 0}; }

// ---------------------------------------------------------------------------------------------- TripletAttention
// C8N = C / 8 channel octets share a pixel (at most one wave's 64), PG = 256 / C8N pixel groups walk the line.
template <int C8N>
__global__ __launch_bounds__(256) void any_sib_ca_stats_kernel(const f16* __restrict__ y, int H, int W, float* __restrict__ maps) {
    constexpr int QL = C8N, PG = 256 / QL, C = C8N * 8, NK = 16;
    __shared__ double red[4 * QL * NK];
    const int img = blockIdx.y, tid = threadIdx.x, wave = tid >> 6;
    const int ql = tid & (QL - 1), pg = tid / QL;
    const bool row = (int)blockIdx.x < H;   // block-uniform
    const int line = row ? (int)blockIdx.x : (int)blockIdx.x - H;
    const int L = row ? W : H;
    const long long step = row ? C : (long long)W * C;
    const int hw = H * W;
    const f16* base = y + ((long long)img * hw + (row ? line * W : line)) * C + ql * 8;
    float* m = maps + (long long)img * 2 * (hw + C * W + H * C);
    double s[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) s[k] = 0.0;
    for (int j0 = 0; j0 < L; j0 += 4 * PG) {   // the same trips for every thread: a pixel group past the line adds zeros
        half8 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u * PG + pg;
            v[u] = zero8();
            if (j < L) v[u] = *(const half8*)(base + (long long)j * step);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            double p1 = 0.0, p2 = 0.0;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const double d = (double)(float)v[u][e];
                s[e] += d;
                s[8 + e] += d * d;
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
    for (int k = 0; k < NK; ++k) {
#pragma unroll
        for (int o = QL; o < 64; o <<= 1) s[k] += __shfl_xor(s[k], o);
    }
    if ((tid & 63) < QL) {
#pragma unroll
        for (int k = 0; k < NK; ++k) red[(wave * QL + ql) * NK + k] = s[k];
    }
    __syncthreads();
    if (tid >= QL) return;
    float sd[8], mu[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k1 = e, k2 = 8 + e;
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
    const int ch = ql * 8;
    if (row) {   // hc plane [2][H][C]
        float* dst = m + 2 * hw + 2 * C * W;
        *(f32x4*)(dst + line * C + ch) = f32x4{sd[0], sd[1], sd[2], sd[3]};
        *(f32x4*)(dst + line * C + ch + 4) = f32x4{sd[4], sd[5], sd[6], sd[7]};
        *(f32x4*)(dst + H * C + line * C + ch) = f32x4{mu[0], mu[1], mu[2], mu[3]};
        *(f32x4*)(dst + H * C + line * C + ch + 4) = f32x4{mu[4], mu[5], mu[6], mu[7]};
    } else {     // cw plane [2][C][W]
        float* dst = m + 2 * hw;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            dst[(ch + e) * W + line] = sd[e];
            dst[C * W + (ch + e) * W + line] = mu[e];
        }
    }
}

// grid (ceil(per / 256), images), one thread per gate element.  prm [3: cw, hc, hw][100].  fp32 in, fp32 out: any_ca_gate_kernel.
__global__ __launch_bounds__(256) void any_sib_ca_gate_kernel(const float* __restrict__ maps, int H, int W, int C, const float* __restrict__ prm,
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

// grid (slabs, images): rows [blockIdx.x * rows, + rows) of the image.  256 % (C / 8) == 0: a thread keeps its channel octet.
__global__ __launch_bounds__(256) void any_sib_ca_apply_kernel(const f16* __restrict__ y, const f16* __restrict__ sc,
                                                               const float* __restrict__ gates, int H, int W, int C, int rows,
                                                               f16* __restrict__ out) {
#pragma clang fp contract(off)
    const int img = blockIdx.y, tid = threadIdx.x;
    const int c8n = C >> 3, sh = __builtin_ctz(c8n);
    const int hw = H * W;
    const int h0 = blockIdx.x * rows;
    const int nrows = min(rows, H - h0);
    if (nrows <= 0) return;
    const float* g_hw = gates + (long long)img * (hw + C * W + H * C);
    const float* g_cw = g_hw + hw;        // [W][C]
    const float* g_hc = g_cw + C * W;     // [H][C]
    const int p0 = h0 * W;
    const long long base = ((long long)img * hw + p0) * C;
    const int total8 = nrows * W * c8n;
    const int ch = (tid & (c8n - 1)) * 8;
    auto finish = [&](int i, const half8 yy, const half8 rr, float ghw, const f32x4 (&gcw)[2], const f32x4 (&ghc)[2]) {
        half8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float yv = (float)yy[e];
            const float a = yv * ghw, b = yv * gcw[e >> 2][e & 3], d = yv * ghc[e >> 2][e & 3];
            const float t = 0.3333333333333333f * ((a + b) + d);
            o[e] = (f16)fmaxf(t + (float)rr[e], 0.f);
        }
        *(half8*)(out + base + (long long)i * 8) = o;
    };
    int i = tid;
    for (; i + 256 < total8; i += 2 * 256) {
        half8 yy[2], rr[2];
        f32x4 gcw[2][2], ghc[2][2];
        float ghw[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int ii = i + u * 256;
            const int p = p0 + (ii >> sh), h = p / W, w = p - h * W;
            yy[u] = *(const half8*)(y + base + (long long)ii * 8);
            rr[u] = *(const half8*)(sc + base + (long long)ii * 8);
            ghw[u] = g_hw[p];
            gcw[u][0] = *(const f32x4*)(g_cw + w * C + ch);
            gcw[u][1] = *(const f32x4*)(g_cw + w * C + ch + 4);
            ghc[u][0] = *(const f32x4*)(g_hc + h * C + ch);
            ghc[u][1] = *(const f32x4*)(g_hc + h * C + ch + 4);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) finish(i + u * 256, yy[u], rr[u], ghw[u], gcw[u], ghc[u]);
    }
    for (; i < total8; i += 256) {
        const int p = p0 + (i >> sh), h = p / W, w = p - h * W;
        const f32x4 gcw[2] = {*(const f32x4*)(g_cw + w * C + ch), *(const f32x4*)(g_cw + w * C + ch + 4)};
        const f32x4 ghc[2] = {*(const f32x4*)(g_hc + h * C + ch), *(const f32x4*)(g_hc + h * C + ch + 4)};
        finish(i, *(const half8*)(y + base + (long long)i * 8), *(const half8*)(sc + base + (long long)i * 8), g_hw[p], gcw, ghc);
    }
}

// ---------------------------------------------------------------------------------------------- EMA
// offsets into prm (floats), cg = C / 32
struct Prm {
    int w1, b1, w3, b3, gw, gb;
    __host__ __device__ constexpr explicit Prm(int cg)
        : w1(0), b1(cg * cg), w3(cg * cg + cg), b3(cg * cg + cg + cg * cg * 9), gw(cg * cg + cg + cg * cg * 9 + cg),
          gb(cg * cg + cg + cg * cg * 9 + 2 * cg) {}
};

// C8N = C / 8 channel octets share a pixel, PG = 256 / C8N pixel groups walk the line.
template <int C8N>
__global__ __launch_bounds__(256) void any_sib_ema_lines_kernel(const f16* __restrict__ y, int H, int W, const float* __restrict__ prm,
                                                                float* __restrict__ sig) {
#pragma clang fp contract(off)
    constexpr int C = C8N * 8, CG = C / 32, PG = 256 / C8N;
    constexpr Prm P(CG);
    __shared__ double red[PG * C];
    __shared__ float meanv[C];
    const int img = blockIdx.y, tid = threadIdx.x;
    const int ql = tid & (C8N - 1), pg = tid / C8N;
    const bool row = (int)blockIdx.x < H;   // block-uniform
    const int line = row ? (int)blockIdx.x : (int)blockIdx.x - H;
    const int L = row ? W : H;
    const long long step = row ? C : (long long)W * C;
    const f16* base = y + ((long long)img * H * W + (row ? line * W : line)) * C + ql * 8;
    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j0 = 0; j0 < L; j0 += 4 * PG) {
        half8 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u * PG + pg;
            v[u] = zero8();
            if (j < L) v[u] = *(const half8*)(base + (long long)j * step);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += (double)(float)v[u][e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[pg * C + ql * 8 + e] = s[e];
    __syncthreads();
    for (int c = tid; c < C; c += 256) {   // the pixel groups in group order
        double t = red[c];
#pragma unroll
        for (int p = 1; p < PG; ++p) t += red[p * C + c];
        meanv[c] = (float)(t / (double)L);
    }
    __syncthreads();
    float* dst = sig + ((long long)img * (H + W) + blockIdx.x) * C;
    for (int c = tid; c < C; c += 256) {
        const int k = c & (CG - 1), g0 = c - k;
        float acc = prm[P.b1 + k];
#pragma unroll
        for (int ci = 0; ci < CG; ++ci) acc = __builtin_fmaf(prm[P.w1 + k * CG + ci], meanv[g0 + ci], acc);
        dst[c] = 1.0f / (1.0f + expf(-acc));
    }
}

// x2 of channel octet o8 at U pixels (h[u], w[u]) of the image at yi; wl (LDS) [ci][tap][co], acc starts as the bias.  A pixel with ok
// false loads nothing.  The order of an output channel's multiply-adds is anysize_ema.h's: (quad of four ci, tap, ci within the quad).
template <int CG, int U>
__device__ __forceinline__ void ema_x2(const f16* __restrict__ yi, int H, int W, int o8, const int (&h)[U], const int (&w)[U],
                                       const bool (&ok)[U], const float* wl, const float (&b3o)[8], float (&acc)[U][8]) {
    constexpr int C = CG * 32, OG = CG >= 8 ? CG / 8 : 1;
    const int go0 = o8 & ~(OG - 1);           // the group's first octet (cg <= 8: the lane's own, which holds whole groups)
    const int cob = (o8 & (OG - 1)) * 8;      // this octet's first channel within the group
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[u][e] = b3o[e];
    auto load = [&](int oo, int r, int s, half8 (&v)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int hh = h[u] + r, ww = w[u] + s;
            v[u] = zero8();
            if (ok[u] && (unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W)
                v[u] = *(const half8*)(yi + (hh * W + ww) * C + (go0 + oo) * 8);
        }
    };
    if constexpr (CG >= 8) {
#pragma unroll 1
        for (int oo = 0; oo < OG; ++oo) {
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {     // the two quads of the octet, one after the other: the second reads the pieces again (L1)
#pragma unroll 1
                for (int r = -1; r <= 1; ++r) {
#pragma unroll
                    for (int s = -1; s <= 1; ++s) {
                        const int t = (r + 1) * 3 + s + 1;
                        half8 v[U];
                        load(oo, r, s, v);
#pragma unroll
                        for (int e2 = 0; e2 < 4; ++e2) {
                            const float* wp = wl + ((oo * 8 + hf * 4 + e2) * 9 + t) * CG + cob;
                            const f32x4 wa = *(const f32x4*)wp, wb = *(const f32x4*)(wp + 4);
#pragma unroll
                            for (int u = 0; u < U; ++u) {
                                const float x = (float)v[u][hf * 4 + e2];
#pragma unroll
                                for (int e = 0; e < 4; ++e) {
                                    acc[u][e] = __builtin_fmaf(wa[e], x, acc[u][e]);
                                    acc[u][4 + e] = __builtin_fmaf(wb[e], x, acc[u][4 + e]);
                                }
                            }
                        }
                    }
                }
            }
        }
    } else {
#pragma unroll 1
        for (int r = -1; r <= 1; ++r) {
#pragma unroll
            for (int s = -1; s <= 1; ++s) {
                const int t = (r + 1) * 3 + s + 1;
                half8 v[U];
                load(0, r, s, v);
                if constexpr (CG == 4) {   // the octet holds two groups, channels (0 .. 3) and (4 .. 7)
#pragma unroll
                    for (int e2 = 0; e2 < 4; ++e2) {
                        const f32x4 w4 = *(const f32x4*)(wl + (e2 * 9 + t) * 4);
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const float xa = (float)v[u][e2], xb = (float)v[u][4 + e2];
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                acc[u][e] = __builtin_fmaf(w4[e], xa, acc[u][e]);
                                acc[u][4 + e] = __builtin_fmaf(w4[e], xb, acc[u][4 + e]);
                            }
                        }
                    }
                } else {                   // cg = 2: four groups, channels (0, 1) .. (6, 7)
#pragma unroll
                    for (int ci = 0; ci < 2; ++ci) {
                        const float w0 = wl[(ci * 9 + t) * 2], w1 = wl[(ci * 9 + t) * 2 + 1];
#pragma unroll
                        for (int u = 0; u < U; ++u)
#pragma unroll
                            for (int g = 0; g < 4; ++g) {
                                const float x = (float)v[u][2 * g + ci];
                                acc[u][2 * g] = __builtin_fmaf(w0, x, acc[u][2 * g]);
                                acc[u][2 * g + 1] = __builtin_fmaf(w1, x, acc[u][2 * g + 1]);
                            }
                    }
                }
            }
        }
    }
}

// grid (slabs, images): rows [blockIdx.x * rows, + rows) of the image.  256 % (C / 8) == 0: a thread keeps its channel octet, and every
// thread makes the same trips (the shuffle of the apply pass needs whole groups).  APPLY false: part [img][slab][3][C]; true: out.
template <int CG, bool APPLY>
__global__ __launch_bounds__(256) void any_sib_ema_pass_kernel(const f16* __restrict__ y, const f16* __restrict__ sc,
                                                               const float* __restrict__ prm, const float* __restrict__ sig,
                                                               const float* __restrict__ small, double* __restrict__ part, int H, int W,
                                                               int rows, f16* __restrict__ out) {
#pragma clang fp contract(off)
    constexpr int C = CG * 32, C8N = CG * 4, SH = __builtin_ctz(C8N), PG = 256 / C8N, U = 2;
    constexpr Prm P(CG);
    __shared__ __attribute__((aligned(16))) float wl[CG * CG * 9];
    __shared__ double red[APPLY ? 1 : 24 * 256];
    const int img = blockIdx.y, tid = threadIdx.x, o8 = tid & (C8N - 1);
    for (int i = tid; i < CG * CG * 9; i += 256) {   // [co][ci][tap] -> [ci][tap][co]
        const int co = i / (CG * 9), rem = i - co * CG * 9, ci = rem / 9, t = rem - ci * 9;
        wl[(ci * 9 + t) * CG + co] = prm[P.w3 + i];
    }
    __syncthreads();
    const int hw = H * W;
    const int h0 = blockIdx.x * rows;
    const int nrows = min(rows, H - h0);
    if (nrows <= 0) return;   // block-uniform; the grid has no such block
    const int p0 = h0 * W, total8 = nrows * W * C8N;
    const long long ibase = (long long)img * hw * C;
    const f16* yi = y + ibase;
    const float* sg = sig + (long long)img * (H + W) * C + o8 * 8;
    float b3o[8], gwo[8], gbo[8], muo[8], rstdo[8], s1o[8], s2o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = (o8 * 8 + e) & (CG - 1);
        b3o[e] = prm[P.b3 + k];
        gwo[e] = prm[P.gw + k];
        gbo[e] = prm[P.gb + k];
        muo[e] = rstdo[e] = s1o[e] = s2o[e] = 0.f;
    }
    if constexpr (APPLY) {
        const float* sm = small + (long long)img * 4 * C + o8 * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            muo[e] = sm[e];
            rstdo[e] = sm[C + e];
            s1o[e] = sm[2 * C + e];
            s2o[e] = sm[3 * C + e];
        }
    }
    double S[24];
#pragma unroll
    for (int a = 0; a < 24; ++a) S[a] = 0.0;
    for (int i0 = 0; i0 < total8; i0 += U * 256) {
        int h[U], w[U], p[U];
        bool ok[U];
        half8 yy[U], rr[U];
        float x2[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int ii = i0 + u * 256 + tid;
            ok[u] = ii < total8;
            p[u] = p0 + (ok[u] ? ii >> SH : 0);
            h[u] = p[u] / W;
            w[u] = p[u] - h[u] * W;
            yy[u] = rr[u] = zero8();
            if (ok[u]) {
                yy[u] = *(const half8*)(yi + p[u] * C + o8 * 8);
                if constexpr (APPLY) rr[u] = *(const half8*)(sc + ibase + p[u] * C + o8 * 8);
            }
        }
        ema_x2<CG, U>(yi, H, W, o8, h, w, ok, wl, b3o, x2);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const f32x4 sh0 = *(const f32x4*)(sg + h[u] * C), sh1 = *(const f32x4*)(sg + h[u] * C + 4);
            const f32x4 sw0 = *(const f32x4*)(sg + (H + w[u]) * C), sw1 = *(const f32x4*)(sg + (H + w[u]) * C + 4);
            float x1p[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) x1p[e] = ((float)yy[u][e] * (e < 4 ? sh0[e & 3] : sh1[e & 3])) * (e < 4 ? sw0[e & 3] : sw1[e & 3]);
            if constexpr (!APPLY) {
                if (ok[u]) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const double d = (double)x1p[e];
                        S[e] += d;
                        S[8 + e] += d * d;
                        S[16 + e] += (double)x2[u][e];
                    }
                }
            } else {
                float x1[8], g[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) x1[e] = __builtin_fmaf((x1p[e] - muo[e]) * rstdo[e], gwo[e], gbo[e]);
                if constexpr (CG >= 4) {   // per quad of channels in k order
                    float tq[2] = {0.f, 0.f};
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        tq[e >> 2] = __builtin_fmaf(s1o[e], x2[u][e], tq[e >> 2]);
                        tq[e >> 2] = __builtin_fmaf(s2o[e], x1[e], tq[e >> 2]);
                    }
                    if constexpr (CG == 4) {          // two groups
#pragma unroll
                        for (int e = 0; e < 8; ++e) g[e] = 1.0f / (1.0f + expf(-tq[e >> 2]));
                    } else {
                        float t = tq[0] + tq[1];      // cg 8: the group; cg 16: (a + b), then + (c + d) of the neighbouring lane
                        if constexpr (CG == 16) t += __shfl_xor(t, 1);
                        const float gt = 1.0f / (1.0f + expf(-t));
#pragma unroll
                        for (int e = 0; e < 8; ++e) g[e] = gt;
                    }
                } else {                   // cg 2: four groups of two channels
#pragma unroll
                    for (int gi = 0; gi < 4; ++gi) {
                        float t = 0.f;
#pragma unroll
                        for (int e = 2 * gi; e < 2 * gi + 2; ++e) {
                            t = __builtin_fmaf(s1o[e], x2[u][e], t);
                            t = __builtin_fmaf(s2o[e], x1[e], t);
                        }
                        g[2 * gi] = g[2 * gi + 1] = 1.0f / (1.0f + expf(-t));
                    }
                }
                if (ok[u]) {
                    half8 o;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float m = (float)yy[u][e] * g[e];
                        o[e] = (f16)fmaxf(m + (float)rr[u][e], 0.f);
                    }
                    *(half8*)(out + ibase + p[u] * C + o8 * 8) = o;
                }
            }
        }
    }
    if constexpr (!APPLY) {
#pragma unroll
        for (int a = 0; a < 24; ++a) red[a * 256 + tid] = S[a];
        __syncthreads();
        double* dst = part + ((long long)img * gridDim.x + blockIdx.x) * 3 * C;
        for (int k = tid; k < 24 * C8N; k += 256) {   // the pixel groups of an octet in thread order
            const int a = k / C8N, oo = k - a * C8N;
            double t = red[a * 256 + oo];
#pragma unroll
            for (int g = 1; g < PG; ++g) t += red[a * 256 + g * C8N + oo];
            dst[(a >> 3) * C + oo * 8 + (a & 7)] = t;
        }
    }
}

// grid (images), C threads: thread c adds its channel's slabs in slab order.  fp64 in, fp32 out: any_ema_finish_kernel.
__global__ __launch_bounds__(512) void any_sib_ema_finish_kernel(const double* __restrict__ part, const float* __restrict__ prm, int hw, int C,
                                                                 int slabs, float* __restrict__ small) {
#pragma clang fp contract(off)
    __shared__ float a2[512];
    const int img = blockIdx.x, c = threadIdx.x;
    const int cg = C >> 5, k = c & (cg - 1), g0 = c - k;
    const Prm P(cg);
    const double* p = part + (long long)img * slabs * 3 * C + c;
    double S1 = 0.0, S2 = 0.0, S3 = 0.0;
    for (int s = 0; s < slabs; ++s) {
        S1 += p[(s * 3 + 0) * C];
        S2 += p[(s * 3 + 1) * C];
        S3 += p[(s * 3 + 2) * C];
    }
    const double mean = S1 / (double)hw;
    double var = (S2 - S1 * mean) / (double)hw;
    if (var < 0.0) var = 0.0;
    float* sm = small + (long long)img * 4 * C;
    sm[c] = (float)mean;
    sm[C + c] = (float)(1.0 / sqrt(var + 1e-5));
    a2[c] = (float)(S3 / (double)hw);
    __syncthreads();
    float m1 = -INFINITY, m2 = -INFINITY;
    for (int j = 0; j < cg; ++j) {
        m1 = fmaxf(m1, prm[P.gb + j]);
        m2 = fmaxf(m2, a2[g0 + j]);
    }
    float d1 = 0.f, d2 = 0.f;
    for (int j = 0; j < cg; ++j) {
        d1 += expf(prm[P.gb + j] - m1);
        d2 += expf(a2[g0 + j] - m2);
    }
    sm[2 * C + c] = expf(prm[P.gb + k] - m1) / d1;   // softmax(agp(x1)) = softmax(GroupNorm bias), anysize_ema.h
    sm[3 * C + c] = expf(a2[c] - m2) / d2;
}

inline bool shape_ok(int n, int H, int W, int C) {
    return n >= 1 && n <= 65535 && H >= 2 && H <= 128 && W >= 2 && W <= 128 && (C == 64 || C == 128 || C == 256 || C == 512);
}

template <int CG>
hipError_t run_ema(hipStream_t stream, const f16* y, const f16* sc, int n, int H, int W, const float* prm, void* ws, f16* out) {
    constexpr int C = CG * 32;
    const int rows = anysize_ema_rows(H, W, C), slabs = anysize_ema_slabs(H, W, C);
    double* part = (double*)ws;
    float* sig = (float*)(part + (size_t)n * slabs * 3 * C);
    float* small = sig + (size_t)n * (H + W) * C;
    hipLaunchKernelGGL(any_sib_ema_lines_kernel<CG * 4>, dim3(H + W, n), dim3(256), 0, stream, y, H, W, prm, sig);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((any_sib_ema_pass_kernel<CG, false>), dim3(slabs, n), dim3(256), 0, stream, y, sc, prm, sig, small, part, H, W, rows, out);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(any_sib_ema_finish_kernel, dim3(n), dim3(C), 0, stream, part, prm, H * W, C, slabs, small);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((any_sib_ema_pass_kernel<CG, true>), dim3(slabs, n), dim3(256), 0, stream, y, sc, prm, sig, small, part, H, W, rows, out);
    return hipGetLastError();
}

}  // namespace

extern "C" size_t anysize_sib_f16_ca_workspace_bytes(int n, int H, int W, int C) {
    if (!shape_ok(n, H, W, C)) return 0;
    return (size_t)n * 3 * ((size_t)H * W + (size_t)C * W + (size_t)H * C) * sizeof(float);
}

extern "C" hipError_t anysize_sib_f16_ca_tail(hipStream_t stream, const _Float16* y, const _Float16* shortcut, int n, int H, int W, int C,
                                              const float* prm, void* ws, _Float16* out) {
    if (!y || !shortcut || !prm || !ws || !out || out == y || out == shortcut || !shape_ok(n, H, W, C)) return hipErrorInvalidValue;
    const int per = H * W + C * W + H * C;
    float* maps = (float*)ws;
    float* gates = maps + (size_t)n * 2 * per;
    const dim3 sgrid(H + W, n);
    switch (C) {
        case 64: hipLaunchKernelGGL(any_sib_ca_stats_kernel<8>, sgrid, dim3(256), 0, stream, y, H, W, maps); break;
        case 128: hipLaunchKernelGGL(any_sib_ca_stats_kernel<16>, sgrid, dim3(256), 0, stream, y, H, W, maps); break;
        case 256: hipLaunchKernelGGL(any_sib_ca_stats_kernel<32>, sgrid, dim3(256), 0, stream, y, H, W, maps); break;
        default: hipLaunchKernelGGL(any_sib_ca_stats_kernel<64>, sgrid, dim3(256), 0, stream, y, H, W, maps); break;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(any_sib_ca_gate_kernel, dim3((per + 255) / 256, n), dim3(256), 0, stream, maps, H, W, C, prm, gates);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    // ~2048 16-byte pieces per block, whole rows: an image's blocks grow with its map, a pass of a few images still has hundreds
    int slabs = (H * W * (C / 8) + 2047) / 2048;
    if (slabs > H) slabs = H;
    const int rows = (H + slabs - 1) / slabs;
    hipLaunchKernelGGL(any_sib_ca_apply_kernel, dim3((H + rows - 1) / rows, n), dim3(256), 0, stream, y, shortcut, gates, H, W, C, rows, out);
    return hipGetLastError();
}

extern "C" size_t anysize_sib_f16_ema_workspace_bytes(int n, int H, int W, int C) {
    if (!shape_ok(n, H, W, C)) return 0;
    const size_t slabs = (size_t)anysize_ema_slabs(H, W, C);
    return (size_t)n * (slabs * 3 * C * sizeof(double) + ((size_t)(H + W) * C + 4 * (size_t)C) * sizeof(float));
}

extern "C" hipError_t anysize_sib_f16_ema_tail(hipStream_t stream, const _Float16* y, const _Float16* shortcut, int n, int H, int W, int C,
                                               const float* prm, void* ws, _Float16* out) {
    if (!y || !shortcut || !prm || !ws || !out || out == y || out == shortcut || !shape_ok(n, H, W, C)) return hipErrorInvalidValue;
    switch (C) {
        case 64: return run_ema<2>(stream, y, shortcut, n, H, W, prm, ws, out);
        case 128: return run_ema<4>(stream, y, shortcut, n, H, W, prm, ws, out);
        case 256: return run_ema<8>(stream, y, shortcut, n, H, W, prm, ws, out);
        default: return run_ema<16>(stream, y, shortcut, n, H, W, prm, ws, out);
    }
}
