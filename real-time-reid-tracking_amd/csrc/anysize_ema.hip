// libreid_hip_anysize_ema.so: the EMA block tail of EMARes18-IBN for any map size (anysize_ema.h: formula, arithmetic, workspace).
//
// Four launches.  (1) any_ema_lines_kernel, grid (H + W, images): a block owns ONE line of the image - blocks [0, H) row h, blocks
// [H, H + W) column w - reduces it per channel in fp64, and, since the 1x1 convolution mixes only the channels of a group at one position
// of the [H + W] vector, finishes that position for all C channels: convolution, sigmoid, one row of sig.  (2) any_ema_pass_kernel<CG,
// false>, grid (row slabs, images): a thread keeps its channel quad and walks the slab's pixels four at a time; it forms x1pre and x2 and
// adds them (and x1pre squared) in fp64; the threads of a quad are added through LDS in thread order, the slab's three sums per channel go
// to the workspace.  (3) any_ema_finish_kernel, one block per image, one thread per channel: slabs in slab order, mu, rstd, both softmaxes.
// (4) any_ema_pass_kernel<CG, true>: the same walk and the same code for x1pre and x2, then x1, the group's weight (lanes of a group are
// neighbours in a wave: at most two xor shuffles), the gate, shortcut and ReLU.
//
// The 3 x 3 neighbourhood: nine 16-byte loads per channel quad of the group, straight from global memory - the lanes of neighbouring
// pixels ask for the same lines, so all but the first come from L1 - and zeros outside the map (fmaf(w, 0, acc) is acc).  The weights lie
// in LDS as [ci][tap][co], so a lane reads its four output channels of one (ci, tap) in one 16-byte read and uses it for four pixels.
#include "anysize_ema.h"
#include <math.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

// offsets into prm (floats), cg = C / 32
struct Prm {
    int w1, b1, w3, b3, gw, gb;
    __host__ __device__ constexpr explicit Prm(int cg)
        : w1(0), b1(cg * cg), w3(cg * cg + cg), b3(cg * cg + cg + cg * cg * 9), gw(cg * cg + cg + cg * cg * 9 + cg),
          gb(cg * cg + cg + cg * cg * 9 + 2 * cg) {}
};

// C4N = C / 4 channel quads share a pixel, PG = 256 / C4N pixel groups walk the line.
template <int C4N>
__global__ __launch_bounds__(256) void any_ema_lines_kernel(const float* __restrict__ y, int H, int W, const float* __restrict__ prm,
                                                            float* __restrict__ sig) {
#pragma clang fp contract(off)
    constexpr int C = C4N * 4, CG = C / 32, PG = 256 / C4N;
    constexpr Prm P(CG);
    __shared__ double red[PG * C];
    __shared__ float meanv[C];
    const int img = blockIdx.y, tid = threadIdx.x;
    const int ql = tid & (C4N - 1), pg = tid / C4N;
    const bool row = (int)blockIdx.x < H;   // block-uniform
    const int line = row ? (int)blockIdx.x : (int)blockIdx.x - H;
    const int L = row ? W : H;
    const long long step = row ? C : (long long)W * C;
    const float* base = y + ((long long)img * H * W + (row ? line * W : line)) * C + ql * 4;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j0 = 0; j0 < L; j0 += 4 * PG) {
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u * PG + pg;
            v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (j < L) v[u] = *(const f32x4*)(base + (long long)j * step);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += (double)v[u][e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) red[pg * C + ql * 4 + e] = s[e];
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

// x2 of channel quad q at U pixels (h[u], w[u]) of the image at yi; wl (LDS) [ci][tap][co], acc starts as the bias.  A pixel with ok false
// loads nothing.
template <int CG, int U>
__device__ __forceinline__ void ema_x2(const float* __restrict__ yi, int H, int W, int q, const int (&h)[U], const int (&w)[U],
                                       const bool (&ok)[U], const float* wl, const f32x4 b3q, f32x4 (&acc)[U]) {
    constexpr int C = CG * 32, QG = CG >= 4 ? CG / 4 : 1;
    const int gq0 = q & ~(QG - 1);            // the group's first quad
    const int cob = (q & (QG - 1)) * 4;       // this quad's first channel within the group
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = b3q;
#pragma unroll 1
    for (int qq = 0; qq < QG; ++qq) {
#pragma unroll 1
      for (int r = -1; r <= 1; ++r) {       // a row of taps per trip: twelve loads in flight, the code stays small
#pragma unroll
        for (int s = -1; s <= 1; ++s) {
            const int t = (r + 1) * 3 + s + 1;
            f32x4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int hh = h[u] + r, ww = w[u] + s;
                v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (ok[u] && (unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W)
                    v[u] = *(const f32x4*)(yi + (hh * W + ww) * C + (gq0 + qq) * 4);
            }
            if constexpr (CG >= 4) {
#pragma unroll
                for (int e2 = 0; e2 < 4; ++e2) {
                    const f32x4 w4 = *(const f32x4*)(wl + ((qq * 4 + e2) * 9 + t) * CG + cob);
#pragma unroll
                    for (int u = 0; u < U; ++u)
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[u][e] = __builtin_fmaf(w4[e], v[u][e2], acc[u][e]);
                }
            } else {   // cg = 2: the quad holds two groups, channels (0, 1) and (2, 3)
#pragma unroll
                for (int ci = 0; ci < 2; ++ci) {
                    const float w0 = wl[(ci * 9 + t) * 2], w1 = wl[(ci * 9 + t) * 2 + 1];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        acc[u][0] = __builtin_fmaf(w0, v[u][ci], acc[u][0]);
                        acc[u][1] = __builtin_fmaf(w1, v[u][ci], acc[u][1]);
                        acc[u][2] = __builtin_fmaf(w0, v[u][2 + ci], acc[u][2]);
                        acc[u][3] = __builtin_fmaf(w1, v[u][2 + ci], acc[u][3]);
                    }
                }
            }
        }
      }
    }
}

// grid (slabs, images): rows [blockIdx.x * rows, + rows) of the image.  256 % (C / 4) == 0: a thread keeps its channel quad, and every
// thread makes the same trips (the shuffles of the apply pass need whole groups).  APPLY false: part [img][slab][3][C]; true: out.
template <int CG, bool APPLY>
__global__ __launch_bounds__(256) void any_ema_pass_kernel(const float* __restrict__ y, const float* __restrict__ sc,
                                                           const float* __restrict__ prm, const float* __restrict__ sig,
                                                           const float* __restrict__ small, double* __restrict__ part, int H, int W, int rows,
                                                           float* __restrict__ out) {
#pragma clang fp contract(off)
    constexpr int C = CG * 32, C4N = CG * 8, SH = __builtin_ctz(C4N), PG = 256 / C4N, U = 4, QG = CG >= 4 ? CG / 4 : 1;
    constexpr Prm P(CG);
    __shared__ __attribute__((aligned(16))) float wl[CG * CG * 9];
    __shared__ double red[APPLY ? 1 : 12 * 256];
    const int img = blockIdx.y, tid = threadIdx.x, q = tid & (C4N - 1);
    for (int i = tid; i < CG * CG * 9; i += 256) {   // [co][ci][tap] -> [ci][tap][co]
        const int co = i / (CG * 9), rem = i - co * CG * 9, ci = rem / 9, t = rem - ci * 9;
        wl[(ci * 9 + t) * CG + co] = prm[P.w3 + i];
    }
    __syncthreads();
    const int hw = H * W;
    const int h0 = blockIdx.x * rows;
    const int nrows = min(rows, H - h0);
    if (nrows <= 0) return;   // block-uniform; the grid has no such block
    const int p0 = h0 * W, total4 = nrows * W * C4N;
    const long long ibase = (long long)img * hw * C;
    const float* yi = y + ibase;
    const float* sg = sig + (long long)img * (H + W) * C + q * 4;
    f32x4 b3q, gwq, gbq;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int k = (q * 4 + e) & (CG - 1);
        b3q[e] = prm[P.b3 + k];
        gwq[e] = prm[P.gw + k];
        gbq[e] = prm[P.gb + k];
    }
    f32x4 muq = b3q, rstdq = b3q, s1q = b3q, s2q = b3q;
    if constexpr (APPLY) {
        const float* sm = small + (long long)img * 4 * C + q * 4;
        muq = *(const f32x4*)sm;
        rstdq = *(const f32x4*)(sm + C);
        s1q = *(const f32x4*)(sm + 2 * C);
        s2q = *(const f32x4*)(sm + 3 * C);
    }
    double S[12];
#pragma unroll
    for (int a = 0; a < 12; ++a) S[a] = 0.0;
    for (int i0 = 0; i0 < total4; i0 += U * 256) {
        int h[U], w[U], p[U];
        bool ok[U];
        f32x4 yy[U], rr[U], x2[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int ii = i0 + u * 256 + tid;
            ok[u] = ii < total4;
            p[u] = p0 + (ok[u] ? ii >> SH : 0);
            h[u] = p[u] / W;
            w[u] = p[u] - h[u] * W;
            yy[u] = rr[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (ok[u]) {
                yy[u] = *(const f32x4*)(yi + p[u] * C + q * 4);
                if constexpr (APPLY) rr[u] = *(const f32x4*)(sc + ibase + p[u] * C + q * 4);
            }
        }
        ema_x2<CG, U>(yi, H, W, q, h, w, ok, wl, b3q, x2);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const f32x4 sh = *(const f32x4*)(sg + h[u] * C), sw = *(const f32x4*)(sg + (H + w[u]) * C);
            f32x4 x1p;
#pragma unroll
            for (int e = 0; e < 4; ++e) x1p[e] = (yy[u][e] * sh[e]) * sw[e];
            if constexpr (!APPLY) {
                if (ok[u]) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const double d = (double)x1p[e];
                        S[e] += d;
                        S[4 + e] += d * d;
                        S[8 + e] += (double)x2[u][e];
                    }
                }
            } else {
                f32x4 x1, g;
#pragma unroll
                for (int e = 0; e < 4; ++e) x1[e] = __builtin_fmaf((x1p[e] - muq[e]) * rstdq[e], gwq[e], gbq[e]);
                if constexpr (CG >= 4) {
                    float t = 0.f;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        t = __builtin_fmaf(s1q[e], x2[u][e], t);
                        t = __builtin_fmaf(s2q[e], x1[e], t);
                    }
#pragma unroll
                    for (int o = 1; o < QG; o <<= 1) t += __shfl_xor(t, o);
                    const float gt = 1.0f / (1.0f + expf(-t));
                    g = f32x4{gt, gt, gt, gt};
                } else {
                    float ta = 0.f, tb = 0.f;
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        ta = __builtin_fmaf(s1q[e], x2[u][e], ta);
                        ta = __builtin_fmaf(s2q[e], x1[e], ta);
                        tb = __builtin_fmaf(s1q[2 + e], x2[u][2 + e], tb);
                        tb = __builtin_fmaf(s2q[2 + e], x1[2 + e], tb);
                    }
                    const float ga = 1.0f / (1.0f + expf(-ta)), gb2 = 1.0f / (1.0f + expf(-tb));
                    g = f32x4{ga, ga, gb2, gb2};
                }
                if (ok[u]) {
                    f32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float m = yy[u][e] * g[e];
                        o[e] = fmaxf(m + rr[u][e], 0.f);
                    }
                    *(f32x4*)(out + ibase + p[u] * C + q * 4) = o;
                }
            }
        }
    }
    if constexpr (!APPLY) {
#pragma unroll
        for (int a = 0; a < 12; ++a) red[a * 256 + tid] = S[a];
        __syncthreads();
        double* dst = part + ((long long)img * gridDim.x + blockIdx.x) * 3 * C;
        for (int k = tid; k < 12 * C4N; k += 256) {   // the pixel groups of a quad in thread order
            const int a = k / C4N, qq = k - a * C4N;
            double t = red[a * 256 + qq];
#pragma unroll
            for (int g = 1; g < PG; ++g) t += red[a * 256 + g * C4N + qq];
            dst[(a >> 2) * C + qq * 4 + (a & 3)] = t;
        }
    }
}

// grid (images), C threads: thread c adds its channel's slabs in slab order.
__global__ __launch_bounds__(512) void any_ema_finish_kernel(const double* __restrict__ part, const float* __restrict__ prm, int hw, int C,
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
hipError_t run(hipStream_t stream, const float* y, const float* sc, int n, int H, int W, const float* prm, void* ws, float* out) {
    constexpr int C = CG * 32;
    const int rows = anysize_ema_rows(H, W, C), slabs = anysize_ema_slabs(H, W, C);
    double* part = (double*)ws;
    float* sig = (float*)(part + (size_t)n * slabs * 3 * C);
    float* small = sig + (size_t)n * (H + W) * C;
    hipLaunchKernelGGL(any_ema_lines_kernel<CG * 8>, dim3(H + W, n), dim3(256), 0, stream, y, H, W, prm, sig);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((any_ema_pass_kernel<CG, false>), dim3(slabs, n), dim3(256), 0, stream, y, sc, prm, sig, small, part, H, W, rows, out);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(any_ema_finish_kernel, dim3(n), dim3(C), 0, stream, part, prm, H * W, C, slabs, small);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((any_ema_pass_kernel<CG, true>), dim3(slabs, n), dim3(256), 0, stream, y, sc, prm, sig, small, part, H, W, rows, out);
    return hipGetLastError();
}

}  // namespace

extern "C" size_t anysize_ema_workspace_bytes(int n, int H, int W, int C) {
    if (!shape_ok(n, H, W, C)) return 0;
    const size_t slabs = (size_t)anysize_ema_slabs(H, W, C);
    return (size_t)n * (slabs * 3 * C * sizeof(double) + ((size_t)(H + W) * C + 4 * (size_t)C) * sizeof(float));
}

extern "C" hipError_t anysize_ema_tail(hipStream_t stream, const float* y, const float* shortcut, int n, int H, int W, int C, const float* prm,
                                       void* ws, float* out) {
    if (!y || !shortcut || !prm || !ws || !out || out == y || out == shortcut || !shape_ok(n, H, W, C)) return hipErrorInvalidValue;
    switch (C) {
        case 64: return run<2>(stream, y, shortcut, n, H, W, prm, ws, out);
        case 128: return run<4>(stream, y, shortcut, n, H, W, prm, ws, out);
        case 256: return run<8>(stream, y, shortcut, n, H, W, prm, ws, out);
        default: return run<16>(stream, y, shortcut, n, H, W, prm, ws, out);
    }
}
