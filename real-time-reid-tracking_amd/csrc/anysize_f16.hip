// libreid_hip_anysize_f16.so: ResNet18-IBN-SE at any input size in fp16 storage with fp32 accumulation (anysize_f16.h).
//
// any_conv_f16_kernel<BN>: the implicit GEMM of anysize_x3.hip without the split - 256 threads = 4 waves (2 pixel halves x 2 channel
// halves), a 128-pixel x BN-channel output tile, K walked tap by tap in steps of 32 input channels, one v_mfma_f32_16x16x32_f16 per
// fragment pair into one fp32 accumulator.  A GEMM row is one output pixel, decoded to (image, oy, ox) by division once per thread (a tile
// may cross image borders, rows >= M load zeros and store nothing), padding taps read as zero.  The loader moves f16 as it lies in memory:
// 16-byte global loads into registers, written to LDS after the MFMAs of the running step (two stages, one barrier per K step).  A row is
// 32 f16 = four 16-byte chunks; chunk g of row r sits at chunk g ^ ((r >> 2) & 3), so the 16 rows of a fragment read cover the 16 slots of a
// 256-byte bank row once.  The weights are the MFMA's first operand and the pixels its second, so a lane ends with four consecutive output
// channels of one pixel: scale / shift as 16-byte loads, residual and output as 8-byte ones.  No launch splits K.
//
// any_stem_f16_kernel: the 7x7 stride-2 stem as a GEMM with K = 8 x 24 = 192 (k = r 24 + s 3 + c, the 45 padding columns zero on both
// sides): a block keeps the 64 x 192 weights in LDS and walks up to four 64-pixel tiles, whose fp32 input taps it rounds to f16 on the way
// into LDS.  Rows are 400 bytes apart (100 dwords: 16 consecutive rows start in 16 different 4-dword bank groups).
//
// The tails share one structure: grid (c / 32, images), 256 threads = 4 channel octets x 64 pixel groups; a lane reads 16 bytes (8 f16), a
// thread adds its pixels pg, pg + 64, ... in fp64, the 16 pixel groups of a wave are combined with four shuffles and the four waves through
// LDS in a fixed order - the sums of an image do not depend on n, and hw below 64 only leaves lanes without pixels.
#include "anysize_f16.h"
#include <math.h>

namespace {

typedef _Float16 f16;
typedef f16 half8 __attribute__((ext_vector_type(8)));
typedef f16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------ trunk convolutions
struct ConvParams {
    const f16* x;
    const f16* w;
    const float* scale;
    const float* shift;
    const f16* residual;
    f16* out;
    int M, H, W, Cin, Cout, Ho, Wo, R, stride, pad;
    int relu, relu_from;
    int ntn;   // channel tiles (Cout / BN): blockIdx.x = pixel tile * ntn + channel tile
};

constexpr int BM = 128;
constexpr int ROWB = 64;   // bytes of a 32-channel f16 row

template <int BN>
__global__ __launch_bounds__(256, 2) void any_conv_f16_kernel(const ConvParams p) {
    constexpr int A_BYTES = BM * ROWB;
    constexpr int B_BYTES = BN * ROWB;
    constexpr int STAGE = A_BYTES + B_BYTES;
    constexpr int NB = BN * 4 / 256;   // 16-byte weight chunks per thread and step
    constexpr int NT = BN / 32;        // 16-channel MFMA tiles per wave
    __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int g = lane >> 4, r16 = lane & 15;
    const int m0 = (int)(blockIdx.x / p.ntn) * BM;
    const int n0 = (int)(blockIdx.x % p.ntn) * BN;
    const int cpb = p.Cin >> 5;
    const int nk = p.R * p.R * cpb;
    const int ldw = p.R * p.R * p.Cin;

    // ---- loader state: A = two rows x 8 channels, B = NB chunks
    const int ac = tid & 3;
    int iy0[2], ix0[2];
    long long pix0[2];
    int a_lds[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = (tid >> 2) + 64 * i;
        const int m = m0 + row;
        a_lds[i] = row * ROWB + ((ac ^ ((row >> 2) & 3)) << 4);
        if (m < p.M) {
            const int img = m / (p.Ho * p.Wo);
            const int rem = m - img * (p.Ho * p.Wo);
            const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
            iy0[i] = oy * p.stride - p.pad;
            ix0[i] = ox * p.stride - p.pad;
            pix0[i] = (long long)img * p.H * p.W;
        } else {
            iy0[i] = -4;   // every tap out of bounds
            ix0[i] = -4;
            pix0[i] = 0;
        }
    }
    int b_src[NB], b_lds[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int idx = tid + 256 * j;
        const int ch = idx & 3, co = idx >> 2;
        b_src[j] = (n0 + co) * ldw + ch * 8;
        b_lds[j] = A_BYTES + co * ROWB + ((ch ^ ((co >> 2) & 3)) << 4);
    }

    half8 av[2], bv[NB];
    int tap = 0, cb = 0;   // the step the next gload() fetches
    auto gload = [&]() {
        const int ty = tap / p.R, tx = tap - ty * p.R;
        const int c0 = cb << 5;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int iy = iy0[i] + ty, ix = ix0[i] + tx;
            if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W)
                av[i] = *(const half8*)(p.x + (pix0[i] + (long long)iy * p.W + ix) * p.Cin + c0 + ac * 8);
            else
                av[i] = half8{0, 0, 0, 0, 0, 0, 0, 0};
        }
        const int boff = tap * p.Cin + c0;
#pragma unroll
        for (int j = 0; j < NB; ++j) bv[j] = *(const half8*)(p.w + b_src[j] + boff);
        if (++cb == cpb) {
            cb = 0;
            ++tap;
        }
    };
    auto lstore = [&](char* st) {
#pragma unroll
        for (int i = 0; i < 2; ++i) *(half8*)(st + a_lds[i]) = av[i];
#pragma unroll
        for (int j = 0; j < NB; ++j) *(half8*)(st + b_lds[j]) = bv[j];
    };

    f32x4 acc[4][NT];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int frag = r16 * ROWB + ((g ^ (r16 >> 2)) << 4);   // rows of a fragment start at multiples of 16: the swizzle is the lane's
    const int a_frag = wm * 64 * ROWB + frag;
    const int b_frag = A_BYTES + wn * (BN / 2) * ROWB + frag;

    gload();
    lstore(lds);
    __syncthreads();
    for (int ks = 0; ks < nk; ++ks) {
        const bool more = ks + 1 < nk;
        if (more) gload();
        const char* st = lds + (ks & 1) * STAGE;
        half8 xf[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) xf[mt] = *(const half8*)(st + a_frag + mt * 16 * ROWB);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const half8 wf = *(const half8*)(st + b_frag + nt * 16 * ROWB);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, xf[mt], acc[mt][nt], 0, 0, 0);
        }
        if (more) lstore(lds + ((ks + 1) & 1) * STAGE);
        __syncthreads();
    }

    // ---- epilogue: a lane holds channels co .. co + 3 of pixel m
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int co = n0 + wn * (BN / 2) + nt * 16 + g * 4;
        f32x4 cs = f32x4{1.f, 1.f, 1.f, 1.f}, sh = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p.scale) {
            cs = *(const f32x4*)(p.scale + co);
            sh = *(const f32x4*)(p.shift + co);
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int m = m0 + wm * 64 + mt * 16 + r16;
            if (m >= p.M) continue;
            const long long idx = (long long)m * p.Cout + co;
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(acc[mt][nt][e], cs[e], sh[e]);
            if (p.residual) {
                const half4 rr = *(const half4*)(p.residual + idx);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += (float)rr[e];
            }
            if (p.relu) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (co + e >= p.relu_from) v[e] = fmaxf(v[e], 0.f);
            }
            half4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (f16)v[e];
            *(half4*)(p.out + idx) = o;
        }
    }
}

// ------------------------------------------------------------------------------------------------ stem
constexpr int SBM = 64;        // pixels per tile
constexpr int SROW = 400;      // bytes between LDS rows of 192 f16
constexpr int STILES = 4;      // tiles per block

__global__ __launch_bounds__(256) void any_stem_f16_kernel(const float* __restrict__ x, const f16* __restrict__ w16,
                                                           const float* __restrict__ scale, const float* __restrict__ shift,
                                                           f16* __restrict__ out, int M, int H, int W, int H1, int W1) {
    __shared__ __attribute__((aligned(16))) char lds[(SBM + 64) * SROW];
    char* const la = lds;
    char* const lb = lds + SBM * SROW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, r16 = lane & 15;
#pragma unroll
    for (int j = 0; j < 6; ++j) {   // 64 x 24 chunks of 16 bytes
        const int idx = tid + 256 * j;
        const int co = idx / 24, ch = idx - co * 24;
        *(half8*)(lb + co * SROW + ch * 16) = *(const half8*)(w16 + co * 192 + ch * 8);
    }
    const int ntiles = (M + SBM - 1) / SBM;
    const int t_end = min(ntiles, ((int)blockIdx.x + 1) * STILES);
    for (int t = (int)blockIdx.x * STILES; t < t_end; ++t) {
        const int m0 = t * SBM;
        __syncthreads();   // the previous tile's fragment reads are done
#pragma unroll
        for (int j = 0; j < 2; ++j) {   // 64 rows x 8 kernel rows
            const int idx = tid + 256 * j;
            const int row = idx >> 3, r = idx & 7;
            const int m = m0 + row;
            f16 v[24];
#pragma unroll
            for (int q = 0; q < 24; ++q) v[q] = (f16)0.f;
            if (m < M && r < 7) {
                const int img = m / (H1 * W1);
                const int rem = m - img * (H1 * W1);
                const int oy = rem / W1, ox = rem - oy * W1;
                const int iy = oy * 2 - 3 + r;
                if ((unsigned)iy < (unsigned)H) {
                    const float* src = x + ((long long)img * H + iy) * W * 3;
#pragma unroll
                    for (int s = 0; s < 7; ++s) {
                        const int ix = ox * 2 - 3 + s;
                        if ((unsigned)ix < (unsigned)W) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) v[s * 3 + c] = (f16)src[(long long)ix * 3 + c];
                        }
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                half8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = v[q * 8 + e];
                *(half8*)(la + row * SROW + r * 48 + q * 16) = o;
            }
        }
        __syncthreads();
        f32x4 acc[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 6; ++ks) {
            const half8 xf = *(const half8*)(la + (wave * 16 + r16) * SROW + ks * 64 + g * 16);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const half8 wf = *(const half8*)(lb + (nt * 16 + r16) * SROW + ks * 64 + g * 16);
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, xf, acc[nt], 0, 0, 0);
            }
        }
        const int m = m0 + wave * 16 + r16;
        if (m < M) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int co = nt * 16 + g * 4;
                const f32x4 cs = *(const f32x4*)(scale + co), sh = *(const f32x4*)(shift + co);
                half4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = (f16)__builtin_fmaf(acc[nt][e], cs[e], sh[e]);
                *(half4*)(out + (long long)m * 64 + co) = o;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ max-pool
__global__ __launch_bounds__(256) void any_maxpool_f16_kernel(const f16* __restrict__ x, long long total, int h, int w, int c8, int ho, int wo,
                                                              f16* __restrict__ out) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int ch = (int)(i % c8);
        long long rest = i / c8;
        const int ox = (int)(rest % wo);
        rest /= wo;
        const int oy = (int)(rest % ho);
        const long long img = rest / ho;
        const f16* xi = x + img * h * w * c8 * 8 + ch * 8;
        half8 m = *(const half8*)(xi + ((long long)(2 * oy) * w + 2 * ox) * c8 * 8);   // the centre tap is inside the map at any size
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int iy = 2 * oy + dy;
            if ((unsigned)iy >= (unsigned)h) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int ix = 2 * ox + dx;
                if ((unsigned)ix >= (unsigned)w) continue;
                const half8 v = *(const half8*)(xi + ((long long)iy * w + ix) * c8 * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) m[e] = v[e] > m[e] ? v[e] : m[e];
            }
        }
        *(half8*)(out + i * 8) = m;
    }
}

// ------------------------------------------------------------------------------------------------ tails
constexpr int OCTS = 4;      // 32 channels per block
constexpr int PGS = 64;      // pixel groups

// v[k] of every thread -> the block's total for that thread's channel octet, k = 0 .. K - 1.  red: K * 16 doubles.  Ends with a barrier.
template <int K>
__device__ __forceinline__ void oct_totals(double (&v)[K], double* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, oct = threadIdx.x & (OCTS - 1);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        v[k] += __shfl_xor(v[k], 4);
        v[k] += __shfl_xor(v[k], 8);
        v[k] += __shfl_xor(v[k], 16);
        v[k] += __shfl_xor(v[k], 32);
    }
    if (lane < OCTS) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[(wave * OCTS + lane) * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k)
        v[k] = ((red[(0 * OCTS + oct) * K + k] + red[(1 * OCTS + oct) * K + k]) + red[(2 * OCTS + oct) * K + k]) +
               red[(3 * OCTS + oct) * K + k];
    __syncthreads();
}

// the pixels pg, pg + 64, ... of one image's channel octet through f(v), four loads in flight
template <class F>
__device__ __forceinline__ void walk_pixels(const f16* xi, int hw, int c, int pg, F f) {
    int px = pg;
    for (; px + 3 * PGS < hw; px += 4 * PGS) {
        half8 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *(const half8*)(xi + (long long)(px + PGS * u) * c);
#pragma unroll
        for (int u = 0; u < 4; ++u) f(v[u]);
    }
    for (; px < hw; px += PGS) f(*(const half8*)(xi + (long long)px * c));
}

__global__ __launch_bounds__(256) void any_norm_f16_kernel(f16* x, int hw, int c, const float* __restrict__ in_gamma,
                                                           const float* __restrict__ in_beta) {
    __shared__ double red[16 * 16];
    const int img = blockIdx.y;
    const int oct = threadIdx.x & (OCTS - 1), pg = threadIdx.x >> 2;
    const int ch = blockIdx.x * 32 + oct * 8;
    f16* xi = x + (long long)img * hw * c + ch;
    double s[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = 0.0;
    walk_pixels(xi, hw, c, pg, [&](const half8 v) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const double d = (double)(float)v[e];
            s[e] += d;
            s[8 + e] += d * d;
        }
    });
    oct_totals<16>(s, red);
    float a[8], b[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const double mean = s[e] / hw;
        double var = s[8 + e] / hw - mean * mean;
        if (var < 0.0) var = 0.0;
        const double inv = 1.0 / sqrt(var + 1e-5);
        a[e] = (float)(inv * (double)in_gamma[ch + e]);
        b[e] = (float)((double)in_beta[ch + e] - mean * inv * (double)in_gamma[ch + e]);
    }
    for (int px = pg; px < hw; px += PGS) {
        half8* ptr = (half8*)(xi + (long long)px * c);
        half8 v = *ptr;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (f16)fmaxf(__builtin_fmaf((float)v[e], a[e], b[e]), 0.f);
        *ptr = v;
    }
}

__global__ __launch_bounds__(256) void any_pool_f16_kernel(const f16* __restrict__ y, int hw, int c, float* __restrict__ pooled) {
    __shared__ double red[8 * 16];
    const int img = blockIdx.y;
    const int oct = threadIdx.x & (OCTS - 1), pg = threadIdx.x >> 2;
    const int ch = blockIdx.x * 32 + oct * 8;
    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    walk_pixels(y + (long long)img * hw * c + ch, hw, c, pg, [&](const half8 v) {
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += (double)(float)v[e];
    });
    oct_totals<8>(s, red);
    if (pg == 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) pooled[(long long)img * c + ch + e] = (float)(s[e] / hw);
    }
}

__device__ __forceinline__ float wave_total(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// grid (slices, images): every block forms its image's gate (a few thousand multiply-adds), then streams rows [blockIdx.x * rows, + rows).
// out may be y: a thread reads the elements it writes before it writes them and no other thread touches them.
__global__ __launch_bounds__(256) void any_se_tail_f16_kernel(const float* __restrict__ pooled_g, int c, int mid, int hw, int rows,
                                                              const float* __restrict__ w1, const float* __restrict__ w2t, const f16* y,
                                                              const f16* __restrict__ sc, f16* out, float* __restrict__ gate_out) {
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
        const float gg = 1.0f / (1.0f + expf(-acc));
        gate[ch] = gg;
        if (gate_out && blockIdx.x == 0) gate_out[(long long)img * c + ch] = gg;
    }
    __syncthreads();
    const int c8n = c >> 3;
    const int r0 = blockIdx.x * rows;
    const int nrows = min(rows, hw - r0);
    if (nrows <= 0) return;
    const long long base = ((long long)img * hw + r0) * c;
    const int total8 = nrows * c8n;
    const int cc = tid % c8n;   // 256 % c8n == 0 (c = 64 .. 512 in powers of two): a thread keeps its channel octet
    float gt[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) gt[e] = gate[cc * 8 + e];
    auto finish = [&](const half8 yy, const half8 rr, long long off) {
        half8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (f16)fmaxf(__builtin_fmaf(gt[e], (float)yy[e], (float)rr[e]), 0.f);
        *(half8*)(out + off) = o;
    };
    int i = tid;
    for (; i + 3 * 256 < total8; i += 4 * 256) {
        half8 yy[4], rr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            yy[u] = *(const half8*)(y + base + (long long)(i + u * 256) * 8);
            rr[u] = *(const half8*)(sc + base + (long long)(i + u * 256) * 8);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) finish(yy[u], rr[u], base + (long long)(i + u * 256) * 8);
    }
    for (; i < total8; i += 256) {
        const long long off = base + (long long)i * 8;
        finish(*(const half8*)(y + off), *(const half8*)(sc + off), off);
    }
}

// x^p for a trained p as any_gem_kernel (anysize.hip) forms it
__global__ __launch_bounds__(256) void any_gem_f16_kernel(const f16* __restrict__ x, int hw, int c, const float* __restrict__ p_ptr,
                                                          const float* __restrict__ scale, const float* __restrict__ shift,
                                                          float* __restrict__ gem_out, float* __restrict__ emb) {
    __shared__ double red[8 * 16];
    const int img = blockIdx.y;
    const int oct = threadIdx.x & (OCTS - 1), pg = threadIdx.x >> 2;
    const int ch = blockIdx.x * 32 + oct * 8;
    const float p = p_ptr[0];
    const bool cube = p == 3.0f;
    auto powp = [&](float f) {
        const float e = p * __builtin_amdgcn_logf(f);
        return e < -126.f ? __builtin_amdgcn_exp2f(e + 64.f) * 0x1p-64f : __builtin_amdgcn_exp2f(e);
    };
    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    walk_pixels(x + (long long)img * hw * c + ch, hw, c, pg, [&](const half8 v) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float f = fmaxf((float)v[e], 1e-6f);
            s[e] += (double)(cube ? f * f * f : powp(f));
        }
    });
    oct_totals<8>(s, red);
    if (pg == 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float m = (float)(s[e] / hw);
            const float gm = cube ? cbrtf(m) : powf(m, 1.0f / p);
            if (gem_out) gem_out[(long long)img * c + ch + e] = gm;
            emb[(long long)img * c + ch + e] = __builtin_fmaf(gm, scale[ch + e], shift[ch + e]);
        }
    }
}

inline bool shape_ok(int n, int hw, int c) { return n >= 1 && n <= 65535 && hw >= 1 && c >= 64 && c <= 512 && (c & (c - 1)) == 0; }

}  // namespace

extern "C" hipError_t anysize_f16_conv(hipStream_t stream, const _Float16* x, int n, int h, int w, int cin, const _Float16* w16, int cout, int r,
                                       int stride, int pad, const float* scale, const float* shift, const _Float16* residual, int relu,
                                       int relu_from, _Float16* out, int* form_out) {
    if (!x || !w16 || !out || n < 1 || h < 1 || w < 1 || cin < 32 || cin > 512 || cin % 32 || cout < 64 || cout > 512 || cout % 64 ||
        !((r == 3 && pad == 1) || (r == 1 && pad == 0)) || (stride != 1 && stride != 2) || (scale == nullptr) != (shift == nullptr) ||
        relu_from < 0)
        return hipErrorInvalidValue;
    ConvParams p;
    p.x = x; p.w = w16; p.scale = scale; p.shift = shift; p.residual = residual; p.out = out;
    p.H = h; p.W = w; p.Cin = cin; p.Cout = cout; p.R = r; p.stride = stride; p.pad = pad;
    p.Ho = (h + 2 * pad - r) / stride + 1;
    p.Wo = (w + 2 * pad - r) / stride + 1;
    const long long M = (long long)n * p.Ho * p.Wo;
    if (M >= (1ll << 31) - BM) return hipErrorInvalidValue;   // a row index is an int in the kernel (element offsets are 64-bit)
    p.M = (int)M;
    p.relu = relu; p.relu_from = relu_from;
    // the tile form is a rule of the geometry alone: 64 output channels take the 64-wide tile, every wider layer the 128-wide one
    const int bn = cout % 128 ? 64 : 128;
    p.ntn = cout / bn;
    const long long blocks = (M + BM - 1) / BM * p.ntn;
    if (blocks >= (1ll << 31)) return hipErrorInvalidValue;
    if (bn == 64) hipLaunchKernelGGL(any_conv_f16_kernel<64>, dim3((unsigned)blocks), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(any_conv_f16_kernel<128>, dim3((unsigned)blocks), dim3(256), 0, stream, p);
    if (form_out) *form_out = bn == 64 ? ANYSIZE_F16_FORM_128x64 : ANYSIZE_F16_FORM_128x128;
    return hipGetLastError();
}

extern "C" hipError_t anysize_f16_stem(hipStream_t stream, const float* x, int n, int h, int w, const _Float16* w16, const float* scale,
                                       const float* shift, _Float16* out) {
    if (!x || !w16 || !scale || !shift || !out || n < 1 || h < 1 || w < 1) return hipErrorInvalidValue;
    const int H1 = (h - 1) / 2 + 1, W1 = (w - 1) / 2 + 1;
    const long long M = (long long)n * H1 * W1;
    if (M >= (1ll << 31) - SBM * STILES) return hipErrorInvalidValue;
    const long long blocks = (M + SBM * STILES - 1) / (SBM * STILES);
    hipLaunchKernelGGL(any_stem_f16_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, w16, scale, shift, out, (int)M, h, w, H1, W1);
    return hipGetLastError();
}

extern "C" hipError_t anysize_f16_maxpool(hipStream_t stream, const _Float16* x, int n, int h, int w, int c, _Float16* out) {
    if (!x || !out || n < 1 || h < 1 || w < 1 || c < 8 || c % 8) return hipErrorInvalidValue;
    const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
    const long long total = (long long)n * ho * wo * (c / 8);
    long long grid = (total + 255) / 256;
    if (grid > 16384) grid = 16384;
    hipLaunchKernelGGL(any_maxpool_f16_kernel, dim3((unsigned)grid), dim3(256), 0, stream, x, total, h, w, c / 8, ho, wo, out);
    return hipGetLastError();
}

extern "C" hipError_t anysize_f16_norm(hipStream_t stream, _Float16* x, int n, int hw, int c, int half, const float* in_gamma,
                                       const float* in_beta) {
    if (!x || !shape_ok(n, hw, c) || half < 32 || half > c || half % 32 || !in_gamma || !in_beta) return hipErrorInvalidValue;
    hipLaunchKernelGGL(any_norm_f16_kernel, dim3(half / 32, n), dim3(256), 0, stream, x, hw, c, in_gamma, in_beta);
    return hipGetLastError();
}

extern "C" hipError_t anysize_f16_se_tail(hipStream_t stream, const _Float16* y, const _Float16* shortcut, int n, int hw, int c, int mid,
                                          const float* w1, const float* w2t, float* pooled, _Float16* out, float* gate_out) {
    if (!y || !shortcut || !w1 || !w2t || !pooled || !out || !shape_ok(n, hw, c) || mid < 1 || mid > 64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(any_pool_f16_kernel, dim3(c / 32, n), dim3(256), 0, stream, y, hw, c, pooled);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // ~8192 16-byte chunks per block: the gate (2 mid c multiply-adds and as many weights from L2) stays a small part of a block's work
    long long slices = ((long long)hw * (c / 8) + 8191) / 8192;
    if (slices > hw) slices = hw;
    if (slices > 65535) slices = 65535;
    const int rows = (int)((hw + slices - 1) / slices);
    hipLaunchKernelGGL(any_se_tail_f16_kernel, dim3((hw + rows - 1) / rows, n), dim3(256), 0, stream, pooled, c, mid, hw, rows, w1, w2t, y,
                       shortcut, out, gate_out);
    return hipGetLastError();
}

extern "C" hipError_t anysize_f16_gem(hipStream_t stream, const _Float16* x, int n, int hw, int c, const float* p, const float* scale,
                                      const float* shift, float* gem_out, float* emb) {
    if (!x || !p || !scale || !shift || !emb || !shape_ok(n, hw, c)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(any_gem_f16_kernel, dim3(c / 32, n), dim3(256), 0, stream, x, hw, c, p, scale, shift, gem_out, emb);
    return hipGetLastError();
}
