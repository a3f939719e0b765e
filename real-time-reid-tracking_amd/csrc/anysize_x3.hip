// libreid_hip_anysize_x3.so: the trunk convolutions of the any-size ResNet18-IBN-SE forward in the fp32-class arithmetic (anysize_x3.h).
//
// One implicit-GEMM kernel, any_conv_x3_kernel<BN>: 256 threads = 4 waves (2 pixel halves x 2 channel halves), a 128-pixel x BN-channel
// output tile, K walked tap by tap in steps of 32 input channels.  A GEMM row is one output pixel, decoded to (image, oy, ox) by division
// once per thread (a 128-row tile may cross image borders, rows >= M load zeros and store nothing), padding taps read as zero.
//
// Arithmetic (unchanged): xh = f16_rn(x), xl' = f16_rn((x - xh) 2^11), weights [wh 2^11 | wh | wl'] f16, and per K step
// three v_mfma_f32_16x16x32_f16 products into ONE fp32 accumulator in the fixed order xh.(wh 2^11), xl'.wh, xh.wl'; the 2^-11 goes into the
// BN scale of the epilogue.  The activations are split by the loader, from the registers the fp32 loads land in, on their way into LDS
// (cvt_f16_rn: one conversion - v_cvt_f16_f32 or gfx950's v_cvt_pk_f16_f32 - of a materialised fp32 value, never a fused v_fma_mixlo_f16;
// x - xh and the product with 2^11 are exact, so each part is rounded once, and
// f16 subnormals survive in both - the conversion and the MFMA do not flush them).  No launch splits K and the k order of an output element
// does not depend on the tile it falls into: the bits of an image do not depend on the pass.
//
// LDS, per stage: A = [xh | xl'] 2 x 128 rows x 64 B (16 KB), B = three weight tiles 3 x BN rows x 64 B (12 / 24 KB); two stages, one
// barrier per K step: the loads of step k + 1 are issued before the MFMAs of step k and written to the other stage after them.  A row is
// 32 f16 = four 16-byte chunks; chunk g of row r sits at chunk g ^ ((r >> 2) & 3), so the 16 rows of a fragment read (ds_read_b128, same
// chunk in every row) cover the 16 slots of the 256-byte bank row once.  The weights are the MFMA's first operand and the pixels its
// second, so a lane ends with four consecutive output channels of one pixel: 16-byte stores, scale / shift / residual as 16-byte loads.
#include "anysize_x3.h"
#include "lin_math.h"        // cvt_f16_rn
#include "reid_internal.h"   // range_acc / range_raise: the helper of every split site

namespace {

typedef _Float16 f16;
typedef f16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct X3Params {
    const float* x;
    const f16* w16;
    const float* scale;
    const float* shift;
    const float* residual;
    float* out;
    int* fault;
    int M, H, W, Cin, Cout, Ho, Wo, R, stride, pad;
    int ldtap;   // f16 elements between the taps of one output channel (terms * Cin)
    int relu, relu_from;
    int ntn;     // channel tiles (Cout / BN): blockIdx.x = pixel tile * ntn + channel tile
};

constexpr int BM = 128;
constexpr int ROWB = 64;   // bytes of a 32-channel f16 row

template <int BN>
__global__ __launch_bounds__(256, 2) void any_conv_x3_kernel(const X3Params p) {
    constexpr int A_BYTES = 2 * BM * ROWB;
    constexpr int B_BYTES = 3 * BN * ROWB;
    constexpr int STAGE = A_BYTES + B_BYTES;
    constexpr int NB = BN * 12 / 256;   // 16-byte weight chunks per thread and step
    constexpr int NT = BN / 32;         // 16-channel MFMA tiles per wave
    __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int g = lane >> 4, r16 = lane & 15;
    const int m0 = (int)(blockIdx.x / p.ntn) * BM;
    const int n0 = (int)(blockIdx.x % p.ntn) * BN;
    const int cpb = p.Cin >> 5;
    const int nk = p.R * p.R * cpb;

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
        const int ch = idx & 3, rest = idx >> 2;
        const int part = rest % 3, co = rest / 3;
        b_src[j] = (n0 + co) * (p.R * p.R * p.ldtap) + part * p.Cin + ch * 8;
        b_lds[j] = A_BYTES + (part * BN + co) * ROWB + ((ch ^ ((co >> 2) & 3)) << 4);
    }

    f32x4 av[2][2];
    half8 bv[NB];
    unsigned vmax = 0u;
    int tap = 0, cb = 0;   // the step the next gload() fetches
    auto gload = [&]() {
        const int ty = tap / p.R, tx = tap - ty * p.R;
        const int c0 = cb << 5;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int iy = iy0[i] + ty, ix = ix0[i] + tx;
            if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) {
                const float* src = p.x + (pix0[i] + (long long)iy * p.W + ix) * p.Cin + c0 + ac * 8;
                av[i][0] = *(const f32x4*)src;
                av[i][1] = *(const f32x4*)(src + 4);
            } else {
                av[i][0] = f32x4{0.f, 0.f, 0.f, 0.f};
                av[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        const int boff = tap * p.ldtap + c0;
#pragma unroll
        for (int j = 0; j < NB; ++j) bv[j] = *(const half8*)(p.w16 + b_src[j] + boff);
        if (++cb == cpb) {
            cb = 0;
            ++tap;
        }
    };
    auto lstore = [&](char* st) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            half8 hi, lo;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = av[i][j >> 2][j & 3];
                vmax = range_acc(vmax, v);
                hi[j] = cvt_f16_rn(v);
                lo[j] = cvt_f16_rn((v - (float)hi[j]) * 2048.0f);
            }
            *(half8*)(st + a_lds[i]) = hi;
            *(half8*)(st + BM * ROWB + a_lds[i]) = lo;
        }
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
        half8 xh[4], xl[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            xh[mt] = *(const half8*)(st + a_frag + mt * 16 * ROWB);
            xl[mt] = *(const half8*)(st + BM * ROWB + a_frag + mt * 16 * ROWB);
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const half8 wq = *(const half8*)(st + b_frag + nt * 16 * ROWB);
            const half8 wh = *(const half8*)(st + BN * ROWB + b_frag + nt * 16 * ROWB);
            const half8 wl = *(const half8*)(st + 2 * BN * ROWB + b_frag + nt * 16 * ROWB);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wq, xh[mt], acc[mt][nt], 0, 0, 0);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xl[mt], acc[mt][nt], 0, 0, 0);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, xh[mt], acc[mt][nt], 0, 0, 0);
        }
        if (more) lstore(lds + ((ks + 1) & 1) * STAGE);
        __syncthreads();
    }
    range_raise(p.fault, vmax);

    // ---- epilogue: a lane holds channels co .. co + 3 of pixel m
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int co = n0 + wn * (BN / 2) + nt * 16 + g * 4;
        f32x4 cs = f32x4{1.f, 1.f, 1.f, 1.f}, sh = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p.scale) {
            cs = *(const f32x4*)(p.scale + co);
            sh = *(const f32x4*)(p.shift + co);
        }
        cs *= 1.0f / 2048.0f;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int m = m0 + wm * 64 + mt * 16 + r16;
            if (m >= p.M) continue;
            const long long idx = (long long)m * p.Cout + co;
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(acc[mt][nt][e], cs[e], sh[e]);
            if (p.residual) v += *(const f32x4*)(p.residual + idx);
            if (p.relu) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (co + e >= p.relu_from) v[e] = fmaxf(v[e], 0.f);
            }
            *(f32x4*)(p.out + idx) = v;
        }
    }
}

}  // namespace

extern "C" hipError_t anysize_x3_conv(hipStream_t stream, const float* x, int n, int h, int w, int cin, const _Float16* w16, int terms, int cout,
                                      int r, int stride, int pad, const float* scale, const float* shift, const float* residual, int relu,
                                      int relu_from, float* out, int* fault, int* form_out) {
    if (!x || !w16 || !out || n < 1 || h < 1 || w < 1 || cin < 32 || cin > 512 || cin % 32 || cout < 64 || cout > 512 || cout % 64 ||
        !((r == 3 && pad == 1) || (r == 1 && pad == 0)) || (stride != 1 && stride != 2) || (terms != 3 && terms != 4) ||
        (scale == nullptr) != (shift == nullptr) || relu_from < 0)
        return hipErrorInvalidValue;
    X3Params p;
    p.x = x; p.w16 = w16; p.scale = scale; p.shift = shift; p.residual = residual; p.out = out; p.fault = fault;
    p.H = h; p.W = w; p.Cin = cin; p.Cout = cout; p.R = r; p.stride = stride; p.pad = pad;
    p.Ho = (h + 2 * pad - r) / stride + 1;
    p.Wo = (w + 2 * pad - r) / stride + 1;
    const long long M = (long long)n * p.Ho * p.Wo;
    if (M >= (1ll << 31) - BM) return hipErrorInvalidValue;   // a row index is an int in the kernel (element offsets are 64-bit)
    p.M = (int)M;
    p.ldtap = terms * cin;
    p.relu = relu; p.relu_from = relu_from;
    // the tile form is a rule of the geometry alone: 64 output channels take the 64-wide tile, every wider layer the 128-wide one
    const int bn = cout % 128 ? 64 : 128;
    p.ntn = cout / bn;
    const long long blocks = (M + BM - 1) / BM * p.ntn;
    if (blocks >= (1ll << 31)) return hipErrorInvalidValue;
    if (bn == 64) hipLaunchKernelGGL(any_conv_x3_kernel<64>, dim3((unsigned)blocks), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(any_conv_x3_kernel<128>, dim3((unsigned)blocks), dim3(256), 0, stream, p);
    if (form_out) *form_out = bn == 64 ? ANYSIZE_X3_FORM_128x64 : ANYSIZE_X3_FORM_128x128;
    return hipGetLastError();
}
