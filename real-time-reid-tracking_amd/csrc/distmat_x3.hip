// libreid_hip_distmat_x3.so: the N x M distance matrix in the fp32-class arithmetic (distmat_x3.h), reid/losses/utils.py:12-35.
//
// One kernel, dist_x3_kernel<BN>, with the structure of any_conv_x3_kernel (anysize_x3.hip): 256 threads = 4 waves (2 query halves x 2
// gallery halves), a 128-query x BN-gallery output tile, K walked in steps of 32 columns.  Rows >= m of x and >= n of y load zeros and
// store nothing; the rows are zero-padded to a multiple of 32 columns by the caller, so the kernel has no K tail.
//
// Arithmetic (unchanged): xh = f16_rn(x), xl' = f16_rn((x - xh) 2^11), yh = f16_rn(y), yq = f16(yh 2^11),
// yl' = f16_rn((y - yh) 2^11), and per K step three v_mfma_f32_16x16x32_f16 products into ONE fp32 accumulator in the fixed order xh.yq,
// xl'.yh, xh.yl'; the 2^-11 is applied once in the epilogue.  BOTH operands are split by the loader, from the registers the fp32 loads land
// in, on their way into LDS (cvt_f16_rn: one conversion of a materialised fp32 value; x - xh, y - yh and the products with 2^11 are exact,
// so each part is rounded once, and f16 subnormals survive - the conversion and the MFMA do not flush them).  No launch splits K and the k
// order of an output element does not depend on the tile it falls into: out[i][j] has the same bits whatever m, n or its position.
//
// LDS, per stage: A = [xh | xl'] 2 x 128 rows x 64 B (16 KB), B = [yq | yh | yl'] 3 x BN rows x 64 B (12 / 24 KB); two stages, one
// barrier per K step: the loads of step k + 1 are issued before the MFMAs of step k and split + written to the other stage after them.
// A row is 32 f16 = four 16-byte chunks; chunk g of row r sits at chunk g ^ ((r >> 2) & 3), so the 16 rows of a fragment read
// (ds_read_b128, same chunk in every row) cover the 16 slots of the 256-byte bank row once.  The gallery is the MFMA's first operand and
// the queries its second, so a lane ends with four consecutive output columns of one query row: 16-byte stores where n % 4 == 0.
#include "distmat_x3.h"
#include "../../include/reid_hip.h"   // REID_METRIC_*
#include "lin_math.h"                 // cvt_f16_rn
#include "reid_internal.h"            // range_acc / range_raise: the helper of every split site; l2sqr_of: the one form of |x - y|^2

namespace {

typedef _Float16 f16;
typedef f16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct DistX3Params {
    const float* x;
    const float* y;
    const float* xx;   // squared row norms of x / y (null for DOT)
    const float* yy;
    float* out;
    int* fault;
    int m, n, ld, metric;
    int ntn;   // gallery tiles: blockIdx.x = query tile * ntn + gallery tile
    int vec;   // n % 4 == 0 and out 16-byte aligned: a lane's four columns leave as one 16-byte store
};

constexpr int BM = 128;
constexpr int ROWB = 64;   // bytes of a 32-column f16 row

template <int BN>
__global__ __launch_bounds__(256, 2) void dist_x3_kernel(const DistX3Params p) {
    constexpr int A_BYTES = 2 * BM * ROWB;
    constexpr int B_BYTES = 3 * BN * ROWB;
    constexpr int STAGE = A_BYTES + B_BYTES;
    constexpr int NBR = BN / 64;   // gallery rows per thread and step (8 columns of each)
    constexpr int NT = BN / 32;    // 16-column MFMA tiles per wave
    __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int g = lane >> 4, r16 = lane & 15;
    const int m0 = (int)(blockIdx.x / p.ntn) * BM;
    const int n0 = (int)(blockIdx.x % p.ntn) * BN;
    const int nk = p.ld >> 5;

    // ---- loader state: A = two query rows x 8 columns, B = NBR gallery rows x 8 columns
    const int ac = tid & 3;
    const float* a_src[2];
    int a_lds[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = (tid >> 2) + 64 * i;
        a_lds[i] = row * ROWB + ((ac ^ ((row >> 2) & 3)) << 4);
        a_src[i] = m0 + row < p.m ? p.x + (long long)(m0 + row) * p.ld + ac * 8 : nullptr;
    }
    const float* b_src[NBR];
    int b_lds[NBR];
#pragma unroll
    for (int j = 0; j < NBR; ++j) {
        const int row = (tid >> 2) + 64 * j;
        b_lds[j] = A_BYTES + row * ROWB + ((ac ^ ((row >> 2) & 3)) << 4);
        b_src[j] = n0 + row < p.n ? p.y + (long long)(n0 + row) * p.ld + ac * 8 : nullptr;
    }

    f32x4 av[2][2], bv[NBR][2];
    unsigned xmax = 0u, ymax = 0u;
    int kb = 0;   // the step the next gload() fetches
    auto gload = [&]() {
        const int k0 = kb << 5;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (a_src[i]) {
                av[i][0] = *(const f32x4*)(a_src[i] + k0);
                av[i][1] = *(const f32x4*)(a_src[i] + k0 + 4);
            } else {
                av[i][0] = f32x4{0.f, 0.f, 0.f, 0.f};
                av[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int j = 0; j < NBR; ++j) {
            if (b_src[j]) {
                bv[j][0] = *(const f32x4*)(b_src[j] + k0);
                bv[j][1] = *(const f32x4*)(b_src[j] + k0 + 4);
            } else {
                bv[j][0] = f32x4{0.f, 0.f, 0.f, 0.f};
                bv[j][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        ++kb;
    };
    auto lstore = [&](char* st) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            half8 hi, lo;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = av[i][j >> 2][j & 3];
                xmax = range_acc(xmax, v);
                hi[j] = cvt_f16_rn(v);
                lo[j] = cvt_f16_rn((v - (float)hi[j]) * 2048.0f);
            }
            *(half8*)(st + a_lds[i]) = hi;
            *(half8*)(st + BM * ROWB + a_lds[i]) = lo;
        }
#pragma unroll
        for (int i = 0; i < NBR; ++i) {
            half8 q, hi, lo;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = bv[i][j >> 2][j & 3];
                ymax = range_acc(ymax, v * 2048.0f);   // the gallery side carries the 2^11: |y| 2^11 has to stay inside f16
                hi[j] = cvt_f16_rn(v);
                q[j] = cvt_f16_rn((float)hi[j] * 2048.0f);
                lo[j] = cvt_f16_rn((v - (float)hi[j]) * 2048.0f);
            }
            *(half8*)(st + b_lds[i]) = q;
            *(half8*)(st + BN * ROWB + b_lds[i]) = hi;
            *(half8*)(st + 2 * BN * ROWB + b_lds[i]) = lo;
        }
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
            const half8 yq = *(const half8*)(st + b_frag + nt * 16 * ROWB);
            const half8 yh = *(const half8*)(st + BN * ROWB + b_frag + nt * 16 * ROWB);
            const half8 yl = *(const half8*)(st + 2 * BN * ROWB + b_frag + nt * 16 * ROWB);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(yq, xh[mt], acc[mt][nt], 0, 0, 0);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(yh, xl[mt], acc[mt][nt], 0, 0, 0);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(yl, xh[mt], acc[mt][nt], 0, 0, 0);
        }
        if (more) lstore(lds + ((ks + 1) & 1) * STAGE);
        __syncthreads();
    }
    range_raise(p.fault, xmax);
    range_raise(p.fault, ymax);

    // ---- epilogue: a lane holds columns co .. co + 3 of query row mr; the metric formulas are gemm_f32_dma.hip's, on dot = acc 2^-11
    const int metric = p.metric;
    const bool cosine = metric == REID_METRIC_COS_HALF || metric == REID_METRIC_COS;
    float rs[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int mr = m0 + wm * 64 + mt * 16 + r16;
        rs[mt] = (p.xx && mr < p.m) ? p.xx[mr] : 0.f;
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int co = n0 + wn * (BN / 2) + nt * 16 + g * 4;
        if (co >= p.n) continue;
        float cq[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            cq[e] = (p.yy && co + e < p.n) ? p.yy[co + e] : 0.f;
            if (cosine) cq[e] = sqrtf(cq[e]);
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int mr = m0 + wm * 64 + mt * 16 + r16;
            if (mr >= p.m) continue;
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float t = acc[mt][nt][e] * (1.0f / 2048.0f);
                if (metric == REID_METRIC_L2) t = sqrtf(fmaxf(l2sqr_of(t, rs[mt], cq[e]), 1e-12f));
                else if (metric == REID_METRIC_L2SQR) t = l2sqr_of(t, rs[mt], cq[e]);
                else if (metric == REID_METRIC_COS_HALF) t = (1.0f - t / (sqrtf(rs[mt]) * cq[e])) / 2.0f;
                else if (metric == REID_METRIC_COS) t = 1.0f - t / (sqrtf(rs[mt]) * cq[e]);
                v[e] = t;
            }
            float* dst = p.out + (long long)mr * p.n + co;
            if (p.vec) {
                *(f32x4*)dst = v;   // n % 4 == 0 and co % 4 == 0: co < n puts co + 3 inside the row
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (co + e < p.n) dst[e] = v[e];
            }
        }
    }
}

}  // namespace

extern "C" hipError_t distmat_x3(hipStream_t stream, const float* x, int m, const float* y, int n, int ld, const float* xx, const float* yy,
                                 int metric, float* out, int* fault, int* form_out) {
    if (!x || !y || !out || m < 1 || n < 1 || ld < 32 || ld % 32 || ((uintptr_t)x & 15) || ((uintptr_t)y & 15) || metric < REID_METRIC_L2 ||
        metric > REID_METRIC_DOT || ((metric != REID_METRIC_DOT) && (!xx || !yy)))
        return hipErrorInvalidValue;
    if (m >= (1ll << 31) - BM || n >= (1ll << 31) - BM) return hipErrorInvalidValue;   // a row index is an int in the kernel (element offsets are 64-bit)
    DistX3Params p;
    p.x = x; p.y = y; p.out = out; p.fault = fault;
    p.xx = metric == REID_METRIC_DOT ? nullptr : xx;
    p.yy = metric == REID_METRIC_DOT ? nullptr : yy;
    p.m = m; p.n = n; p.ld = ld; p.metric = metric;
    p.vec = n % 4 == 0 && ((uintptr_t)out & 15) == 0;
    // the tile form is a rule of n alone: up to 64 gallery rows take the 64-wide tile (half the LDS, no MFMA on columns that do not exist),
    // every wider gallery the 128-wide one.  The bits of an element are the same in both.
    const int bn = n <= 64 ? 64 : 128;
    p.ntn = (n + bn - 1) / bn;
    const long long blocks = ((long long)m + BM - 1) / BM * p.ntn;
    if (blocks >= (1ll << 31)) return hipErrorInvalidValue;
    if (bn == 64) hipLaunchKernelGGL(dist_x3_kernel<64>, dim3((unsigned)blocks), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(dist_x3_kernel<128>, dim3((unsigned)blocks), dim3(256), 0, stream, p);
    if (form_out) *form_out = bn == 64 ? DISTMAT_X3_FORM_128x64 : DISTMAT_X3_FORM_128x128;
    return hipGetLastError();
}
