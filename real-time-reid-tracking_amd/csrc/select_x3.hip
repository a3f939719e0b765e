// libreid_hip_select_x3.so: rank-exact arg-min (reid/evaluate.py:58-63) and k-NN (reid/faiss_utils.py:56-139) with the candidates from the
// fp32-class arithmetic (select_x3.h).  The answer is the exact entries' bit for bit; the f16 matrix pipe only decides WHICH columns the
// exact arithmetic looks at, and a proof per row says when that was enough.
//
//   1. cand_x3_kernel<BN, MODE_BOUND> on a sample, the first max(512, n / 16) columns (all n of them where that is more): the arithmetic of dist_x3_kernel (distmat_x3.hip - the loader, the
//      LDS layout and the K loop are copied from there: both fp32 operands split to f16 parts on their way into LDS, three
//      v_mfma_f32_16x16x32_f16 products per 32 columns into ONE fp32 accumulator in the order xh.yq, xl'.yh, xh.yl', K never split, no packed
//      operand in HBM).  The epilogue keeps per row the minimum of each of 128 column groups (column mod 128).  thr_kernel takes the
//      KK-th smallest group minimum as the row's threshold thr0: at least KK columns lie at or below it.
//   2. cand_x3_kernel<BN, MODE_LIST> on all n columns: the same arithmetic (an element has the same bits in both launches: its k order
//      depends on ld alone).  No tile is stored: its keys at or below thr0 go to LDS, and one wave per row writes them - at most C = KK
//      per row and tile - to the workspace [m][column tiles][C] with their count.  Up to C keys leave in column order (a ballot and two
//      popcounts); of more, the C smallest by (value, column) leave in that order (ranked by counting: the rare path), so the list's
//      last key bounds every key of the tile it left out.  The row's KK smallest values are therefore always listed.
//   3. merge_kernel (one block per row): the KK best keys over all tiles by (value, column) - pack_key's order, ties to the lower
//      column; a second threshold of the same kind as thr0 first cuts the listed keys down to a few dozen - and the row's threshold T,
//      the smallest value a non-candidate can have: the minimum of thr0 (a column the filter dropped lies above it), of the last key of
//      every tile list that left keys out, and of the first key the merge dropped.  T is never below the row's KK-th smallest value.
//   4. refine_kernel: the candidates' distances in EXACT fp32 - an fmaf chain in the k order of the fp32 MFMA loops (gemm_f32.hip,
//      gemm_f32_dma.hip, dist_select.hip: per eight columns k = 0, 4, 1, 5, 2, 6, 3, 7; zero columns add nothing, so the exact entries'
//      different row padding gives the same bits) through the metric formulas of gemm_f32_dma.hip - and the k smallest by (value, index).
//      Proof: with B >= |fp32-class value - exact value| for the row (bound_of: a closed form of ld, |x_i|^2, max |y|^2 and, for the
//      cosine metrics, min |y|^2), every non-candidate's exact value is >= T - B; the row is proven when its k-th exact value is STRICTLY
//      below that.  REID_METRIC_L2: candidates, T and B live on the squared distance and the comparison is made after the same clamp and
//      sqrtf the answer went through (a monotone map), strictly - two different squares can share a root, and then the column decides.
//   5. exact_row_kernel: a row that is not proven (or that a test forces) is recomputed from all n columns in the same exact arithmetic.
// Launches are ordered by the stream alone: no block waits for, counts or signals another.
#include "select_x3.h"
#include "../../include/reid_hip.h"   // REID_METRIC_*
#include "lin_math.h"                 // cvt_f16_rn
#include "reid_internal.h"            // range_acc / range_raise, l2sqr_of, l2_of_sqr
#include <math.h>

namespace {

typedef _Float16 f16;
typedef f16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int BM = 128;
constexpr int ROWB = 64;                 // bytes of a 32-column f16 row
constexpr int KK = SELECT_X3_KK;         // candidates per row = keys a tile list can hold
constexpr int GROUPS = 128;              // column groups of the threshold pass
constexpr int MODE_BOUND = 0, MODE_LIST = 1;
constexpr int MERGE_CAP = 2048;          // keys a row's merge can hold
constexpr int SURV_CAP = 512;            // ... and how many of them may pass its second threshold
constexpr int ROW_CH = 2048;             // columns per sweep of the exact-row kernel

// ---- keys: knn_wide.hip's order (value ascending with -0 < +0, then column)
__device__ __forceinline__ unsigned key32(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unkey32(unsigned u) {
    u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    return __uint_as_float(u);
}
__device__ __forceinline__ u64 pack_key(float v, int idx) { return ((u64)key32(v) << 32) | (unsigned)idx; }
__device__ __forceinline__ float unpack_val(u64 k) { return unkey32((unsigned)(k >> 32)); }

// A dot product in the order the fp32 MFMA loops accumulate it (knn_wide.hip, mfma_order_dot8): a lane half reads four consecutive k of a
// 16-byte chunk, v_mfma_f32_32x32x2_f32 number e takes element e of the low half's chunk (k = e) and of the high half's (k = 4 + e), and
// the instruction is a two-step fmaf chain: per eight columns k = 0, 4, 1, 5, 2, 6, 3, 7.
// ld % 32 == 0: four groups of eight per step, their sixteen loads issued before the first fmaf (the chain's order is the loop's)
__device__ __forceinline__ float exact_dot(const float* __restrict__ xr, const float* __restrict__ yr, int ld) {
    float dot = 0.f;
    for (int q = 0; q < ld; q += 32) {
        f32x4 a[8], b[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            a[i] = *(const f32x4*)(xr + q + 4 * i);
            b[i] = *(const f32x4*)(yr + q + 4 * i);
        }
#pragma unroll
        for (int i = 0; i < 8; i += 2) {
            dot = fmaf(a[i].x, b[i].x, dot); dot = fmaf(a[i + 1].x, b[i + 1].x, dot);
            dot = fmaf(a[i].y, b[i].y, dot); dot = fmaf(a[i + 1].y, b[i + 1].y, dot);
            dot = fmaf(a[i].z, b[i].z, dot); dot = fmaf(a[i + 1].z, b[i + 1].z, dot);
            dot = fmaf(a[i].w, b[i].w, dot); dot = fmaf(a[i + 1].w, b[i + 1].w, dot);
        }
    }
    return dot;
}
// the metric formulas of gemm_f32_dma.hip's dist_epilogue (rs, cq: squared norms)
__device__ __forceinline__ float exact_of(int metric, float dot, float rs, float cq) {
    if (metric == REID_METRIC_L2) return l2_of_sqr(l2sqr_of(dot, rs, cq));
    if (metric == REID_METRIC_L2SQR) return l2sqr_of(dot, rs, cq);
    if (metric == REID_METRIC_COS_HALF) return (1.0f - dot / (sqrtf(rs) * sqrtf(cq))) / 2.0f;
    if (metric == REID_METRIC_COS) return 1.0f - dot / (sqrtf(rs) * sqrtf(cq));
    return dot;
}

// B >= |fp32-class value - exact value| of one row under `metric` (REID_METRIC_L2: of the SQUARED distance): 1.25 times the sum of the
// two entries' derived bounds (tests/distmat_x3_ref.py, tests/matching_ref.py) with every per-column quantity replaced by its largest
// value over the columns - sum_k |x_k y_k| <= |x| |y| (Cauchy-Schwarz), |y_j|^2 <= ymax, and for the cosine metrics |y_j|^2 >= ymin.
// tests/select_x3_ref.py restates it (bound_closed) and tests/test_select_x3_host.py holds it against both derivations.
__host__ __device__ __forceinline__ float bound_of(int metric, int ld, float X, float ymax, float ymin) {
    const float u = 5.9604645e-8f, u16 = 4.8828125e-4f, a25 = 2.9802322e-8f, a36 = 1.4551915e-11f, tiny = 1.4e-45f;
    const float r = sqrtf((float)ld), nx = sqrtf(X), ny = sqrtf(ymax);
    const float n3 = 3.0f * (float)ld * 1.1920929e-7f, g3 = n3 / (1.0f - n3);
    const float ns = (float)((ld + 63) / 64 + 7) * u, gs = ns / (1.0f - ns);
    const float dm = (float)(ld + 4) * u;
    float sum;
    if (metric == REID_METRIC_COS || metric == REID_METRIC_COS_HALF) {
        const float nymin = sqrtf(ymin), qx = r / nx, qy = r / nymin;
        const float lx = u16 + a25 * qx, dx = u16 * lx + a36 * qx, hx = 1.0f + lx;
        const float ly = u16 + a25 * qy, dy = u16 * ly + a36 * qy, hy = 1.0f + ly;
        const float e3r = dx * hy + hx * dy + lx * ly + g3 * (hx * hy + (lx + dx) * hy + hx * (ly + dy)) + tiny / (nx * nymin);
        const float eta = gs + (1.0f + gs) * (3.0f * u + 3.0f * u * u + u * u * u);   // (1 + gs)(1 + u)^3 - 1 without the cancellation
        const float bq = (eta + e3r) / (1.0f - eta) * (1.0f + u) + u;
        sum = bq + u * (2.0f + bq) + dm * (nx / nymin + ny / nx + 2.0f);
        if (metric == REID_METRIC_COS_HALF) sum *= 0.5f;
    } else {
        const float LX = u16 * nx + a25 * r, DX = u16 * LX + a36 * r, HX = nx + LX;
        const float LY = u16 * ny + a25 * r, DY = u16 * LY + a36 * r, HY = ny + LY;
        const float e3 = DX * HY + HX * DY + LX * LY + g3 * (HX * HY + (LX + DX) * HY + HX * (LY + DY)) + tiny;
        const float s2 = (nx + ny) * (nx + ny);
        if (metric == REID_METRIC_DOT) {
            sum = e3 + dm * nx * ny;
        } else {
            const float b2 = ((gs * (1.0f + u) + u) * (X + ymax) + 2.0f * e3) * (1.0f + u) + u * s2, bm = dm * s2;
            if (metric == REID_METRIC_L2SQR) {
                sum = b2 + bm;
            } else {   // the two derivations bound got^2 against the float64 square: twice the squared bound and the roots' roundings
                const float w = 2.0f * b2 + 2e-12f;
                sum = w + 3.0f * u * (s2 + w) + bm + 3.0f * u * (fmaxf(s2, 1e-12f) + bm);
            }
        }
    }
    return 1.25f * sum;
}

struct SelX3Params {
    const float* x;
    const float* y;
    const float* xx;   // squared row norms of x / y
    const float* yy;
    int* fault;
    int m, n, ld, metric;
    int ntn;                  // gallery tiles of this launch: blockIdx.x = query tile * ntn + gallery tile
    int ntl;                  // gallery tiles of the lists' layout (MODE_LIST: == ntn)
    unsigned* gm;             // MODE_BOUND: [m][GROUPS] group minima (keys), preset to ~0
    const unsigned* thr0;     // MODE_LIST: [m] the row's filter threshold (key)
    u64* lists;               // MODE_LIST: [m][ntl][KK]
    int* counts;              // MODE_LIST: [m][ntl] keys at or below thr0 in the tile (> KK: the list holds KK of them)
};

// The loader, the LDS layout and the K loop of dist_x3_kernel (distmat_x3.hip, which stays as it is: its kernels are pinned); the epilogue
// selects instead of storing.  The candidate value under REID_METRIC_L2 is the squared distance (the clamp and the root are monotone).
template <int BN, int MODE>
__global__ __launch_bounds__(256, 2) void cand_x3_kernel(const SelX3Params p) {
    constexpr int A_BYTES = 2 * BM * ROWB;
    constexpr int B_BYTES = 3 * BN * ROWB;
    constexpr int STAGE = A_BYTES + B_BYTES;
    constexpr int NBR = BN / 64;   // gallery rows per thread and step (8 columns of each)
    constexpr int NT = BN / 32;    // 16-column MFMA tiles per wave
    __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int g = lane >> 4, r16 = lane & 15;
    const int tile = (int)(blockIdx.x % p.ntn);
    const int m0 = (int)(blockIdx.x / p.ntn) * BM;
    const int n0 = tile * BN;
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

    // ---- epilogue: a lane holds columns co .. co + 3 of query row mr; the metric formulas are gemm_f32_dma.hip's, on dot = acc 2^-11.
    // The stage buffers are free after the loop's last barrier: they take the tile's keys, [BM][BN] with a row pitch of BN + 1 words (the 16
    // rows a wave's lanes write at once fall into different banks); ~0 = filtered out, or outside the problem.
    constexpr int TS = BN + 1;
    static_assert(BM * TS * 4 <= 2 * STAGE, "the tile's keys fit the stage buffers");
    unsigned* tk = (unsigned*)lds;
    if (MODE == MODE_LIST) {
        for (int i = tid; i < BM * TS; i += 256) tk[i] = ~0u;
        __syncthreads();
    }
    const int metric = p.metric;
    const bool cosine = metric == REID_METRIC_COS_HALF || metric == REID_METRIC_COS;
    float rs[4];
    unsigned th[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int mr = m0 + wm * 64 + mt * 16 + r16;
        rs[mt] = mr < p.m ? p.xx[mr] : 0.f;
        th[mt] = (MODE == MODE_LIST && mr < p.m) ? p.thr0[mr] : 0u;
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int co = n0 + wn * (BN / 2) + nt * 16 + g * 4;
        if (co >= p.n) continue;
        float cq[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            cq[e] = co + e < p.n ? p.yy[co + e] : 0.f;
            if (cosine) cq[e] = sqrtf(cq[e]);
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int rl = wm * 64 + mt * 16 + r16, mr = m0 + rl;
            if (mr >= p.m) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (co + e >= p.n) continue;
                float t = acc[mt][nt][e] * (1.0f / 2048.0f);
                if (metric == REID_METRIC_L2 || metric == REID_METRIC_L2SQR) t = l2sqr_of(t, rs[mt], cq[e]);
                else if (metric == REID_METRIC_COS_HALF) t = (1.0f - t / (sqrtf(rs[mt]) * cq[e])) / 2.0f;
                else if (metric == REID_METRIC_COS) t = 1.0f - t / (sqrtf(rs[mt]) * cq[e]);
                const unsigned key = key32(t);
                if (MODE == MODE_BOUND) {
                    atomicMin(p.gm + (long long)mr * GROUPS + ((co + e) & (GROUPS - 1)), key);
                } else if (key <= th[mt]) {
                    tk[rl * TS + (co + e - n0)] = key;
                }
            }
        }
    }
    if (MODE == MODE_LIST) {
        // one wave per row: up to KK passing keys leave in column order; of more, the KK smallest by (key, column) leave in that order,
        // so that the list's last key bounds every key of the tile that was left out (merge_kernel reads it where count > KK)
        __syncthreads();
        for (int r = wave; r < BM; r += 4) {
            const int mr = m0 + r;
            if (mr >= p.m) break;
            const unsigned k0 = tk[r * TS + lane], k1 = BN == 128 ? tk[r * TS + 64 + lane] : ~0u;
            const bool p0 = k0 != ~0u, p1 = k1 != ~0u;
            const u64 b0 = __ballot(p0), b1 = __ballot(p1);
            const int c = __popcll(b0) + __popcll(b1);
            u64* dst = p.lists + ((long long)mr * p.ntl + tile) * KK;
            int s0, s1;
            if (c <= KK) {
                const u64 below = (1ull << lane) - 1ull;
                s0 = __popcll(b0 & below);
                s1 = __popcll(b0) + __popcll(b1 & below);
            } else {
                s0 = s1 = 0;
                for (int o = 0; o < BN; ++o) {
                    const unsigned other = tk[r * TS + o];
                    s0 += (other < k0) || (other == k0 && o < lane);
                    s1 += (other < k1) || (other == k1 && o < 64 + lane);
                }
            }
            if (p0 && s0 < KK) dst[s0] = ((u64)k0 << 32) | (unsigned)(n0 + lane);
            if (p1 && s1 < KK) dst[s1] = ((u64)k1 << 32) | (unsigned)(n0 + 64 + lane);
            if (lane == 0) p.counts[(long long)mr * p.ntl + tile] = c;
        }
    }
}

// ---- thr0[row] = the KK-th smallest of the row's GROUPS group minima (by (key, group): ranks are unique); one wave per row.
// Fewer than KK groups with a column: the key ~0, which every value passes.
__global__ __launch_bounds__(256) void thr_kernel(const unsigned* __restrict__ gm, int m, unsigned* __restrict__ thr0) {
    __shared__ unsigned sh[4][GROUPS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + w;
    const bool live = row < m;
    const unsigned a = live ? gm[(long long)row * GROUPS + lane] : ~0u, b = live ? gm[(long long)row * GROUPS + 64 + lane] : ~0u;
    sh[w][lane] = a;
    sh[w][64 + lane] = b;
    __syncthreads();
    int ra = 0, rb = 0;
    for (int o = 0; o < GROUPS; ++o) {
        const unsigned other = sh[w][o];
        ra += (other < a) || (other == a && o < lane);
        rb += (other < b) || (other == b && o < 64 + lane);
    }
    if (live && ra == KK - 1) thr0[row] = a;
    if (live && rb == KK - 1) thr0[row] = b;
}

// ---- the KK best keys of a row over all its tile lists, and T.  One block per row.
__global__ __launch_bounds__(256) void merge_kernel(const u64* __restrict__ lists, const int* __restrict__ counts, int ntl,
                                                    const unsigned* __restrict__ thr0, u64* __restrict__ cand, float* __restrict__ T) {
    __shared__ u64 list[MERGE_CAP];
    __shared__ u64 surv[SURV_CAP];
    __shared__ unsigned gmin2[64], thr2, tilemin;
    __shared__ int cnt, lost, nsurv, wsum[4];
    __shared__ u64 dropped;
    const int row = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) { cnt = 0; lost = 0; nsurv = 0; thr2 = ~0u; tilemin = ~0u; dropped = ~0ull; }
    if (tid < 64) gmin2[tid] = ~0u;
    __syncthreads();
    // a thread's tiles (t, t + 256, ..) land behind those of the threads before it: offsets from a scan, no two threads share a slot
    int mine = 0;
    for (int t = tid; t < ntl; t += 256) {
        const int c = counts[(long long)row * ntl + t];
        // the tile passed more keys than its list holds: the list is its KK smallest in order, and its last bounds the others
        if (c > KK) atomicMin(&tilemin, (unsigned)(lists[((long long)row * ntl + t) * KK + KK - 1] >> 32));
        mine += c > KK ? KK : c;
    }
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if ((tid & 63) >= o) incl += up;
    }
    if ((tid & 63) == 63) wsum[tid >> 6] = incl;
    __syncthreads();
    int s = incl - mine;
    for (int w = 0; w < (tid >> 6); ++w) s += wsum[w];
    if (tid == 255) cnt = s + mine;
    for (int t = tid; t < ntl; t += 256) {
        int c = counts[(long long)row * ntl + t];
        c = c > KK ? KK : c;
        const u64* src = lists + ((long long)row * ntl + t) * KK;
        for (int e = 0; e < c; ++e, ++s)
            if (s < MERGE_CAP) list[s] = src[e];
    }
    __syncthreads();
    const int c = cnt < MERGE_CAP ? cnt : MERGE_CAP;
    // Ranking all c keys against each other is c^2 work (c is about 600 at n / sample = 16).  First a threshold that keeps KK + 1 keys
    // for certain: the (KK + 1)-th smallest of the minima of 64 groups (slot mod 64) has at least KK + 1 keys at or below it.
    if (c > 64) {
        for (int e = tid; e < c; e += 256) atomicMin(&gmin2[e & 63], (unsigned)(list[e] >> 32));
        __syncthreads();
        if (tid < 64) {
            const unsigned v = gmin2[tid];
            int rank = 0;
            for (int o = 0; o < 64; ++o) rank += (gmin2[o] < v) || (gmin2[o] == v && o < tid);
            if (rank == KK) thr2 = v;
        }
        __syncthreads();
    }
    const unsigned t2 = thr2;
    for (int e = tid; e < c; e += 256) {
        const u64 key = list[e];
        if ((unsigned)(key >> 32) <= t2) {
            const int s2 = atomicAdd(&nsurv, 1);
            if (s2 < SURV_CAP) surv[s2] = key;
        }
    }
    __syncthreads();
    if (nsurv > SURV_CAP && tid == 0) lost = 1;                // hundreds of ties at the threshold: the exact-row kernel takes the row
    const int c2 = nsurv < SURV_CAP ? nsurv : SURV_CAP;
    u64* out = cand + (long long)row * KK;
    for (int e = tid; e < c2; e += 256) {
        const u64 me = surv[e];
        int rank = 0;
        for (int o = 0; o < c2; ++o) rank += surv[o] < me;     // keys are unique: they carry the column
        if (rank < KK) out[rank] = me;
        if (rank == KK) dropped = me;                          // the first key the merge leaves out
    }
    for (int e = c2 + tid; e < KK; e += 256) out[e] = ~0ull;
    __syncthreads();
    if (tid == 0) {
        const unsigned tk = thr0[row];
        float t = tk == ~0u ? INFINITY : unkey32(tk);          // a column the filter dropped lies above thr0
        if (dropped != ~0ull) t = fminf(t, unpack_val(dropped));
        if (tilemin != ~0u) t = fminf(t, unkey32(tilemin));     // ... and so does a column its tile's full list left out
        T[row] = (lost || cnt > MERGE_CAP) ? -INFINITY : t;    // nothing is known about a column that was in no list: never proven
    }
}

// ---- exact distances of the candidates, the k smallest of them, and the proof.  64 lanes = two rows x KK candidates.
__global__ __launch_bounds__(256) void refine_kernel(const float* __restrict__ x, const float* __restrict__ y, int ld, const float* __restrict__ xx,
                                                     const float* __restrict__ yy, const float* __restrict__ sc, const u64* __restrict__ cand,
                                                     const float* __restrict__ T, int rows, int row_base, int n, int k, int metric, int force_every,
                                                     float* __restrict__ D, int32_t* __restrict__ I, int* __restrict__ flags) {
    const int lane = threadIdx.x & 63, half = lane >> 5, c = lane & 31;
    const int row = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + half;
    const bool live = row < rows;
    const u64 ak = live ? cand[(long long)row * KK + c] : ~0ull;
    const unsigned idx = (unsigned)(ak & 0xffffffffu);
    const bool valid = live && ak != ~0ull && idx < (unsigned)n;
    const float r2 = live ? xx[row] : 0.f;
    float e = INFINITY;
    if (valid) e = exact_of(metric, exact_dot(x + (long long)row * ld, y + (long long)idx * ld, ld), r2, yy[idx]);
    // an empty slot ranks behind every value, and the empty slots among themselves by their lane: each rank is taken once
    const u64 ek = valid ? pack_key(e, (int)idx) : (0xffffffffffffff00ull | (unsigned)c);
    int rank = 0;
#pragma unroll
    for (int o = 0; o < KK; ++o) {
        const u64 other = __shfl(ek, half * 32 + o);
        rank += other < ek;
    }
    if (live && rank < k) {
        if (D) D[(long long)row * k + rank] = valid ? e : INFINITY;
        I[(long long)row * k + rank] = valid ? (int32_t)idx : -1;
    }
    float vk = (valid && rank == k - 1) ? e : -INFINITY;   // at most one lane of the row holds rank k - 1
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) vk = fmaxf(vk, __shfl_xor(vk, o));
    if (live && c == 0) {
        const float t = T[row];
        bool proven = n <= KK || t == INFINITY;             // every column is a candidate / nothing was dropped anywhere
        if (!proven) {
            float lb = t - bound_of(metric, ld, r2, sc[0], sc[1]);
            lb -= fabsf(lb) * 2.4e-7f;                      // the subtraction's own rounding, downwards
            const float floor_of_rest = metric == REID_METRIC_L2 ? l2_of_sqr(lb) : lb;
            // strictly: a tie with a non-candidate would go to the lower column.  vk = -inf: no valid candidate holds rank k - 1 (cannot
            // happen while both launches of cand_x3_kernel give an element the same bits, which is what puts KK columns at or below
            // thr0) - such a row is not proven
            proven = vk > -INFINITY && vk < floor_of_rest;
        }
        flags[row] = (!proven || (force_every > 0 && (row_base + row) % force_every == 0)) ? 1 : 0;
    }
}

// ---- a flagged row from scratch, one block of 1024 threads per row.  The block streams the whole gallery through one CU: about a
// millisecond at 15913 x 512 whether one row is flagged or a few hundred (measured: DESIGN).  Exact distances to all n columns, ROW_CH at a time, merged with the k best so far by k rounds of
// "smallest key above the last one"
__global__ __launch_bounds__(1024) void exact_row_kernel(const float* __restrict__ x, const float* __restrict__ y, int ld, const float* __restrict__ xx,
                                                        const float* __restrict__ yy, int n, int k, int metric, float* __restrict__ D,
                                                        int32_t* __restrict__ I, const int* __restrict__ flags) {
    const int row = blockIdx.x;
    if (!flags[row]) return;
    __shared__ u64 keys[ROW_CH + SELECT_X3_KMAX];
    __shared__ u64 best[SELECT_X3_KMAX];
    __shared__ u64 sh[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* xr = x + (long long)row * ld;
    const float r2 = xx[row];
    if (tid < k) best[tid] = ~0ull;
    __syncthreads();
    for (int j0 = 0; j0 < n; j0 += ROW_CH) {
        const int c = n - j0 < ROW_CH ? n - j0 : ROW_CH;
        for (int j = tid; j < c; j += 1024)
            keys[j] = pack_key(exact_of(metric, exact_dot(xr, y + (long long)(j0 + j) * ld, ld), r2, yy[j0 + j]), j0 + j);
        if (tid < k) keys[c + tid] = best[tid];
        __syncthreads();
        u64 last = 0;
        for (int r = 0; r < k; ++r) {
            u64 b = ~0ull;
            for (int j = tid; j < c + k; j += 1024) {
                const u64 key = keys[j];
                if ((r == 0 || key > last) && key < b) b = key;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const u64 other = __shfl_xor(b, o);
                b = other < b ? other : b;
            }
            if (lane == 0) sh[wave] = b;
            __syncthreads();
            b = sh[0];
            for (int w = 1; w < 16; ++w) b = sh[w] < b ? sh[w] : b;
            if (tid == 0) best[r] = b;
            last = b;
            __syncthreads();
            if (b == ~0ull) break;     // fewer than r + 1 columns so far (uniform: every thread holds the same b)
        }
        __syncthreads();
    }
    if (tid < k) {
        const u64 b = best[tid];
        if (D) D[(long long)row * k + tid] = b == ~0ull ? INFINITY : unpack_val(b);
        I[(long long)row * k + tid] = b == ~0ull ? -1 : (int32_t)(b & 0xffffffffu);
    }
}

// ---- sc[0] = max |y_j|^2, sc[1] = min |y_j|^2
__global__ __launch_bounds__(1024) void norm_range_kernel(const float* __restrict__ yy, int n, float* __restrict__ sc) {
    __shared__ float sh[2][16];
    float mx = 0.f, mn = INFINITY;
    for (int i = threadIdx.x; i < n; i += 1024) {
        mx = fmaxf(mx, yy[i]);
        mn = fminf(mn, yy[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, o));
        mn = fminf(mn, __shfl_xor(mn, o));
    }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = mx; sh[1][threadIdx.x >> 6] = mn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) {
            mx = fmaxf(mx, sh[0][w]);
            mn = fminf(mn, sh[1][w]);
        }
        sc[0] = mx;
        sc[1] = mn;
    }
}

inline int tile_width(int n) { return n <= 64 ? 64 : 128; }   // the rule of distmat_x3.h
inline size_t row_bytes(int ntl) { return (size_t)ntl * KK * 8 + (size_t)KK * 8 + (size_t)ntl * 4 + GROUPS * 4 + 8; }
constexpr size_t FIXED = 64;   // sc

}  // namespace

// bound_of on the host: the function the device evaluates, for the test that holds it against its numpy restatement
extern "C" float select_x3_bound(int metric, int ld, float xx, float ymax, float ymin) { return bound_of(metric, ld, xx, ymax, ymin); }

extern "C" size_t select_x3_ws_bytes(int m, int n) {
    if (m < 1 || n < 1) return FIXED;
    const int bn = tile_width(n), ntl = (n + bn - 1) / bn;
    const size_t per = row_bytes(ntl);
    size_t rows = (size_t)m;
    if (FIXED + rows * per > SELECT_X3_WS_CAP) {
        rows = (SELECT_X3_WS_CAP - FIXED) / per;
        if (rows < 128) rows = 128;
        if (rows > (size_t)m) rows = (size_t)m;
    }
    return FIXED + rows * per;
}

extern "C" hipError_t select_x3(hipStream_t stream, const float* x, int m, const float* y, int n, int ld, const float* xx, const float* yy,
                                int metric, int k, float* D, int32_t* I, void* ws, size_t ws_bytes, int* fault, int force_every, int* flags,
                                int* form_out) {
    if (!x || !y || !xx || !yy || !I || !ws || !flags || m < 1 || n < 1 || ld < 32 || ld % 32 || ((uintptr_t)x & 15) || ((uintptr_t)y & 15) ||
        ((uintptr_t)ws & 15) || metric < REID_METRIC_L2 || metric > REID_METRIC_DOT || k < 1 || k > SELECT_X3_KMAX)
        return hipErrorInvalidValue;
    if (m >= (1ll << 31) - BM || n >= (1ll << 31) - BM) return hipErrorInvalidValue;   // a row index is an int in the kernels (offsets are 64-bit)
    const int bn = tile_width(n), ntl = (n + bn - 1) / bn;
    const size_t per = row_bytes(ntl);
    if (ws_bytes < FIXED + per) return hipErrorInvalidValue;
    const long long fit = (long long)((ws_bytes - FIXED) / per);
    const int rows_per = fit < m ? (int)fit : m;
    // the threshold pass looks at the first 512 columns, from 8192 columns on at a sixteenth of them (whole 128-column tiles): the keys
    // that pass the filter are then about 600 per row whatever n (about 37 n / sample: nine per tile at 512, so a tile list of 32 does
    // not fill on unordered data), and the pass costs a sixteenth of the sweep
    const int sixteenth = (n / 16 + 127) / 128 * 128;
    const int wide = sixteenth > SELECT_X3_SAMPLE ? sixteenth : SELECT_X3_SAMPLE;
    const int sample = n < wide ? n : wide;
    if (((long long)rows_per + BM - 1) / BM * ntl >= (1ll << 31)) return hipErrorInvalidValue;

    char* base = (char*)ws;
    float* sc = (float*)base;
    u64* lists = (u64*)(base + FIXED);
    u64* cand = lists + (size_t)rows_per * ntl * KK;
    int* counts = (int*)(cand + (size_t)rows_per * KK);
    unsigned* gm = (unsigned*)(counts + (size_t)rows_per * ntl);
    unsigned* thr0 = gm + (size_t)rows_per * GROUPS;
    float* T = (float*)(thr0 + rows_per);

    hipLaunchKernelGGL(norm_range_kernel, dim3(1), dim3(1024), 0, stream, yy, n, sc);
    for (int i0 = 0; i0 < m; i0 += rows_per) {
        const int rows = m - i0 < rows_per ? m - i0 : rows_per;
        const hipError_t e = hipMemsetAsync(gm, 0xff, (size_t)rows * GROUPS * 4, stream);
        if (e != hipSuccess) return e;
        SelX3Params p;
        p.x = x + (size_t)i0 * ld; p.y = y; p.xx = xx + i0; p.yy = yy; p.fault = fault;
        p.m = rows; p.ld = ld; p.metric = metric; p.ntl = ntl;
        p.gm = gm; p.thr0 = thr0; p.lists = lists; p.counts = counts;
        const unsigned mt = (unsigned)((rows + BM - 1) / BM);
        p.n = sample; p.ntn = (sample + bn - 1) / bn;
        if (bn == 64) hipLaunchKernelGGL((cand_x3_kernel<64, MODE_BOUND>), dim3(mt * p.ntn), dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((cand_x3_kernel<128, MODE_BOUND>), dim3(mt * p.ntn), dim3(256), 0, stream, p);
        hipLaunchKernelGGL(thr_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, gm, rows, thr0);
        p.n = n; p.ntn = ntl;
        if (bn == 64) hipLaunchKernelGGL((cand_x3_kernel<64, MODE_LIST>), dim3(mt * p.ntn), dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((cand_x3_kernel<128, MODE_LIST>), dim3(mt * p.ntn), dim3(256), 0, stream, p);
        hipLaunchKernelGGL(merge_kernel, dim3(rows), dim3(256), 0, stream, lists, counts, ntl, thr0, cand, T);
        float* Dc = D ? D + (size_t)i0 * k : nullptr;
        hipLaunchKernelGGL(refine_kernel, dim3((rows + 7) / 8), dim3(256), 0, stream, p.x, y, ld, p.xx, yy, sc, cand, T, rows, i0, n, k, metric,
                           force_every, Dc, I + (size_t)i0 * k, flags + i0);
        hipLaunchKernelGGL(exact_row_kernel, dim3(rows), dim3(1024), 0, stream, p.x, y, ld, p.xx, yy, n, k, metric, Dc, I + (size_t)i0 * k,
                           flags + i0);
    }
    if (form_out) *form_out = bn == 64 ? SELECT_X3_FORM_128x64 : SELECT_X3_FORM_128x128;
    return hipGetLastError();
}
