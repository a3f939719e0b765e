// Two links of the evaluation script's chain (reid/image_reid_inference.py) that lie beside the forward and the re-ranking:
//
//   data_transforms.py:130-191       get_inference_transforms_flipped(strong_inference=True), the second view of every ResNet-family
//                                    descriptor: Resize -> RandomHorizontalFlip(p=1) -> Pad(10) -> RandomCrop((H, W)) -> ToTensor ->
//                                    Normalize, i.e. the mirrored image shifted by up to +-pad pixels on each axis over a black border,
//                                    and black is (0 - mean) / std after Normalize          -> shift_mirror_nchw_kernel
//   image_reid_inference.py:276-289  jaccard + get_attribute_dist(labels, path) before DBSCAN; the term is euclidean_dist
//   losses/utils.py:21-35            (sqrt(clamp(xx + yy - 2 x.y, min = 1e-12))) of the normalised 30-wide attribute rows with
//                                    themselves                                             -> dist_add_l2_kernel
//
// Built as a library of its own, libreid_hip_eval_links.so (eval_links.h): libreid_hip.so, its dependencies and its kernel list
// (tests/golden/kernels.json) stay what they were; this library's kernels are held to tests/golden/kernels_eval_links.json.
#include "eval_links.h"
#include <math.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kGridCap = 4096;   // 256 CUs x 16 blocks; the loop strides over the rest
struct Fill3 {
    float r, g, b;
};

// One thread per output pixel (vec != 0: per four pixels of a row, w % 4 == 0), consecutive threads along the row: a wave's stores are one
// contiguous run, and its loads x[..][sy][w - 1 - sx] one contiguous run of the source row in descending order - the same cache lines
// as an ascending read.  The source columns of a vec thread are four scalar loads: left - pad is any integer, so they share no alignment
// with the stores.  Reads stay inside image img: row sy in [0, h), column w - 1 - sx in [0, w - 1]; shift_tl is read at 2 img + 1 < 2 m.
__global__ __launch_bounds__(256) void shift_mirror_nchw_kernel(const float* __restrict__ x, int m, int h, int w,
                                                                const int32_t* __restrict__ shift_tl, int pad, Fill3 fill, int vec,
                                                                float* __restrict__ y) {
    const int wq = vec ? w / 4 : w;
    const long long total = (long long)m * 3 * h * wq;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int q = (int)(i % wq);
        long long t = i / wq;
        const int oy = (int)(t % h);
        t /= h;
        const int c = (int)(t % 3);
        const int img = (int)(t / 3);
        const int sy = oy + shift_tl[2 * img] - pad;
        const int dx = shift_tl[2 * img + 1] - pad;
        const float f = c == 0 ? fill.r : (c == 1 ? fill.g : fill.b);
        const bool row_ok = sy >= 0 && sy < h;
        const float* row = x + (((long long)img * 3 + c) * h + (row_ok ? sy : 0)) * w;
        if (vec) {
            f32x4 v;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int sx = 4 * q + k + dx;
                v[k] = (row_ok && sx >= 0 && sx < w) ? row[w - 1 - sx] : f;
            }
            *(f32x4*)(y + 4 * i) = v;
        } else {
            const int sx = q + dx;
            y[i] = (row_ok && sx >= 0 && sx < w) ? row[w - 1 - sx] : f;
        }
    }
}

// ---- d_inout [n][n] += sqrt(max(s_i + s_j - 2 a_i.a_j, 1e-12)), euclidean_dist(a, a) of reid/losses/utils.py:21-35 added in place.
// A block owns rows [i0, i0 + 64) and, PER ROW, the 64 columns from j0 - s_i on, s_i = (i n) mod 4: that column is a 16-byte boundary of
// row i whatever n (rows of an odd n, 19 281 for Market, start at every alignment), so the matrix moves in 16-byte loads and stores; the
// column tiles of a row still partition it ([-s_i, 64 T - s_i) over T = ceil((n + 3) / 64) tiles, columns outside [0, n) skipped - a quad
// that straddles a row end is finished element by element).  Thread (r, g) = (tid / 16, tid % 16) computes rows i0 + r + 16 t, t = 0 .. 3
// - which share s_i, 16 n being a multiple of 4 - times the quad g of those rows: a 4 x 4 register block, and the 16 threads of a row
// cover 256 contiguous bytes of it.  LDS: the row panel [64][32] and the column panel [64 + 3][32] (three more rows in front for the
// shift), zero-padded from d to 32 columns and 33 floats apart (the 16 quads of a wave's row read panel rows 4 apart: banks 4 g, distinct).
constexpr int kTile = 64, kK = 32, kLd = kK + 1, kSlack = 3, kColRows = kTile + kSlack;

// the clamp of torch.clamp(min = 1e-12): NaN stays NaN (fmaxf would return 1e-12 for it), every other value gets fmaxf's bits
__device__ __forceinline__ float l2_of_sqr(float v) { return sqrtf(__builtin_elementwise_maximum(v, 1e-12f)); }

__global__ __launch_bounds__(256) void dist_add_l2_kernel(const float* __restrict__ a, int n, int d, float* __restrict__ d_inout) {
    __shared__ float sa[kTile * kLd], sb[kColRows * kLd], na[kTile], nb[kColRows];
    const int tid = threadIdx.x;
    const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
    for (int e = tid; e < kTile * kK; e += 256) {
        const int r = e >> 5, k = e & 31, gi = i0 + r;
        sa[r * kLd + k] = (gi < n && k < d) ? a[(long long)gi * d + k] : 0.f;
    }
    for (int e = tid; e < kColRows * kK; e += 256) {
        const int r = e >> 5, k = e & 31, gj = j0 - kSlack + r;
        sb[r * kLd + k] = (gj >= 0 && gj < n && k < d) ? a[(long long)gj * d + k] : 0.f;
    }
    __syncthreads();
    // squared norms: one ascending-k FMA chain per panel row - a function of the row alone, so row i has the same s_i in either panel
    if (tid < kTile + kColRows) {
        const float* p = tid < kTile ? sa + tid * kLd : sb + (tid - kTile) * kLd;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < kK; ++k) s = fmaf(p[k], p[k], s);
        if (tid < kTile) na[tid] = s;
        else nb[tid - kTile] = s;
    }
    __syncthreads();
    const int r = tid >> 4, g = tid & 15;
    const int s = (int)(((long long)(i0 + r) * n) & 3);
    const int cb = 4 * g - s + kSlack;   // the panel row of the thread's first column, 0 .. 63
    float acc[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[t][c] = 0.f;
#pragma unroll 8
    for (int k = 0; k < kK; ++k) {
        float av[4], bv[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) av[t] = sa[(r + 16 * t) * kLd + k];
#pragma unroll
        for (int c = 0; c < 4; ++c) bv[c] = sb[(cb + c) * kLd + k];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[t][c] = fmaf(av[t], bv[c], acc[t][c]);
    }
    const int c0 = j0 + 4 * g - s;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int i = i0 + r + 16 * t;
        if (i >= n) continue;
        float v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = l2_of_sqr(fmaf(-2.0f, acc[t][c], na[r + 16 * t] + nb[cb + c]));
        float* p = d_inout + (long long)i * n + c0;   // (i n + c0) % 4 == 0
        if (c0 >= 0 && c0 + 3 < n) {
            f32x4 o = *(const f32x4*)p;
            o[0] += v[0];
            o[1] += v[1];
            o[2] += v[2];
            o[3] += v[3];
            *(f32x4*)p = o;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c0 + c >= 0 && c0 + c < n) p[c] += v[c];
        }
    }
}

}  // namespace

extern "C" int eval_links_grid_cap(void) { return kGridCap; }
extern "C" int eval_links_tile(void) { return kTile; }
extern "C" int eval_links_max_d(void) { return kK; }

extern "C" hipError_t eval_links_shift_mirror(hipStream_t stream, const float* x, int m, int h, int w, const int32_t* shift_tl, int pad,
                                              const float* fill3, float* y) {
    if (!x || !shift_tl || !fill3 || !y || m < 1 || h < 1 || w < 1 || pad < 0) return hipErrorInvalidValue;
    const Fill3 fill{fill3[0], fill3[1], fill3[2]};
    const bool vec = (w % 4 == 0) && (((uintptr_t)y & 15) == 0);
    const long long work = (long long)m * 3 * h * (vec ? w / 4 : w);
    const long long blocks = (work + 255) / 256;
    const dim3 grid((unsigned)(blocks > kGridCap ? kGridCap : blocks));
    hipLaunchKernelGGL(shift_mirror_nchw_kernel, grid, dim3(256), 0, stream, x, m, h, w, shift_tl, pad, fill, vec ? 1 : 0, y);
    return hipGetLastError();
}

extern "C" hipError_t eval_links_dist_add_l2(hipStream_t stream, const float* a, int n, int d, float* d_inout) {
    if (!a || !d_inout || n < 1 || d < 1 || d > kK || ((uintptr_t)d_inout & 15)) return hipErrorInvalidValue;
    const long long gy = ((long long)n + kTile - 1) / kTile, gx = ((long long)n + kSlack + kTile - 1) / kTile;
    if (gy > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dist_add_l2_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, stream, a, n, d, d_inout);
    return hipGetLastError();
}
