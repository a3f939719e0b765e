// libreid_hip_anysize_front.so: uint8 crops (or windows of one frame) -> the pooled stem map of ResNet18-IBN-SE at any input size, in one
// kernel (anysize_front.h).  The any-size forward of api.hip opens with three launches: any_resize_norm_kernel writes an fp32 image, the
// generic implicit GEMM convolves it with a per-element predicated gather and writes the largest activation of the network, and
// maxpool3s2_kernel reads that map back.  Here neither the image nor the stem map reaches memory, as in stem_f32.hip for 256 x 128.
//
// A block owns one image, one column tile and a strip of bands (anysize_front.h: the cut is a function of H and W alone).  Per band:
//   * stage: the 15 resized + normalised input rows of the band go into LDS, computed from the uint8 source with the expressions of
//     any_resize_norm_kernel (anysize.hip) under fp contract(off); pixels outside the image are the convolution's zero padding;
//   * convolve: stem pixels are numbered row after row, 32 of them are the rows of one 32 x 32 MFMA tile, and a wave takes a
//     (tile, channel half) pair.  The A operand is read straight from the LDS image - the 21 taps of a kernel row are 21 consecutive
//     floats - and the weights from LDS, where they stay for the block's whole life.  k order: kernel rows ascending, 8-groups ascending,
//     MFMA e of a group sums k = 8 g + e (lanes 0 - 31) and 8 g + 4 + e (lanes 32 - 63): the generic GEMM's order (gemm_f32.hip) without
//     its last 24 k, which are zero on both sides.  Padded taps (k = 21 .. 23 of a kernel row) meet zero weights.
//     Epilogue v * scale + shift (contracted to one fma as there), into a ring of three stem rows in LDS;
//   * pool: MaxPool2d(3, 2, 1) of one pooled row from the ring; a tap outside the map does not take part.
// A band's five stem rows are computed as three (first pooled row) and two more (second pooled row, over ring slots 0 and 1);
// neighbouring bands each compute the stem row they share.
#include "anysize_front.h"
#include <math.h>

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int BAND = ANYSIZE_FRONT_BAND_ROWS, IN_ROWS = ANYSIZE_FRONT_IN_ROWS, NCOL = ANYSIZE_FRONT_MAX_NCOL;
constexpr int PITCH = ANYSIZE_FRONT_IN_PITCH, WP = ANYSIZE_FRONT_WP, PX = PITCH / 3;

struct MeanStd { float v[6]; };

__host__ __device__ inline void plan_geom(int H, int W, anysize_front_geom& g) {
    g.H1 = (H - 1) / 2 + 1;
    g.W1 = (W - 1) / 2 + 1;
    g.H2 = (g.H1 - 1) / 2 + 1;
    g.W2 = (g.W1 - 1) / 2 + 1;
    g.nbands = (g.H2 + BAND - 1) / BAND;
    g.ncoltiles = g.W2 <= 16 ? 1 : 1 + (g.W2 - 16 + 14) / 15;
    // a block restages nothing but its bands' rows, yet loads 44 KB of weights: about 32 blocks per image, at most 8 bands each
    int bpb = g.nbands * g.ncoltiles / 32;
    bpb = bpb < 1 ? 1 : (bpb > 8 ? 8 : bpb);
    g.bands_per_block = bpb;
    g.nstrips = (g.nbands + bpb - 1) / bpb;
    g.lds_bytes = ANYSIZE_FRONT_LDS_BYTES;
    g.in_rows = IN_ROWS;
    g.in_pitch = PITCH;
    g.max_ncol = NCOL;
}
__host__ __device__ inline void plan_band(const anysize_front_geom& g, int band, anysize_front_band& b) {
    b.p0 = band * BAND;
    b.np = g.H2 - b.p0 < BAND ? g.H2 - b.p0 : BAND;
    b.y_lo = 2 * b.p0 - 1;
    b.iy_lo = 2 * b.y_lo - 3;
}
__host__ __device__ inline void plan_coltile(const anysize_front_geom& g, int tile, anysize_front_coltile& c) {
    c.q0 = tile == 0 ? 0 : 16 + 15 * (tile - 1);
    const int cap = tile == 0 ? 16 : 15;
    c.nq = g.W2 - c.q0 < cap ? g.W2 - c.q0 : cap;
    c.x0 = 2 * c.q0 - 1 < 0 ? 0 : 2 * c.q0 - 1;
    const int x1 = 2 * (c.q0 + c.nq) < g.W1 ? 2 * (c.q0 + c.nq) : g.W1;
    c.ncol = x1 - c.x0;
    c.ix_lo = 2 * c.x0 - 3;
    c.npx = 2 * c.ncol + 5;
}

// any_resize_norm_kernel's tap (anysize.hip), restated
__device__ __forceinline__ void lin_tap(int d, int dst, int src, int& s, float& f) {
#pragma clang fp contract(off)
    const double scale = (double)src / (double)dst;
    float fx = (float)(((double)d + 0.5) * scale - 0.5);
    int sx = (int)floorf(fx);
    fx = fx - (float)sx;
    if (sx < 0) { sx = 0; fx = 0.f; }
    if (sx >= src - 1) { sx = src - 1; fx = 0.f; }
    s = sx;
    f = fx;
}

// ... and its pixel: the three channels of output pixel (dy, dx) of an h x w source resized to H x W
__device__ __forceinline__ void resized_pixel(const uint8_t* __restrict__ src, long long ps, int h, int w, int H, int W, int dy, int dx,
                                              const MeanStd& ms, float (&out)[3]) {
#pragma clang fp contract(off)
    int sx, sy;
    float fx, fy;
    lin_tap(dx, W, w, sx, fx);
    lin_tap(dy, H, h, sy, fy);
    const int sx1 = min(sx + 1, w - 1), sy1 = min(sy + 1, h - 1);
    const float gx = 1.0f - fx, gy = 1.0f - fy;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float p00 = (float)src[(sy * ps + sx) * 3 + ch] / 255.0f;
        const float p01 = (float)src[(sy * ps + sx1) * 3 + ch] / 255.0f;
        const float p10 = (float)src[(sy1 * ps + sx) * 3 + ch] / 255.0f;
        const float p11 = (float)src[(sy1 * ps + sx1) * 3 + ch] / 255.0f;
        const float r0 = p00 * gx + p01 * fx;
        const float r1 = p10 * gx + p11 * fx;
        const float v = r0 * gy + r1 * fy;
        out[ch] = (v - ms.v[ch]) / ms.v[3 + ch];
    }
}

__global__ __launch_bounds__(256, 2) void any_front_kernel(const uint8_t* __restrict__ packed, const long long* __restrict__ offsets,
                                                           const int* __restrict__ hw, int H, int W, int pitch, MeanStd ms,
                                                           const float* __restrict__ wgt, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float w_lds[64 * WP];
    __shared__ __attribute__((aligned(16))) float in_lds[IN_ROWS * PITCH];
    __shared__ __attribute__((aligned(16))) float ring[3 * NCOL * 64];     // stem rows: local row j in slot j % 3, [slot][column][channel]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;

    anysize_front_geom g;
    plan_geom(H, W, g);
    int bid = blockIdx.x;
    const int tile = bid % g.ncoltiles;
    bid /= g.ncoltiles;
    const int strip = bid % g.nstrips, img = bid / g.nstrips;
    anysize_front_coltile ct;
    plan_coltile(g, tile, ct);

    for (int i = tid; i < 64 * 168; i += 256) {                                        // weights [64][8][24] -> kernel rows 0 .. 6
        const int nrow = i / 168, k = i - nrow * 168;
        w_lds[nrow * WP + k] = wgt[nrow * 192 + k];
    }
    for (int i = tid; i < 64 * 4; i += 256) w_lds[(i >> 2) * WP + 168 + (i & 3)] = 0.f;

    const int sh_ = hw[2 * img], sw_ = hw[2 * img + 1];
    const uint8_t* src = packed + offsets[img];
    const long long ps = pitch ? pitch : sw_;
    float* const out_img = out + (long long)img * g.H2 * g.W2 * 64;

    const int band_end = min((strip + 1) * g.bands_per_block, g.nbands);
    for (int band = strip * g.bands_per_block; band < band_end; ++band) {
        anysize_front_band bd;
        plan_band(g, band, bd);
        // ---- stage: every float of the LDS image is written, so nothing of the previous band is left
        for (int i = tid; i < IN_ROWS * PX; i += 256) {
            const int row = i / PX, px = i - row * PX;
            const int iy = bd.iy_lo + row, ix = ct.ix_lo + px;
            float v[3] = {0.f, 0.f, 0.f};
            if (px < ct.npx && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) resized_pixel(src, ps, sh_, sw_, H, W, iy, ix, ms, v);
            float* dst = in_lds + row * PITCH + px * 3;
            dst[0] = v[0];
            dst[1] = v[1];
            dst[2] = v[2];
        }
        __syncthreads();   // the image (and, in the first band, the weights); every wave has left the previous band's pooling

        for (int phase = 0; phase < bd.np; ++phase) {
            // ---- convolve local stem rows [j0, j0 + nr): pixels m = (row - j0) * ncol + column, 32 per MFMA tile
            const int j0 = phase ? 3 : 0, nr = phase ? 2 : 3;
            const int count = nr * ct.ncol;
            const int ntask = 2 * ((count + 31) / 32);
            for (int task = wave; task < ntask; task += 4) {   // wave-uniform
                const int mt = task >> 1, b = task & 1;
                int m = mt * 32 + li;
                if (m >= count) m = 0;                          // a row of the tile behind the last pixel: computed, never stored
                const int rr = m / ct.ncol, cc = m - rr * ct.ncol;
                const float* a_rd = in_lds + 2 * (j0 + rr) * PITCH + 6 * cc + 4 * lh;   // + r * PITCH + 8 g   (even: ds_read_b64)
                const float* b_rd = w_lds + (li + 32 * b) * WP + 4 * lh;                // + r * 24 + 8 g
                f32x16 acc;
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
                for (int r = 0; r < 7; ++r)
#pragma unroll
                    for (int gq = 0; gq < 3; ++gq) {
                        const f32x2 a0 = *(const f32x2*)(a_rd + r * PITCH + 8 * gq);
                        const f32x2 a1 = *(const f32x2*)(a_rd + r * PITCH + 8 * gq + 2);
                        const float av[4] = {a0.x, a0.y, a1.x, a1.y};
                        const f32x4 bv = *(const f32x4*)(b_rd + r * 24 + 8 * gq);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], bv[e], acc, 0, 0, 0);
                    }
                // C layout: column = lane & 31 (channel), row = (e & 3) + 8 (e >> 2) + 4 lh (pixel of the tile)
                const float cs = scale[li + 32 * b], sh = shift[li + 32 * b];
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int mo = mt * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                    if (mo < count) {
                        const int ro = mo / ct.ncol, co = mo - ro * ct.ncol;
                        ring[(((j0 + ro) % 3) * NCOL + co) * 64 + li + 32 * b] = acc[e] * cs + sh;
                    }
                }
            }
            __syncthreads();
            // ---- pool row p of the band: stem rows 2 p - 1 .. 2 p + 1 = local rows 2 phase .. 2 phase + 2, the taps inside the map only
            const int p = bd.p0 + phase;
            for (int i = tid; i < ct.nq * 64; i += 256) {
                const int ch = i & 63, q = ct.q0 + (i >> 6);
                float mx = -INFINITY;
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    const int y = 2 * p - 1 + dy;
                    if ((unsigned)y >= (unsigned)g.H1) continue;
                    const int slot = (y - bd.y_lo) % 3;
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const int x = 2 * q - 1 + dx;
                        if ((unsigned)x >= (unsigned)g.W1) continue;
                        mx = fmaxf(mx, ring[(slot * NCOL + (x - ct.x0)) * 64 + ch]);
                    }
                }
                out_img[((long long)p * g.W2 + q) * 64 + ch] = mx;
            }
            __syncthreads();   // the ring's slots 0 and 1 and the LDS image are free again
        }
    }
}

inline bool size_ok(int H, int W) { return H >= 32 && H <= 512 && W >= 32 && W <= 512; }

}  // namespace

extern "C" hipError_t anysize_front_plan(int H, int W, anysize_front_geom* geom) {
    if (!geom || !size_ok(H, W)) return hipErrorInvalidValue;
    plan_geom(H, W, *geom);
    return hipSuccess;
}

extern "C" hipError_t anysize_front_plan_band(int H, int W, int band, anysize_front_band* out) {
    anysize_front_geom g;
    if (!out || !size_ok(H, W)) return hipErrorInvalidValue;
    plan_geom(H, W, g);
    if (band < 0 || band >= g.nbands) return hipErrorInvalidValue;
    plan_band(g, band, *out);
    return hipSuccess;
}

extern "C" hipError_t anysize_front_plan_coltile(int H, int W, int tile, anysize_front_coltile* out) {
    anysize_front_geom g;
    if (!out || !size_ok(H, W)) return hipErrorInvalidValue;
    plan_geom(H, W, g);
    if (tile < 0 || tile >= g.ncoltiles) return hipErrorInvalidValue;
    plan_coltile(g, tile, *out);
    return hipSuccess;
}

extern "C" hipError_t anysize_front(hipStream_t stream, const uint8_t* packed, const long long* offsets, const int* hw, int n, int H, int W,
                                    int pitch, const float* mean_std6_host, const float* stem_w, const float* scale, const float* shift,
                                    float* out) {
    if (!packed || !offsets || !hw || !mean_std6_host || !stem_w || !scale || !shift || !out || n < 1 || !size_ok(H, W) || pitch < 0)
        return hipErrorInvalidValue;
    anysize_front_geom g;
    plan_geom(H, W, g);
    const long long blocks = (long long)n * g.nstrips * g.ncoltiles;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    MeanStd ms;
    for (int i = 0; i < 6; ++i) ms.v[i] = mean_std6_host[i];
    hipLaunchKernelGGL(any_front_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, packed, offsets, hw, H, W, pitch, ms, stem_w, scale,
                       shift, out);
    return hipGetLastError();
}
