// Internal declarations shared by the HIP translation units of libreid_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <initializer_list>
#include <string>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>
#include "../../include/reid_hip.h"
struct reid_ctx;

void reid_set_error(const char* fmt, ...);

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            reid_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return REID_ERR_HIP;                                                              \
        }                                                                                     \
    } while (0)

#define REID_TRY(expr)            \
    do {                          \
        int _s = (expr);          \
        if (_s != REID_OK) return _s; \
    } while (0)

#define ARG_CHECK(cond)                                                         \
    do {                                                                        \
        if (!(cond)) {                                                          \
            reid_set_error("%s:%d bad argument: %s", __FILE__, __LINE__, #cond); \
            return REID_ERR_ARG;                                                \
        }                                                                       \
    } while (0)

// ------------------------------------------------------------------------------------------------
// GEMM  C[M][N] = A'[M][K] . B[N][K]^T  on v_mfma_f32_32x32x2_f32, A' produced by one of the loaders.
// ------------------------------------------------------------------------------------------------
enum AMode {
    A_DENSE = 0,     // A[M][lda], K contiguous, K % 4 == 0, 16-byte aligned rows
    A_IM2COL = 1,    // NHWC fp32 activations, k = (r*S+s)*Cin + c, Cin % 32 == 0
    A_STEM_F32 = 2,  // NHWC fp32 [N][H][W][3], 7x7 s2 p3, k = r*24 + (s*3+c), 8 x 24 = 192 (zero padded)
    A_STEM_U8 = 3    // same from uint8 crops with (v/255-0.5)/0.5 fused into the loader
};
enum EpiMode {
    E_CONV = 0,  // optional col scale/shift, residual, relu, per-(m-tile, col) sum/sumsq partials
    E_DIST = 1,  // distance epilogue from row/col squared norms
    E_BIAS = 2   // optional bias[n], GELU, residual, ConvTranspose parity scatter
};

struct GemmParams {
    const void* A;
    long long lda;
    // im2col geometry
    int H, W, Cin, Ho, Wo, R, S, stride, pad_y, pad_x;
    const float* a_scale;  // [img][Cin] input transform x' = relu?(x*scale+shift) applied to in-bounds pixels
    const float* a_shift;
    int a_relu;
    const float* B;        // [N][ldb]
    long long ldb;
    int M, N, K;
    float* C;
    long long ldc;
    const float* col_scale;
    const float* col_shift;
    const float* residual;
    int relu;
    int relu_from;         // conv_f32.hip: ReLU applies to columns >= relu_from (0 = all; IBN: BatchNorm half only)
    float* stats;          // [M/128][N][2] or null
    // E_BIAS extras: act 1 = exact (erf) GELU after the bias; residual is added after the activation.
    // scat_h > 0: row m = (img, j, i) of a scat_h x scat_w grid is written to pixel (2j+scat_py, 2i+scat_px) of the
    // 2x up-sampled grid (one output parity of a ConvTranspose2d(4, 2, 1)); residual uses the same index.
    int act, scat_h, scat_w, scat_py, scat_px;
    int split_k;           // conv_f32_dma (small launches): blocks per output tile, fp32 partial tiles, per-tile arrival counters
    float* splitk_ws;
    int* splitk_cnt;
    unsigned scat_mhw, scat_mw;   // ceil(2^32 / (scat_h * scat_w)), ceil(2^32 / scat_w): row -> (img, j, i) by multiply-high (set_scatter)
    // par4 != 0 (conv_f32_dma general variant): the FOUR output parities of a ConvTranspose2d(4, 2, 1) in one launch - the grid
    // is four copies of the tile grid, copy q = (py, px) uses weights B + q * par_stride, padding (1 - py, 1 - px), scatter (py, px)
    int par4;
    long long par_stride;
    unsigned long long* diag;   // diagnostic builds of conv_f32.hip only: per-wave cycle sums [block<64][8][5]
    const float* row_sq;   // E_DIST
    const float* col_sq;
    int metric;
};

// ---- distance GEMM with fused selection (dist_select.hip): the k smallest per row, no m x n matrix
constexpr int SEL_CAP = 128;    // keys per (row, segment) candidate list
constexpr int SEL_KMAX = 64;    // largest k of the fused path (a list is compacted to k once it passes 64 keys)
struct SelectParams {
    const float* A;             // x [M][lda]
    const float* B;             // y [N][ldb]
    int lda, ldb, M, N, K;      // K % 64 == 0 (zero-padded rows)
    const float* row_sq;        // |x_i|^2, |y_j|^2 (null for REID_METRIC_DOT)
    const float* col_sq;
    unsigned int* gmin;         // [M][k] group minima of a sample of y as order-preserving keys (null: start from +inf)
    int metric, k, S, index_base, exp_skip;
    int empty_nan;              // k = 1: the value of a row without a candidate (every distance NaN) is NaN (reid_argmin_rows), else +inf (reid_knn)
    unsigned long long* lists;  // scratch [M][S][SEL_CAP] (k > 1)
    int* counts;                // scratch [M][S]: lengths of the lists when the sweep ends (k > 1)
    unsigned long long* final_keys;   // scratch [M][S]: every segment's arg-min key (k = 1)
};
int select_segments(int m, int n);
bool dist_select_supported(const SelectParams& p);
int launch_dist_bound(reid_ctx* ctx, const SelectParams& p);
int launch_dist_select(reid_ctx* ctx, const SelectParams& p, float* d_D, int32_t* d_I);

// ---- fp16-input / fp32-accumulate GEMM (gemm_f16.hip)
enum A16Mode {
    A16_DENSE = 0,   // A[M][lda] f16
    A16_IM2COL = 1,  // NHWC f16 activations, Cin % 64 == 0
    A16_STEM = 2     // zero-padded NHWC4 f16 image [n][Hp][Wp][4], 7x7 s2 as k = r*32 + s*4 + c (K = 256)
};
struct Gemm16Params {
    const _Float16* A;
    long long lda;
    int H, W, Cin, Ho, Wo, R, S, stride, pad, Hp, Wp;
    const _Float16* B;  // [N][ldb]
    long long ldb;
    int M, N, K;
    _Float16* C;
    long long ldc;
    const float* col_scale;
    const float* col_shift;
    const _Float16* residual;
    int relu;
    float* stats;
    const _Float16* zero_page;
    unsigned long long* diag;   // diagnostic builds only: per-wave cycle sums [block<64][wave][4]
    // linear-layer epilogue (Swin): out = act(acc + col_shift) + res32, stored as fp32 (C32) or f16 (C); ragged M, N
    int lin, act, n_real;       // lin != 0 selects it; act 1 = erf-GELU; n_real = columns that exist (0: N)
    int asym, pad_y, pad_x;     // asym != 0: separate top / left padding of the im2col gather (ConvTranspose parities)
    int scat_h, scat_w, scat_py, scat_px;   // > 0: output row (img, j, i) -> (img, 2j+py, 2i+px) of a 2x upsampled map
    float* C32;
    const float* res32;
    // conv3x3_f16.hip split-K (small launches): blocks per output tile, fp32 partial tiles, per-tile arrival counters
    unsigned scat_mhw, scat_mw; // as GemmParams
    int par4;                   // as GemmParams.par4 (LIN im2col build): four ConvTranspose parities in one launch
    long long par_stride;
    int split_k;
    float* splitk_ws;
    int* splitk_cnt;
    // conv3x3_f16.hip, SPLIT build ("fp32-class" arithmetic on the f16 matrix pipe, reid_ctx_set_precision(ctx, 2)):
    // x = xh + xl with xh = f16(x), xl' = f16((x - xh) * 2^11); x.w ~= xh.wh + (xl'.wh + xh.wl') / 2^11.  A holds [xh | xl'] per
    // pixel (2C f16 = the bytes of fp32), the weights [wh * 2^11 | wh | wl'] per tap (Cin = 3C "virtual" channels: the third
    // third re-reads xh), so ONE fp32 accumulator collects 2^11 times the product; acc_scale = 2^-11 goes into the BN scale.
    // Output fp32 (C32), residual fp32 (res32), ReLU from column relu_from on.
    _Float16* pack16;        // SPLIT builds: columns >= pack_from leave as [yh | yl'] f16 [M][2N] here instead of fp32 in C32
    int pack_from;
    int loader_prio;         // LDS-halo kernel: loader waves at raised issue priority
    int frag_ahead;          // LDS-halo kernel: fragment reads pinned one k-step ahead of their MFMAs
    float acc_scale;
    int relu_from;
    int split_terms;            // 3 (default) or 4 (adds the xl.wl product)
    int pack_out;               // LIN staged epilogue: C is [yh | yl'] f16 [M][2 n_real] (hi tile at column n_blk, low tile n_real further)
    int a_k;                    // LIN dense build with split_terms != 0: columns of A ([xh | xl'] = 2 K); K-tile k0 reads column k0 % a_k
    int pair_early;             // PAIR loop: the step barrier in front of the step's last MFMA group (REID_SPLIT_PAIR=2) instead of behind it
    int general_epi;            // SPLIT builds: the general (predicated, 64-bit addressed) epilogue instead of the lean one (A/B)
    int ablate;                 // experiments only (reid_debug_conv_split): phases of the PAIR loop switched off, results wrong
    int* fault;                 // reid_ctx.fault (may be null): [0] raised when a value packed as [yh | yl'] lies outside f16's range
};

// |x - y|^2 from the dot product and the squared norms: ONE explicit form for every kernel that computes or bounds a distance
// (gemm_f32.hip, gemm_f32_dma.hip, dist_select.hip's bound pass and sweep).  Left as (rs + cq) - 2 * dot the multiply-add is
// contracted or not per call site by the compiler, and a bound computed one way need not bound a value computed the other way.
__device__ __forceinline__ float l2sqr_of(float dot, float rs, float cq) { return fmaf(-2.0f, dot, rs + cq); }
// REID_METRIC_L2 = sqrt(clamp(|x - y|^2, min = 1e-12)) (reid/losses/utils.py:34).  The clamp keeps NaN as torch.clamp does - fmaxf would
// return 1e-12 for it, the smallest value the metric takes, and a row with one NaN would be every query's nearest neighbour.  Every
// other value gets fmaxf's bits.  IEEE 754-2019 maximum (NaN if either operand is): one v_maximum3_f32 on gfx950, where fmaxf was one
// v_max_f32 - a compare and a select would be two instructions in an epilogue that is VALU-bound beside the other block's MFMAs.
__device__ __forceinline__ float l2_of_sqr(float v) { return sqrtf(__builtin_elementwise_maximum(v, 1e-12f)); }

// precision 2 range guard (reid_ctx.fault; include/reid_hip.h, reid_ctx_set_precision): every site that writes a split operand
// [xh | xl'] keeps the largest magnitude it packed - as bits, so that NaN > inf > every finite value - and raises fault[0] when f16
// cannot hold it.  fault[1]: a non-finite embedding left the neck.
__device__ __forceinline__ unsigned range_acc(unsigned m, float v) {
    const unsigned b = __float_as_uint(v) & 0x7fffffffu;
    return b > m ? b : m;
}
__device__ __forceinline__ void range_raise(int* fault, unsigned m) {
    if (fault && m >= 0x477fe000u) fault[0] = 1;   // 65504.0f
}

// reciprocals for the scatter epilogues: floor(x / d) == umulhi(x, ceil(2^32 / d)) for x < 2^32 / d (rows of one pass: < 2^20)
template <class P>
inline void set_scatter(P& p, int scat_h, int scat_w, int py, int px) {
    p.scat_h = scat_h; p.scat_w = scat_w; p.scat_py = py; p.scat_px = px;
    p.scat_mhw = p.scat_mw = 0;
    if (scat_h > 0) {
        p.scat_mhw = (unsigned)(((1ull << 32) + (unsigned long long)(scat_h * scat_w) - 1) / (unsigned long long)(scat_h * scat_w));
        p.scat_mw = (unsigned)(((1ull << 32) + (unsigned long long)scat_w - 1) / (unsigned long long)scat_w);
    }
}

struct reid_ctx;
int launch_gemm_f16(reid_ctx* ctx, int amode, const Gemm16Params& p, int kind, double flops, double bytes);
bool conv3x3_f16_supported(const Gemm16Params& p);   // conv3x3_f16.hip: 3x3 s1 p1 with the input halo tile kept in LDS
int launch_conv3x3_f16(reid_ctx* ctx, const Gemm16Params& p, int kind, double flops, double bytes);
int launch_conv3x3_split(reid_ctx* ctx, const Gemm16Params& p, int kind, double flops, double bytes);   // SPLIT build, see Gemm16Params
bool conv3x3_x3_supported(const reid_ctx* ctx, const Gemm16Params& p);   // conv3x3_x3.hip: the same convolution as two 4-wave blocks per CU (large launches)
int launch_conv3x3_x3(reid_ctx* ctx, const Gemm16Params& p);
bool lin_x3_supported(const reid_ctx* ctx, const Gemm16Params& p);        // conv3x3_x3.hip: the dense form (Swin linears of stages 3-4, fp32-class mode)
int launch_lin_x3(reid_ctx* ctx, const Gemm16Params& p, int kind, double flops, double bytes);
bool conv_x3s_supported(const reid_ctx* ctx, const Gemm16Params& p);      // conv3x3_x3.hip: strided 3x3 / 1x1 convolutions, fp32-class mode
int launch_conv_x3s(reid_ctx* ctx, const Gemm16Params& p, int kind, double flops, double bytes);
int launch_gemm_f16_split(reid_ctx* ctx, const Gemm16Params& p, int kind, double flops, double bytes);   // SPLIT build of gemm_f16 (im2col: strided / 1x1)
bool two_linear_supported(const reid_ctx*, long long T, int C, int hid);
int launch_two_linear(reid_ctx*, const _Float16* a16, long long T, int C, int hid, const float* w1, const float* b1, const float* w2,
                      const float* b2, int act, const float* res, float* out, const float* x32 = nullptr, const float* ln_g = nullptr,
                      const float* ln_b = nullptr);
bool ln_linear_supported(const reid_ctx*, long long T, int C, int n);
int launch_ln_linear(reid_ctx*, const float* x32, const float* ln_g, const float* ln_b, long long T, int C, int n, const float* w, const float* bias,
                     float* out, int ldc);
// swin.hip: cosine window attention and the post-norm of the Swin "v2" blocks through libreid_hip_swin_v2.so (argument layouts: swin_v2.h)
int launch_window_attn_cos(reid_ctx* ctx, int mode, const void* qkv, int ldq, int n_img, int H, int W, int heads, int shifted,
                           const float* bias_t, const float* scale, void* out);
int launch_post_norm(reid_ctx* ctx, int side_mode, const float* x, const float* y, long long T, int C, const float* g, const float* b,
                     float* out, _Float16* side);
// swin.hip: the v1 kernels through the functions the forward calls (argument layouts at their definitions); the harnesses of
// include/reid_hip_debug.h call the same ones
void swin_bias_table(const float* pos169, float* tab4096);   // host: pos [13][13] -> [key 64][query 64], -inf on padded keys
int swin_attn_ldq(const reid_ctx* ctx, int C);
int launch_window_attn(reid_ctx* ctx, const void* qkv, int n, int Hs, int Ws, int heads, int shifted, const float* pos, const float* bias_tab,
                       void* out);
int launch_swin_layernorm(reid_ctx* ctx, int form, const float* x, long long T, int C, const float* g, const float* b, void* out);
int launch_sfe_norm_fc(reid_ctx* ctx, const float* c1, int n, int h1, int w1, const float* in_g, const float* in_b, const float* bn_s,
                       const float* bn_t, const float* c2_w, const float* c2_b, const float* fc_w, const float* fc_b, float* ab, float* tok);
int launch_swin_tail(reid_ctx* ctx, const float* x, int n, int ntok, const float* g, const float* b, const float* p, const float* bn_s,
                     const float* bn_t, float* gem, float* emb);
int swin_loaded_merge(reid_ctx* ctx, int stage, const float* x, int n, int h, int w, float* scratch, float* out);
int swin_loaded_fuse(reid_ctx* ctx, const float* sfe, float* const* xs, int n, int h1, int w1, float* scratch16, float* a0, float* f3, float* f2,
                     float* f1);
int swin_linear_for_test(reid_ctx* ctx, int f16_storage, const float* x32, const _Float16* x16, long long m, int k, const void* w,
                         const float* bias, int n, int act, const float* res, float* out32, _Float16* out16, int ldc);
// swin.hip: the two stems of the Swin forward, each writing c1 [n][h / 2][w / 2][12] - sfe_conv1_kernel from normalised NCHW images, and
// swin_crop_front_kernel (libreid_hip_swin_crops.so, swin_crops.h) from uint8 windows; mean_std6 is a host pointer
int launch_sfe_conv1(reid_ctx* ctx, const float* x, int n, int h, int w, const float* c1_w, const float* c1_b, float* c1);
int swin_crops_check(int out_h, int out_w, const float* mean_std6);   // sizes multiples of 224, mean finite, std > 0 (REID_ERR_ARG otherwise)
int launch_swin_crop_front(reid_ctx* ctx, const uint8_t* d_src, const long long* d_off, const int* d_hw, int n, int h, int w, int pitch,
                           const float* mean_std6, const float* c1_w, const float* c1_b, float* c1);
// swin.hip: what the Swin descriptor entries launch from libreid_hip_swin_eval.so (swin_eval.h) - the two stems of the mirrored view
// (arguments as the plain stems above) and the descriptor kernel: e1 / e2 (or nullptr) [n][96], cls_w [num_class][96] -> out rows of
// num_class + 96 floats, ld floats apart
int launch_sfe_conv1_mirror(reid_ctx* ctx, const float* x, int n, int h, int w, const float* c1_w, const float* c1_b, float* c1);
int launch_swin_crop_front_mirror(reid_ctx* ctx, const uint8_t* d_src, const long long* d_off, const int* d_hw, int n, int h, int w, int pitch,
                                  const float* mean_std6, const float* c1_w, const float* c1_b, float* c1);
int launch_swin_descriptor(reid_ctx* ctx, const float* e1, const float* e2, const float* cls_w, int n, int num_class, long long ld, float* out);
int launch_split_pack(reid_ctx* ctx, const float* x, long long rows, int C, _Float16* out, const float* d_scale = nullptr, bool range_fault = true);  // fp32 [rows][C] -> f16 [rows][2C] = [xh | xl']; range_fault = false: a value outside f16 leaves the fault word alone (knn_wide.hip answers such a call in exact fp32)
int launch_split_weights(reid_ctx* ctx, const float* w, int cout, int taps, int cin, int terms, _Float16* out, const float* d_scale = nullptr);  // fp32 [cout][taps][cin] -> f16 [cout][taps][terms * cin]
// fp16 elementwise kernels (elementwise_f16.hip)
int launch_prep_u8_pad_f16(reid_ctx*, const uint8_t* crops, int n, int h, int w, int hp, int wp, _Float16* out);
int launch_prep_f32_pad_f16(reid_ctx*, const float* nhwc3, int n, int h, int w, int hp, int wp, _Float16* out);
int launch_maxpool3s2_f16(reid_ctx*, const _Float16* x, int n, int h, int w, int c, _Float16* out);
int launch_affine_relu_f16(reid_ctx*, _Float16* x, const float* a_scale, const float* a_shift, int n_img, int hw, int c);
int launch_norm_apply_f16(reid_ctx*, _Float16* x, const float* stats, int n_img, int tiles, int c, int half, int hw,
                          const float* in_gamma, const float* in_beta, const float* bn_scale, const float* bn_shift);
int launch_se_tail_f16(reid_ctx*, const float* stats, int n_img, int tiles, int c, int mid, int hw, const float* w1, const float* w2t,
                       const _Float16* y, const _Float16* sc, _Float16* out);
int launch_se_combine_f16(reid_ctx*, const _Float16* y, const _Float16* sc, const float* s, int n_img, int hw, int c,
                          _Float16* out);
int launch_gem_neck_f16(reid_ctx*, const _Float16* x, int n_img, int hw, int c, const float* p, const float* scale,
                        const float* shift, float* gem_out, float* emb);
int launch_f32_to_f16(reid_ctx*, const float* x, size_t n, _Float16* out);
int launch_stem_w16(reid_ctx*, const float* stem_w_f32, _Float16* out);
bool conv3x3_c64_f16_supported(int H, int W, int Cin, int Cout, int R, int S, int stride, int pad);
int launch_scale_rows_f16(reid_ctx*, const float* w, const float* scale, int rows, int k, _Float16* out);
int launch_conv3x3_c64_f16(reid_ctx*, const _Float16* in, int n, const _Float16* w_scaled, const float* shift,
                           const _Float16* residual, int relu, float* stats, _Float16* out, const _Float16* zero_page,
                           const float* se_w1 = nullptr, const float* se_w2t = nullptr);
int launch_stem_w16_scaled(reid_ctx*, const float* stem_w_f32, const float* scale, _Float16* out);
int launch_stem_pool_f16(reid_ctx*, const _Float16* pad_in, const uint8_t* crops_u8, int n, const _Float16* w16s, const float* shift,
                         _Float16* pooled);
int launch_conv_w16_chunked(reid_ctx*, const float* w_f32, int cout, int rs, int cin, _Float16* out);  // -> [Cout][Cin/64][RS][64]   // [64][8][24] -> [64][8][8][4]
int launch_gemm_f32(reid_ctx* ctx, int amode, int epi, const GemmParams& p, int kind, double flops, double bytes);
int launch_ta_tail(reid_ctx* ctx, const float* y, const float* sc, int n_img, int H, int W, int C, const float* wts, float* out);
int launch_ema_tail(reid_ctx* ctx, const float* y, const float* sc, int n_img, int H, int W, int C, const float* prm, float* out);
int launch_stem_split(reid_ctx* ctx, const void* x, bool is_u8, int n, const float* wgt, const float* scale, const float* shift, float* out,
                      _Float16* packed);   // precision 2: 7x7 stem + BN + max-pool on split f16 operands (stem_split.hip)
int launch_stem_f32(reid_ctx* ctx, const void* x, bool is_u8, int n, const float* wgt, const float* scale, const float* shift,
                    float* out, bool pooled);   // stem_f32.hip: 7x7 s2 conv + BN (+ MaxPool(3,2,1) on the accumulators) of the fp32 path
bool gemm_f32_dma_supported(int amode, int epi, const GemmParams& p);   // gemm_f32_dma.hip: dense GEMM with LDS-DMA staging
int launch_gemm_f32_dma(reid_ctx* ctx, int epi, const GemmParams& p, int kind, double flops, double bytes);
bool conv_f32_supported(const GemmParams& p);   // conv_f32.hip: pipelined implicit-GEMM convolution of the fp32 path (full tiles)
int launch_conv_f32(reid_ctx* ctx, const GemmParams& p, int kind, double flops, double bytes);
bool conv_f32_general_supported(const GemmParams& p);   // same kernel, general geometry + bias epilogue (Swin's convolutions)
int launch_conv_f32_general(reid_ctx* ctx, const GemmParams& p, int kind, double flops, double bytes);

// elementwise / reduction kernels (elementwise.hip)
int launch_nchw_to_nhwc3(reid_ctx*, const float* x_nchw, int n, int h, int w, float* out_nhwc);
int launch_resize_norm(reid_ctx*, const uint8_t* packed, const long long* offsets, const int* hw, int n, int H, int W,
                       int pitch, float* out_nhwc);
int launch_maxpool3s2(reid_ctx*, const float* x, int n, int h, int w, int c, float* out);
int launch_norm_finalize(reid_ctx*, const float* stats, int n_img, int tiles, int c, int half, int hw,
                         const float* in_gamma, const float* in_beta, const float* bn_scale, const float* bn_shift,
                         float* a_scale, float* a_shift);
int launch_in_apply(reid_ctx*, float* x, const float* stats, int n_img, int tiles, int c, int half, int hw, const float* in_gamma,
                    const float* in_beta);
int launch_se_finalize(reid_ctx*, const float* stats, int n_img, int tiles, int c, int mid, int hw, const float* w1,
                       const float* w2, float* s);
int tail_slices(int n_img, int hw);   // elementwise.hip: blocks per image of the fused tail kernels
int launch_se_tail(reid_ctx*, const float* stats, int n_img, int tiles, int c, int mid, int hw, const float* w1, const float* w2,
                   const float* y, const float* sc, float* out, _Float16* packed = nullptr);   // packed: also [oh | ol'] f16 [.., 2c]
// the same launch with its kernel chosen by the caller (correctness harness): form -1 = launch_se_tail's rule, 0 = se_tail_kernel<false>,
// 1 = se_tail_kernel<true> (mid <= 32)
int launch_se_tail_form(reid_ctx*, int form, const float* stats, int n_img, int tiles, int c, int mid, int hw, const float* w1,
                        const float* w2, const float* y, const float* sc, float* out, _Float16* packed);
int launch_se_combine(reid_ctx*, const float* y, const float* sc, const float* s, int n_img, int hw, int c, float* out);
int launch_in_apply_pack(reid_ctx*, const float* x, const float* stats, int n_img, int tiles, int c, int half, int hw,
                         const float* in_gamma, const float* in_beta, _Float16* packed,   // precision 2: IBN finish -> [xh | xl']
                         bool in_half_only = false);   // the BatchNorm half was packed by the conv epilogue already
int launch_gem_neck(reid_ctx*, const float* x, int n_img, int hw, int c, const float* p, const float* scale,
                    const float* shift, float* gem_out, float* emb);
// the same of relu(gate * y + sc) with the gate of launch_se_tail: the last block's tail and GeM in one kernel, no activation tensor between
int launch_gem_neck_tail(reid_ctx*, const float* stats, int n_img, int tiles, int c, int mid, int hw, const float* w1, const float* w2,
                         const float* y, const float* sc, const float* p, const float* scale, const float* shift, float* gem_out,
                         float* emb);
int launch_row_sqnorm(reid_ctx*, const float* x, int m, int d, long long ld, float* out);
// selection kernels (select.hip)
int launch_argmin_rows(reid_ctx*, const float* dist, int m, int n, long long ld, int32_t* idx, float* val);
int launch_topk_rows(reid_ctx*, const float* dist, int m, int n, long long ld, int k, float* D, int32_t* I);
int launch_rank_eval(reid_ctx*, const float* score, int nq, int ng, long long ld, const long long* ql,
                     const long long* qc, const long long* gl, const long long* gc, int32_t* cmc_sum, double* ap,
                     int32_t* valid);
int launch_diou_cost(reid_ctx*, const double* tracks, int t, const double* dets, int m, double* out, int as_cost);
// evaluation-script post-processing (postproc.hip): the retrieval descriptor of e1 / e2 [n][de], l1 / l2 [n][dl] (e2 and l2 both nullptr: a
// single view, not renormalised) -> out [n][de + dl], and the column mirror of x [rows][w]
int launch_descriptor(reid_ctx*, const float* e1, const float* l1, const float* e2, const float* l2, int n, int de, int dl, float* out);
int launch_flip_w_nchw(reid_ctx*, const float* x, long long rows, int w, float* y);
// postproc.hip: the two kernels of libreid_hip_eval_links.so (eval_links.h), opened on the first call - the shifted mirrored view
// y = crop(pad(mirror(x))) of x [m][3][h][w] with (top, left) per image from the device array d_shift_tl and fill3 on the host, and
// d_inout [n][n] += euclidean_dist(a, a) in place.  A missing library is REID_ERR_STATE naming it.
int launch_shift_mirror(reid_ctx*, const float* x, int m, int h, int w, const int32_t* d_shift_tl, int pad, const float* fill3, float* y);
int launch_dist_add_l2(reid_ctx*, const float* a, int n, int d, float* d_inout);

// ------------------------------------------------------------------------------------------------
struct ProfSlot {
    double ms = 0, flops = 0, bytes = 0;
    long long launches = 0;
};

struct Se18Block {
    int c, cin, stride, ibn, ds, mid;
    const float *conv1_w, *in_gamma, *in_beta, *bn1_scale, *bn1_shift, *conv2_w, *bn2_scale, *bn2_shift;
    const float *ds_w, *ds_scale, *ds_shift, *se_w1, *se_w2;
    const float *ta, *ema;   // sibling backbones: TripletAttention gates [3][100] / EMA parameters (attention_f32.hip)
};

struct Se18Weights {
    bool loaded = false;
    float* blob = nullptr;
    size_t n_floats = 0;
    int num_class = 0;
    int arch = 0;                 // 0 SERse18_IBN, 1 CARes18_IBN (TripletAttention), 2 EMARes18_IBN
    const float *stem_w, *stem_scale, *stem_shift;
    Se18Block blk[8];
    const float *gem_p, *neck_scale, *neck_shift, *cls_w;
    const float* cam_bias = nullptr;   // [num_cams][512] (cam.bias; optional) and the constructor's cam_factor (cam.factor)
    int num_cams = 0;
    float cam_factor = -1.0f;
    _Float16* blob16 = nullptr;   // fp16 copy of the whole blob (same element offsets) for the fp16 path
    _Float16* stem_w16 = nullptr; // [64][256] stem weights of the padded-NHWC4 formulation
    _Float16* l1_conv2_w16s[2] = {nullptr, nullptr};   // layer-1 conv2 weights x BN scale (conv3x3_c64_f16.hip)
    _Float16* stem_w16s = nullptr; // same with the folded BN scale multiplied in (fused stem + maxpool kernel)
    _Float16* zero_page = nullptr;
    float* ep = nullptr;          // [8 blocks][2][512]: conv1 epilogue scale / shift of the IBN blocks: (1, 0) on the InstanceNorm
                                  // half, the folded BatchNorm on the other (conv_f32.hip flow)
    const _Float16* h(const float* p) const { return blob16 + (p - blob); }
};

// comm.hip: the RCCL communicator of this rank.  `loop` is a TEST transport (libreid_hip_debug.so, reid_debug_comm_loopback):
// several contexts of ONE process on ONE device act as the ranks, so that the multi-rank C code (ragged gathers, index_base,
// padding rows, the merge) runs with world > 1 on a one-GPU box.  The product never sets it: reid_comm_init is RCCL only.
struct reid_comm_loop {
    virtual int allgather(int rank, const void* d_send, void* d_recv, size_t bytes, hipStream_t st) = 0;
    virtual int allreduce(int rank, double* inout, int count, int op) = 0;
    virtual void detach(int rank) = 0;
    virtual ~reid_comm_loop() {}
};
struct reid_comm {
    void* comm = nullptr;   // ncclComm_t
    int rank = 0, world = 1;
    reid_comm_loop* loop = nullptr;
};
void comm_release(reid_ctx* ctx);
// k-way merge of per-shard top-k lists [world][nq][kk] (global indices, -1 = padding) -> [nq][k] (comm.hip)
int launch_knn_merge(reid_ctx* ctx, const float* Dall, const int32_t* Iall, int world, int nq, int kk, int k, float* D, int32_t* I);

struct reid_ctx {
    int device = 0;
    reid_comm* comm = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    int chunk = 1024;        // crops per pass (reid_ctx_set_chunk).  64 until round 4: 45 k crops/s in mode 2 where 1024 gives 68 k; the parity
                             // sets give the reference's arg-min on every row at 64, 128, 256 and 1024 (tools/config1_chunk_check.py)
    int precision = 0;
    bool profile = false;
    ProfSlot prof[REID_K_COUNT];
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    struct Pending { int kind; hipEvent_t a, b; double flops, bytes; };
    std::vector<Pending> pending;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    // growable device workspaces, keyed by name
    std::map<std::string, std::pair<void*, size_t>> ws;
    std::map<std::string, std::pair<void*, size_t>> pinned;   // pinned host staging buffers (ctx_pinned)
    std::map<const void*, void*> split_w;   // precision 2: conv weights (fp32, in the blob) -> their [wh * 2^11 | wh | wl'] f16 form
    // Switches below: fixed defaults in the product library.  The REID_* names in their comments are the environment variables that
    // set them until round 4; since round 5 the product library reads none of them (api.hip, reid_ctx_create) and experiments move a
    // field by its NAME through libreid_hip_debug.so: reid_debug_set_switch(ctx, "split_pair", 1) (debug.hip, kSwitches).
    int bank_fast = 1;                    // d = 512 feature-bank cost on the register-tiled kernel (REID_BANK_FAST=0: generic kernel)
    Se18Weights se18;
    int last_n = 0;  // crops in the last embed chunk (for reid_debug_stage)
    int swin_last_n = 0, swin_last_tok = 0;   // images / stage-1 tokens per image of the last Swin pass (reid_debug_swin_stage)
    int debug_keep = 0;      // 0 off, 1 stage buffers + unfused kernels, 2 stage buffers + production kernels
    bool last_f16 = false;
    int f16_wide_splitk = 1;  // LDS-halo kernel, small launches with a long K loop: 128-wide tiles split four ways (REID_F16_WIDE_SPLITK=0: 64-wide)
    int f16_frag_ahead = 1;   // LDS-halo kernel: fragments of k-step kk + 1 read before the MFMAs of kk (REID_F16_FRAG_AHEAD=0: compiler's order)
    int f16_loader_prio = 1;  // loader waves of the LDS-halo kernel at s_setprio 3: 1 = SPLIT builds (mode 2: 15.25 -> 15.10 ms per 1024 crops;
                              // the plain f16 build loses 0.6 %), 2 = all, 0 = none (REID_F16_LOADER_PRIO)
    int f16_loader_waves = 1; // LDS-halo kernel: 8 compute + 4 dedicated loader waves (REID_F16_LOADERS)
    int f16_halo = 1;        // 3x3 stride-1 convs of the fp16 path use the LDS-halo kernel (REID_F16_HALO=0: implicit GEMM)
    int gem_tail_min = 120;  // fp32-class ResNet18-SE: from this many images the last block's tail runs inside GeM (launch_gem_neck_tail):
                             // 120 crops 25.4 us against 28.9 + 8.1, 30 crops 16.3 against 12.6 + 4.9 (profiles/tails_stream_ab.txt)
    int f16_se_tail = 1;     // fp16 path: SE gate + combine in one launch per block (REID_F16_SETAIL=0: se_finalize + se_combine)
    int f16_c64 = 2;         // fp16 path: layer-1 convs on the register-resident-weight kernel, 2 = with the SE tail fused
                             // into conv2 (REID_F16_C64=1: separate se_finalize / se_combine kernels, 0: implicit GEMM)
    int f16_stem_fused = 2;  // fp16 path: stem conv + BN + maxpool as one kernel, 2 = fed with the uint8 crops directly
                             // (REID_F16_STEMPOOL=1: from the padded f16 image, 0: GEMM + pool kernels)
    int f32_conv = 1;        // fp32 path (REID_F32_CONV): 1 = conv_f32.hip LDS-DMA kernel, norms in the producer's epilogue / in_apply;
                             // 2 = conv_f32.hip register-staged kernel, norm in the loader; 0 = gemm_f32_kernel<A_IM2COL> (round 1)
    int f32_split_k = 1;     // fp32 conv: split the K-tiles over 2-4 blocks per output tile when a launch has <= 256 tiles (REID_F32_SPLITK)
    int lin_x3 = 1;          // Swin, fp32-class mode: linears with N % 128 == 0 on conv3x3_x3.hip's dense kernel (0: gemm_f16.hip's linear build)
    int f32_dist_bk16 = 1;   // distance matrix, 128-wide tiles: K-tiles of 16 -> three blocks per CU (gemm_f32_dma.hip); 0 = K-tiles of 32, two blocks
    int pack_epilogue = 1;   // precision 2: conv1 epilogues write [yh | yl'] for conv2 themselves (REID_PACK_EPILOGUE=0: fp32 + pack passes)
    int split_lean_epi = 1;  // precision 2: buffer-instruction epilogue of the SPLIT convolution builds (REID_SPLIT_LEAN=0: general loop)
    int split_x3 = 3;        // precision 2, large launches: conv3x3_x3.hip instead of conv3x3_f16.hip's 12-wave kernel: 3 (default) = on
                             // v_mfma_f32_16x16x32_f16, two blocks per CU for the 128-wide tiles (layers 2-4) and FOUR for the 64-wide ones
                             // (layer 1); 2 = the 128-wide tiles only; 1 = the first form on 32x32x16; 0 = off
    int split_gemm_min_tiles = 128;   // precision 2: strided / 1x1 convolutions take the SPLIT build of gemm_f16.hip from this many 256 x 128 tiles on (below: the exact-fp32 split-K kernel)
    int chain = 0;           // EXPERIMENTS=1 builds only: precision 2, batches of up to 64 crops, layer 4 as ONE chain launch (conv3x3_x3.hip chain_kernel;
                             // 536 us against 255 us for the six launches it replaces: DESIGN.md section 8); bit 2 = timing variant (wrong results)
    int x3_sk_cap = 0;       // experiments: upper bound of the split-K factor of conv3x3_x3.hip's small launches (0 = the heuristic's)
    int split_x3_small = 2;  // ... and smaller launches: 2 (default) = where they measured faster than conv3x3_f16.hip's 12-wave kernel (conv3x3_x3_supported),
                             // 1 = every launch, 0 = none; K split over up to 8 blocks per tile (x3m16_tail: reduce-scatter)
    int x3s_sk_cap = 8;      // conv_x3s_kernel: most blocks per output tile
    int conv_x3s = 1;        // conv3x3_x3.hip conv_x3s_kernel for the strided 3x3 / 1x1 convolutions of the fp32-class mode: 1 = wherever gemm_f16.hip's SPLIT build served (launches of >= ~100 tiles), 2 = also the small launches that run in exact fp32, 0 = off
    int x3_l4_narrow_nmt = 31;  // conv3x3_x3.hip x3_wide_tiles: layer 4 on 64-wide tiles where its 128-wide launch fills the chip unevenly (0: never; split launches up to this many tile rows)
    int x3_narrow = 1;       // conv3x3_x3.hip, 64-wide tiles (four blocks per CU) beyond layer 1: bit 0 = the 16-wide maps (layer 2: 14.03 -> 13.87 ms per
                             // 1024-crop pass; default), bit 1 = the 8-wide ones (layers 3-4: 14.03 -> 14.70, off)
    int x3_unroll = 3;       // conv3x3_x3.hip: the form with a chunk's 27 steps unrolled (addresses, DMA offsets made once, waits immediates): 1 = the
                             // 128-wide tiles, 3 (default) = and the 64-wide ones at THREE blocks per CU (134-148 registers; at four they spill:
                             // 12.59 / 12.32 / 14.05 ms per 1024-crop pass for 1 / 3 / 4), 0 = the looped kernels
    int x3_ablate = 0;       // timing experiments on conv3x3_x3.hip (debug switch; WRONG results while set)
    int split_x3_min_blocks = 512;   // ... from this many blocks on (two for every CU)
    int split_pair = 0;      // precision 2, 128-wide halo tiles (REID_SPLIT_PAIR): 0 = three passes over the virtual channels (default),
                             // 1 / 2 = the operand-sharing PAIR order of conv3x3_f16.hip (barrier behind / in front of a step's last
                             // MFMA group).  Measured at 1024 crops per pass: +1.1 % / -0.9 %; it changes the summation order, and the
                             // config-1 noise set has a row whose top-2 gap (2.7e-7) any reordering can flip - not worth 1 %
    int stem_split = 1;      // precision 2: the 7x7 stem on split f16 operands (REID_STEM_SPLIT=0: the fp32-pipe stem + split_pack)
    int f32_stem_pool = 1;   // fp32 path: MaxPool(3,2,1) on the stem kernel's accumulators (REID_F32_STEMPOOL=0: separate kernel)
    int split_terms = 3;     // precision 2: f16 products per multiply (REID_SPLIT_TERMS=4 adds the low x low product)
    int knn_wide = 1;        // large k-NN searches: candidates on the f16 matrix pipe + exact fp32 refinement (knn_wide.hip; REID_KNN_WIDE=0:
                             // the fused fp32 search for every size)
    long long knn_wide_min = 1ll << 25;   // query x gallery pairs from which the wide path is taken (REID_KNN_WIDE_MIN): Market-size (3368 x 15913) 0.68 -> 0.41 ms
    int knn_wide_force = 0;  // tests (reid_debug_knn_wide): every row whose index is a multiple of it takes the exact-row fallback
    int knn_wide_tile_rows = 0;   // tests (reid_debug_knn_wide_run): query rows per tile of the wide path instead of its 1 GiB rule; a multiple of 256
    int select_exp = 0;      // experiments only (reid_debug_select_exp, debug.hip): 1 / 2 skip phases of the fused selection (results
                             // are then incomplete), 4 prints candidate-list statistics
    int select_two_pass = 0; // REID_SELECT_TWO_PASS=1: arg-min / k-NN through the full distance matrix (A/B against dist_select.hip)
    int rerank_hbm_acc = 0;  // tests (debug switch): 1 = re-ranking's query-expansion and Jaccard accumulators in HBM scratch at every n
    int swin_stop = -1;      // diagnostics (REID_SWIN_STOP = block * 10 + phase): skip the rest of the Swin blocks after that point
    int swin_fold = 1;       // Swin, fp16-storage mode: to_out and post_proj folded into one Linear (REID_SWIN_FOLD=0: two launches)
    int swin_two_linear = 1; // Swin, fp32-class mode, C = 96: to_out -> post_proj and fc1 -> GELU -> fc2 as one launch each, the hidden
                             // values in registers (two_linear_f16.hip; REID_SWIN_TWO_LINEAR=0: two launches through gemm_f16.hip)
    int swin_attn_split = 0; // REID_SWIN_ATTN_SPLIT=1: Swin window attention of the fp32-class mode on the matrix cores, split operands, instead
                             // of the exact-fp32 VALU kernel (measured: 14.0 k against 14.7 k img/s - see window_attn_mfma_split_kernel)
    int two_linear_ablate = 0;   // reid_debug_two_linear_ablate (timing experiments: WRONG results): 1 = no weight refills, 2 = no barriers
    int swin_attn_mfma = 1;  // Swin window attention (REID_SWIN_ATTN): 1 = matrix cores in fp16-storage mode, VALU kernel in exact fp32
                             // (v_mfma_f32_32x32x2_f32 runs at the fp32 VALU rate: no gain); 2 = matrix cores in both; 0 = VALU in both
    int f16_split_k = 1;     // LDS-halo kernel: split the input channels over 2-4 blocks per tile when a launch has < 128 tiles (REID_F16_SPLITK)
    int swin_chunk_cap = 1024;   // images per Swin pass at most (REID_SWIN_CHUNK_MAX lowers it, read at context creation)
    int f16_lin_256 = 1;     // fp32-class Swin linears / trunk convolutions with N % 256 == 0 and K >= 1152 on 256 x 256 tiles, BK 64 (REID_F16_LIN_256=0:
                             // 256 x 128, BK 32).  Same K order per output: bit-identical; 16.11 -> 16.25 k img/s
    int f16_cfg = 0;         // fp16 GEMM tile/ring override: BN*1000 + BK*10 + NST, 0 = heuristic (REID_F16_CFG)
    int frame_m[2] = {0, 0};                        // frame pipeline (bank.hip): detections / device embeddings per frame slot
    float* frame_emb[2] = {nullptr, nullptr};
    int frame_d[2] = {512, 512};                    // width of the slot's embeddings: 512 after reid_frame_submit, the Swin's embed_dim after reid_frame_submit_swin
    int frame_pending[2] = {0, 0}, frame_has[2] = {0, 0};
    size_t frame_tm[2] = {0, 0};        // elements of the cost stage's output (sum over the camera groups of tracks x detections)
    hipEvent_t frame_ev[2] = {nullptr, nullptr};
    hipStream_t match_stream = nullptr;  // reid_frame_match_stream(ctx, 1): cost / update stages of the frame pipeline on a stream of their own, so that a
                                         // group of look-ahead frames walks its serial cost -> assign -> update chain beside the next group's forward
    int match_async = 0;
    hipEvent_t join_ev = nullptr;        // orders the bank's other entry points between the two streams
    hipEvent_t fwd_ev[2] = {nullptr, nullptr}, match_ev[2] = {nullptr, nullptr};   // slot's forward queued / its last reader on the match stream queued
    hipStream_t copy_stream = nullptr;   // uploads of the frame pipeline (beside the kernels of the previous frame)
    hipEvent_t copy_ev = nullptr;
    std::vector<hipEvent_t> pipe_ev;     // host_passes (api.hip): "pass k uploaded" / "pass k computed" events of the host-in / host-out entry points
    int host_pipeline = 1;               // host entry points with more than one pass: pass k + 1's upload and pass k - 1's download on the copy stream
                                         // under pass k's kernels (0: whole batch up, compute, whole result down - the form of rounds 1-5)
    int side_copy = 1;                   // REID_SIDE_COPY=0: uploads in the compute stream
    std::vector<int32_t> side_idx;       // reid_ctx_set_side_index: camera / view index per image of the following embed call(s)
    size_t side_cursor = 0;              // how many of them the passes so far have consumed
    const char* frame_out[2] = {nullptr, nullptr};
    float* stage_ptr[11] = {nullptr};
    size_t stage_elems[11] = {0};   // floats per image of each stage tap of the last pass, when that pass ran the any-size forward (else 0)
    int anysize_force = 0;   // libreid_hip_debug.so switch: 256 x 128 through the any-size forward too (reid_*_hw entries; A/B and tests)
    int any_front = 2;       // libreid_hip_debug.so switch: the front end of reid_frame_submit_hw / reid_embed_frame_u8_hw: 1 = any_front_kernel
                             // (libreid_hip_anysize_front.so), 0 = the three launches of the other reid_*_hw entries (A/B inside one call),
                             // 2 (default) = the kernel where it measured faster - passes of at most ANY_FRONT_MAX_STEM_PIXELS - else the launches
    int hw_precision = -1;   // reid_ctx_set_hw_precision: the arithmetic of the any-size forward: -1 = it needs the context in mode 0 (default),
                             // 0 = exact fp32 whatever the mode, 2 = fp32-class whatever the mode (libreid_hip_anysize_x3.so)
    int hw_siblings = 0;     // reid_ctx_set_hw_siblings: 1 = a loaded cares18_ibn runs at other sizes too (libreid_hip_anysize_ca.so)
    int hw_ema = 0;          // reid_ctx_set_hw_ema: 1 = a loaded emares18_ibn runs at other sizes too (libreid_hip_anysize_ema.so)
    int hw_f16 = 0;          // reid_ctx_set_hw_f16: 1 = a loaded seres18_ibn runs at other sizes in fp16 storage with fp32 accumulation, whatever
                             // the mode and hw_precision (libreid_hip_anysize_f16.so)
    int hw_sib_f16 = 0;      // reid_ctx_set_hw_sib_f16: 1 = a loaded cares18_ibn / emares18_ibn runs at other sizes in fp16 storage with fp32
                             // accumulation, whatever the mode and the other hw_* settings (libreid_hip_anysize_f16.so + ..._anysize_sib_f16.so)
    int any_f16_form = 0;    // the tile form the last fp16-storage any-size convolution launched (anysize_f16.h), written on the host only
    int any_ema = 1;         // libreid_hip_debug.so switch: the EMA tail of the any-size trunk: 1 = libreid_hip_anysize_ema.so, 0 =
                             // launch_ema_tail (attention_f32.hip; refuses a map whose slab does not fit LDS), for A/B timing in one process
    int any_ca = 1;          // libreid_hip_debug.so switch: the TripletAttention tail of the any-size trunk: 1 = libreid_hip_anysize_ca.so,
                             // 0 = launch_ta_tail (attention_f32.hip), for A/B timing of whole passes in one process
    int any_conv_form = 0;   // the tile form the last fp32-class any-size convolution launched (anysize_x3.h), written on the host only
    unsigned long long* conv_diag = nullptr;   // experiments (debug.hip): stamps of the loader-wave conv kernel
    // Which launch the last f16 convolution launcher made, written on the host only (harnesses read it, include/reid_hip_debug.h:
    // reid_debug_conv_layer_f16).  launch_gemm_f16: the tile configuration BN*1000 + BK*10 + NST; launch_conv3x3_f16: BN*10 + split K;
    // launch_conv3x3_c64_f16: 1 plain, 2 with the fused SE tail.  The dense launchers a Linear layer can reach name themselves too
    // (reid_debug_swin_linear): launch_epi (gemm_f32_dma.hip) 5000000 + BN * 1000 + BK * 10 (5064320, 5128320, 5128160), launch_bn
    // (gemm_f32.hip) 6000000 + BN * 1000 (6064000, 6128000), launch_lin_x3 7128000.  No kernel sees it and no launch depends on it.
    int conv_form = 0;
    // precision 2 guards (include/reid_hip.h, reid_ctx_set_precision): the first conv / linear weight of the loaded checkpoint that
    // cannot be split ([wh 2^11 | wh | wl'] needs |w| 2^11 < 65504), empty when all can ...
    std::string split_bad_se18, split_bad_swin;
    // ... and a sticky fault word in pinned host memory that kernels raise: REID_FAULT_RANGE = an activation outside f16's range
    // reached a split ([xh | xl']) site, REID_FAULT_NONFINITE = a non-finite embedding left the neck.  Every entry point returns
    // REID_ERR_STATE while it is set (ctx_fault_status); reid_ctx_clear_fault resets it.
    int* fault = nullptr;
};
enum { REID_FAULT_RANGE = 1, REID_FAULT_NONFINITE = 2 };
int ctx_fault_status(reid_ctx* ctx);
// knn_wide.hip: brute-force k-NN for large problems (candidates in fp32-class arithmetic, exact fp32 refinement)
bool knn_wide_eligible(reid_ctx* ctx, int nq, int nb, int d, int k);
// cand_out (tests, reid_debug_knn_wide_run; may be null): device [nq][ceil256(nb)], receives the candidate matrix as rowsel_kernel and
// refine_kernel saw it - exact_row_kernel reuses a flagged row's slot; the other stages stay in the workspaces knnw.keys / .flags / .sc
int knn_wide_dev(reid_ctx* ctx, const float* xp, int nq, const float* yp, int nb, int ld, const float* rs, const float* cq, int k, float* d_D,
                 int32_t* d_I, float* cand_out = nullptr);
// api.hip: zero-padded copy of d_x [m][d] with rows of a multiple of `mult` floats (the operand itself when it has such rows already)
int pad_rows_to(reid_ctx* ctx, const char* name, const float* d_x, int m, int d, int mult, const float** out, int* ld);
// api.hip: the launcher of reid_argmin_rows_x3* / reid_knn_x3* (libreid_hip_select_x3.so, select_x3.h) on device operands; d_D may be null;
// force_every > 0: rows whose index is a multiple of it take the exact-row kernel; stats (host, may be null): waits for the stream,
// then {rows proven, rows recomputed, tile form, candidates per row}
int select_x3_launch(reid_ctx* ctx, const float* d_x, int m, const float* d_y, int n, int d, int metric, int k, float* d_D, int32_t* d_I,
                     int force_every, int32_t* stats);

// precision 2: largest |w| of the named tensors against the bound their split form allows; returns "" or "name (max |w| = v)"
inline std::string split_range_violation(const float* blob, const std::map<std::string, std::pair<size_t, size_t>>& tab,
                                         const std::vector<std::pair<std::string, float>>& suffix_bound) {
    for (const auto& kv : tab) {
        for (const auto& sb : suffix_bound) {
            const std::string& suf = sb.first;
            if (kv.first.size() < suf.size() || kv.first.compare(kv.first.size() - suf.size(), suf.size(), suf) != 0) continue;
            float mx = 0.f;
            const float* w = blob + kv.second.first;
            for (size_t i = 0; i < kv.second.second; ++i) {
                const float a = w[i] < 0 ? -w[i] : w[i];
                if (!(a <= mx)) mx = a;        // NaN counts as a violation
            }
            if (!(mx < sb.second)) {
                char buf[160];
                snprintf(buf, sizeof(buf), "%s (max |w| = %g, limit %g)", kv.first.c_str(), (double)mx, (double)sb.second);
                return buf;
            }
            break;
        }
    }
    return std::string();
}

// ---- chain kernels (conv3x3_x3.hip, round 6): ONE persistent launch runs all the 3x3 stride-1 convolutions, InstanceNorm finishes
// and SE tails of a ResNet layer for a small batch.  Work items are claimed in list order with one atomic; an item waits only for
// counters of ITS OWN image(s) (crops are independent in eval mode: SERes18_IBN.py:32-41,88-93,120-128), never for a grid barrier.
struct ChainElem {             // an InstanceNorm finish + pack (kind 1) or an SE gate + tail (kind 2) over the images of the batch
    const float* x;            // kind 1: conv1 output fp32 [n][hw][c] (InstanceNorm half raw); kind 2: conv2 output y fp32
    const float* stats;        // per-128-row column sums [n * tiles][c][2] of the producing convolution
    const float* sc;           // kind 2: shortcut fp32 [n][hw][c]
    const float *g, *b;        // kind 1: IN gamma / beta [half]; kind 2: SE fc1 [mid][c] / fc2^T [mid][c]
    float* out;                // kind 2: block output fp32 (may be null)
    _Float16* packed;          // [n][hw][2c] as [xh | xl'] (kind 1: the InstanceNorm half's columns only; kind 2: may be null)
    int c, half, hw, tiles, mid, slices;
};
struct ChainStage {
    int kind;                  // 0 convolution, 1 InstanceNorm finish + pack, 2 SE tail
    int idx;                   // index into ChainParams::conv / ::el
    int first, items;          // range of the stage in the item list
    int dep;                   // stage this one waits for (per image), -1: its input was ready at launch
    int target;                // ... until that stage's counter of the image has reached this
    int sk;                    // convolution: blocks per output tile
};
struct ChainParams {
    int n_img, n_stages, total_items, flags;
    ChainStage st[8];
    Gemm16Params conv[4];
    ChainElem el[4];
    int* counters;             // [0] next item, [1] blocks that have left, [64 + stage * 64 + image] items of the stage finished for the image
    int* fault;
};
int launch_chain(reid_ctx* ctx, const ChainParams& cp, int W);      // conv3x3_x3.hip

// convolution launchers of the two arithmetic modes (api.hip); also used by the experiment harnesses in debug.hip
int conv_gemm(reid_ctx* ctx, int amode, const void* x, int n, int H, int W, int Cin, const float* wgt, int Cout, int R,
              int S, int stride, int pad, int Kpad, const float* a_scale, const float* a_shift, int a_relu,
              const float* col_scale, const float* col_shift, const float* residual, int relu, float* stats, float* out,
              int relu_from = 0, const _Float16* x_packed = nullptr,
              _Float16* out_packed = nullptr, int pack_from = 0, bool* packed_written = nullptr);   // x_packed (precision 2): x already as [xh | xl']
int conv_weights_fresh(reid_ctx* ctx, const float* d_w);   // drops the cached split form of a reused weight workspace (api.hip)
int conv_weights_splittable(reid_ctx* ctx, const float* h_w, size_t count, const char* who);   // precision 2: host weights inside the split range
int conv_gemm16(reid_ctx* ctx, int amode, const _Float16* x, int n, int H, int W, int Cin, const _Float16* wgt, int Cout,
                int R, int S, int stride, int pad, int K, const float* col_scale, const float* col_shift,
                const _Float16* residual, int relu, float* stats, _Float16* out, int Hp = 0, int Wp = 0);

// Every entry point runs on the context's device, whatever device the calling thread had current (hipSetDevice is
// per-thread: a worker thread starts on device 0; a host application may have switched devices).  Restores on exit.
struct DeviceGuard {
    int prev = -1, dev = -1;
    explicit DeviceGuard(int d) : dev(d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define CTX_GUARD(ctx) DeviceGuard _dev_guard((ctx)->device)
// entry points that start new work: device guard + the sticky fault word (a raised fault makes every later call fail loudly)
#define CTX_ENTER(ctx)            \
    CTX_GUARD(ctx);               \
    REID_TRY(ctx_fault_status(ctx))

void swin_release(reid_ctx* ctx);   // frees the Swin weights held for this context (swin.hip)
int ctx_ws(reid_ctx* ctx, const char* name, size_t bytes, void** out);  // grow-only named workspace
// pending side indices of the next n images (reid_ctx_set_side_index): *d_idx = device array of n entries, or nullptr when none are
// pending; entries must be < rows (the table of the loaded weights, 0 = the weights have none)
int ctx_take_side(reid_ctx* ctx, int n, int rows, const char* what, const int32_t** d_idx);
// x[img][p][c] += coeff * table[idx[img]][c] (elementwise.hip)
int launch_add_indexed_rows(reid_ctx* ctx, float* x, int n, long long hw, int C, const float* table, const int32_t* d_idx, float coeff);
int ctx_pinned(reid_ctx* ctx, const char* name, size_t bytes, void** out);   // grow-only named pinned host buffer
int ctx_pipe_events(reid_ctx* ctx, int passes);   // api.hip: the copy stream + 2 events per pass (host_passes)

// Host in -> host out in passes.  The reference's loops move every batch across PCIe (feature_extractor.py:48-53 `.to(device)` ...
// `.cpu().numpy()`, image_reid_inference.py:116-122); a caller that hands over host buffers pays that too, so the entry points hide it:
// pass k + 1's upload and pass k - 1's download are queued on the context's copy stream while pass k's kernels run on its compute
// stream (pinned sources copy asynchronously; a pageable one blocks the HOST inside hipMemcpyAsync, after pass k has been queued, so
// the device stays busy either way).  up(i, m, s) queues the upload of items [i, i + m) on stream s, run(i, m) the kernels on
// ctx->stream, down(i, m, s) the download.  The passes are the same passes, in the same order, on the same stream as without the
// pipeline: results are bit-identical.  One pass (or host_pipeline = 0): everything on the compute stream, as before.
template <class Up, class Run, class Down>
int host_passes(reid_ctx* ctx, int n, int pass, Up up, Run run, Down down) {
    const int passes = (n + pass - 1) / pass;
    if (passes <= 1 || !ctx->host_pipeline) {
        REID_TRY(up(0, n, ctx->stream));
        for (int i = 0; i < n; i += pass) REID_TRY(run(i, n - i < pass ? n - i : pass));
        REID_TRY(down(0, n, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return REID_OK;
    }
    REID_TRY(ctx_pipe_events(ctx, passes));
    hipStream_t cs = ctx->copy_stream;
    hipEvent_t* up_ev = ctx->pipe_ev.data();
    hipEvent_t* run_ev = ctx->pipe_ev.data() + passes;
    auto span = [&](int k, int* i, int* m) { *i = k * pass; *m = n - *i < pass ? n - *i : pass; };
    int i, m, rc = REID_OK;
    span(0, &i, &m);
    rc = up(i, m, cs);
    if (rc == REID_OK && hipEventRecord(up_ev[0], cs) != hipSuccess) rc = REID_ERR_HIP;
    for (int k = 0; k < passes && rc == REID_OK; ++k) {
        span(k, &i, &m);
        if (hipStreamWaitEvent(ctx->stream, up_ev[k], 0) != hipSuccess) { rc = REID_ERR_HIP; break; }
        if ((rc = run(i, m)) != REID_OK) break;
        if (hipEventRecord(run_ev[k], ctx->stream) != hipSuccess) { rc = REID_ERR_HIP; break; }
        if (k + 1 < passes) {
            span(k + 1, &i, &m);
            if ((rc = up(i, m, cs)) != REID_OK) break;
            if (hipEventRecord(up_ev[k + 1], cs) != hipSuccess) { rc = REID_ERR_HIP; break; }
        }
        if (k >= 1) {
            span(k - 1, &i, &m);
            if (hipStreamWaitEvent(cs, run_ev[k - 1], 0) != hipSuccess) { rc = REID_ERR_HIP; break; }
            if ((rc = down(i, m, cs)) != REID_OK) break;
        }
    }
    if (rc == REID_OK) {
        span(passes - 1, &i, &m);
        if (hipStreamWaitEvent(cs, run_ev[passes - 1], 0) != hipSuccess) rc = REID_ERR_HIP;
        else rc = down(i, m, cs);
    }
    // both streams are drained on every path: the caller's buffers must not be touched after the call returns
    const hipError_t e1 = hipStreamSynchronize(cs), e2 = hipStreamSynchronize(ctx->stream);
    if (rc == REID_OK && (e1 != hipSuccess || e2 != hipSuccess)) {
        reid_set_error("host_passes: stream synchronisation -> %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
        rc = REID_ERR_HIP;
    }
    return rc;
}

// ---- The host entry points of both backbones (api.hip, swin.hip) are built from the pieces below: a source that knows how to bring items
// [i, i + m) to the device (a dense array: a lambda in the entry; ragged crops or windows of one frame: RaggedSrc), the entry's own
// "run one pass" lambda, and EmbedOut for the way back.  Definitions of the non-templates: api.hip.

// Where the embeddings [n][dim] (and logits [n][nc], optional) of a call go on the host, and their device buffers.
struct EmbedOut {
    float *emb, *logits;   // host (the entry's arguments; logits may be null)
    int dim, nc;
    float *d_emb = nullptr, *d_log = nullptr;
    // <tag>.emb for n + pad_rows rows and, when wanted, <tag>.logits (16 bytes of slack: the classifier GEMM stores whole vectors)
    int alloc(reid_ctx* ctx, const char* tag, int n, int pad_rows, bool want_logits);
    int down(int i, int m, hipStream_t s) const;   // queues the download of rows [i, i + m)
};

// n uint8 windows of one host buffer: packed crops (pitch 0: window i is hw[2i] x hw[2i + 1] pixels at byte offsets[i], its rows one after
// the other) or windows of ONE frame `pitch` pixels wide (frame()).  On the device: <tag>.in and <tag>.meta = [offsets n x 8 | hw n x 8].
struct RaggedSrc {
    const uint8_t* src = nullptr;
    const int64_t* offsets = nullptr;
    const int32_t* hw = nullptr;
    int n = 0;
    int pitch = 0;
    size_t total = 0;   // bytes of src that go up: the highest end of a crop, or the whole frame
    uint8_t* d_src = nullptr;
    long long* d_off = nullptr;
    int* d_hw = nullptr;
    std::vector<int64_t> win;   // a frame source's own [offsets | hw]: offsets / hw point into it, so a RaggedSrc is not copied
    RaggedSrc() = default;
    RaggedSrc(const uint8_t* packed, const int64_t* offsets_, const int32_t* hw_, int n_) : src(packed), offsets(offsets_), hw(hw_), n(n_) {}
    RaggedSrc(const RaggedSrc&) = delete;
    RaggedSrc& operator=(const RaggedSrc&) = delete;
    int check();                // packed crops: every crop has pixels and a non-negative offset (REID_ERR_ARG); sets total
    int frame(const uint8_t* frame_u8, int fh, int fw, const int32_t* boxes_xyxy, int n_boxes);   // windows_from_boxes into `win`
    int alloc(reid_ctx* ctx, const char* tag);
    // The bytes items [i, i + m) read: packed crops, the span [lowest offset, highest end) - crop after crop, the usual packing, makes
    // the passes' spans a partition of the buffer, any other layout copies some bytes twice, which is harmless; a frame, all of it at
    // i == 0 and nothing afterwards.  Behind them, at i == 0, the metadata of all n items, in one copy when hw directly follows offsets
    // (Engine._pack_ragged's arrays need not; the frame pipeline's pinned block and a frame source do).
    int up(int i, int m, hipStream_t s) const;
};
// boxes (x1, y1, x2, y2) inside an fh x fw frame -> byte offsets and (h, w) of the windows frame[y1:y2, x1:x2]; REID_ERR_ARG for an empty
// or out-of-frame box
int windows_from_boxes(const int32_t* boxes_xyxy, int n, int fh, int fw, int64_t* off, int32_t* hw);

// host_passes, the embeddings (and logits) back through `out`, and the fault word.  run(i, m, d_emb_i, d_log_i) queues the kernels of
// items [i, i + m) on ctx->stream; d_log_i is null when no logits are wanted.
template <class Up, class Run>
int embed_host(reid_ctx* ctx, int n, int pass, Up up, Run run, const EmbedOut& out) {
    const int rc = host_passes(
        ctx, n, pass, up,
        [&](int i, int m) -> int { return run(i, m, out.d_emb + (size_t)i * out.dim, out.d_log ? out.d_log + (size_t)i * out.nc : nullptr); },
        [&](int i, int m, hipStream_t s) -> int { return out.down(i, m, s); });
    if (rc != REID_OK) {   // host_passes' one-pass branch returns at the first error: no copy from the caller's buffers, or from a
        (void)hipStreamSynchronize(ctx->stream);   // frame source's own metadata, stays queued behind this call
        return rc;
    }
    return ctx_fault_status(ctx);
}
// the passes of an entry whose operands are on the device already: run(i, m), nothing else
template <class Run>
int embed_dev_passes(int n, int pass, Run run) {
    for (int i = 0; i < n; i += pass) REID_TRY(run(i, n - i < pass ? n - i : pass));
    return REID_OK;
}
// The frame pipeline's way in (bank.hip: one buffer set per frame slot): RaggedSrc + EmbedOut under `tag` with NO synchronisation and no
// download.  ragged_enqueue_begin checks the crops, allocates <tag>.in / .meta / .emb (one row more than n: the padding row of
// reid_frame_gather) / .logits and queues the upload - side_copy: on the context's copy stream, beside the previous frame's kernels, the
// compute stream waiting for it.  offsets / hw must be pinned or outlive the stream's work.  The pass loop that follows is the backbone's:
// embed_ragged_enqueue (api.hip) runs ResNet18-SE passes of `chunk` crops, swin_ragged_enqueue (swin.hip) swin_forward_crops in passes
// of swin_pass(ctx) crops to out_h x out_w (*dim_out = the loaded Swin's embed_dim).  swin_ragged_ready: everything the latter would
// refuse, checked with nothing queued - arguments (REID_ERR_ARG), loaded weights and libreid_hip_swin_crops.so (REID_ERR_STATE).
int ragged_enqueue_begin(reid_ctx* ctx, const char* tag, RaggedSrc& src, EmbedOut& out, bool want_logits, bool side_copy);
int embed_ragged_enqueue(reid_ctx* ctx, const char* tag, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n,
                         float** d_emb_out, float** d_log_out, bool side_copy);
int swin_ragged_ready(reid_ctx* ctx, int out_h, int out_w, const float** mean_std6, int* dim_out);
int swin_ragged_enqueue(reid_ctx* ctx, const char* tag, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n, int out_h,
                        int out_w, const float* mean_std6, float** d_emb_out, bool side_copy);
// bank.hip: the launch of the frame pipeline's cost stage on the caller's device operands (metric 0 cosine / 1 squared euclidean; a
// 96-wide bank with bank_fast on takes bank_cost96_kernel of libreid_hip_bank96.so), and a bank's sizes - for reid_debug_bank_cost96
int bank_frame_cost_launch(reid_ctx* ctx, reid_bank* b, const int32_t* d_slots, int t, const float* d_dets, int m, int metric, float max_dist,
                           float* d_out);
int bank_geometry(const reid_bank* b, int* max_tracks, int* budget, int* d);
// ---- The loader of the libraries that lie beside this one and are opened on first use (api.hip).  A library is described once, as a
// struct derived from SideLib: its file, its "<what> needs" text, and one SIDE_FN member per function it exports, in the order a missing
// symbol is reported in.  SIDE_FN takes the pointer type from the side header's declaration (decltype: unevaluated, so no reference to the
// side library reaches this one's symbol table) and the symbol name from the same token; the member is then called like the function.
//   open(): under the library's mutex, once: dlopen (RTLD_NOW | RTLD_LOCAL) from the directory this library lies in, then every symbol.
//     A missing file ("<what> <path> beside libreid_hip.so: <dlerror>") or symbol ("<path> lacks a / b", the handle closed again) is
//     REID_ERR_STATE and leaves the library unloaded: the next call tries again and reports again.
//   status(e, fn): the hipError_t of a launch function of the library as a status: hipSuccess REID_OK; otherwise
//     "<file> <fn> -> <hip error>", hipErrorInvalidValue REID_ERR_ARG, anything else REID_ERR_HIP.
struct SideSym {
    const char* name;
    void* p = nullptr;
};
struct SideLib {
    SideLib(const char* file, const char* what) : file(file), what(what) {}
    SideLib(const SideLib&) = delete;
    int open();
    int status(hipError_t e, const SideSym& fn) const;
    void add(SideSym* s) { syms.push_back(s); }
    const char* const file;
    const char* const what;

private:
    std::mutex m;
    std::vector<SideSym*> syms;
    bool loaded = false;
};
template <class F>
struct SideFn;
template <class R, class... A>
struct SideFn<R (*)(A...)> : SideSym {
    SideFn(SideLib* lib, const char* name) : SideSym{name} { lib->add(this); }
    R operator()(A... a) const { return ((R(*)(A...))p)(a...); }
};
#define SIDE_FN(member, fn) SideFn<decltype(&fn)> member{this, #fn}
// ---- ResNet18-IBN-SE at input sizes other than 256 x 128 (api.hip; kernels: anysize.h).  The reid_*_hw entries hand 256 x 128 to the
// existing entries unless the debug switch anysize_force is set (se_any_routes).  se_any_ready: everything such a call would refuse, with
// nothing queued - a side outside 32 .. 512 (REID_ERR_ARG), weights not loaded (REID_ERR_STATE), an architecture other than seres18_ibn
// (or, with reid_ctx_set_hw_siblings 1, cares18_ibn, which then needs libreid_hip_anysize_ca.so: REID_ERR_STATE; with reid_ctx_set_hw_ema 1,
// emares18_ibn, which then needs libreid_hip_anysize_ema.so: REID_ERR_STATE) or
// a precision mode other than 0 while reid_ctx_set_hw_precision is -1 (REID_ERR_ARG naming both), libreid_hip_anysize.so and, at
// hw_precision 2, libreid_hip_anysize_x3.so (REID_ERR_STATE).  With reid_ctx_set_hw_f16 1 instead: an architecture other than seres18_ibn
// (REID_ERR_ARG naming it, whatever hw_siblings / hw_ema), libreid_hip_anysize.so and libreid_hip_anysize_f16.so (REID_ERR_STATE); the mode
// and hw_precision are not looked at.  With reid_ctx_set_hw_sib_f16 1 and a sibling loaded, before all of these: libreid_hip_anysize.so,
// libreid_hip_anysize_f16.so and libreid_hip_anysize_sib_f16.so (REID_ERR_STATE), no other setting is looked at.  se_any_pass: images per pass, the
// context's chunk scaled by 256 * 128 / (h * w) and clamped to 1 .. 4096.  se_any_run_nchw: one pass from fp32 NCHW [m][3][h][w] on the
// device (mirror: the horizontally flipped view); se_any_run_windows: from uploaded uint8 windows through the cv2-style resize.
struct RaggedSrc;
bool se_any_routes(const reid_ctx* ctx, int h, int w);
int se_any_ready(reid_ctx* ctx, int h, int w, const char* who);
int se_any_pass(const reid_ctx* ctx, int h, int w);
int se_any_run_nchw(reid_ctx* ctx, const float* d_x, int m, int h, int w, int mirror, float* d_emb, float* d_log);
// The frame pipeline at out_h x out_w (reid_frame_submit_hw, reid_embed_frame_u8_hw).  se_any_front_ready: what such a call refuses, with
// nothing queued - *mean_std6 NULL becomes 0.5 / 0.5, a value that is not finite or a std <= 0 is REID_ERR_ARG, then se_any_ready's rules,
// at 256 x 128 another mean_std6 than 0.5 / 0.5 (REID_ERR_ARG), elsewhere libreid_hip_anysize_front.so (REID_ERR_STATE; not with
// reid_ctx_set_hw_f16 1, whose passes never take the fused front end).
// any_ragged_enqueue: ragged_enqueue_begin + passes of se_any_pass crops, as embed_ragged_enqueue.  launch_any_front: the front end of
// one pass on uploaded windows -> pool [n][H2][W2][64]; fused 1 = any_front_kernel, 0 = resize, stem GEMM (into stem [n][H1][W1][64]) and
// max-pool, the same bits - the forward and reid_debug_any_front call this one function.
int se_any_front_ready(reid_ctx* ctx, int h, int w, const float** mean_std6, const char* who);
int any_ragged_enqueue(reid_ctx* ctx, const char* tag, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n, int out_h,
                       int out_w, const float* mean_std6, float** d_emb_out, bool side_copy);
int launch_any_front(reid_ctx* ctx, int fused, const uint8_t* d_src, const long long* d_off, const int* d_hw, int n, int h, int w, int pitch,
                     const float* mean_std6, const float* stem_w, const float* scale, const float* shift, float* stem, float* pool);
// debug.hip harnesses: the three kernel families of libreid_hip_anysize.so on device operands, with the context's profiling slot
int launch_any_norm(reid_ctx* ctx, float* x, int n, int hw, int c, int half, const float* in_gamma, const float* in_beta, const float* bn_scale,
                    const float* bn_shift);
int launch_any_se_tail(reid_ctx* ctx, const float* y, const float* sc, int n, int hw, int c, int mid, const float* w1, const float* w2t,
                       float* out, float* gate_out);
int launch_any_gem(reid_ctx* ctx, const float* x, int n, int hw, int c, const float* p, const float* scale, const float* shift, float* gem_out,
                   float* emb);
// the TripletAttention tail of the any-size trunk (cares18_ibn; anysize_ca.h) on device operands [n][H][W][C], prm = Se18Block::ta; the
// workspace ("any.ca", anysize_ca_workspace_bytes) comes from ctx_ws.  maps_out / gates_out (may be NULL): where the call's maps and gates
// lie in it, in the layout of anysize_ca.h, valid until the next call.  The forward and reid_debug_any_ca_tail call this one function.
int launch_any_ca_tail(reid_ctx* ctx, const float* y, const float* sc, int n, int H, int W, int C, const float* prm, float* out,
                       const float** maps_out = nullptr, const float** gates_out = nullptr);
// the EMA tail of the any-size trunk (emares18_ibn with reid_ctx_set_hw_ema 1; anysize_ema.h) on device operands [n][H][W][C], prm =
// Se18Block::ema; the workspace ("any.ema", anysize_ema_workspace_bytes) comes from ctx_ws.  sig_out / small_out (may be NULL): where the
// call's sigmoid vectors [n][H + W][C] and mu | rstd | s1 | s2 [n][4][C] lie in it, valid until the next call.  The forward and
// reid_debug_any_ema_tail call this one function.
int launch_any_ema_tail(reid_ctx* ctx, const float* y, const float* sc, int n, int H, int W, int C, const float* prm, float* out,
                        const float** sig_out = nullptr, const float** small_out = nullptr);
// one trunk convolution of the any-size forward (NHWC fp32 in / out, folded BN, identity residual, ReLU from column relu_from on) in the
// arithmetic `arith`: 0 = launch_gemm_f32 (exact fp32), 2 = any_conv_x3_kernel of libreid_hip_anysize_x3.so (fp32-class; R = 3 pad 1 or
// R = 1 pad 0) on the cached split form of wgt.  The forward and reid_debug_any_conv call this one function.
int launch_any_conv(reid_ctx* ctx, int arith, const float* x, int n, int H, int W, int Cin, const float* wgt, int Cout, int R, int stride, int pad,
                    const float* scale, const float* shift, const float* residual, int relu, int relu_from, float* out);
// The any-size forward in fp16 storage (reid_ctx_set_hw_f16 1; kernels: anysize_f16.h) on device operands, NHWC f16 activations, with the
// context's profiling slot.  The forward and the reid_debug_any_*_f16 harnesses call these functions.  launch_any_conv_f16: w16 f16
// [Cout][R R][Cin]; the tile form lands in ctx->any_f16_form.  launch_any_stem_f16: x fp32 NHWC [n][h][w][3], w16 [64][192] f16.
int launch_any_conv_f16(reid_ctx* ctx, const _Float16* x, int n, int H, int W, int Cin, const _Float16* w16, int Cout, int R, int stride, int pad,
                        const float* scale, const float* shift, const _Float16* residual, int relu, int relu_from, _Float16* out);
int launch_any_stem_f16(reid_ctx* ctx, const float* x, int n, int h, int w, const _Float16* w16, const float* scale, const float* shift,
                        _Float16* out);
int launch_any_maxpool_f16(reid_ctx* ctx, const _Float16* x, int n, int h, int w, int c, _Float16* out);
int launch_any_norm_f16(reid_ctx* ctx, _Float16* x, int n, int hw, int c, int half, const float* in_gamma, const float* in_beta);
int launch_any_se_tail_f16(reid_ctx* ctx, const _Float16* y, const _Float16* sc, int n, int hw, int c, int mid, const float* w1,
                           const float* w2t, _Float16* out, float* gate_out);
int launch_any_gem_f16(reid_ctx* ctx, const _Float16* x, int n, int hw, int c, const float* p, const float* scale, const float* shift,
                       float* gem_out, float* emb);
// the TripletAttention / EMA tails of the any-size trunk on f16 maps (cares18_ibn / emares18_ibn with reid_ctx_set_hw_sib_f16 1;
// anysize_sib_f16.h): launch_any_ca_tail / launch_any_ema_tail with f16 y, shortcut and out; the workspaces keep their names ("any.ca",
// "any.ema"), sizes and layouts, so maps_out / gates_out and sig_out / small_out mean what they mean there.  The forward and the
// reid_debug_any_ca_tail_f16 / reid_debug_any_ema_tail_f16 harnesses call these functions.
int launch_any_ca_tail_f16(reid_ctx* ctx, const _Float16* y, const _Float16* sc, int n, int H, int W, int C, const float* prm, _Float16* out,
                           const float** maps_out = nullptr, const float** gates_out = nullptr);
int launch_any_ema_tail_f16(reid_ctx* ctx, const _Float16* y, const _Float16* sc, int n, int H, int W, int C, const float* prm, _Float16* out,
                            const float** sig_out = nullptr, const float** small_out = nullptr);
void prof_begin(reid_ctx* ctx, int kind, double flops, double bytes);
void prof_end(reid_ctx* ctx);

#define LAUNCH_CHECK()                                                                 \
    do {                                                                               \
        hipError_t _e = hipGetLastError();                                             \
        if (_e != hipSuccess) {                                                        \
            reid_set_error("%s:%d kernel launch -> %s", __FILE__, __LINE__, hipGetErrorString(_e)); \
            return REID_ERR_HIP;                                                       \
        }                                                                              \
    } while (0)
