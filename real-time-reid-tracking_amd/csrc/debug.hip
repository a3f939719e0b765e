// Kernel experiments and correctness harnesses (include/reid_hip_debug.h).  Built into libreid_hip_debug.so, which links
// against libreid_hip.so: nothing here is part of the product library or of the drop-in C ABI.
#include "reid_internal.h"
#include "pil_launch.h"
#include "anysize_ema.h"
#include <string.h>
#include <stdlib.h>
#include <vector>

// ------------------------------------------------------------------------------------------------ experiment switches
// Every kernel-selection / arithmetic-form / summation-order switch of a context, by the name of its reid_ctx field.  Until round 5
// these were environment variables read by reid_ctx_create in the PRODUCT library (a stray REID_* in a tracker's environment
// silently changed embeddings); now the product library has fixed defaults and only this library can move them.
namespace {
struct Switch { const char* name; int reid_ctx::* field; };
const Switch kSwitches[] = {
    {"f16_cfg", &reid_ctx::f16_cfg}, {"f16_lin_256", &reid_ctx::f16_lin_256}, {"f16_split_k", &reid_ctx::f16_split_k},
    {"bank_fast", &reid_ctx::bank_fast}, {"side_copy", &reid_ctx::side_copy}, {"f32_stem_pool", &reid_ctx::f32_stem_pool},
    {"stem_split", &reid_ctx::stem_split}, {"split_pair", &reid_ctx::split_pair}, {"split_lean_epi", &reid_ctx::split_lean_epi},
    {"knn_wide", &reid_ctx::knn_wide}, {"f16_loader_prio", &reid_ctx::f16_loader_prio}, {"f16_frag_ahead", &reid_ctx::f16_frag_ahead},
    {"pack_epilogue", &reid_ctx::pack_epilogue}, {"f16_wide_splitk", &reid_ctx::f16_wide_splitk}, {"f32_split_k", &reid_ctx::f32_split_k},
    {"swin_fold", &reid_ctx::swin_fold}, {"swin_stop", &reid_ctx::swin_stop}, {"select_two_pass", &reid_ctx::select_two_pass},
    {"split_terms", &reid_ctx::split_terms}, {"f32_conv", &reid_ctx::f32_conv}, {"swin_attn_mfma", &reid_ctx::swin_attn_mfma},
    {"swin_attn_split", &reid_ctx::swin_attn_split}, {"swin_two_linear", &reid_ctx::swin_two_linear},
    {"f16_loader_waves", &reid_ctx::f16_loader_waves}, {"f16_halo", &reid_ctx::f16_halo}, {"f16_stem_fused", &reid_ctx::f16_stem_fused},
    {"f16_se_tail", &reid_ctx::f16_se_tail}, {"f16_c64", &reid_ctx::f16_c64}, {"swin_chunk_cap", &reid_ctx::swin_chunk_cap},
    {"split_x3", &reid_ctx::split_x3}, {"x3_ablate", &reid_ctx::x3_ablate}, {"x3_unroll", &reid_ctx::x3_unroll}, {"x3_narrow", &reid_ctx::x3_narrow}, {"conv_x3s", &reid_ctx::conv_x3s}, {"x3s_sk_cap", &reid_ctx::x3s_sk_cap}, {"x3_l4_narrow_nmt", &reid_ctx::x3_l4_narrow_nmt}, {"split_x3_small", &reid_ctx::split_x3_small}, {"split_x3_min_blocks", &reid_ctx::split_x3_min_blocks}, {"f32_dist_bk16", &reid_ctx::f32_dist_bk16}, {"lin_x3", &reid_ctx::lin_x3},
    {"host_pipeline", &reid_ctx::host_pipeline}, {"x3_sk_cap", &reid_ctx::x3_sk_cap}, {"chain", &reid_ctx::chain}, {"split_gemm_min_tiles", &reid_ctx::split_gemm_min_tiles},
    {"rerank_hbm_acc", &reid_ctx::rerank_hbm_acc}, {"gem_tail_min", &reid_ctx::gem_tail_min}, {"anysize_force", &reid_ctx::anysize_force},
    {"any_front", &reid_ctx::any_front}, {"any_ca", &reid_ctx::any_ca}, {"any_ema", &reid_ctx::any_ema},
};
}  // namespace

extern "C" int reid_debug_set_switch(reid_ctx* ctx, const char* name, long long value) {
    ARG_CHECK(ctx && name);
    CTX_GUARD(ctx);
    HIP_TRY(hipStreamSynchronize(ctx->stream));       // nothing in flight may see the switch move
    if (!strcmp(name, "knn_wide_min")) {
        ctx->knn_wide_min = value;
        return REID_OK;
    }
    for (const Switch& s : kSwitches)
        if (!strcmp(name, s.name)) {
            if (!strcmp(name, "split_terms") && value != 3 && value != 4) break;
            ctx->*(s.field) = (int)value;
            return REID_OK;
        }
    reid_set_error("reid_debug_set_switch: no switch '%s' (or a value it does not take)", name);
    return REID_ERR_ARG;
}

extern "C" int reid_debug_get_switch(reid_ctx* ctx, const char* name, long long* value) {
    ARG_CHECK(ctx && name && value);
    if (!strcmp(name, "knn_wide_min")) {
        *value = ctx->knn_wide_min;
        return REID_OK;
    }
    for (const Switch& s : kSwitches)
        if (!strcmp(name, s.name)) {
            *value = ctx->*(s.field);
            return REID_OK;
        }
    reid_set_error("reid_debug_get_switch: no switch '%s'", name);
    return REID_ERR_ARG;
}

// ------------------------------------------------------------------------------------------------ kernel experiments
// Times `iters` launches of one fp16 implicit-GEMM convolution on random device data (not part of the public header).
extern "C" int reid_debug_conv_f16(reid_ctx* ctx, int n, int h, int w, int cin, int cout, int r, int stride, int pad, int cfg,
                                   int iters, float* ms_per_launch) {
    ARG_CHECK(ctx && ms_per_launch && ctx->se18.loaded);
    CTX_GUARD(ctx);
    typedef _Float16 f16;
    const int ho = (h + 2 * pad - r) / stride + 1, wo = (w + 2 * pad - r) / stride + 1;
    const size_t nin = (size_t)n * h * w * cin, nw = (size_t)cout * r * r * cin, nout = (size_t)n * ho * wo * cout;
    f16 *x, *wt, *out;
    REID_TRY(ctx_ws(ctx, "dbg.x", nin * 2, (void**)&x));
    REID_TRY(ctx_ws(ctx, "dbg.w", nw * 2, (void**)&wt));
    REID_TRY(ctx_ws(ctx, "dbg.out", nout * 2, (void**)&out));
    // random-ish operands: the loaded weight blob (f32 -> f16), cycled
    const size_t src_n = ctx->se18.n_floats;
    for (size_t o = 0; o < nin; o += src_n) REID_TRY(launch_f32_to_f16(ctx, ctx->se18.blob, nin - o < src_n ? nin - o : src_n, x + o));
    for (size_t o = 0; o < nw; o += src_n) REID_TRY(launch_f32_to_f16(ctx, ctx->se18.blob, nw - o < src_n ? nw - o : src_n, wt + o));
    if (getenv("REID_DEBUG_ZERO")) {   // clock experiment: all-zero operands draw less power (DVFS give-back)
        HIP_TRY(hipMemsetAsync(x, 0, nin * 2, ctx->stream));
        HIP_TRY(hipMemsetAsync(wt, 0, nw * 2, ctx->stream));
    }
    const int c0 = ctx->f16_cfg;
    const int h0 = ctx->f16_halo;
    ctx->f16_halo = cfg >= 2000000 ? 2 : 0;   // 2xxxxxx: force the LDS-halo kernel, 2000001: with loader waves
    const int l0 = ctx->f16_loader_waves;
    if (cfg >= 2000000) ctx->f16_loader_waves = cfg & 1;
    ctx->f16_cfg = cfg >= 2000000 ? 0 : cfg;
    int st = REID_OK;
    for (int i = 0; i < 2 && st == REID_OK; ++i)
        st = conv_gemm16(ctx, A16_IM2COL, x, n, h, w, cin, wt, cout, r, r, stride, pad, r * r * cin, nullptr, nullptr, nullptr, 0, nullptr, out);
    if (st == REID_OK) st = reid_timer_start(ctx);
    for (int i = 0; i < iters && st == REID_OK; ++i)
        st = conv_gemm16(ctx, A16_IM2COL, x, n, h, w, cin, wt, cout, r, r, stride, pad, r * r * cin, nullptr, nullptr, nullptr, 0, nullptr, out);
    float ms = 0.f;
    if (st == REID_OK) st = reid_timer_stop(ctx, &ms);
    ctx->f16_cfg = c0;
    ctx->f16_halo = h0;
    ctx->f16_loader_waves = l0;
    *ms_per_launch = ms / (iters > 0 ? iters : 1);
    return st;
}


// Times `iters` launches of one fp32-class 3x3 stride-1 convolution (SPLIT build of the LDS-halo kernel: c real channels as
// [xh | xl'] against [wh 2^11 | wh | wl'] weights, fp32 out with BN + ReLU epilogue) on operands cut from the loaded weight blob.
// ablate: experiment switches of the PAIR loop (Gemm16Params.ablate; results are then wrong): 1 no weight DMA after the first step,
// 2 no halo DMA after the first phase, 4 no MFMAs, 8 no fragment reads, 16 no block barriers.
extern "C" int reid_debug_conv_split(reid_ctx* ctx, int n, int h, int w, int c, int cout, int ablate, int iters, float* ms_per_launch) {
    ARG_CHECK(ctx && ms_per_launch && ctx->se18.loaded && c % 64 == 0 && cout % 64 == 0);
    CTX_GUARD(ctx);
    typedef _Float16 f16;
    const size_t nin = (size_t)n * h * w * 2 * c, nw = (size_t)cout * 9 * 3 * c, nout = (size_t)n * h * w * cout;
    f16 *x, *wt;
    float *out, *sc;
    REID_TRY(ctx_ws(ctx, "dbgs.x", nin * 2, (void**)&x));
    REID_TRY(ctx_ws(ctx, "dbgs.w", nw * 2, (void**)&wt));
    REID_TRY(ctx_ws(ctx, "dbgs.out", nout * 4, (void**)&out));
    REID_TRY(ctx_ws(ctx, "dbgs.sc", (size_t)cout * 2 * 4, (void**)&sc));
    const size_t src_n = ctx->se18.n_floats;
    for (size_t o = 0; o < nin; o += src_n) REID_TRY(launch_f32_to_f16(ctx, ctx->se18.blob, nin - o < src_n ? nin - o : src_n, x + o));
    for (size_t o = 0; o < nw; o += src_n) REID_TRY(launch_f32_to_f16(ctx, ctx->se18.blob, nw - o < src_n ? nw - o : src_n, wt + o));
    HIP_TRY(hipMemcpyAsync(sc, ctx->se18.blob, (size_t)cout * 2 * 4, hipMemcpyDeviceToDevice, ctx->stream));
    if (ablate & 128) {   // clock experiment: all-zero operands draw less power (is the kernel power-limited?)
        HIP_TRY(hipMemsetAsync(x, 0, nin * 2, ctx->stream));
        HIP_TRY(hipMemsetAsync(wt, 0, nw * 2, ctx->stream));
    }
    Gemm16Params q;
    memset(&q, 0, sizeof(q));
    q.split_terms = 3;
    q.H = h; q.W = w; q.Cin = 3 * c; q.R = 3; q.S = 3; q.stride = 1; q.pad = 1; q.Ho = h; q.Wo = w;
    q.M = n * h * w; q.N = cout; q.K = 27 * c; q.ldb = q.K;
    q.A = x; q.B = wt; q.C32 = out; q.ldc = cout;
    q.col_scale = sc; q.col_shift = sc + cout; q.relu = 1;
    q.acc_scale = 1.0f / 2048.0f;
    q.zero_page = ctx->se18.zero_page;
    q.ablate = ablate & 127;
    q.diag = ctx->conv_diag;
    int st = REID_OK;
    for (int i = 0; i < 2 && st == REID_OK; ++i) st = launch_conv3x3_split(ctx, q, REID_K_CONV_GEMM, 0, 0);
    if (st == REID_OK) st = reid_timer_start(ctx);
    for (int i = 0; i < iters && st == REID_OK; ++i) st = launch_conv3x3_split(ctx, q, REID_K_CONV_GEMM, 0, 0);
    float ms = 0.f;
    if (st == REID_OK) st = reid_timer_stop(ctx, &ms);
    *ms_per_launch = ms / (iters > 0 ? iters : 1);
    return st;
}

// Correctness harness for conv3x3_c64_f16.hip (tests only, not part of the C ABI): fp32 host operands are rounded to f16,
// the kernel runs once, the f16 result and the fp32 per-image statistics come back as fp32.
extern "C" int reid_debug_conv_c64(reid_ctx* ctx, int n, const float* x, const float* w_krsc, const float* scale,
                                   const float* shift, const float* residual, int relu, float* out, float* stats) {
    ARG_CHECK(ctx && x && w_krsc && out && n >= 1);
    CTX_GUARD(ctx);
    typedef _Float16 f16;
    const size_t nact = (size_t)n * 64 * 32 * 64, nw = 64 * 576;
    float *xf, *wf, *rf = nullptr, *sc = nullptr, *sh = nullptr, *st = nullptr, *of;
    f16 *xh, *wh, *rh = nullptr, *oh, *zp;
    REID_TRY(ctx_ws(ctx, "dbg64.xf", nact * 4, (void**)&xf));
    REID_TRY(ctx_ws(ctx, "dbg64.wf", nw * 4, (void**)&wf));
    REID_TRY(ctx_ws(ctx, "dbg64.xh", nact * 2, (void**)&xh));
    REID_TRY(ctx_ws(ctx, "dbg64.wh", nw * 2, (void**)&wh));
    REID_TRY(ctx_ws(ctx, "dbg64.oh", nact * 2, (void**)&oh));
    REID_TRY(ctx_ws(ctx, "dbg64.of", nact * 4, (void**)&of));
    REID_TRY(ctx_ws(ctx, "dbg64.zp", 256, (void**)&zp));
    REID_TRY(ctx_ws(ctx, "dbg64.sc", 64 * 4, (void**)&sc));
    REID_TRY(ctx_ws(ctx, "dbg64.sh", 64 * 4, (void**)&sh));
    REID_TRY(ctx_ws(ctx, "dbg64.st", (size_t)n * 128 * 4, (void**)&st));
    HIP_TRY(hipMemsetAsync(zp, 0, 256, ctx->stream));
    HIP_TRY(hipMemcpyAsync(xf, x, nact * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(wf, w_krsc, nw * 4, hipMemcpyHostToDevice, ctx->stream));
    std::vector<float> ones(64, 1.f);
    HIP_TRY(hipMemcpyAsync(sc, scale ? scale : ones.data(), 64 * 4, hipMemcpyHostToDevice, ctx->stream));
    if (shift) HIP_TRY(hipMemcpyAsync(sh, shift, 64 * 4, hipMemcpyHostToDevice, ctx->stream));
    REID_TRY(launch_f32_to_f16(ctx, xf, nact, xh));
    REID_TRY(launch_scale_rows_f16(ctx, wf, sc, 64, 576, wh));
    if (residual) {
        REID_TRY(ctx_ws(ctx, "dbg64.rf", nact * 4, (void**)&rf));
        REID_TRY(ctx_ws(ctx, "dbg64.rh", nact * 2, (void**)&rh));
        HIP_TRY(hipMemcpyAsync(rf, residual, nact * 4, hipMemcpyHostToDevice, ctx->stream));
        REID_TRY(launch_f32_to_f16(ctx, rf, nact, rh));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));   // `ones` is a local
    REID_TRY(launch_conv3x3_c64_f16(ctx, xh, n, wh, shift ? sh : nullptr, rh, relu, stats ? st : nullptr, oh, zp));
    std::vector<f16> tmp(nact);
    HIP_TRY(hipMemcpyAsync(tmp.data(), oh, nact * 2, hipMemcpyDeviceToHost, ctx->stream));
    if (stats) HIP_TRY(hipMemcpyAsync(stats, st, (size_t)n * 128 * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < nact; ++i) out[i] = (float)tmp[i];
    return REID_OK;
}

// Times one dense fp16 GEMM C[m][n] = A[m][k] . B[n][k]^T (experiments: separates the im2col gather from the tile loop).
extern "C" int reid_debug_gemm_f16(reid_ctx* ctx, int m, int n, int k, int cfg, int iters, float* ms_per_launch,
                                   unsigned long long* diag_host /* [64*8*4] or NULL */) {
    ARG_CHECK(ctx && ms_per_launch && ctx->se18.loaded);
    CTX_GUARD(ctx);
    unsigned long long* d_diag = nullptr;
    if (diag_host) {
        REID_TRY(ctx_ws(ctx, "dbg.diag", 64 * 8 * 4 * 8, (void**)&d_diag));
        HIP_TRY(hipMemsetAsync(d_diag, 0, 64 * 8 * 4 * 8, ctx->stream));
    }
    typedef _Float16 f16;
    f16 *a, *b, *c;
    REID_TRY(ctx_ws(ctx, "dbg.x", (size_t)m * k * 2, (void**)&a));
    REID_TRY(ctx_ws(ctx, "dbg.w", (size_t)n * k * 2, (void**)&b));
    REID_TRY(ctx_ws(ctx, "dbg.out", (size_t)m * n * 2, (void**)&c));
    const size_t src_n = ctx->se18.n_floats;
    for (size_t o = 0; o < (size_t)m * k; o += src_n)
        REID_TRY(launch_f32_to_f16(ctx, ctx->se18.blob, (size_t)m * k - o < src_n ? (size_t)m * k - o : src_n, a + o));
    for (size_t o = 0; o < (size_t)n * k; o += src_n)
        REID_TRY(launch_f32_to_f16(ctx, ctx->se18.blob, (size_t)n * k - o < src_n ? (size_t)n * k - o : src_n, b + o));
    Gemm16Params p;
    memset(&p, 0, sizeof(p));
    p.A = a; p.lda = k; p.B = b; p.ldb = k; p.M = m; p.N = n; p.K = k; p.C = c; p.ldc = n;
    p.zero_page = ctx->se18.zero_page;
    p.diag = d_diag;
    const int c0 = ctx->f16_cfg;
    ctx->f16_cfg = cfg;
    int st = REID_OK;
    for (int i = 0; i < 2 && st == REID_OK; ++i) st = launch_gemm_f16(ctx, A16_DENSE, p, REID_K_CONV_GEMM, 0, 0);
    if (st == REID_OK) st = reid_timer_start(ctx);
    for (int i = 0; i < iters && st == REID_OK; ++i) st = launch_gemm_f16(ctx, A16_DENSE, p, REID_K_CONV_GEMM, 0, 0);
    float ms = 0.f;
    if (st == REID_OK) st = reid_timer_stop(ctx, &ms);
    ctx->f16_cfg = c0;
    *ms_per_launch = ms / (iters > 0 ? iters : 1);
    if (st == REID_OK && diag_host) {
        HIP_TRY(hipMemcpyAsync(diag_host, d_diag, 64 * 8 * 4 * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return st;
}

extern "C" int reid_debug_conv_diag(reid_ctx* ctx, int enable, unsigned long long* out_host /* [64*8*4] when disabling */) {
    ARG_CHECK(ctx);
    CTX_GUARD(ctx);
    if (enable) {
        REID_TRY(ctx_ws(ctx, "dbg.cdiag", 64 * 8 * 5 * 8, (void**)&ctx->conv_diag));
        HIP_TRY(hipMemsetAsync(ctx->conv_diag, 0, 64 * 8 * 5 * 8, ctx->stream));
    } else {
        if (out_host && ctx->conv_diag) {
            HIP_TRY(hipMemcpyAsync(out_host, ctx->conv_diag, 64 * 8 * 5 * 8, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
        }
        ctx->conv_diag = nullptr;
    }
    return REID_OK;
}

// Times `iters` launches of one exact-fp32 convolution of the ResNet18-SE path on random device data.
// flags: 1 = fused input affine + ReLU (conv2 of an SE block), 2 = BN scale/shift epilogue, 4 = residual + ReLU, 8 = statistics.
// variant: 0 = gemm_f32_kernel<A_IM2COL> (round-1 kernel), 1 = conv_f32.hip.
extern "C" int reid_debug_conv_f32(reid_ctx* ctx, int n, int h, int w, int cin, int cout, int r, int stride, int pad, int flags,
                                   int variant, int iters, float* ms_per_launch) {
    ARG_CHECK(ctx && ms_per_launch && ctx->se18.loaded && n >= 1);
    CTX_GUARD(ctx);
    const int ho = (h + 2 * pad - r) / stride + 1, wo = (w + 2 * pad - r) / stride + 1;
    const size_t nin = (size_t)n * h * w * cin, nw = (size_t)cout * r * r * cin, nout = (size_t)n * ho * wo * cout;
    float *x, *wt, *out, *res, *asc, *ash, *stats;
    REID_TRY(ctx_ws(ctx, "dbg32.x", nin * 4, (void**)&x));
    REID_TRY(ctx_ws(ctx, "dbg32.w", nw * 4, (void**)&wt));
    REID_TRY(ctx_ws(ctx, "dbg32.out", nout * 4, (void**)&out));
    REID_TRY(ctx_ws(ctx, "dbg32.res", nout * 4, (void**)&res));
    REID_TRY(ctx_ws(ctx, "dbg32.asc", (size_t)n * cin * 4, (void**)&asc));
    REID_TRY(ctx_ws(ctx, "dbg32.ash", (size_t)n * cin * 4, (void**)&ash));
    REID_TRY(ctx_ws(ctx, "dbg32.stats", (size_t)n * 2048 * 4 * 16, (void**)&stats));
    // random-ish operands: the loaded weight blob, cycled
    const size_t src_n = ctx->se18.n_floats;
    auto fill = [&](float* dst, size_t cnt) -> int {
        for (size_t o = 0; o < cnt; o += src_n)
            HIP_TRY(hipMemcpyAsync(dst + o, ctx->se18.blob, (cnt - o < src_n ? cnt - o : src_n) * 4, hipMemcpyDeviceToDevice, ctx->stream));
        return REID_OK;
    };
    REID_TRY(fill(x, nin));
    REID_TRY(fill(wt, nw));
    REID_TRY(fill(res, nout));
    REID_TRY(fill(asc, (size_t)n * cin));
    REID_TRY(fill(ash, (size_t)n * cin));
    const int v0 = ctx->f32_conv;
    ctx->f32_conv = variant;
    const float* cs = (flags & 2) ? ctx->se18.neck_scale : nullptr;   // any 512 floats
    const float* sh = (flags & 2) ? ctx->se18.neck_shift : nullptr;
    auto run = [&]() {
        return conv_gemm(ctx, A_IM2COL, x, n, h, w, cin, wt, cout, r, r, stride, pad, r * r * cin, (flags & 1) ? asc : nullptr,
                         (flags & 1) ? ash : nullptr, (flags & 1), cs, sh, (flags & 4) ? res : nullptr, (flags & 4) ? 1 : 0,
                         (flags & 8) ? stats : nullptr, out);
    };
    int st = REID_OK;
    for (int i = 0; i < 2 && st == REID_OK; ++i) st = run();
    if (st == REID_OK) st = reid_timer_start(ctx);
    for (int i = 0; i < iters && st == REID_OK; ++i) st = run();
    float ms = 0.f;
    if (st == REID_OK) st = reid_timer_stop(ctx, &ms);
    ctx->f32_conv = v0;
    *ms_per_launch = ms / (iters > 0 ? iters : 1);
    return st;
}

// The device k-way merge of reid_knn_gallery_sharded_dev on host lists (tests: any number of virtual shards on one GPU).
extern "C" int reid_debug_knn_merge(reid_ctx* ctx, const float* Dall, const int32_t* Iall, int world, int nq, int kk, int k, float* D,
                                    int32_t* I) {
    ARG_CHECK(ctx && Dall && Iall && D && I && world >= 1 && nq >= 1 && kk >= 1 && k >= 1);
    CTX_GUARD(ctx);
    float *dD, *oD;
    int32_t *dI, *oI;
    const size_t cnt = (size_t)world * nq * kk;
    REID_TRY(ctx_ws(ctx, "dbg.mD", cnt * 4, (void**)&dD));
    REID_TRY(ctx_ws(ctx, "dbg.mI", cnt * 4, (void**)&dI));
    REID_TRY(ctx_ws(ctx, "dbg.moD", (size_t)nq * k * 4, (void**)&oD));
    REID_TRY(ctx_ws(ctx, "dbg.moI", (size_t)nq * k * 4, (void**)&oI));
    HIP_TRY(hipMemcpyAsync(dD, Dall, cnt * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dI, Iall, cnt * 4, hipMemcpyHostToDevice, ctx->stream));
    REID_TRY(launch_knn_merge(ctx, dD, dI, world, nq, kk, k, oD, oI));
    HIP_TRY(hipMemcpyAsync(D, oD, (size_t)nq * k * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(I, oI, (size_t)nq * k * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return REID_OK;
}

// One Swin Linear layer (swin_transformer.py:23-39, 191-232) on random device data: mode bit 0 = fp16-storage GEMM (else exact
// fp32), bits 1-2 = epilogue: 0 bias, 1 bias + erf-GELU, 2 bias + fp32 residual into the fp32 stream.
extern "C" int reid_debug_linear(reid_ctx* ctx, int m, int n, int k, int mode, int iters, float* ms_per_launch) {
    ARG_CHECK(ctx && ms_per_launch && ctx->se18.loaded && m > 0 && n > 0 && k > 0);
    CTX_GUARD(ctx);
    typedef _Float16 f16;
    const bool h = mode & 1;
    const int epi = (mode >> 1) & 3;
    const int npad = (n + 63) / 64 * 64;
    float *a32, *b32, *bias, *res, *c32;
    f16 *a16, *b16, *c16;
    REID_TRY(ctx_ws(ctx, "dbg.x", (size_t)m * k * 4, (void**)&a32));
    REID_TRY(ctx_ws(ctx, "dbg.w", (size_t)npad * k * 4, (void**)&b32));
    REID_TRY(ctx_ws(ctx, "dbg.bias", (size_t)npad * 4, (void**)&bias));
    REID_TRY(ctx_ws(ctx, "dbg.res", (size_t)m * n * 4, (void**)&res));
    REID_TRY(ctx_ws(ctx, "dbg.out", (size_t)m * n * 4, (void**)&c32));
    REID_TRY(ctx_ws(ctx, "dbg.x16", (size_t)m * k * 2, (void**)&a16));
    REID_TRY(ctx_ws(ctx, "dbg.w16", (size_t)npad * k * 2, (void**)&b16));
    REID_TRY(ctx_ws(ctx, "dbg.out16", (size_t)m * n * 2, (void**)&c16));
    const size_t src_n = ctx->se18.n_floats;
    for (size_t o = 0; o < (size_t)m * k; o += src_n) {
        const size_t cnt = (size_t)m * k - o < src_n ? (size_t)m * k - o : src_n;
        HIP_TRY(hipMemcpyAsync(a32 + o, ctx->se18.blob, cnt * 4, hipMemcpyDeviceToDevice, ctx->stream));
        REID_TRY(launch_f32_to_f16(ctx, ctx->se18.blob, cnt, a16 + o));
    }
    for (size_t o = 0; o < (size_t)npad * k; o += src_n) {
        const size_t cnt = (size_t)npad * k - o < src_n ? (size_t)npad * k - o : src_n;
        HIP_TRY(hipMemcpyAsync(b32 + o, ctx->se18.blob, cnt * 4, hipMemcpyDeviceToDevice, ctx->stream));
        REID_TRY(launch_f32_to_f16(ctx, ctx->se18.blob, cnt, b16 + o));
    }
    HIP_TRY(hipMemsetAsync(bias, 0, (size_t)npad * 4, ctx->stream));
    HIP_TRY(hipMemsetAsync(res, 0, (size_t)m * n * 4, ctx->stream));
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.A = a32; p.lda = k; p.B = b32; p.ldb = k; p.M = m; p.N = n; p.K = k; p.C = c32; p.ldc = n;
    p.col_shift = bias; p.act = epi == 1; p.residual = epi == 2 ? res : nullptr;
    Gemm16Params q;
    memset(&q, 0, sizeof(q));
    q.A = a16; q.lda = k; q.B = b16; q.ldb = k; q.M = m; q.N = npad; q.K = k; q.ldc = n;
    q.C = epi == 2 ? nullptr : c16; q.C32 = epi == 2 ? c32 : nullptr; q.res32 = epi == 2 ? res : nullptr;
    q.col_shift = bias; q.lin = 1; q.act = epi == 1; q.n_real = n;
    q.zero_page = ctx->se18.zero_page;
    auto run = [&]() { return h ? launch_gemm_f16(ctx, A16_DENSE, q, REID_K_CONV_GEMM, 0, 0) : launch_gemm_f32(ctx, A_DENSE, E_BIAS, p, REID_K_CONV_GEMM, 0, 0); };
    int st = REID_OK;
    for (int i = 0; i < 2 && st == REID_OK; ++i) st = run();
    if (st == REID_OK) st = reid_timer_start(ctx);
    for (int i = 0; i < iters && st == REID_OK; ++i) st = run();
    float ms = 0.f;
    if (st == REID_OK) st = reid_timer_stop(ctx, &ms);
    *ms_per_launch = ms / (iters > 0 ? iters : 1);
    return st;
}

// Experiment switch of the fused distance + selection kernel (dist_select.hip: 1 = no filter phase, 2 = no list writes - both
// leave results incomplete -, 4 = print candidate-list statistics).  Lives here so that no environment variable can thin out the
// product's k-NN.
extern "C" int reid_debug_select_exp(reid_ctx* ctx, int mode) {
    ARG_CHECK(ctx && mode >= 0 && mode <= 4);
    ctx->select_exp = mode;
    return REID_OK;
}

// Test switch of the large k-NN path (knn_wide.hip): enable = 0 sends every search through the fused fp32 kernel; force > 0 makes
// every row whose index is a multiple of it take the exact-row fallback.
extern "C" int reid_debug_knn_wide(reid_ctx* ctx, int enable, int force) {
    ARG_CHECK(ctx && force >= 0);
    ctx->knn_wide = enable != 0;
    ctx->knn_wide_force = force;
    return REID_OK;
}

extern "C" int reid_debug_knn_wide_eligible(reid_ctx* ctx, int nq, int nb, int d, int k) {
    return ctx && knn_wide_eligible(ctx, nq, nb, d, k) ? 1 : 0;
}

// knn_wide_dev on host operands, called as reid_knn_dev calls it (rows zero-padded to a multiple of 64 floats, squared norms from
// launch_row_sqnorm) whatever knn_wide_eligible says, with the stages the product entry does not expose (include/reid_hip_debug.h).
// D / I [nq + 1][k]: the device outputs carry one guard row preset to 0xff bytes, which comes back with them.  tile_rows > 0 (a multiple
// of 256) replaces the query-tile rule for this call.  mat [nq][ceil256(nb)], keys [nq][32], flags [nq], sc [4] (each may be null) are
// filled for a call of ONE tile only (with several, keys belong to the last tile: REID_ERR_ARG); nflagged: the rows exact_row_kernel redid.
extern "C" int reid_debug_knn_wide_run(reid_ctx* ctx, const float* xq, int nq, const float* xb, int nb, int d, int k, int tile_rows, float* D,
                                       int32_t* I, float* mat, unsigned long long* keys, int32_t* flags, float* sc, int32_t* nflagged) {
    ARG_CHECK(ctx && xq && xb && D && I && nflagged && nq >= 1 && nb >= 1 && d >= 1 && k >= 1 && k <= 24 && tile_rows >= 0 && tile_rows % 256 == 0);
    const size_t nbpad = ((size_t)nb + 255) / 256 * 256;
    const bool one_tile = (tile_rows == 0 || nq <= tile_rows) && (size_t)nq * nbpad <= ((size_t)1 << 28);
    ARG_CHECK(one_tile || (!mat && !keys && !flags && !sc));
    CTX_ENTER(ctx);
    float *dx, *dy, *xx, *yy, *dD, *dmat = nullptr;
    int32_t* dI;
    REID_TRY(ctx_ws(ctx, "dbgk.x", (size_t)nq * d * 4, (void**)&dx));
    REID_TRY(ctx_ws(ctx, "dbgk.y", (size_t)nb * d * 4, (void**)&dy));
    REID_TRY(ctx_ws(ctx, "dbgk.D", (size_t)(nq + 1) * k * 4, (void**)&dD));
    REID_TRY(ctx_ws(ctx, "dbgk.I", (size_t)(nq + 1) * k * 4, (void**)&dI));
    if (mat) REID_TRY(ctx_ws(ctx, "dbgk.mat", (size_t)nq * nbpad * 4, (void**)&dmat));
    HIP_TRY(hipMemcpyAsync(dx, xq, (size_t)nq * d * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dy, xb, (size_t)nb * d * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(dD, 0xff, (size_t)(nq + 1) * k * 4, ctx->stream));
    HIP_TRY(hipMemsetAsync(dI, 0xff, (size_t)(nq + 1) * k * 4, ctx->stream));
    if (dmat) HIP_TRY(hipMemsetAsync(dmat, 0xff, (size_t)nq * nbpad * 4, ctx->stream));
    const float *xp, *yp;
    int ldx, ldy;
    REID_TRY(pad_rows_to(ctx, "sel.xpad", dx, nq, d, 64, &xp, &ldx));
    REID_TRY(pad_rows_to(ctx, "sel.ypad", dy, nb, d, 64, &yp, &ldy));
    REID_TRY(ctx_ws(ctx, "dist.xx", (size_t)nq * 4, (void**)&xx));
    REID_TRY(ctx_ws(ctx, "dist.yy", (size_t)nb * 4, (void**)&yy));
    REID_TRY(launch_row_sqnorm(ctx, xp, nq, ldx, ldx, xx));
    REID_TRY(launch_row_sqnorm(ctx, yp, nb, ldy, ldy, yy));
    const int t0 = ctx->knn_wide_tile_rows;
    ctx->knn_wide_tile_rows = tile_rows;
    const int st = knn_wide_dev(ctx, xp, nq, yp, nb, ldx, xx, yy, k, dD, dI, dmat);
    ctx->knn_wide_tile_rows = t0;
    REID_TRY(st);
    // the stage buffers, by the names and sizes knn_wide_dev asked for (ctx_ws hands an existing buffer back)
    unsigned long long* dkeys = nullptr;
    int32_t* dflags;
    float* dsc;
    if (keys) REID_TRY(ctx_ws(ctx, "knnw.keys", (size_t)nq * 32 * 8, (void**)&dkeys));
    REID_TRY(ctx_ws(ctx, "knnw.flags", (size_t)nq * 4 + 16, (void**)&dflags));
    REID_TRY(ctx_ws(ctx, "knnw.sc", 16, (void**)&dsc));
    HIP_TRY(hipMemcpyAsync(D, dD, (size_t)(nq + 1) * k * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(I, dI, (size_t)(nq + 1) * k * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(nflagged, dflags + nq, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (mat) HIP_TRY(hipMemcpyAsync(mat, dmat, (size_t)nq * nbpad * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (keys) HIP_TRY(hipMemcpyAsync(keys, dkeys, (size_t)nq * 32 * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (flags) HIP_TRY(hipMemcpyAsync(flags, dflags, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (sc) HIP_TRY(hipMemcpyAsync(sc, dsc, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return REID_OK;
}

// The selection with fp32-class candidates (libreid_hip_select_x3.so) through the launcher reid_argmin_rows_x3_dev / reid_knn_x3_dev call,
// on device operands, with the test hook and the statistics those entries do not expose: force_fallback_every > 0 sends every row whose
// index is a multiple of it through the exact-row kernel; stats = {rows proven, rows recomputed, tile form, candidates per row}.
extern "C" int reid_debug_select_x3(reid_ctx* ctx, const float* d_x, int m, const float* d_y, int n, int d, int metric, int k, float* d_D,
                                    int32_t* d_I, int force_fallback_every, int32_t* stats) {
    ARG_CHECK(ctx && d_x && d_y && d_I && stats && m >= 1 && n >= 1 && d >= 1 && force_fallback_every >= 0);
    ARG_CHECK(metric >= REID_METRIC_L2 && metric <= REID_METRIC_DOT && k >= 1 && k <= 24);
    CTX_ENTER(ctx);
    return select_x3_launch(ctx, d_x, m, d_y, n, d, metric, k, d_D, d_I, force_fallback_every, stats);
}

// One Swin Linear layer on HOST operands through the f16 linear build of gemm_f16.hip, results back on the host (correctness
// harness: row-position invariance, tests/test_gpu_parity.py).  mode 1 = fp16 storage (operands rounded to f16), 2 = fp32-class
// (x packed to [xh | xl'], weights to [wh 2^11 | wh | wl'], K = 3 k virtual columns).  flags bit 0 = erf-GELU; bit 1 = f16 output
// through the LDS-staged epilogue (mode 1: plain f16; mode 2: [yh | yl'], returned as yh + yl' / 2^11), else fp32 output through
// the buffer-store epilogue with `res` (may be null) added.  out: [m][n] fp32.
extern "C" int reid_debug_linear_rows(reid_ctx* ctx, const float* x, const float* w, const float* bias, const float* res, int m, int n,
                                      int k, int mode, int flags, float* out) {
    ARG_CHECK(ctx && x && w && out && m > 0 && n > 0 && k > 0 && k % 32 == 0 && (mode == 1 || mode == 2) && ctx->se18.zero_page);
    CTX_GUARD(ctx);
    typedef _Float16 f16;
    const bool act = flags & 1, f16out = flags & 2;
    const int npad = (n + 63) / 64 * 64;
    float *x32, *w32, *b32, *r32, *c32;
    f16 *a16, *w16, *c16;
    REID_TRY(ctx_ws(ctx, "dbgr.x", (size_t)m * k * 4, (void**)&x32));
    REID_TRY(ctx_ws(ctx, "dbgr.w", (size_t)npad * k * 4, (void**)&w32));
    REID_TRY(ctx_ws(ctx, "dbgr.bias", (size_t)npad * 4, (void**)&b32));
    REID_TRY(ctx_ws(ctx, "dbgr.res", (size_t)m * n * 4, (void**)&r32));
    REID_TRY(ctx_ws(ctx, "dbgr.out", (size_t)m * n * 4, (void**)&c32));
    REID_TRY(ctx_ws(ctx, "dbgr.a16", (size_t)m * 2 * k * 2, (void**)&a16));
    REID_TRY(ctx_ws(ctx, "dbgr.w16", (size_t)npad * 3 * k * 2, (void**)&w16));
    REID_TRY(ctx_ws(ctx, "dbgr.c16", (size_t)m * 2 * n * 2, (void**)&c16));
    HIP_TRY(hipMemsetAsync(w32, 0, (size_t)npad * k * 4, ctx->stream));
    HIP_TRY(hipMemsetAsync(b32, 0, (size_t)npad * 4, ctx->stream));
    HIP_TRY(hipMemsetAsync(w16, 0, (size_t)npad * 3 * k * 2, ctx->stream));
    HIP_TRY(hipMemcpyAsync(x32, x, (size_t)m * k * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(w32, w, (size_t)n * k * 4, hipMemcpyHostToDevice, ctx->stream));
    if (bias) HIP_TRY(hipMemcpyAsync(b32, bias, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    if (res) HIP_TRY(hipMemcpyAsync(r32, res, (size_t)m * n * 4, hipMemcpyHostToDevice, ctx->stream));
    Gemm16Params q;
    memset(&q, 0, sizeof(q));
    q.M = m; q.N = npad; q.n_real = n; q.lin = 1; q.act = act; q.col_shift = b32; q.zero_page = ctx->se18.zero_page;
    if (mode == 1) {
        REID_TRY(launch_f32_to_f16(ctx, x32, (size_t)m * k, a16));
        REID_TRY(launch_f32_to_f16(ctx, w32, (size_t)npad * k, w16));
        q.A = a16; q.lda = k; q.B = w16; q.ldb = k; q.K = k;
    } else {
        REID_TRY(launch_split_pack(ctx, x32, m, k, a16));
        REID_TRY(launch_split_weights(ctx, w32, n, 1, k, 3, w16));
        q.A = a16; q.lda = 2 * k; q.B = w16; q.ldb = 3 * k; q.K = 3 * k;
        q.split_terms = 3; q.a_k = 2 * k; q.acc_scale = 1.0f / 2048.0f;
    }
    if (f16out) {
        q.C = c16;
        q.ldc = mode == 2 ? 2 * n : n;
        q.pack_out = mode == 2;
    } else {
        q.C32 = c32; q.ldc = n; q.res32 = res ? r32 : nullptr;
    }
    REID_TRY(launch_gemm_f16(ctx, A16_DENSE, q, REID_K_CONV_GEMM, 0, 0));
    if (!f16out) {
        HIP_TRY(hipMemcpyAsync(out, c32, (size_t)m * n * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return REID_OK;
    }
    const size_t cols = mode == 2 ? 2 * (size_t)n : (size_t)n;
    std::vector<f16> h((size_t)m * cols);
    HIP_TRY(hipMemcpyAsync(h.data(), c16, h.size() * 2, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < n; ++j)
            out[(size_t)i * n + j] = mode == 2 ? (float)h[i * cols + j] + (float)h[i * cols + n + j] * (1.0f / 2048.0f) : (float)h[i * cols + j];
    return REID_OK;
}

// One convolution of the ResNet trunk through conv_gemm - the launch the forward makes, on host operands (include/reid_hip_debug.h).
// The context's precision and switches pick the kernel; outputs the epilogue does not write keep the NaN fill put there first.
extern "C" int reid_debug_conv_layer(reid_ctx* ctx, const float* x, int n, int h, int w, int cin, const float* wgt, int cout, int r,
                                     int stride, int pad, const float* scale, const float* shift, const float* residual, int relu,
                                     int relu_from, int pack_from, int want_stats, const float* a_scale, const float* a_shift, int a_relu,
                                     float* out, uint16_t* packed, float* stats, int* packed_written) {
    ARG_CHECK(ctx && x && wgt && out && n >= 1 && h >= 1 && w >= 1 && cin >= 1 && cout >= 1 && r >= 1 && stride >= 1 && pad >= 0);
    ARG_CHECK((scale == nullptr) == (shift == nullptr) && (a_scale == nullptr) == (a_shift == nullptr) && (!want_stats || stats) &&
              (pack_from < 0 || (packed && packed_written)));
    CTX_ENTER(ctx);
    const int ho = (h + 2 * pad - r) / stride + 1, wo = (w + 2 * pad - r) / stride + 1;
    ARG_CHECK(ho >= 1 && wo >= 1);
    const long long m = (long long)n * ho * wo;
    ARG_CHECK(!want_stats || m % 128 == 0);
    const size_t nin = (size_t)n * h * w * cin, nw = (size_t)cout * r * r * cin, nout = (size_t)m * cout;
    const size_t nstats = want_stats ? (size_t)(m / 128) * cout * 2 : 0;
    REID_TRY(conv_weights_splittable(ctx, wgt, nw, "reid_debug_conv_layer"));
    float *dx, *dw, *dout, *dsc = nullptr, *dsh = nullptr, *dres = nullptr, *dasc = nullptr, *dash = nullptr, *dstats = nullptr;
    _Float16* dpk = nullptr;
    REID_TRY(ctx_ws(ctx, "dbgc.x", nin * 4, (void**)&dx));
    REID_TRY(ctx_ws(ctx, "dbgc.w", nw * 4, (void**)&dw));
    REID_TRY(ctx_ws(ctx, "dbgc.out", nout * 4, (void**)&dout));
    HIP_TRY(hipMemcpyAsync(dx, x, nin * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dw, wgt, nw * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(dout, 0xff, nout * 4, ctx->stream));
    if (scale) {
        REID_TRY(ctx_ws(ctx, "dbgc.scale", (size_t)cout * 4, (void**)&dsc));
        REID_TRY(ctx_ws(ctx, "dbgc.shift", (size_t)cout * 4, (void**)&dsh));
        HIP_TRY(hipMemcpyAsync(dsc, scale, (size_t)cout * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(dsh, shift, (size_t)cout * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    if (residual) {
        REID_TRY(ctx_ws(ctx, "dbgc.res", nout * 4, (void**)&dres));
        HIP_TRY(hipMemcpyAsync(dres, residual, nout * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    if (a_scale) {   // the loader's input affine, per (image, input channel)
        REID_TRY(ctx_ws(ctx, "dbgc.ascale", (size_t)n * cin * 4, (void**)&dasc));
        REID_TRY(ctx_ws(ctx, "dbgc.ashift", (size_t)n * cin * 4, (void**)&dash));
        HIP_TRY(hipMemcpyAsync(dasc, a_scale, (size_t)n * cin * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(dash, a_shift, (size_t)n * cin * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    if (want_stats) {
        REID_TRY(ctx_ws(ctx, "dbgc.stats", nstats * 4, (void**)&dstats));
        HIP_TRY(hipMemsetAsync(dstats, 0xff, nstats * 4, ctx->stream));
    }
    if (pack_from >= 0) {
        REID_TRY(ctx_ws(ctx, "dbgc.packed", nout * 2 * 2, (void**)&dpk));
        HIP_TRY(hipMemsetAsync(dpk, 0xff, nout * 2 * 2, ctx->stream));
    }
    REID_TRY(conv_weights_fresh(ctx, dw));
    bool written = false;
    REID_TRY(conv_gemm(ctx, A_IM2COL, dx, n, h, w, cin, dw, cout, r, r, stride, pad, r * r * cin, dasc, dash, a_relu, dsc, dsh, dres, relu,
                       dstats, dout, relu_from, nullptr, dpk, pack_from < 0 ? 0 : pack_from, pack_from < 0 ? nullptr : &written));
    HIP_TRY(hipMemcpyAsync(out, dout, nout * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (want_stats) HIP_TRY(hipMemcpyAsync(stats, dstats, nstats * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (dpk) HIP_TRY(hipMemcpyAsync(packed, dpk, nout * 2 * 2, hipMemcpyDeviceToHost, ctx->stream));
    if (packed_written) *packed_written = written ? 1 : 0;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// ------------------------------------------------------------------------------------------------ block tails (tests/test_gpu_tail.py)
// The kernels that finish a residual block and the neck, each through the launcher the forward calls, on host operands.  Outputs are
// set to 0xff bytes first (NaN / 0xffff where a launch leaves them alone); every call returns the context's fault status.
namespace {
template <class T>
int dbg_upload(reid_ctx* ctx, const char* name, const T* host, size_t count, T** dev) {
    *dev = nullptr;
    if (!host) return REID_OK;
    REID_TRY(ctx_ws(ctx, name, count * sizeof(T), (void**)dev));
    HIP_TRY(hipMemcpyAsync(*dev, host, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return REID_OK;
}
template <class T>
int dbg_output(reid_ctx* ctx, const char* name, size_t count, T** dev) {
    REID_TRY(ctx_ws(ctx, name, count * sizeof(T), (void**)dev));
    HIP_TRY(hipMemsetAsync(*dev, 0xff, count * sizeof(T), ctx->stream));
    return REID_OK;
}
template <class T>
int dbg_download(reid_ctx* ctx, T* host, const T* dev, size_t count) {
    if (host) HIP_TRY(hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    return REID_OK;
}
}  // namespace

extern "C" int reid_debug_norm_finish(reid_ctx* ctx, int form, int n, int hw, int c, int half, int tiles, const void* x, const float* stats,
                                      const float* in_gamma, const float* in_beta, const float* bn_scale, const float* bn_shift, float* out,
                                      uint16_t* out16, float* a_scale, float* a_shift) {
    ARG_CHECK(ctx && form >= 0 && form <= 5 && n >= 1 && hw >= 1 && c >= 4 && half >= 4 && half <= c && tiles >= 1 && stats && in_gamma &&
              in_beta);
    ARG_CHECK((form == 0 || x) && (form != 1 || out) && (form < 2 || form > 5 || out16) && (form != 0 || (a_scale && a_shift)));
    ARG_CHECK((form != 0 && form < 4) || half == c || (bn_scale && bn_shift));
    CTX_ENTER(ctx);
    const size_t nx = (size_t)n * hw * c, nab = (size_t)n * c, cb = (size_t)(c - half);
    float *dst, *dg, *db, *dbs = nullptr, *dbh = nullptr, *dx = nullptr, *da = nullptr, *dbb = nullptr;
    _Float16* dh = nullptr;
    REID_TRY(dbg_upload(ctx, "dbgt.stats", stats, (size_t)n * tiles * c * 2, &dst));
    REID_TRY(dbg_upload(ctx, "dbgt.gamma", in_gamma, (size_t)half, &dg));
    REID_TRY(dbg_upload(ctx, "dbgt.beta", in_beta, (size_t)half, &db));
    if (cb) {
        REID_TRY(dbg_upload(ctx, "dbgt.bns", bn_scale, cb, &dbs));
        REID_TRY(dbg_upload(ctx, "dbgt.bnh", bn_shift, cb, &dbh));
    }
    if (form == 0 || form == 5) {
        REID_TRY(dbg_output(ctx, "dbgt.a", nab, &da));
        REID_TRY(dbg_output(ctx, "dbgt.b", nab, &dbb));
    }
    if (form >= 1 && form <= 3) REID_TRY(dbg_upload(ctx, "dbgt.x", (const float*)x, nx, &dx));
    if (form >= 4) REID_TRY(dbg_upload(ctx, "dbgt.x16", (const _Float16*)x, nx, &dh));
    if (form == 2 || form == 3) REID_TRY(dbg_output(ctx, "dbgt.pk", nx * 2, &dh));
    switch (form) {
    case 0: REID_TRY(launch_norm_finalize(ctx, dst, n, tiles, c, half, hw, dg, db, dbs, dbh, da, dbb)); break;
    case 1: REID_TRY(launch_in_apply(ctx, dx, dst, n, tiles, c, half, hw, dg, db)); break;
    case 2:
    case 3: REID_TRY(launch_in_apply_pack(ctx, dx, dst, n, tiles, c, half, hw, dg, db, dh, form == 3)); break;
    case 4: REID_TRY(launch_norm_apply_f16(ctx, dh, dst, n, tiles, c, half, hw, dg, db, dbs, dbh)); break;
    case 5:
        REID_TRY(launch_norm_finalize(ctx, dst, n, tiles, c, half, hw, dg, db, dbs, dbh, da, dbb));
        REID_TRY(launch_affine_relu_f16(ctx, dh, da, dbb, n, hw, c));
        break;
    }
    if (dx) REID_TRY(dbg_download(ctx, out, dx, nx));
    if (dh) REID_TRY(dbg_download(ctx, (_Float16*)out16, dh, form == 2 || form == 3 ? nx * 2 : nx));
    if (da) {
        REID_TRY(dbg_download(ctx, a_scale, da, nab));
        REID_TRY(dbg_download(ctx, a_shift, dbb, nab));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

extern "C" int reid_debug_se_tail(reid_ctx* ctx, int form, int n, int hw, int c, int mid, int tiles, const float* stats, const float* w1,
                                  const float* w2t, const void* y, const void* shortcut, float* out, uint16_t* out16, float* gate) {
    ARG_CHECK(ctx && form >= 0 && form <= 11 && n >= 1 && hw >= 1 && c >= 4 && mid >= 1 && tiles >= 1 && stats && w1 && w2t && y && shortcut);
    const bool f16 = form >= 10, tail = form >= 1 && form <= 9;
    const bool want_out = !f16 && (!tail || ((form - 1) % 3 != 1)), want_pk = tail && (form - 1) % 3 != 0;
    ARG_CHECK((!want_out || out) && ((!want_pk && !f16) || out16) && ((form != 0 && form != 11) || gate));
    CTX_ENTER(ctx);
    const size_t ny = (size_t)n * hw * c;
    float *dst, *dw1, *dw2, *dy = nullptr, *dsc = nullptr, *dout = nullptr, *dgate = nullptr;
    _Float16 *dy16 = nullptr, *dsc16 = nullptr, *dh = nullptr;
    REID_TRY(dbg_upload(ctx, "dbgt.stats", stats, (size_t)n * tiles * c * 2, &dst));
    REID_TRY(dbg_upload(ctx, "dbgt.w1", w1, (size_t)mid * c, &dw1));
    REID_TRY(dbg_upload(ctx, "dbgt.w2", w2t, (size_t)mid * c, &dw2));
    if (f16) {
        REID_TRY(dbg_upload(ctx, "dbgt.x16", (const _Float16*)y, ny, &dy16));
        REID_TRY(dbg_upload(ctx, "dbgt.sc16", (const _Float16*)shortcut, ny, &dsc16));
        REID_TRY(dbg_output(ctx, "dbgt.pk", ny, &dh));
    } else {
        REID_TRY(dbg_upload(ctx, "dbgt.x", (const float*)y, ny, &dy));
        REID_TRY(dbg_upload(ctx, "dbgt.sc", (const float*)shortcut, ny, &dsc));
        if (want_out) REID_TRY(dbg_output(ctx, "dbgt.out", ny, &dout));
        if (want_pk) REID_TRY(dbg_output(ctx, "dbgt.pk", ny * 2, &dh));
    }
    if (form == 0 || form == 11) REID_TRY(dbg_output(ctx, "dbgt.a", (size_t)n * c, &dgate));
    if (form == 0) {
        REID_TRY(launch_se_finalize(ctx, dst, n, tiles, c, mid, hw, dw1, dw2, dgate));
        REID_TRY(launch_se_combine(ctx, dy, dsc, dgate, n, hw, c, dout));
    } else if (tail) {   // 1-3 the launcher's rule, 4-6 se_tail_kernel<false>, 7-9 <true>: fp32 out, packed, both
        REID_TRY(launch_se_tail_form(ctx, (form - 1) / 3 - 1, dst, n, tiles, c, mid, hw, dw1, dw2, dy, dsc, dout, dh));
    } else if (form == 10) {
        REID_TRY(launch_se_tail_f16(ctx, dst, n, tiles, c, mid, hw, dw1, dw2, dy16, dsc16, dh));
    } else {
        REID_TRY(launch_se_finalize(ctx, dst, n, tiles, c, mid, hw, dw1, dw2, dgate));
        REID_TRY(launch_se_combine_f16(ctx, dy16, dsc16, dgate, n, hw, c, dh));
    }
    if (dout) REID_TRY(dbg_download(ctx, out, dout, ny));
    if (dh) REID_TRY(dbg_download(ctx, (_Float16*)out16, dh, f16 ? ny : ny * 2));
    if (dgate) REID_TRY(dbg_download(ctx, gate, dgate, (size_t)n * c));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

extern "C" int reid_debug_sibling_tail(reid_ctx* ctx, int arch, int n, int h, int w, int c, const float* prm, const float* y,
                                       const float* shortcut, float* out) {
    ARG_CHECK(ctx && (arch == 1 || arch == 2) && n >= 1 && h >= 1 && w >= 1 && c >= 32 && c % 32 == 0 && prm && y && shortcut && out);
    CTX_ENTER(ctx);
    const size_t ny = (size_t)n * h * w * c, cg = (size_t)c / 32;
    float *dp, *dy, *dsc, *dout;
    REID_TRY(dbg_upload(ctx, "dbgt.w1", prm, arch == 1 ? (size_t)300 : cg * cg * 10 + 4 * cg, &dp));
    REID_TRY(dbg_upload(ctx, "dbgt.x", y, ny, &dy));
    REID_TRY(dbg_upload(ctx, "dbgt.sc", shortcut, ny, &dsc));
    REID_TRY(dbg_output(ctx, "dbgt.out", ny, &dout));
    if (arch == 1) REID_TRY(launch_ta_tail(ctx, dy, dsc, n, h, w, c, dp, dout));
    else REID_TRY(launch_ema_tail(ctx, dy, dsc, n, h, w, c, dp, dout));
    REID_TRY(dbg_download(ctx, out, dout, ny));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

extern "C" int reid_debug_gem_neck(reid_ctx* ctx, int f16, int n, int hw, int c, float p, const void* x, const float* scale,
                                   const float* shift, float* gem_out, float* emb) {
    ARG_CHECK(ctx && n >= 1 && hw >= 1 && c >= 64 && x && scale && shift && emb);
    CTX_ENTER(ctx);
    const size_t nx = (size_t)n * hw * c, ne = (size_t)n * c;
    float *dx = nullptr, *dp, *dsc, *dsh, *dg = nullptr, *de;
    _Float16* dh = nullptr;
    REID_TRY(dbg_upload(ctx, "dbgt.p", &p, 1, &dp));
    REID_TRY(dbg_upload(ctx, "dbgt.bns", scale, (size_t)c, &dsc));
    REID_TRY(dbg_upload(ctx, "dbgt.bnh", shift, (size_t)c, &dsh));
    if (gem_out) REID_TRY(dbg_output(ctx, "dbgt.a", ne, &dg));
    REID_TRY(dbg_output(ctx, "dbgt.b", ne, &de));
    if (f16) {
        REID_TRY(dbg_upload(ctx, "dbgt.x16", (const _Float16*)x, nx, &dh));
        REID_TRY(launch_gem_neck_f16(ctx, dh, n, hw, c, dp, dsc, dsh, dg, de));
    } else {
        REID_TRY(dbg_upload(ctx, "dbgt.x", (const float*)x, nx, &dx));
        REID_TRY(launch_gem_neck(ctx, dx, n, hw, c, dp, dsc, dsh, dg, de));
    }
    if (dg) REID_TRY(dbg_download(ctx, gem_out, dg, ne));
    REID_TRY(dbg_download(ctx, emb, de, ne));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// ---- the kernels of libreid_hip_anysize.so (anysize.h; tests/test_gpu_anysize.py) through the launchers the any-size forward calls.  Every
// output buffer carries one guard pixel (c floats) behind the last image, set to 0xff bytes with the rest and returned with it.
extern "C" int reid_debug_any_norm(reid_ctx* ctx, int n, int hw, int c, int half, const float* x, const float* in_gamma, const float* in_beta,
                                   const float* bn_scale, const float* bn_shift, float* out) {
    ARG_CHECK(ctx && n >= 1 && hw >= 1 && c >= 64 && half >= 32 && half <= c && x && in_gamma && in_beta && out &&
              (bn_scale == nullptr) == (bn_shift == nullptr));
    CTX_ENTER(ctx);
    const size_t nx = (size_t)n * hw * c;
    float *dx, *dg, *db, *dbs = nullptr, *dbh = nullptr;
    REID_TRY(dbg_output(ctx, "dbgt.x", nx + c, &dx));
    HIP_TRY(hipMemcpyAsync(dx, x, nx * 4, hipMemcpyHostToDevice, ctx->stream));
    REID_TRY(dbg_upload(ctx, "dbgt.gamma", in_gamma, (size_t)half, &dg));
    REID_TRY(dbg_upload(ctx, "dbgt.beta", in_beta, (size_t)half, &db));
    if (bn_scale && c > half) {
        REID_TRY(dbg_upload(ctx, "dbgt.bns", bn_scale, (size_t)(c - half), &dbs));
        REID_TRY(dbg_upload(ctx, "dbgt.bnh", bn_shift, (size_t)(c - half), &dbh));
    }
    REID_TRY(launch_any_norm(ctx, dx, n, hw, c, half, dg, db, dbs, dbh));
    REID_TRY(dbg_download(ctx, out, dx, nx + c));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

extern "C" int reid_debug_any_se_tail(reid_ctx* ctx, int n, int hw, int c, int mid, const float* w1, const float* w2t, const float* y,
                                      const float* shortcut, float* out, float* gate) {
    ARG_CHECK(ctx && n >= 1 && hw >= 1 && c >= 64 && mid >= 1 && w1 && w2t && y && shortcut && out);
    CTX_ENTER(ctx);
    const size_t ny = (size_t)n * hw * c;
    float *dw1, *dw2, *dy, *dsc, *dout, *dgate = nullptr;
    REID_TRY(dbg_upload(ctx, "dbgt.w1", w1, (size_t)mid * c, &dw1));
    REID_TRY(dbg_upload(ctx, "dbgt.w2", w2t, (size_t)mid * c, &dw2));
    REID_TRY(dbg_upload(ctx, "dbgt.x", y, ny, &dy));
    REID_TRY(dbg_upload(ctx, "dbgt.sc", shortcut, ny, &dsc));
    REID_TRY(dbg_output(ctx, "dbgt.out", ny + c, &dout));
    if (gate) REID_TRY(dbg_output(ctx, "dbgt.a", (size_t)n * c + c, &dgate));
    REID_TRY(launch_any_se_tail(ctx, dy, dsc, n, hw, c, mid, dw1, dw2, dout, dgate));
    REID_TRY(dbg_download(ctx, out, dout, ny + c));
    if (dgate) REID_TRY(dbg_download(ctx, gate, dgate, (size_t)n * c + c));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

extern "C" int reid_debug_any_gem(reid_ctx* ctx, int n, int hw, int c, float p, const float* x, const float* scale, const float* shift,
                                  float* gem_out, float* emb) {
    ARG_CHECK(ctx && n >= 1 && hw >= 1 && c >= 64 && x && scale && shift && emb);
    CTX_ENTER(ctx);
    const size_t nx = (size_t)n * hw * c, ne = (size_t)n * c + c;
    float *dx, *dp, *dsc, *dsh, *dg = nullptr, *de;
    REID_TRY(dbg_upload(ctx, "dbgt.p", &p, 1, &dp));
    REID_TRY(dbg_upload(ctx, "dbgt.bns", scale, (size_t)c, &dsc));
    REID_TRY(dbg_upload(ctx, "dbgt.bnh", shift, (size_t)c, &dsh));
    REID_TRY(dbg_upload(ctx, "dbgt.x", x, nx, &dx));
    if (gem_out) REID_TRY(dbg_output(ctx, "dbgt.a", ne, &dg));
    REID_TRY(dbg_output(ctx, "dbgt.b", ne, &de));
    REID_TRY(launch_any_gem(ctx, dx, n, hw, c, dp, dsc, dsh, dg, de));
    if (dg) REID_TRY(dbg_download(ctx, gem_out, dg, ne));
    REID_TRY(dbg_download(ctx, emb, de, ne));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// The TripletAttention tail of libreid_hip_anysize_ca.so (anysize_ca.h; tests/test_gpu_anysize_ca.py) through launch_any_ca_tail, the function
// the any-size forward calls.  The workspace is set to 0xff bytes with one guard pixel behind it before the launch, as out is.
extern "C" int reid_debug_any_ca_tail(reid_ctx* ctx, int n, int h, int w, int c, const float* prm, const float* y, const float* shortcut,
                                      float* out, float* maps, float* gates) {
    ARG_CHECK(ctx && n >= 1 && h >= 1 && w >= 1 && c >= 64 && prm && y && shortcut && out);
    CTX_ENTER(ctx);
    const size_t ny = (size_t)n * h * w * c, per = (size_t)h * w + (size_t)c * w + (size_t)h * c;
    float *dprm, *dy, *dsc, *dout, *dws;
    REID_TRY(dbg_upload(ctx, "dbgt.w1", prm, (size_t)300, &dprm));
    REID_TRY(dbg_upload(ctx, "dbgt.x", y, ny, &dy));
    REID_TRY(dbg_upload(ctx, "dbgt.sc", shortcut, ny, &dsc));
    REID_TRY(dbg_output(ctx, "dbgt.out", ny + c, &dout));
    REID_TRY(dbg_output(ctx, "any.ca", (size_t)n * 3 * per + c, &dws));   // the workspace launch_any_ca_tail takes: grown first, so it is this one
    const float *dmaps, *dgates;
    REID_TRY(launch_any_ca_tail(ctx, dy, dsc, n, h, w, c, dprm, dout, &dmaps, &dgates));
    ARG_CHECK(dmaps == dws && dgates == dws + (size_t)n * 2 * per);
    REID_TRY(dbg_download(ctx, out, dout, ny + c));
    REID_TRY(dbg_download(ctx, maps, dmaps, (size_t)n * 2 * per));
    REID_TRY(dbg_download(ctx, gates, dgates, (size_t)n * per + c));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// The EMA tail of libreid_hip_anysize_ema.so (anysize_ema.h; tests/test_gpu_anysize_ema.py) through launch_any_ema_tail, the function the
// any-size forward calls.  The workspace is set to 0xff bytes with one guard pixel behind it before the launch, as out is.
extern "C" int reid_debug_any_ema_tail(reid_ctx* ctx, int n, int h, int w, int c, const float* prm, const float* y, const float* shortcut,
                                       float* out, float* sig, float* small) {
    ARG_CHECK(ctx && n >= 1 && h >= 1 && w >= 1 && c >= 64 && c <= 512 && c % 32 == 0 && prm && y && shortcut && out);
    CTX_ENTER(ctx);
    const int cg = c / 32;
    const size_t ny = (size_t)n * h * w * c, nsig = (size_t)n * (h + w) * c, nsmall = (size_t)n * 4 * c;
    const size_t npart = (size_t)n * anysize_ema_slabs(h, w, c) * 3 * c;   // doubles
    float *dprm, *dy, *dsc, *dout, *dws;
    REID_TRY(dbg_upload(ctx, "dbgt.w1", prm, (size_t)cg * cg * 10 + 4 * cg, &dprm));
    REID_TRY(dbg_upload(ctx, "dbgt.x", y, ny, &dy));
    REID_TRY(dbg_upload(ctx, "dbgt.sc", shortcut, ny, &dsc));
    REID_TRY(dbg_output(ctx, "dbgt.out", ny + c, &dout));
    REID_TRY(dbg_output(ctx, "any.ema", 2 * npart + nsig + nsmall + c, &dws));   // the workspace launch_any_ema_tail takes: grown first, so it is this one
    const float *dsig, *dsmall;
    REID_TRY(launch_any_ema_tail(ctx, dy, dsc, n, h, w, c, dprm, dout, &dsig, &dsmall));
    ARG_CHECK(dsig == dws + 2 * npart && dsmall == dsig + nsig);
    REID_TRY(dbg_download(ctx, out, dout, ny + c));
    REID_TRY(dbg_download(ctx, sig, dsig, nsig));
    REID_TRY(dbg_download(ctx, small, dsmall, nsmall + c));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// One trunk convolution of the any-size forward through launch_any_conv, the function the forward calls: hw_precision 2 =
// any_conv_x3_kernel (libreid_hip_anysize_x3.so), 0 = the exact-fp32 GEMM.  The weights land in a reused workspace, so the split form cached
// under that address goes first.  form_out: the tile form an fp32-class launch took (anysize_x3.h), 0 for exact fp32.
extern "C" int reid_debug_any_conv(reid_ctx* ctx, int hw_precision, const float* x, int n, int h, int w, int cin, const float* wgt, int cout,
                                   int r, int stride, int pad, const float* scale, const float* shift, const float* residual, int relu,
                                   int relu_from, float* out, int* form_out) {
    ARG_CHECK(ctx && (hw_precision == 0 || hw_precision == 2) && x && wgt && out && n >= 1 && h >= 1 && w >= 1 && cin >= 32 && cin % 32 == 0 &&
              cout >= 64 && cout % 64 == 0 && ((r == 3 && pad == 1) || (r == 1 && pad == 0)) && (stride == 1 || stride == 2) &&
              (scale == nullptr) == (shift == nullptr) && relu_from >= 0 && relu_from <= cout);
    CTX_ENTER(ctx);
    const int ho = (h + 2 * pad - r) / stride + 1, wo = (w + 2 * pad - r) / stride + 1;
    const size_t nx = (size_t)n * h * w * cin, nw = (size_t)cout * r * r * cin, ny = (size_t)n * ho * wo * cout;
    if (hw_precision == 2)
        for (size_t i = 0; i < nw; ++i)
            if (!(fabsf(wgt[i]) * 2048.0f < 65504.0f)) {
                reid_set_error("reid_debug_any_conv: weight %zu (%g) is outside the range the fp32-class arithmetic can split (|w| 2^11 < 65504)",
                               i, (double)wgt[i]);
                return REID_ERR_ARG;
            }
    float *dx, *dw, *ds, *dh, *dr, *dout;
    REID_TRY(dbg_upload(ctx, "dbgc.x", x, nx, &dx));
    REID_TRY(dbg_upload(ctx, "dbgc.w", wgt, nw, &dw));
    REID_TRY(conv_weights_fresh(ctx, dw));
    REID_TRY(dbg_upload(ctx, "dbgc.scale", scale, (size_t)cout, &ds));
    REID_TRY(dbg_upload(ctx, "dbgc.shift", shift, (size_t)cout, &dh));
    REID_TRY(dbg_upload(ctx, "dbgc.res", residual, ny, &dr));
    REID_TRY(dbg_output(ctx, "dbgc.out", ny + cout, &dout));
    ctx->any_conv_form = 0;
    REID_TRY(launch_any_conv(ctx, hw_precision, dx, n, h, w, cin, dw, cout, r, stride, pad, ds, dh, dr, relu, relu_from, dout));
    if (form_out) *form_out = ctx->any_conv_form;
    REID_TRY(dbg_download(ctx, out, dout, ny + cout));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// ---- the kernels of libreid_hip_anysize_f16.so (anysize_f16.h; tests/test_gpu_anysize_f16.py) through the launchers the any-size forward
// calls under reid_ctx_set_hw_f16 1.  f16 operands and results travel as their bits (uint16_t).  Every output buffer carries one guard row
// behind the last pixel, set to 0xff bytes (NaN in f16 and fp32) with the rest and returned with it.
extern "C" int reid_debug_any_conv_f16(reid_ctx* ctx, const uint16_t* x, int n, int h, int w, int cin, const uint16_t* wgt, int cout, int r,
                                       int stride, int pad, const float* scale, const float* shift, const uint16_t* residual, int relu,
                                       int relu_from, uint16_t* out, int* form_out) {
    ARG_CHECK(ctx && x && wgt && out && n >= 1 && h >= 1 && w >= 1 && cin >= 32 && cin % 32 == 0 && cout >= 64 && cout % 64 == 0 &&
              ((r == 3 && pad == 1) || (r == 1 && pad == 0)) && (stride == 1 || stride == 2) && (scale == nullptr) == (shift == nullptr) &&
              relu_from >= 0 && relu_from <= cout);
    CTX_ENTER(ctx);
    const int ho = (h + 2 * pad - r) / stride + 1, wo = (w + 2 * pad - r) / stride + 1;
    const size_t nx = (size_t)n * h * w * cin, nw = (size_t)cout * r * r * cin, ny = (size_t)n * ho * wo * cout;
    uint16_t *dx, *dw, *dr, *dout;
    float *ds, *dh;
    REID_TRY(dbg_upload(ctx, "dbgh.x", x, nx, &dx));
    REID_TRY(dbg_upload(ctx, "dbgh.w", wgt, nw, &dw));
    REID_TRY(dbg_upload(ctx, "dbgc.scale", scale, (size_t)cout, &ds));
    REID_TRY(dbg_upload(ctx, "dbgc.shift", shift, (size_t)cout, &dh));
    REID_TRY(dbg_upload(ctx, "dbgh.res", residual, ny, &dr));
    REID_TRY(dbg_output(ctx, "dbgh.out", ny + cout, &dout));
    ctx->any_f16_form = 0;
    REID_TRY(launch_any_conv_f16(ctx, (const _Float16*)dx, n, h, w, cin, (const _Float16*)dw, cout, r, stride, pad, ds, dh, (const _Float16*)dr,
                                 relu, relu_from, (_Float16*)dout));
    if (form_out) *form_out = ctx->any_f16_form;
    REID_TRY(dbg_download(ctx, out, dout, ny + cout));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

extern "C" int reid_debug_any_stem_f16(reid_ctx* ctx, const float* x, int n, int h, int w, const uint16_t* w16, const float* scale,
                                       const float* shift, uint16_t* stem_out, uint16_t* pool_out) {
    ARG_CHECK(ctx && x && w16 && scale && shift && stem_out && pool_out && n >= 1 && h >= 1 && w >= 1);
    CTX_ENTER(ctx);
    const int H1 = (h - 1) / 2 + 1, W1 = (w - 1) / 2 + 1, H2 = (H1 - 1) / 2 + 1, W2 = (W1 - 1) / 2 + 1;
    const size_t ns = (size_t)n * H1 * W1 * 64, np_ = (size_t)n * H2 * W2 * 64;
    float *dx, *ds, *dh;
    uint16_t *dw, *dstem, *dpool;
    REID_TRY(dbg_upload(ctx, "dbgc.x", x, (size_t)n * h * w * 3, &dx));
    REID_TRY(dbg_upload(ctx, "dbgh.w", w16, (size_t)64 * 192, &dw));
    REID_TRY(dbg_upload(ctx, "dbgc.scale", scale, (size_t)64, &ds));
    REID_TRY(dbg_upload(ctx, "dbgc.shift", shift, (size_t)64, &dh));
    REID_TRY(dbg_output(ctx, "dbgh.out", ns + 64, &dstem));
    REID_TRY(dbg_output(ctx, "dbgh.res", np_ + 64, &dpool));
    REID_TRY(launch_any_stem_f16(ctx, dx, n, h, w, (const _Float16*)dw, ds, dh, (_Float16*)dstem));
    REID_TRY(launch_any_maxpool_f16(ctx, (const _Float16*)dstem, n, H1, W1, 64, (_Float16*)dpool));
    REID_TRY(dbg_download(ctx, stem_out, dstem, ns + 64));
    REID_TRY(dbg_download(ctx, pool_out, dpool, np_ + 64));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

extern "C" int reid_debug_any_norm_f16(reid_ctx* ctx, int n, int hw, int c, int half, const uint16_t* x, const float* in_gamma,
                                       const float* in_beta, uint16_t* out) {
    ARG_CHECK(ctx && n >= 1 && hw >= 1 && c >= 64 && half >= 32 && half <= c && x && in_gamma && in_beta && out);
    CTX_ENTER(ctx);
    const size_t nx = (size_t)n * hw * c;
    uint16_t* dx;
    float *dg, *db;
    REID_TRY(dbg_output(ctx, "dbgh.x", nx + c, &dx));
    HIP_TRY(hipMemcpyAsync(dx, x, nx * 2, hipMemcpyHostToDevice, ctx->stream));
    REID_TRY(dbg_upload(ctx, "dbgt.gamma", in_gamma, (size_t)half, &dg));
    REID_TRY(dbg_upload(ctx, "dbgt.beta", in_beta, (size_t)half, &db));
    REID_TRY(launch_any_norm_f16(ctx, (_Float16*)dx, n, hw, c, half, dg, db));
    REID_TRY(dbg_download(ctx, out, dx, nx + c));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// alias != 0: out is y's buffer (the launch the forward could make in place); the guard row then lies behind y
extern "C" int reid_debug_any_se_tail_f16(reid_ctx* ctx, int n, int hw, int c, int mid, const float* w1, const float* w2t, const uint16_t* y,
                                          const uint16_t* shortcut, int alias, uint16_t* out, float* gate) {
    ARG_CHECK(ctx && n >= 1 && hw >= 1 && c >= 64 && mid >= 1 && w1 && w2t && y && shortcut && out);
    CTX_ENTER(ctx);
    const size_t ny = (size_t)n * hw * c;
    float *dw1, *dw2, *dgate = nullptr;
    uint16_t *dy, *dsc, *dout;
    REID_TRY(dbg_upload(ctx, "dbgt.w1", w1, (size_t)mid * c, &dw1));
    REID_TRY(dbg_upload(ctx, "dbgt.w2", w2t, (size_t)mid * c, &dw2));
    REID_TRY(dbg_output(ctx, "dbgh.x", ny + c, &dy));
    HIP_TRY(hipMemcpyAsync(dy, y, ny * 2, hipMemcpyHostToDevice, ctx->stream));
    REID_TRY(dbg_upload(ctx, "dbgh.res", shortcut, ny, &dsc));
    REID_TRY(dbg_output(ctx, "dbgh.out", ny + c, &dout));
    if (alias) dout = dy;
    if (gate) REID_TRY(dbg_output(ctx, "dbgt.a", (size_t)n * c + c, &dgate));
    REID_TRY(launch_any_se_tail_f16(ctx, (const _Float16*)dy, (const _Float16*)dsc, n, hw, c, mid, dw1, dw2, (_Float16*)dout, dgate));
    REID_TRY(dbg_download(ctx, out, dout, ny + c));
    if (dgate) REID_TRY(dbg_download(ctx, gate, dgate, (size_t)n * c + c));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// The TripletAttention / EMA tails of libreid_hip_anysize_sib_f16.so (anysize_sib_f16.h; tests/test_gpu_anysize_sib_f16.py) through
// launch_any_ca_tail_f16 / launch_any_ema_tail_f16, the functions the any-size forward calls under reid_ctx_set_hw_sib_f16 1.  The workspace
// is set to 0xff bytes with one guard pixel behind it before the launch, as out is; the statistics come back as the fp32 harnesses
// (reid_debug_any_ca_tail, reid_debug_any_ema_tail) return them.
extern "C" int reid_debug_any_ca_tail_f16(reid_ctx* ctx, int n, int h, int w, int c, const float* prm, const uint16_t* y,
                                          const uint16_t* shortcut, uint16_t* out, float* maps, float* gates) {
    ARG_CHECK(ctx && n >= 1 && h >= 1 && w >= 1 && c >= 64 && prm && y && shortcut && out);
    CTX_ENTER(ctx);
    const size_t ny = (size_t)n * h * w * c, per = (size_t)h * w + (size_t)c * w + (size_t)h * c;
    float *dprm, *dws;
    uint16_t *dy, *dsc, *dout;
    REID_TRY(dbg_upload(ctx, "dbgt.w1", prm, (size_t)300, &dprm));
    REID_TRY(dbg_upload(ctx, "dbgh.x", y, ny, &dy));
    REID_TRY(dbg_upload(ctx, "dbgh.res", shortcut, ny, &dsc));
    REID_TRY(dbg_output(ctx, "dbgh.out", ny + c, &dout));
    REID_TRY(dbg_output(ctx, "any.ca", (size_t)n * 3 * per + c, &dws));   // the workspace launch_any_ca_tail_f16 takes: grown first, so it is this one
    const float *dmaps, *dgates;
    REID_TRY(launch_any_ca_tail_f16(ctx, (const _Float16*)dy, (const _Float16*)dsc, n, h, w, c, dprm, (_Float16*)dout, &dmaps, &dgates));
    ARG_CHECK(dmaps == dws && dgates == dws + (size_t)n * 2 * per);
    REID_TRY(dbg_download(ctx, out, dout, ny + c));
    REID_TRY(dbg_download(ctx, maps, dmaps, (size_t)n * 2 * per));
    REID_TRY(dbg_download(ctx, gates, dgates, (size_t)n * per + c));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

extern "C" int reid_debug_any_ema_tail_f16(reid_ctx* ctx, int n, int h, int w, int c, const float* prm, const uint16_t* y,
                                           const uint16_t* shortcut, uint16_t* out, float* sig, float* small) {
    ARG_CHECK(ctx && n >= 1 && h >= 1 && w >= 1 && c >= 64 && c <= 512 && c % 32 == 0 && prm && y && shortcut && out);
    CTX_ENTER(ctx);
    const int cg = c / 32;
    const size_t ny = (size_t)n * h * w * c, nsig = (size_t)n * (h + w) * c, nsmall = (size_t)n * 4 * c;
    const size_t npart = (size_t)n * anysize_ema_slabs(h, w, c) * 3 * c;   // doubles
    float *dprm, *dws;
    uint16_t *dy, *dsc, *dout;
    REID_TRY(dbg_upload(ctx, "dbgt.w1", prm, (size_t)cg * cg * 10 + 4 * cg, &dprm));
    REID_TRY(dbg_upload(ctx, "dbgh.x", y, ny, &dy));
    REID_TRY(dbg_upload(ctx, "dbgh.res", shortcut, ny, &dsc));
    REID_TRY(dbg_output(ctx, "dbgh.out", ny + c, &dout));
    REID_TRY(dbg_output(ctx, "any.ema", 2 * npart + nsig + nsmall + c, &dws));   // the workspace launch_any_ema_tail_f16 takes: grown first, so it is this one
    const float *dsig, *dsmall;
    REID_TRY(launch_any_ema_tail_f16(ctx, (const _Float16*)dy, (const _Float16*)dsc, n, h, w, c, dprm, (_Float16*)dout, &dsig, &dsmall));
    ARG_CHECK(dsig == dws + 2 * npart && dsmall == dsig + nsig);
    REID_TRY(dbg_download(ctx, out, dout, ny + c));
    REID_TRY(dbg_download(ctx, sig, dsig, nsig));
    REID_TRY(dbg_download(ctx, small, dsmall, nsmall + c));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

extern "C" int reid_debug_any_gem_f16(reid_ctx* ctx, int n, int hw, int c, float p, const uint16_t* x, const float* scale, const float* shift,
                                      float* gem_out, float* emb) {
    ARG_CHECK(ctx && n >= 1 && hw >= 1 && c >= 64 && x && scale && shift && emb);
    CTX_ENTER(ctx);
    const size_t nx = (size_t)n * hw * c, ne = (size_t)n * c + c;
    uint16_t* dx;
    float *dp, *dsc, *dsh, *dg = nullptr, *de;
    REID_TRY(dbg_upload(ctx, "dbgt.p", &p, 1, &dp));
    REID_TRY(dbg_upload(ctx, "dbgt.bns", scale, (size_t)c, &dsc));
    REID_TRY(dbg_upload(ctx, "dbgt.bnh", shift, (size_t)c, &dsh));
    REID_TRY(dbg_upload(ctx, "dbgh.x", x, nx, &dx));
    if (gem_out) REID_TRY(dbg_output(ctx, "dbgt.a", ne, &dg));
    REID_TRY(dbg_output(ctx, "dbgt.b", ne, &de));
    REID_TRY(launch_any_gem_f16(ctx, (const _Float16*)dx, n, hw, c, dp, dsc, dsh, dg, de));
    if (dg) REID_TRY(dbg_download(ctx, gem_out, dg, ne));
    REID_TRY(dbg_download(ctx, emb, de, ne));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// The front end of the any-size forward from uint8 windows through launch_any_front, the function reid_frame_submit_hw and
// reid_embed_frame_u8_hw call: fused 1 = any_front_kernel (libreid_hip_anysize_front.so), 0 = resize, stem GEMM and max-pool in three launches.
extern "C" int reid_debug_any_front(reid_ctx* ctx, int fused, const uint8_t* src, int64_t src_bytes, const int64_t* offsets, const int32_t* hw,
                                    int n, int pitch, int out_h, int out_w, const float* mean_std6, const float* stem_w, const float* scale,
                                    const float* shift, float* out) {
    ARG_CHECK(ctx && (fused == 0 || fused == 1) && src && src_bytes >= 1 && offsets && hw && n >= 1 && pitch >= 0 && out_h >= 32 && out_h <= 512 &&
              out_w >= 32 && out_w <= 512 && stem_w && scale && shift && out);
    static const float kHalf[6] = {0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f};
    if (!mean_std6) mean_std6 = kHalf;
    for (int i = 0; i < 6; ++i) ARG_CHECK(std::isfinite(mean_std6[i]) && (i < 3 || mean_std6[i] > 0.f));
    for (int i = 0; i < n; ++i) {   // every window inside the source
        const int64_t h = hw[2 * i], w = hw[2 * i + 1];
        ARG_CHECK(h >= 1 && w >= 1 && offsets[i] >= 0 && (pitch == 0 || w <= pitch));
        ARG_CHECK(offsets[i] + (pitch ? ((h - 1) * pitch + w) * 3 : h * w * 3) <= src_bytes);
    }
    CTX_ENTER(ctx);
    const int H1 = (out_h - 1) / 2 + 1, W1 = (out_w - 1) / 2 + 1, H2 = (H1 - 1) / 2 + 1, W2 = (W1 - 1) / 2 + 1;
    const size_t ny = (size_t)n * H2 * W2 * 64 + (size_t)W2 * 64;
    uint8_t* dsrc;
    long long* doff;
    int* dhw;
    float *dw, *ds, *dh, *dstem = nullptr, *dout;
    REID_TRY(dbg_upload(ctx, "dbgf.src", src, (size_t)src_bytes, &dsrc));
    REID_TRY(dbg_upload(ctx, "dbgf.off", (const long long*)offsets, (size_t)n, &doff));
    REID_TRY(dbg_upload(ctx, "dbgf.hw", (const int*)hw, (size_t)2 * n, &dhw));
    REID_TRY(dbg_upload(ctx, "dbgf.w", stem_w, (size_t)64 * 192, &dw));
    REID_TRY(dbg_upload(ctx, "dbgf.scale", scale, (size_t)64, &ds));
    REID_TRY(dbg_upload(ctx, "dbgf.shift", shift, (size_t)64, &dh));
    if (!fused) REID_TRY(ctx_ws(ctx, "dbgf.stem", (size_t)n * H1 * W1 * 64 * 4, (void**)&dstem));
    REID_TRY(dbg_output(ctx, "dbgf.out", ny, &dout));
    REID_TRY(launch_any_front(ctx, fused, dsrc, doff, dhw, n, out_h, out_w, pitch, mean_std6, dw, ds, dh, dstem, dout));
    REID_TRY(dbg_download(ctx, out, dout, ny));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// GeM + BNNeck of the last block's tail in one launch (launch_gem_neck_tail): what reid_debug_se_tail form 4 followed by
// reid_debug_gem_neck computes, without the tensor between them.
extern "C" int reid_debug_gem_neck_fused(reid_ctx* ctx, int n, int hw, int c, int mid, int tiles, float p, const float* stats, const float* w1,
                                         const float* w2t, const float* y, const float* shortcut, const float* scale, const float* shift,
                                         float* gem_out, float* emb) {
    ARG_CHECK(ctx && n >= 1 && hw >= 1 && c >= 64 && mid >= 1 && tiles >= 1 && stats && w1 && w2t && y && shortcut && scale && shift && emb);
    CTX_ENTER(ctx);
    const size_t ny = (size_t)n * hw * c, ne = (size_t)n * c;
    float *dst, *dw1, *dw2, *dy, *dsc, *dp, *dbs, *dbh, *dg = nullptr, *de;
    REID_TRY(dbg_upload(ctx, "dbgt.stats", stats, (size_t)n * tiles * c * 2, &dst));
    REID_TRY(dbg_upload(ctx, "dbgt.w1", w1, (size_t)mid * c, &dw1));
    REID_TRY(dbg_upload(ctx, "dbgt.w2", w2t, (size_t)mid * c, &dw2));
    REID_TRY(dbg_upload(ctx, "dbgt.x", y, ny, &dy));
    REID_TRY(dbg_upload(ctx, "dbgt.sc", shortcut, ny, &dsc));
    REID_TRY(dbg_upload(ctx, "dbgt.p", &p, 1, &dp));
    REID_TRY(dbg_upload(ctx, "dbgt.bns", scale, (size_t)c, &dbs));
    REID_TRY(dbg_upload(ctx, "dbgt.bnh", shift, (size_t)c, &dbh));
    if (gem_out) REID_TRY(dbg_output(ctx, "dbgt.a", ne, &dg));
    REID_TRY(dbg_output(ctx, "dbgt.b", ne, &de));
    REID_TRY(launch_gem_neck_tail(ctx, dst, n, tiles, c, mid, hw, dw1, dw2, dy, dsc, dp, dbs, dbh, dg, de));
    if (dg) REID_TRY(dbg_download(ctx, gem_out, dg, ne));
    REID_TRY(dbg_download(ctx, emb, de, ne));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// ------------------------------------------------------------------------------------------------ fp16-storage convolutions (tests/test_gpu_conv_f16.py)
// One convolution of the fp16-storage trunk through conv_gemm16(A16_IM2COL, ...) - the call seres18_forward_f16 makes - on raw f16 bits, so
// that the caller owns the exact operands.  The context's switches pick the kernel; what conv_gemm16's launchers refuse comes back as their
// REID_ERR_ARG, nothing launched.  *form = reid_ctx::conv_form of the launch (0: none).
extern "C" int reid_debug_conv_layer_f16(reid_ctx* ctx, const uint16_t* x, int n, int h, int w, int cin, const uint16_t* wgt, int cout, int r,
                                         int stride, int pad, const float* scale, const float* shift, const uint16_t* residual, int relu,
                                         int want_stats, uint16_t* out, float* stats, int* form) {
    ARG_CHECK(ctx && x && wgt && out && form && n >= 1 && h >= 1 && w >= 1 && cin >= 1 && cout >= 1 && r >= 1 && stride >= 1 && pad >= 0);
    ARG_CHECK((scale == nullptr) == (shift == nullptr) && (!want_stats || stats) && ctx->se18.zero_page);
    CTX_ENTER(ctx);
    typedef _Float16 f16;
    const int ho = (h + 2 * pad - r) / stride + 1, wo = (w + 2 * pad - r) / stride + 1;
    ARG_CHECK(ho >= 1 && wo >= 1 && (long long)n * ho * wo < (1LL << 31) / cout && (long long)n * h * w < (1LL << 31) / cin);
    const size_t m = (size_t)n * ho * wo, nout = m * cout, nstats = (m + 127) / 128 * cout * 2;
    uint16_t *dx, *dw, *dres, *dout;
    float *dsc, *dsh, *dstats = nullptr;
    REID_TRY(dbg_upload(ctx, "dbgh.x", x, (size_t)n * h * w * cin, &dx));
    REID_TRY(dbg_upload(ctx, "dbgh.w", wgt, (size_t)cout * r * r * cin, &dw));
    REID_TRY(dbg_upload(ctx, "dbgh.scale", scale, (size_t)cout, &dsc));
    REID_TRY(dbg_upload(ctx, "dbgh.shift", shift, (size_t)cout, &dsh));
    REID_TRY(dbg_upload(ctx, "dbgh.res", residual, nout, &dres));
    REID_TRY(dbg_output(ctx, "dbgh.out", nout, &dout));
    if (want_stats) REID_TRY(dbg_output(ctx, "dbgh.stats", nstats, &dstats));
    ctx->conv_form = 0;
    *form = 0;
    const int st = conv_gemm16(ctx, A16_IM2COL, (const f16*)dx, n, h, w, cin, (const f16*)dw, cout, r, r, stride, pad, r * r * cin, dsc, dsh,
                               (const f16*)dres, relu, dstats, (f16*)dout);
    *form = ctx->conv_form;
    if (st != REID_OK) {   // refused: the uploads above still read the caller's arrays
        (void)hipStreamSynchronize(ctx->stream);
        return st;
    }
    REID_TRY(dbg_download(ctx, out, dout, nout));
    if (want_stats) REID_TRY(dbg_download(ctx, stats, dstats, (size_t)(m / 128) * cout * 2));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// launch_conv3x3_c64_f16 on raw f16 bits: x / residual [n][64][32][64], w_folded [64][576] (the BN scale already folded in, as
// scale_rows_f16_kernel leaves it), fp32 shift [64].  With se_w1 / se_w2t [8][64] the launch is conv2 with the fused SE tail (`out` = the
// block output); with both null it is the plain launch, which also returns the per-image stats [n][64][2] when asked.
extern "C" int reid_debug_conv_c64_se(reid_ctx* ctx, int n, const uint16_t* x, const uint16_t* w_folded, const float* shift,
                                      const uint16_t* residual, int relu, const float* se_w1, const float* se_w2t, uint16_t* out, float* stats,
                                      int* form) {
    ARG_CHECK(ctx && x && w_folded && out && n >= 1 && n <= 4096 && (se_w1 == nullptr) == (se_w2t == nullptr));
    CTX_ENTER(ctx);
    typedef _Float16 f16;
    const size_t nact = (size_t)n * 64 * 32 * 64, nstats = (size_t)n * 64 * 2;
    uint16_t *dx, *dw, *dres, *dout, *zp;
    float *dsh, *dw1, *dw2, *dstats = nullptr;
    REID_TRY(dbg_upload(ctx, "dbgh.x", x, nact, &dx));
    REID_TRY(dbg_upload(ctx, "dbgh.w", w_folded, (size_t)64 * 576, &dw));
    REID_TRY(dbg_upload(ctx, "dbgh.shift", shift, (size_t)64, &dsh));
    REID_TRY(dbg_upload(ctx, "dbgh.res", residual, nact, &dres));
    REID_TRY(dbg_upload(ctx, "dbgh.w1", se_w1, (size_t)8 * 64, &dw1));
    REID_TRY(dbg_upload(ctx, "dbgh.w2", se_w2t, (size_t)8 * 64, &dw2));
    REID_TRY(dbg_output(ctx, "dbgh.out", nact, &dout));
    if (stats) REID_TRY(dbg_output(ctx, "dbgh.stats", nstats, &dstats));
    REID_TRY(ctx_ws(ctx, "dbg64.zp", 256, (void**)&zp));
    HIP_TRY(hipMemsetAsync(zp, 0, 256, ctx->stream));
    ctx->conv_form = 0;
    if (form) *form = 0;
    const int st = launch_conv3x3_c64_f16(ctx, (const f16*)dx, n, (const f16*)dw, dsh, (const f16*)dres, relu, dstats, (f16*)dout, (const f16*)zp,
                                          dw1, dw2);
    if (form) *form = ctx->conv_form;
    if (st != REID_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return st;
    }
    REID_TRY(dbg_download(ctx, out, dout, nact));
    if (stats) REID_TRY(dbg_download(ctx, stats, dstats, nstats));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// Timing experiments on the fused pair of linears: bit 0 = no weight refills after the first two steps, bit 1 = no block barriers.
// The results are WRONG while a bit is set (which is why this lives here and not behind an environment variable of the library).
extern "C" int reid_debug_two_linear_ablate(reid_ctx* ctx, int bits) {
    ARG_CHECK(ctx && bits >= 0 && bits < 4);
    ctx->two_linear_ablate = bits;
    return REID_OK;
}

// The fused pair of linears (two_linear_f16.hip) on its own: out = res + w2 . act(w1 . x + b1) + b2 through launch_split_pack +
// launch_two_linear, x [m][c], w1 [hid][c], w2 [c][hid], res / out [m][c] fp32 on the host.  iters > 1 repeats the launch and
// returns the mean time in *ms (may be null).  The context must be in precision 2.
extern "C" int reid_debug_two_linear(reid_ctx* ctx, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                                     const float* res, int m, int c, int hid, int act, int iters, float* out, float* ms, const float* ln_g,
                                     const float* ln_b) {
    ARG_CHECK(ctx && x && w1 && b1 && w2 && b2 && res && out && m > 0 && iters >= 1);
    CTX_GUARD(ctx);
    ARG_CHECK(two_linear_supported(ctx, m, c, hid));
    typedef _Float16 f16;
    float *x32, *dw1, *dw2, *db1, *db2, *r32, *o32;
    f16* a16;
    REID_TRY(ctx_ws(ctx, "dbg2.x", (size_t)m * c * 4, (void**)&x32));
    REID_TRY(ctx_ws(ctx, "dbg2.w1", (size_t)hid * c * 4, (void**)&dw1));
    REID_TRY(ctx_ws(ctx, "dbg2.w2", (size_t)hid * c * 4, (void**)&dw2));
    REID_TRY(ctx_ws(ctx, "dbg2.b1", (size_t)hid * 4, (void**)&db1));
    REID_TRY(ctx_ws(ctx, "dbg2.b2", (size_t)c * 4, (void**)&db2));
    REID_TRY(ctx_ws(ctx, "dbg2.res", (size_t)m * c * 4, (void**)&r32));
    REID_TRY(ctx_ws(ctx, "dbg2.out", (size_t)m * c * 4, (void**)&o32));
    REID_TRY(ctx_ws(ctx, "dbg2.a16", (size_t)m * 2 * c * 2, (void**)&a16));
    float *dg = nullptr, *dbt = nullptr;
    if (ln_g && ln_b) {   // LayerNorm(x) in the kernel instead of the packed input
        REID_TRY(ctx_ws(ctx, "dbg2.lng", (size_t)c * 4, (void**)&dg));
        REID_TRY(ctx_ws(ctx, "dbg2.lnb", (size_t)c * 4, (void**)&dbt));
        HIP_TRY(hipMemcpyAsync(dg, ln_g, (size_t)c * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(dbt, ln_b, (size_t)c * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    const _Float16* ain = dg ? nullptr : a16;
    HIP_TRY(hipMemcpyAsync(x32, x, (size_t)m * c * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dw1, w1, (size_t)hid * c * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dw2, w2, (size_t)hid * c * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(db1, b1, (size_t)hid * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(db2, b2, (size_t)c * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(r32, res, (size_t)m * c * 4, hipMemcpyHostToDevice, ctx->stream));
    REID_TRY(launch_split_pack(ctx, x32, m, c, a16));
    // the tiled weight images are cached by blob address: this harness re-uses its buffers, so drop what an earlier call left
    for (const void* key : {(const void*)((const char*)dw1 + 1), (const void*)((const char*)dw2 + 1)}) {
        auto it = ctx->split_w.find(key);
        if (it != ctx->split_w.end()) {
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            (void)hipFree(it->second);
            ctx->split_w.erase(it);
        }
    }
    REID_TRY(launch_two_linear(ctx, ain, m, c, hid, dw1, db1, dw2, db2, act, r32, o32, x32, dg, dbt));
    if (iters > 1) {
        hipEvent_t e0, e1;
        HIP_TRY(hipEventCreate(&e0));
        HIP_TRY(hipEventCreate(&e1));
        HIP_TRY(hipEventRecord(e0, ctx->stream));
        for (int i = 0; i < iters; ++i) REID_TRY(launch_two_linear(ctx, ain, m, c, hid, dw1, db1, dw2, db2, act, r32, o32, x32, dg, dbt));
        HIP_TRY(hipEventRecord(e1, ctx->stream));
        HIP_TRY(hipEventSynchronize(e1));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, e0, e1));
        if (ms) *ms = t / iters;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    }
    HIP_TRY(hipMemcpyAsync(out, o32, (size_t)m * c * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return REID_OK;
}

// The same pair as a TEST harness (tests/test_gpu_two_linear.py), by the conventions of reid_debug_swin_linear below: one launch through
// launch_split_pack (packed builds) + launch_two_linear in the context's own precision and switches, a guarded output returned whole,
// the tile images of the harness's weight buffers dropped in front of the launch, the context's fault status as the result.
// flags: bit 0 erf-GELU; bit 1 the LN build (x stays fp32, LayerNorm(ln_g, ln_b) in the kernel's prologue); bit 2 the forward's aliasing -
// LN build: ONE buffer is x32, res and out (res must be null: the residual is x); packed build: the output rows hold res and res == out.
extern "C" int reid_debug_two_linear_form(reid_ctx* ctx, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                                          const float* res, int m, int c, int hid, int flags, const float* ln_g, const float* ln_b, float* out) {
    ARG_CHECK(ctx && x && w1 && b1 && w2 && b2 && out && m > 0 && c > 0 && c % 8 == 0 && hid > 0 && flags >= 0 && flags < 8);
    const bool act = flags & 1, ln = flags & 2, alias = flags & 4;
    ARG_CHECK(ln ? (ln_g && ln_b) : (!ln_g && !ln_b));
    ARG_CHECK(ln && alias ? !res : res != nullptr);
    ARG_CHECK(((long long)m + 8) * c < (1ll << 31) && (long long)hid * c < (1ll << 29));
    CTX_ENTER(ctx);
    typedef _Float16 f16;
    const size_t front = 64, nx = (size_t)m * c, total = front + (size_t)(m + 8) * c;
    float *dx, *dw1, *dw2, *db1, *db2, *dres, *dg, *dbt, *dout;
    f16* a16 = nullptr;
    REID_TRY(dbg_upload(ctx, "dbg2f.x", x, nx, &dx));
    REID_TRY(dbg_upload(ctx, "dbg2f.w1", w1, (size_t)hid * c, &dw1));
    REID_TRY(dbg_upload(ctx, "dbg2f.w2", w2, (size_t)hid * c, &dw2));
    REID_TRY(dbg_upload(ctx, "dbg2f.b1", b1, (size_t)hid, &db1));
    REID_TRY(dbg_upload(ctx, "dbg2f.b2", b2, (size_t)c, &db2));
    REID_TRY(dbg_upload(ctx, "dbg2f.res", res, nx, &dres));
    REID_TRY(dbg_upload(ctx, "dbg2f.lng", ln_g, (size_t)c, &dg));
    REID_TRY(dbg_upload(ctx, "dbg2f.lnb", ln_b, (size_t)c, &dbt));
    REID_TRY(dbg_output(ctx, "dbg2f.out", total, &dout));
    float* o = dout + front;
    const float *r = dres, *x32 = dx;
    if (alias) {   // the output rows hold the residual when the launch starts; the LN build reads its input there too
        HIP_TRY(hipMemcpyAsync(o, ln ? dx : dres, nx * 4, hipMemcpyDeviceToDevice, ctx->stream));
        r = o;
        if (ln) x32 = o;
    }
    auto drop_images = [&]() {   // cached by blob address + 1 (launch_two_linear): this harness re-uses its buffers
        for (const void* key : {(const void*)((const char*)dw1 + 1), (const void*)((const char*)dw2 + 1)}) {
            auto it = ctx->split_w.find(key);
            if (it == ctx->split_w.end()) continue;
            (void)hipStreamSynchronize(ctx->stream);
            (void)hipFree(it->second);
            ctx->split_w.erase(it);
        }
    };
    drop_images();
    int st = REID_OK;
    if (!ln) {
        REID_TRY(ctx_ws(ctx, "dbg2f.a16", nx * 2 * 2, (void**)&a16));
        st = launch_split_pack(ctx, dx, m, c, a16);
    }
    if (st == REID_OK) st = launch_two_linear(ctx, a16, m, c, hid, dw1, db1, dw2, db2, act, r, o, ln ? x32 : nullptr, dg, dbt);
    // a refusal returns the launcher's code - with the output as it stands, so that the caller sees that nothing was written
    REID_TRY(dbg_download(ctx, out, dout, total));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    drop_images();
    return st != REID_OK ? st : ctx_fault_status(ctx);
}

// ------------------------------------------------------------------------------------------------ loop-back communicator (tests)
// Several contexts of THIS process on ONE device act as the ranks of a job: every collective of csrc/comm.hip
// (reid_allgather_dev and what is built on it - ragged row gathers, reid_frame_gather, reid_knn_gallery_sharded_dev -
// reid_allreduce_f64) then runs with world > 1 on a one-GPU box, driven by one host thread per rank.  The exchange itself is
// a host rendezvous + device-to-device copies; RCCL is not involved (the product's only transport, reid_comm_init, is).
#include <condition_variable>
#include <chrono>
#include <mutex>

namespace {
struct LoopComm : reid_comm_loop {
    int world, attached;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    long gen = 0;
    std::vector<const void*> send;
    std::vector<double> red;
    explicit LoopComm(int w) : world(w), attached(w), send(w, nullptr), red((size_t)w * 64, 0.0) {}

    // reusable barrier; gives up after 60 s (a rank that failed never arrives: the others must not hang the box)
    bool barrier() {
        std::unique_lock<std::mutex> lk(mu);
        const long g = gen;
        if (++arrived == world) {
            arrived = 0;
            ++gen;
            cv.notify_all();
            return true;
        }
        return cv.wait_for(lk, std::chrono::seconds(60), [&] { return gen != g; });
    }
    int allgather(int rank, const void* d_send, void* d_recv, size_t bytes, hipStream_t st) override {
        HIP_TRY(hipStreamSynchronize(st));            // this rank's payload is complete
        send[rank] = d_send;
        if (!barrier()) { reid_set_error("loop-back all-gather: rank %d waited 60 s for the others", rank); return REID_ERR_STATE; }
        for (int r = 0; r < world; ++r)
            HIP_TRY(hipMemcpyAsync((char*)d_recv + (size_t)r * bytes, send[r], bytes, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (!barrier()) { reid_set_error("loop-back all-gather: rank %d waited 60 s for the others", rank); return REID_ERR_STATE; }
        return REID_OK;
    }
    int allreduce(int rank, double* inout, int count, int op) override {
        for (int i = 0; i < count; ++i) red[(size_t)rank * 64 + i] = inout[i];
        if (!barrier()) { reid_set_error("loop-back all-reduce: rank %d waited 60 s for the others", rank); return REID_ERR_STATE; }
        for (int i = 0; i < count; ++i) {
            double v = red[i];
            for (int r = 1; r < world; ++r) v = op == 0 ? v + red[(size_t)r * 64 + i] : (red[(size_t)r * 64 + i] > v ? red[(size_t)r * 64 + i] : v);
            inout[i] = v;
        }
        if (!barrier()) { reid_set_error("loop-back all-reduce: rank %d waited 60 s for the others", rank); return REID_ERR_STATE; }
        return REID_OK;
    }
    void detach(int) override {
        bool last;
        {
            std::lock_guard<std::mutex> lk(mu);
            last = --attached == 0;
        }
        if (last) delete this;
    }
};
}  // namespace

extern "C" int reid_debug_comm_loopback(reid_ctx** ctxs, int world) {
    ARG_CHECK(ctxs && world >= 1 && world <= 64);
    for (int r = 0; r < world; ++r) {
        ARG_CHECK(ctxs[r] && ctxs[r]->device == ctxs[0]->device);
        for (int q = 0; q < r; ++q) ARG_CHECK(ctxs[q] != ctxs[r]);
        if (ctxs[r]->comm) {
            reid_set_error("reid_debug_comm_loopback: context %d already has a communicator", r);
            return REID_ERR_STATE;
        }
    }
    LoopComm* lc = new LoopComm(world);
    for (int r = 0; r < world; ++r) {
        reid_comm* c = new reid_comm();
        c->rank = r;
        c->world = world;
        c->loop = lc;
        ctxs[r]->comm = c;
    }
    return REID_OK;
}

// ------------------------------------------------------------------------------------------------ Swin v2 kernels alone
// window_attn_cos_kernel (swin_v2.hip) through the launcher the forward calls, on host operands: qkv fp32 [n H W][3 heads 32]
// (mode 1: rounded to f16 on the device first), bias [heads][49 queries][49 keys], scale [heads].  mode 0 -> out fp32 [tokens][C];
// mode 2 -> out16 = [oh | ol'] raw f16 bits [tokens][2C]; mode 1 -> out16 raw f16 bits [tokens][C].
extern "C" int reid_debug_window_attn_cos(reid_ctx* ctx, int mode, const float* qkv, int n, int h, int w, int heads, int shifted,
                                          const float* bias, const float* scale, float* out, uint16_t* out16) {
    ARG_CHECK(ctx && mode >= 0 && mode <= 2 && qkv && bias && scale && n >= 1 && heads >= 1 && heads <= 64 && h >= 7 && w >= 7 && h % 7 == 0 &&
              w % 7 == 0);
    ARG_CHECK(mode == 0 ? out != nullptr : out16 != nullptr);
    CTX_ENTER(ctx);
    const int C = heads * 32;
    const size_t T = (size_t)n * h * w;
    std::vector<float> bt((size_t)heads * 49 * 64, 0.f);   // [head][key][query padded to 64], as reid_swin_load makes it
    for (int hd = 0; hd < heads; ++hd)
        for (int query = 0; query < 49; ++query)
            for (int key = 0; key < 49; ++key) bt[((size_t)hd * 49 + key) * 64 + query] = bias[((size_t)hd * 49 + query) * 49 + key];
    float *dq, *dbt, *dsc, *dout = nullptr;
    _Float16 *dq16 = nullptr, *dout16 = nullptr;
    REID_TRY(dbg_upload(ctx, "dbgv2.qkv", qkv, T * 3 * C, &dq));
    REID_TRY(dbg_upload(ctx, "dbgv2.bt", bt.data(), bt.size(), &dbt));
    REID_TRY(dbg_upload(ctx, "dbgv2.sc", scale, (size_t)heads, &dsc));
    HIP_TRY(hipStreamSynchronize(ctx->stream));            // bt is a local
    const void* src = dq;
    void* dst;
    if (mode == 1) {
        REID_TRY(ctx_ws(ctx, "dbgv2.q16", T * 3 * C * 2, (void**)&dq16));
        REID_TRY(launch_f32_to_f16(ctx, dq, T * 3 * C, dq16));
        src = dq16;
    }
    if (mode == 0) {
        REID_TRY(dbg_output(ctx, "dbgv2.out", T * C, &dout));
        dst = dout;
    } else {
        REID_TRY(dbg_output(ctx, "dbgv2.o16", T * C * (mode == 2 ? 2 : 1), &dout16));
        dst = dout16;
    }
    REID_TRY(launch_window_attn_cos(ctx, mode, src, 3 * C, n, h, w, heads, shifted, dbt, dsc, dst));
    if (mode == 0) REID_TRY(dbg_download(ctx, out, dout, T * C));
    else REID_TRY(dbg_download(ctx, (_Float16*)out16, dout16, T * C * (mode == 2 ? 2 : 1)));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// post_norm_kernel (swin_v2.hip) through its launcher: out = x + (LayerNorm(y) g + b), x / y / out fp32 [t][c]; side 1 -> out16 = f16 copy
// of out (raw bits, [t][c]); side 2 -> out16 = [oh | ol'] raw f16 bits [t][2c].  in_place != 0: the launch writes out over its x.
extern "C" int reid_debug_post_norm(reid_ctx* ctx, int side, const float* x, const float* y, int t, int c, const float* g, const float* b,
                                    int in_place, float* out, uint16_t* out16) {
    ARG_CHECK(ctx && side >= 0 && side <= 2 && x && y && g && b && out && t >= 1 && c >= 4 && c <= 768 && c % 4 == 0 && (side == 0 || out16));
    CTX_ENTER(ctx);
    const size_t nx = (size_t)t * c;
    float *dx, *dy, *dg, *db, *dout;
    _Float16* dside = nullptr;
    REID_TRY(dbg_upload(ctx, "dbgv2.x", x, nx, &dx));
    REID_TRY(dbg_upload(ctx, "dbgv2.y", y, nx, &dy));
    REID_TRY(dbg_upload(ctx, "dbgv2.g", g, (size_t)c, &dg));
    REID_TRY(dbg_upload(ctx, "dbgv2.b", b, (size_t)c, &db));
    if (in_place) dout = dx;
    else REID_TRY(dbg_output(ctx, "dbgv2.out", nx, &dout));
    if (side) REID_TRY(dbg_output(ctx, "dbgv2.o16", nx * (side == 2 ? 2 : 1), &dside));
    REID_TRY(launch_post_norm(ctx, side, dx, dy, t, c, dg, db, dout, dside));
    REID_TRY(dbg_download(ctx, out, dout, nx));
    if (side) REID_TRY(dbg_download(ctx, (_Float16*)out16, dside, nx * (side == 2 ? 2 : 1)));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// ------------------------------------------------------------------------------------------------ front end (tests/test_gpu_frontend.py)
// What runs before layer 1 of a ResNet pass, each through the launcher the forward calls, on host operands.  Outputs are set to 0xff
// bytes first (NaN / 0xffff where a launch leaves them alone); every call returns the context's fault status.
extern "C" int reid_debug_stem(reid_ctx* ctx, int form, int is_u8, const void* x, int n, const float* w, const float* scale,
                               const float* shift, float* out, uint16_t* out16) {
    ARG_CHECK(ctx && form >= 0 && form <= 6 && x && n >= 1 && w && scale && shift);
    ARG_CHECK((form == 3 ? is_u8 != 0 : true) && (form >= 3 && form <= 5 ? out16 != nullptr : out != nullptr) && (form != 2 || out16));
    CTX_ENTER(ctx);
    typedef _Float16 f16;
    const int PAD_H = 262, PAD_W = 136;                      // the padded NHWC4 image of the fp16 path (api.hip)
    const size_t npix = (size_t)n * 256 * 128, nmap = (size_t)n * 128 * 64 * 64, npool = (size_t)n * 64 * 32 * 64;
    // [64][7][7][3] -> stem.w [64][8][24] (k = r 24 + s 3 + c, zero padded: weights.stem_pack), then the two f16 forms reid_seres18_load makes
    std::vector<float> wp((size_t)64 * 192, 0.f);
    for (int co = 0; co < 64; ++co)
        for (int r = 0; r < 7; ++r)
            for (int k = 0; k < 21; ++k) wp[(size_t)co * 192 + r * 24 + k] = w[((size_t)co * 7 + r) * 21 + k];
    float *dw, *dsc, *dsh, *dxf = nullptr, *dmap = nullptr, *dout = nullptr;
    uint8_t* dxu = nullptr;
    f16 *dw16 = nullptr, *dpad = nullptr, *dmap16 = nullptr, *dout16 = nullptr;
    REID_TRY(dbg_upload(ctx, "dbgf.w", wp.data(), wp.size(), &dw));
    REID_TRY(dbg_upload(ctx, "dbgf.scale", scale, (size_t)64, &dsc));
    REID_TRY(dbg_upload(ctx, "dbgf.shift", shift, (size_t)64, &dsh));
    if (is_u8) REID_TRY(dbg_upload(ctx, "dbgf.xu8", (const uint8_t*)x, npix * 3, &dxu));
    else REID_TRY(dbg_upload(ctx, "dbgf.xf32", (const float*)x, npix * 3, &dxf));
    HIP_TRY(hipStreamSynchronize(ctx->stream));              // wp is a local
    const void* dx = is_u8 ? (const void*)dxu : (const void*)dxf;
    if (form >= 3 && form <= 5) {
        REID_TRY(ctx_ws(ctx, "dbgf.w16", (size_t)64 * 256 * 2, (void**)&dw16));
        if (form == 5) REID_TRY(launch_stem_w16(ctx, dw, dw16));
        else REID_TRY(launch_stem_w16_scaled(ctx, dw, dsc, dw16));
        REID_TRY(dbg_output(ctx, "dbgf.out16", npool, &dout16));
        if (form >= 4) {
            REID_TRY(dbg_output(ctx, "dbgf.pad", (size_t)n * PAD_H * PAD_W * 4, &dpad));
            if (is_u8) REID_TRY(launch_prep_u8_pad_f16(ctx, dxu, n, 256, 128, PAD_H, PAD_W, dpad));
            else REID_TRY(launch_prep_f32_pad_f16(ctx, dxf, n, 256, 128, PAD_H, PAD_W, dpad));
        }
    }
    switch (form) {
    case 0:
        REID_TRY(dbg_output(ctx, "dbgf.map", nmap, &dout));
        REID_TRY(launch_stem_f32(ctx, dx, is_u8 != 0, n, dw, dsc, dsh, dout, false));
        break;
    case 1:
        REID_TRY(dbg_output(ctx, "dbgf.out", npool, &dout));
        REID_TRY(launch_stem_f32(ctx, dx, is_u8 != 0, n, dw, dsc, dsh, dout, true));
        break;
    case 2:
        REID_TRY(dbg_output(ctx, "dbgf.out", npool, &dout));
        REID_TRY(dbg_output(ctx, "dbgf.out16", npool * 2, &dout16));
        REID_TRY(launch_stem_split(ctx, dx, is_u8 != 0, n, dw, dsc, dsh, dout, dout16));
        break;
    case 3: REID_TRY(launch_stem_pool_f16(ctx, nullptr, dxu, n, dw16, dsh, dout16)); break;
    case 4: REID_TRY(launch_stem_pool_f16(ctx, dpad, nullptr, n, dw16, dsh, dout16)); break;
    case 5:
        REID_TRY(dbg_output(ctx, "dbgf.map16", nmap, &dmap16));
        REID_TRY(conv_gemm16(ctx, A16_STEM, dpad, n, 256, 128, 4, dw16, 64, 7, 7, 2, 3, 224, dsc, dsh, nullptr, 0, nullptr, dmap16, PAD_H, PAD_W));
        REID_TRY(launch_maxpool3s2_f16(ctx, dmap16, n, 128, 64, 64, dout16));
        break;
    case 6:
        REID_TRY(dbg_output(ctx, "dbgf.map", nmap, &dmap));
        REID_TRY(dbg_output(ctx, "dbgf.out", npool, &dout));
        REID_TRY(conv_gemm(ctx, is_u8 ? A_STEM_U8 : A_STEM_F32, dx, n, 256, 128, 3, dw, 64, 7, 7, 2, 3, 192, nullptr, nullptr, 0, dsc, dsh, nullptr,
                           0, nullptr, dmap));
        REID_TRY(launch_maxpool3s2(ctx, dmap, n, 128, 64, 64, dout));
        break;
    }
    if (dout) REID_TRY(dbg_download(ctx, out, dout, form == 0 ? nmap : npool));
    if (dout16) REID_TRY(dbg_download(ctx, (f16*)out16, dout16, form == 2 ? npool * 2 : npool));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

extern "C" int reid_debug_resize_norm(reid_ctx* ctx, const uint8_t* packed, const long long* offsets, const int* hw, int n, int pitch,
                                      float* out) {
    ARG_CHECK(ctx && packed && offsets && hw && n >= 1 && pitch >= 0 && out);
    size_t bytes = 0;                                        // the source bytes the n windows span
    for (int i = 0; i < n; ++i) {
        const int h = hw[2 * i], w = hw[2 * i + 1];
        ARG_CHECK(h >= 1 && w >= 1 && offsets[i] >= 0 && (pitch == 0 || w <= pitch));
        const size_t end = (size_t)offsets[i] + ((size_t)(h - 1) * (pitch ? pitch : w) + w) * 3;
        if (end > bytes) bytes = end;
    }
    CTX_ENTER(ctx);
    uint8_t* dpk;
    long long* doff;
    int* dhw;
    float* dout;
    REID_TRY(dbg_upload(ctx, "dbgf.xu8", packed, bytes, &dpk));
    REID_TRY(dbg_upload(ctx, "dbgf.off", offsets, (size_t)n, &doff));
    REID_TRY(dbg_upload(ctx, "dbgf.hw", hw, (size_t)2 * n, &dhw));
    REID_TRY(dbg_output(ctx, "dbgf.xf32", (size_t)n * 256 * 128 * 3, &dout));
    REID_TRY(launch_resize_norm(ctx, dpk, doff, dhw, n, 256, 128, pitch, dout));
    REID_TRY(dbg_download(ctx, out, dout, (size_t)n * 256 * 128 * 3));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// The two kernels of libreid_hip_pil_resize.so through PilPlan, the launcher the *_images_u8 entry points call, on host operands: n packed
// uint8 RGB images -> Pillow's Image.resize((out_w, out_h), BILINEAR) as u8_out [n][out_h][out_w][3] (may be NULL) and
// ToTensor + Normalize(mean_std6; NULL = ImageNet) of it as f32_out [n][3][out_h][out_w].  One launch of all n images.
extern "C" int reid_debug_pil_resize(reid_ctx* ctx, const uint8_t* packed, const long long* offsets, const int* hw, int n, int out_h, int out_w,
                                     const float* mean_std6, uint8_t* u8_out, float* f32_out) {
    ARG_CHECK(ctx && packed && offsets && hw && n >= 1 && f32_out);
    REID_TRY(pil_mean_std(&mean_std6));
    RaggedSrc src{packed, (const int64_t*)offsets, hw, n};
    REID_TRY(src.check());
    CTX_ENTER(ctx);
    PilPlan plan;
    REID_TRY(plan.build(src, out_h, out_w, mean_std6, n));
    const size_t px = (size_t)n * out_h * out_w;
    uint8_t* du8 = nullptr;
    float* df32;
    REID_TRY(src.alloc(ctx, "dbgp"));
    REID_TRY(plan.alloc(ctx, "dbgp"));
    if (u8_out) REID_TRY(dbg_output(ctx, "dbgp.u8", px * 3, &du8));
    REID_TRY(dbg_output(ctx, "dbgp.f32", px * 3, &df32));
    int rc = src.up(0, n, ctx->stream);
    if (rc == REID_OK) rc = plan.up(ctx->stream);
    if (rc == REID_OK) rc = plan.launch(ctx, src, 0, n, du8, df32);
    if (rc != REID_OK) {
        (void)hipStreamSynchronize(ctx->stream);   // the uploads read the caller's buffers and this call's plan
        return rc;
    }
    REID_TRY(dbg_download(ctx, u8_out, (const uint8_t*)du8, px * 3));
    REID_TRY(dbg_download(ctx, f32_out, (const float*)df32, px * 3));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// swin_crop_front_kernel (swin_crops.hip) through the launcher the crops entry points call, on host operands: windows as for
// reid_debug_resize_norm, c1_w [12][(kh, kw, c)], c1_b [12] -> out [n][out_h / 2][out_w / 2][12].  Every window is checked against the
// bytes uploaded before anything is launched.
static int debug_swin_crop_front(reid_ctx* ctx, bool mirror, const uint8_t* packed, const long long* offsets, const int* hw, int n, int pitch,
                                 int out_h, int out_w, const float* mean_std6, const float* c1_w, const float* c1_b, float* out) {
    ARG_CHECK(ctx && packed && offsets && hw && n >= 1 && pitch >= 0 && mean_std6 && c1_w && c1_b && out);
    REID_TRY(swin_crops_check(out_h, out_w, mean_std6));
    size_t bytes = 0;                                        // the source bytes the n windows span
    for (int i = 0; i < n; ++i) {
        const int h = hw[2 * i], w = hw[2 * i + 1];
        ARG_CHECK(h >= 1 && w >= 1 && offsets[i] >= 0 && (pitch == 0 || w <= pitch));
        const size_t end = (size_t)offsets[i] + ((size_t)(h - 1) * (pitch ? pitch : w) + w) * 3;
        if (end > bytes) bytes = end;
    }
    CTX_ENTER(ctx);
    uint8_t* dpk;
    long long* doff;
    int* dhw;
    float *dw, *db, *dout;
    const size_t nout = (size_t)n * (out_h / 2) * (out_w / 2) * 12;
    REID_TRY(dbg_upload(ctx, "dbgf.xu8", packed, bytes, &dpk));
    REID_TRY(dbg_upload(ctx, "dbgf.off", offsets, (size_t)n, &doff));
    REID_TRY(dbg_upload(ctx, "dbgf.hw", hw, (size_t)2 * n, &dhw));
    REID_TRY(dbg_upload(ctx, "dbgf.c1w", c1_w, (size_t)144, &dw));
    REID_TRY(dbg_upload(ctx, "dbgf.c1b", c1_b, (size_t)12, &db));
    REID_TRY(dbg_output(ctx, "dbgf.c1", nout, &dout));
    REID_TRY((mirror ? launch_swin_crop_front_mirror : launch_swin_crop_front)(ctx, dpk, doff, dhw, n, out_h, out_w, pitch, mean_std6, dw, db, dout));
    REID_TRY(dbg_download(ctx, out, dout, nout));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}
extern "C" int reid_debug_swin_crop_front(reid_ctx* ctx, const uint8_t* packed, const long long* offsets, const int* hw, int n, int pitch,
                                          int out_h, int out_w, const float* mean_std6, const float* c1_w, const float* c1_b, float* out) {
    return debug_swin_crop_front(ctx, false, packed, offsets, hw, n, pitch, out_h, out_w, mean_std6, c1_w, c1_b, out);
}
// swin_crop_front_mirror_kernel (swin_eval.hip): the same windows, the resized image's columns reversed
extern "C" int reid_debug_swin_crop_front_mirror(reid_ctx* ctx, const uint8_t* packed, const long long* offsets, const int* hw, int n, int pitch,
                                                 int out_h, int out_w, const float* mean_std6, const float* c1_w, const float* c1_b, float* out) {
    return debug_swin_crop_front(ctx, true, packed, offsets, hw, n, pitch, out_h, out_w, mean_std6, c1_w, c1_b, out);
}

// sfe_conv1_kernel (swin.hip), the stem the float entry points run, through its launcher: x fp32 NCHW [n][3][h][w] -> out [n][h / 2][w / 2][12]
static int debug_swin_conv1(reid_ctx* ctx, bool mirror, const float* x, int n, int h, int w, const float* c1_w, const float* c1_b, float* out) {
    ARG_CHECK(ctx && x && n >= 1 && h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0 && c1_w && c1_b && out);
    CTX_ENTER(ctx);
    float *dx, *dw, *db, *dout;
    const size_t nout = (size_t)n * (h / 2) * (w / 2) * 12;
    REID_TRY(dbg_upload(ctx, "dbgf.xf32", x, (size_t)n * 3 * h * w, &dx));
    REID_TRY(dbg_upload(ctx, "dbgf.c1w", c1_w, (size_t)144, &dw));
    REID_TRY(dbg_upload(ctx, "dbgf.c1b", c1_b, (size_t)12, &db));
    REID_TRY(dbg_output(ctx, "dbgf.c1", nout, &dout));
    REID_TRY((mirror ? launch_sfe_conv1_mirror : launch_sfe_conv1)(ctx, dx, n, h, w, dw, db, dout));
    REID_TRY(dbg_download(ctx, out, dout, nout));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}
extern "C" int reid_debug_swin_conv1(reid_ctx* ctx, const float* x, int n, int h, int w, const float* c1_w, const float* c1_b, float* out) {
    return debug_swin_conv1(ctx, false, x, n, h, w, c1_w, c1_b, out);
}
// sfe_conv1_mirror_kernel (swin_eval.hip): the same image read with reversed columns
extern "C" int reid_debug_swin_conv1_mirror(reid_ctx* ctx, const float* x, int n, int h, int w, const float* c1_w, const float* c1_b, float* out) {
    return debug_swin_conv1(ctx, true, x, n, h, w, c1_w, c1_b, out);
}

// swin_descriptor_kernel (swin_eval.hip) through launch_swin_descriptor: e1 / e2 (nullptr: one view) [n][96], cls_w [num_class][96] ->
// rows [0, n) x columns [0, num_class + 96) of out [out_rows][ld]; the rest of out keeps the 0xff fill (NaN)
extern "C" int reid_debug_swin_descriptor(reid_ctx* ctx, const float* e1, const float* e2, const float* cls_w, int n, int num_class, int out_rows,
                                          int ld, float* out) {
    ARG_CHECK(ctx && e1 && cls_w && out && n >= 1 && num_class >= 1 && out_rows >= n && ld >= num_class + 96);
    CTX_ENTER(ctx);
    float *d1, *d2, *dw, *dout;
    REID_TRY(dbg_upload(ctx, "dbgf.e1", e1, (size_t)n * 96, &d1));
    REID_TRY(dbg_upload(ctx, "dbgf.e2", e2, (size_t)n * 96, &d2));
    REID_TRY(dbg_upload(ctx, "dbgf.clsw", cls_w, (size_t)num_class * 96, &dw));
    REID_TRY(dbg_output(ctx, "dbgf.desc", (size_t)out_rows * ld, &dout));
    REID_TRY(launch_swin_descriptor(ctx, d1, d2, dw, n, num_class, ld, dout));
    REID_TRY(dbg_download(ctx, out, dout, (size_t)out_rows * ld));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

extern "C" int reid_debug_maxpool(reid_ctx* ctx, int f16, const void* x, int n, int h, int w, int c, void* out) {
    ARG_CHECK(ctx && x && out && n >= 1 && h >= 1 && w >= 1 && c >= 1);
    CTX_ENTER(ctx);
    const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
    const size_t nin = (size_t)n * h * w * c, nout = (size_t)n * ho * wo * c;
    if (f16) {
        _Float16 *dx, *dout;
        REID_TRY(dbg_upload(ctx, "dbgf.map16", (const _Float16*)x, nin, &dx));
        REID_TRY(dbg_output(ctx, "dbgf.out16", nout, &dout));
        REID_TRY(launch_maxpool3s2_f16(ctx, dx, n, h, w, c, dout));
        REID_TRY(dbg_download(ctx, (_Float16*)out, dout, nout));
    } else {
        float *dx, *dout;
        REID_TRY(dbg_upload(ctx, "dbgf.map", (const float*)x, nin, &dx));
        REID_TRY(dbg_output(ctx, "dbgf.out", nout, &dout));
        REID_TRY(launch_maxpool3s2(ctx, dx, n, h, w, c, dout));
        REID_TRY(dbg_download(ctx, (float*)out, dout, nout));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// ------------------------------------------------------------------------------------------------ Swin v1 kernels alone (tests/test_gpu_swin_kernels.py)
// The kernels of the v1 forward that are not GEMMs, and its geometric convolutions, each through the function the forward calls
// (reid_internal.h: launch_window_attn, launch_swin_layernorm, launch_ln_linear, launch_sfe_norm_fc, launch_swin_tail, swin_loaded_merge,
// swin_loaded_fuse), on host operands.  Outputs are set to 0xff bytes first (NaN / 0xffff where a launch leaves them alone); every call
// returns the context's fault status.
namespace {
// a harness that runs a launcher in another precision / with other switches than the context's puts them back on every way out
struct CtxModes {
    reid_ctx* ctx;
    int precision, attn_mfma, attn_split;
    explicit CtxModes(reid_ctx* c) : ctx(c), precision(c->precision), attn_mfma(c->swin_attn_mfma), attn_split(c->swin_attn_split) {}
    ~CtxModes() {
        ctx->precision = precision;
        ctx->swin_attn_mfma = attn_mfma;
        ctx->swin_attn_split = attn_split;
    }
};
}  // namespace

// launch_window_attn in the precision and switches that reach kernel `form`: 0 window_attn_kernel<float> -> out fp32 [T][C]; 1 the same
// with the packed store -> out16 [T][2C]; 2 window_attn_kernel<f16> and 3 window_attn_mfma_f16_kernel -> out16 [T][C] (qkv rounded to f16 on
// the device into rows of swin_attn_ldq f16, the padding columns NaN); 4 window_attn_mfma_split_kernel -> out16 [T][2C];
// 5 window_attn_mfma_f32_kernel -> out.  qkv fp32 [n h w][3 heads 32], pos169 the block's [13][13] table.
extern "C" int reid_debug_window_attn(reid_ctx* ctx, int form, const float* qkv, int n, int h, int w, int heads, int shifted,
                                      const float* pos169, float* out, uint16_t* out16) {
    ARG_CHECK(ctx && form >= 0 && form <= 5 && qkv && pos169 && n >= 1 && heads >= 1 && heads <= 64 && h >= 7 && w >= 7 && h % 7 == 0 &&
              w % 7 == 0);
    ARG_CHECK(form == 0 || form == 5 ? out != nullptr : out16 != nullptr);
    CTX_ENTER(ctx);
    CtxModes keep(ctx);
    static const int prec[6] = {0, 2, 1, 1, 2, 0}, mfma[6] = {1, 1, 0, 1, 1, 2}, split[6] = {0, 0, 0, 0, 1, 0};
    ctx->precision = prec[form];
    ctx->swin_attn_mfma = mfma[form];
    ctx->swin_attn_split = split[form];
    const int C = heads * 32, ldq = swin_attn_ldq(ctx, C);
    const size_t T = (size_t)n * h * w;
    std::vector<float> tab(4096);
    swin_bias_table(pos169, tab.data());
    float *dq, *dpos, *dtab, *dout = nullptr;
    _Float16 *dq16 = nullptr, *dq16c = nullptr, *dout16 = nullptr;
    REID_TRY(dbg_upload(ctx, "dbgsw.qkv", qkv, T * 3 * C, &dq));
    REID_TRY(dbg_upload(ctx, "dbgsw.pos", pos169, (size_t)169, &dpos));
    REID_TRY(dbg_upload(ctx, "dbgsw.tab", tab.data(), tab.size(), &dtab));
    HIP_TRY(hipStreamSynchronize(ctx->stream));            // tab is a local
    const void* src = dq;
    if (ctx->precision == 1) {
        REID_TRY(ctx_ws(ctx, "dbgsw.q16c", T * 3 * C * 2, (void**)&dq16c));
        REID_TRY(dbg_output(ctx, "dbgsw.q16", T * ldq, &dq16));
        REID_TRY(launch_f32_to_f16(ctx, dq, T * 3 * C, dq16c));
        HIP_TRY(hipMemcpy2DAsync(dq16, (size_t)ldq * 2, dq16c, (size_t)3 * C * 2, (size_t)3 * C * 2, T, hipMemcpyDeviceToDevice, ctx->stream));
        src = dq16;
    }
    void* dst;
    const size_t nout16 = T * C * (ctx->precision == 2 ? 2 : 1);
    if (ctx->precision == 0) {
        REID_TRY(dbg_output(ctx, "dbgsw.out", T * C, &dout));
        dst = dout;
    } else {
        REID_TRY(dbg_output(ctx, "dbgsw.o16", nout16, &dout16));
        dst = dout16;
    }
    REID_TRY(launch_window_attn(ctx, src, n, h, w, heads, shifted, dpos, dtab, dst));
    if (dout) REID_TRY(dbg_download(ctx, out, dout, T * C));
    else REID_TRY(dbg_download(ctx, (_Float16*)out16, dout16, nout16));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// launch_layernorm<float> (form 0 -> out [t][c]), launch_layernorm<f16> (1 -> out16 [t][c]), launch_layernorm_packed (2 -> out16 [t][2c])
extern "C" int reid_debug_layernorm(reid_ctx* ctx, int form, const float* x, int t, int c, const float* g, const float* b, float* out,
                                    uint16_t* out16) {
    ARG_CHECK(ctx && form >= 0 && form <= 2 && x && g && b && t >= 1 && c >= 4 && c <= 768 && c % 4 == 0 && (form == 0 ? out != nullptr : out16 != nullptr));
    CTX_ENTER(ctx);
    const size_t nx = (size_t)t * c, nout16 = nx * (form == 2 ? 2 : 1);
    float *dx, *dg, *db, *dout = nullptr;
    _Float16* dout16 = nullptr;
    REID_TRY(dbg_upload(ctx, "dbgsw.x", x, nx, &dx));
    REID_TRY(dbg_upload(ctx, "dbgsw.g", g, (size_t)c, &dg));
    REID_TRY(dbg_upload(ctx, "dbgsw.b", b, (size_t)c, &db));
    if (form == 0) REID_TRY(dbg_output(ctx, "dbgsw.out", nx, &dout));
    else REID_TRY(dbg_output(ctx, "dbgsw.o16", nout16, &dout16));
    REID_TRY(launch_swin_layernorm(ctx, form, dx, t, c, dg, db, form == 0 ? (void*)dout : (void*)dout16));
    if (dout) REID_TRY(dbg_download(ctx, out, dout, nx));
    else REID_TRY(dbg_download(ctx, (_Float16*)out16, dout16, nout16));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// launch_ln_linear with the context in precision 2: out [t][n] = LayerNorm(x [t][c]; ln_g, ln_b) . w [n][c]^T (+ bias, may be null)
extern "C" int reid_debug_ln_linear(reid_ctx* ctx, const float* x, const float* ln_g, const float* ln_b, const float* w, const float* bias, int t,
                                    int c, int n, float* out) {
    ARG_CHECK(ctx && x && ln_g && ln_b && w && out && t >= 1 && c >= 4 && n >= 1);
    CTX_ENTER(ctx);
    CtxModes keep(ctx);
    ctx->precision = 2;
    ARG_CHECK(ln_linear_supported(ctx, t, c, n));
    float *dx, *dg, *db, *dw, *dbias, *dout;
    REID_TRY(dbg_upload(ctx, "dbgsw.x", x, (size_t)t * c, &dx));
    REID_TRY(dbg_upload(ctx, "dbgsw.g", ln_g, (size_t)c, &dg));
    REID_TRY(dbg_upload(ctx, "dbgsw.b", ln_b, (size_t)c, &db));
    REID_TRY(dbg_upload(ctx, "dbgsw.w", w, (size_t)n * c, &dw));
    REID_TRY(dbg_upload(ctx, "dbgsw.bias", bias, (size_t)n, &dbias));
    REID_TRY(dbg_output(ctx, "dbgsw.out", (size_t)t * n, &dout));
    // the tiled weight image is cached by blob address: this harness re-uses its buffer, so drop what an earlier call left
    auto it = ctx->split_w.find((const void*)((const char*)dw + 1));
    if (it != ctx->split_w.end()) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        (void)hipFree(it->second);
        ctx->split_w.erase(it);
    }
    REID_TRY(launch_ln_linear(ctx, dx, dg, db, t, c, n, dw, dbias, dout, n));
    REID_TRY(dbg_download(ctx, out, dout, (size_t)t * n));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// One Linear layer through linear() / linear16() of swin.hip (swin_linear_for_test), operands prepared as the forward prepares them
// (include/reid_hip_debug.h).  flags: bit 0 erf-GELU, bit 1 the residual IS the output buffer (fc2 / post_proj run in place), bit 2
// precision 2 with x left in fp32 (the classifier's call).  The whole guarded output comes back: front elements, then m + 8 rows of ld.
extern "C" int reid_debug_swin_linear(reid_ctx* ctx, const float* x, const float* w, const float* bias, const float* res, int m, int n, int k,
                                      int precision, int flags, int out_form, int ldc, float* out, uint16_t* out16, int* form) {
    ARG_CHECK(ctx && x && w && form && m > 0 && n > 0 && k > 0 && k % 4 == 0 && precision >= 0 && precision <= 2 && out_form >= 0 && out_form <= 2 &&
              flags >= 0 && flags < 8);
    const bool act = flags & 1, alias = flags & 2, x_fp32 = precision != 1 && (precision == 0 || (flags & 4));
    ARG_CHECK(x_fp32 || k % 32 == 0);
    ARG_CHECK(out_form == 0 ? out != nullptr : out16 != nullptr);
    ARG_CHECK(out_form == 0 || (out_form == precision && !x_fp32 && !res));          // f16 rows: fp16 storage; [yh | yl']: fp32-class, packed x
    ARG_CHECK(ldc >= n && (precision == 1 || ldc == n) && (out_form != 1 || n % 8 != 0 || ldc % 8 == 0));
    ARG_CHECK((!alias || (res && out_form == 0)) && ((long long)m + 8) * (out_form == 2 ? 2 * (long long)n : ldc) < (1ll << 31));
    CTX_ENTER(ctx);
    CtxModes keep(ctx);
    ctx->precision = precision;
    typedef _Float16 f16;
    const int npad = (n + 63) / 64 * 64, ld = out_form == 2 ? 2 * n : ldc;
    const size_t front = out_form == 0 ? 64 : 128, total = front + (size_t)(m + 8) * ld;
    float *dx, *dw, *dbias, *dres, *dout = nullptr;
    f16 *dx16 = nullptr, *dw16 = nullptr, *dout16 = nullptr;
    REID_TRY(dbg_upload(ctx, "dbgsl.x", x, (size_t)m * k, &dx));
    REID_TRY(ctx_ws(ctx, "dbgsl.w", (size_t)npad * k * 4, (void**)&dw));
    HIP_TRY(hipMemsetAsync(dw, 0, (size_t)npad * k * 4, ctx->stream));               // rows n .. npad - 1 of the f16 image are zeros, as reid_swin_load leaves them
    HIP_TRY(hipMemcpyAsync(dw, w, (size_t)n * k * 4, hipMemcpyHostToDevice, ctx->stream));
    REID_TRY(dbg_upload(ctx, "dbgsl.bias", bias, (size_t)n, &dbias));
    REID_TRY(dbg_upload(ctx, "dbgsl.res", res, (size_t)m * n, &dres));
    if (out_form == 0) REID_TRY(dbg_output(ctx, "dbgsl.out", total, &dout));
    else REID_TRY(dbg_output(ctx, "dbgsl.o16", total, &dout16));
    const float* r = dres;
    if (alias) {   // the forward's in-place form: the output rows hold the residual when the launch starts
        HIP_TRY(hipMemcpy2DAsync(dout + front, (size_t)ld * 4, dres, (size_t)n * 4, (size_t)n * 4, m, hipMemcpyDeviceToDevice, ctx->stream));
        r = dout + front;
    }
    const void* wdev = dw;
    if (precision == 1) {
        REID_TRY(ctx_ws(ctx, "dbgsl.x16", (size_t)m * k * 2, (void**)&dx16));
        REID_TRY(ctx_ws(ctx, "dbgsl.w16", (size_t)npad * k * 2, (void**)&dw16));
        REID_TRY(launch_f32_to_f16(ctx, dx, (size_t)m * k, dx16));
        REID_TRY(launch_f32_to_f16(ctx, dw, (size_t)npad * k, dw16));
        wdev = dw16;
    } else if (!x_fp32) {
        REID_TRY(ctx_ws(ctx, "dbgsl.x16", (size_t)m * 2 * k * 2, (void**)&dx16));
        REID_TRY(launch_split_pack(ctx, dx, m, k, dx16));
    }
    // linear() caches the split weight image by the weights' address: this harness re-uses its buffer, so it drops the image in front of
    // the call (what an earlier one left) and behind it
    auto drop_image = [&]() {
        auto it = ctx->split_w.find((const void*)dw);
        if (it == ctx->split_w.end()) return;
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(it->second);
        ctx->split_w.erase(it);
    };
    drop_image();
    ctx->conv_form = 0;
    *form = 0;
    const int st = swin_linear_for_test(ctx, precision == 1, dx, dx16, m, k, wdev, dbias, n, act, r, dout ? dout + front : nullptr,
                                        dout16 ? dout16 + front : nullptr, ldc);
    *form = ctx->conv_form;
    if (st != REID_OK) {   // refused: the uploads above still read the caller's arrays
        (void)hipStreamSynchronize(ctx->stream);
        drop_image();
        return st;
    }
    if (dout) REID_TRY(dbg_download(ctx, out, dout, total));
    else REID_TRY(dbg_download(ctx, (f16*)out16, dout16, total));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    drop_image();
    return ctx_fault_status(ctx);
}

// launch_sfe_norm_fc: sfe_norm_kernel + sfe_conv2_fc_kernel with the forward's grids.  c1 [n][h1][w1][12] -> ab [n][24] (12 scales, 12
// shifts) and tok [n][h1 / 2][w1 / 2][96]
extern "C" int reid_debug_swin_sfe(reid_ctx* ctx, const float* c1, int n, int h1, int w1, const float* in_g, const float* in_b, const float* bn_s,
                                   const float* bn_t, const float* c2_w, const float* c2_b, const float* fc_w, const float* fc_b, float* ab,
                                   float* tok) {
    ARG_CHECK(ctx && c1 && n >= 1 && h1 >= 2 && w1 >= 2 && h1 % 2 == 0 && w1 % 2 == 0 && in_g && in_b && bn_s && bn_t && c2_w && c2_b && fc_w && fc_b &&
              ab && tok);
    CTX_ENTER(ctx);
    const size_t ntok = (size_t)n * (h1 / 2) * (w1 / 2) * 96;
    float *dc1, *dig, *dib, *dbs, *dbt, *dw2, *db2, *dwf, *dbf, *dab, *dtok;
    REID_TRY(dbg_upload(ctx, "dbgsw.x", c1, (size_t)n * h1 * w1 * 12, &dc1));
    REID_TRY(dbg_upload(ctx, "dbgsw.ing", in_g, (size_t)6, &dig));
    REID_TRY(dbg_upload(ctx, "dbgsw.inb", in_b, (size_t)6, &dib));
    REID_TRY(dbg_upload(ctx, "dbgsw.bns", bn_s, (size_t)6, &dbs));
    REID_TRY(dbg_upload(ctx, "dbgsw.bnt", bn_t, (size_t)6, &dbt));
    REID_TRY(dbg_upload(ctx, "dbgsw.c2w", c2_w, (size_t)48 * 48, &dw2));
    REID_TRY(dbg_upload(ctx, "dbgsw.c2b", c2_b, (size_t)48, &db2));
    REID_TRY(dbg_upload(ctx, "dbgsw.fcw", fc_w, (size_t)96 * 48, &dwf));
    REID_TRY(dbg_upload(ctx, "dbgsw.fcb", fc_b, (size_t)96, &dbf));
    REID_TRY(dbg_output(ctx, "dbgsw.ab", (size_t)n * 24, &dab));
    REID_TRY(dbg_output(ctx, "dbgsw.out", ntok, &dtok));
    REID_TRY(launch_sfe_norm_fc(ctx, dc1, n, h1, w1, dig, dib, dbs, dbt, dw2, db2, dwf, dbf, dab, dtok));
    REID_TRY(dbg_download(ctx, ab, dab, (size_t)n * 24));
    REID_TRY(dbg_download(ctx, tok, dtok, ntok));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// launch_swin_tail: swin_tail_partial_kernel + swin_tail_final_kernel with the forward's grids.  x [n][ntok][96], g / b the tail LayerNorm's,
// p the GeM exponent, bn_s / bn_t [96] -> gem [n][96], emb [n][96]
extern "C" int reid_debug_swin_tail(reid_ctx* ctx, const float* x, int n, int ntok, const float* g, const float* b, float p, const float* bn_s,
                                    const float* bn_t, float* gem, float* emb) {
    ARG_CHECK(ctx && x && n >= 1 && ntok >= 1 && g && b && bn_s && bn_t && gem && emb);
    CTX_ENTER(ctx);
    float *dx, *dg, *db, *dp, *dbs, *dbt, *dgem, *demb;
    REID_TRY(dbg_upload(ctx, "dbgsw.x", x, (size_t)n * ntok * 96, &dx));
    REID_TRY(dbg_upload(ctx, "dbgsw.g", g, (size_t)96, &dg));
    REID_TRY(dbg_upload(ctx, "dbgsw.b", b, (size_t)96, &db));
    REID_TRY(dbg_upload(ctx, "dbgsw.p", &p, (size_t)1, &dp));
    REID_TRY(dbg_upload(ctx, "dbgsw.bns", bn_s, (size_t)96, &dbs));
    REID_TRY(dbg_upload(ctx, "dbgsw.bnt", bn_t, (size_t)96, &dbt));
    REID_TRY(dbg_output(ctx, "dbgsw.ab", (size_t)n * 96, &dgem));
    REID_TRY(dbg_output(ctx, "dbgsw.out", (size_t)n * 96, &demb));
    HIP_TRY(hipStreamSynchronize(ctx->stream));            // p is an argument
    REID_TRY(launch_swin_tail(ctx, dx, n, ntok, dg, db, dp, dbs, dbt, dgem, demb));
    REID_TRY(dbg_download(ctx, gem, dgem, (size_t)n * 96));
    REID_TRY(dbg_download(ctx, emb, demb, (size_t)n * 96));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// Patch merging in front of `stage` (2 .. 4) on the weights this context has loaded, in its precision: x [n][h][w][48 2^(stage - 1)] ->
// out fp32 [n][h / 2][w / 2][96 2^(stage - 1)]
extern "C" int reid_debug_swin_merge(reid_ctx* ctx, int stage, const float* x, int n, int h, int w, float* out) {
    ARG_CHECK(ctx && stage >= 2 && stage <= 4 && x && out && n >= 1 && h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0);
    CTX_ENTER(ctx);
    const size_t cin = (size_t)48 << (stage - 1), nin = (size_t)n * h * w * cin, nout = (size_t)n * (h / 2) * (w / 2) * cin * 2;
    float *dx, *dout;
    _Float16* dscr;
    REID_TRY(dbg_upload(ctx, "dbgsw.x", x, nin, &dx));
    REID_TRY(dbg_output(ctx, "dbgsw.o16", nin, &dscr));
    REID_TRY(dbg_output(ctx, "dbgsw.out", nout, &dout));
    REID_TRY(swin_loaded_merge(ctx, stage, dx, n, h, w, (float*)dscr, dout));
    REID_TRY(dbg_download(ctx, out, dout, nout));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// The top-down fusion on the weights this context has loaded, in its precision: sfe / x1 [n][h1][w1][96], x2 [n][h1/2][w1/2][192], x3
// [..][384], x4 [n][h1/8][w1/8][768] -> a0 = x4 + Conv8x8s8(sfe) [..][768], f3 [..][384], f2 [..][192] (fp32; precision 1: raw f16 bits) and
// f1 [n][h1][w1][96] fp32
extern "C" int reid_debug_swin_fuse(reid_ctx* ctx, const float* sfe, const float* x1, const float* x2, const float* x3, const float* x4, int n,
                                    int h1, int w1, void* a0, void* f3, void* f2, float* f1) {
    ARG_CHECK(ctx && sfe && x1 && x2 && x3 && x4 && n >= 1 && h1 >= 8 && w1 >= 8 && h1 % 8 == 0 && w1 % 8 == 0 && a0 && f3 && f2 && f1);
    CTX_ENTER(ctx);
    const size_t n1 = (size_t)n * h1 * w1 * 96;   // elements of stage 1; each later stage holds half as many
    const size_t esz = ctx->precision == 1 ? 2 : 4;
    float *dsfe, *dxs[4], *da0, *df3, *df2, *df1;
    _Float16* dscr;
    REID_TRY(dbg_upload(ctx, "dbgsw.x", sfe, n1, &dsfe));
    REID_TRY(dbg_upload(ctx, "dbgsw.x1", x1, n1, &dxs[0]));
    REID_TRY(dbg_upload(ctx, "dbgsw.x2", x2, n1 / 2, &dxs[1]));
    REID_TRY(dbg_upload(ctx, "dbgsw.x3", x3, n1 / 4, &dxs[2]));
    REID_TRY(dbg_upload(ctx, "dbgsw.x4", x4, n1 / 8, &dxs[3]));
    REID_TRY(dbg_output(ctx, "dbgsw.o16", n1, &dscr));
    REID_TRY(dbg_output(ctx, "dbgsw.a0", n1 / 8, &da0));
    REID_TRY(dbg_output(ctx, "dbgsw.f3", n1 / 4, &df3));
    REID_TRY(dbg_output(ctx, "dbgsw.f2", n1 / 2, &df2));
    REID_TRY(dbg_output(ctx, "dbgsw.out", n1, &df1));
    REID_TRY(swin_loaded_fuse(ctx, dsfe, dxs, n, h1, w1, (float*)dscr, da0, df3, df2, df1));
    HIP_TRY(hipMemcpyAsync(a0, da0, n1 / 8 * esz, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(f3, df3, n1 / 4 * esz, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(f2, df2, n1 / 2 * esz, hipMemcpyDeviceToHost, ctx->stream));
    REID_TRY(dbg_download(ctx, f1, df1, n1));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// bank_cost96_kernel (bank96.hip, libreid_hip_bank96.so) through the launch the frame pipeline's cost stage makes (bank.hip), on host
// operands: the costs of the bank's track slots[t] against dets [m][96] -> out [t][m], set to 0xff bytes first (an entry the launch leaves alone reads NaN); metric
// REID_METRIC_COS / REID_METRIC_L2SQR, gate < 0 raw.  With the `bank_fast` switch at 0 the same call runs bank_cost_kernel, as the pipeline does.  The bank must be 96 wide.
extern "C" int reid_debug_bank_cost96(reid_ctx* ctx, reid_bank* bank, const int32_t* slots, int t, const float* dets, int m, int metric,
                                      float gate, float* out) {
    ARG_CHECK(ctx && bank && slots && dets && out && t >= 1 && m >= 1 && (metric == REID_METRIC_COS || metric == REID_METRIC_L2SQR));
    int max_tracks, budget, d;
    REID_TRY(bank_geometry(bank, &max_tracks, &budget, &d));
    ARG_CHECK(d == 96);
    for (int i = 0; i < t; ++i) ARG_CHECK(slots[i] >= 0 && slots[i] < max_tracks);
    CTX_ENTER(ctx);
    int32_t* dslots;
    float *ddets, *dout;
    REID_TRY(dbg_upload(ctx, "dbgb.slots", slots, (size_t)t, &dslots));
    REID_TRY(dbg_upload(ctx, "dbgb.dets", dets, (size_t)m * 96, &ddets));
    REID_TRY(dbg_output(ctx, "dbgb.out", (size_t)t * m + 16, &dout));
    REID_TRY(bank_frame_cost_launch(ctx, bank, dslots, t, ddets, m, metric == REID_METRIC_COS ? 0 : 1, gate, dout));
    uint32_t guard[16];   // the 16 words behind the matrix: a launch that wrote past its t x m entries is an error of this call
    REID_TRY(dbg_download(ctx, out, dout, (size_t)t * m));
    REID_TRY(dbg_download(ctx, guard, (const uint32_t*)(dout + (size_t)t * m), (size_t)16));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 16; ++i)
        if (guard[i] != 0xffffffffu) {
            reid_set_error("reid_debug_bank_cost96: the launch wrote word %d past its %d x %d outputs", i, t, m);
            return REID_ERR_STATE;
        }
    return ctx_fault_status(ctx);
}

// ------------------------------------------------------------------------------------------------ post-processing (tests/test_gpu_postproc.py)
// descriptor_kernel through launch_descriptor, the launch the descriptor entries make, on host operands: e1 / e2 [n][de], l1 / l2 [n][dl],
// e2 and l2 both NULL for a single view -> out [(n + 1)(de + dl)]: n rows and ONE guard row behind them, preset to 0xff bytes with the rest.
extern "C" int reid_debug_descriptor(reid_ctx* ctx, const float* e1, const float* l1, const float* e2, const float* l2, int n, int de, int dl,
                                     float* out) {
    ARG_CHECK(ctx && e1 && l1 && out && n >= 1 && de >= 1 && dl >= 1 && (e2 == nullptr) == (l2 == nullptr));
    CTX_ENTER(ctx);
    const size_t d = (size_t)de + dl, no = ((size_t)n + 1) * d;
    float *d1, *dl1, *d2, *dl2, *dout;
    REID_TRY(dbg_upload(ctx, "dbgp.e1", e1, (size_t)n * de, &d1));
    REID_TRY(dbg_upload(ctx, "dbgp.l1", l1, (size_t)n * dl, &dl1));
    REID_TRY(dbg_upload(ctx, "dbgp.e2", e2, (size_t)n * de, &d2));
    REID_TRY(dbg_upload(ctx, "dbgp.l2", l2, (size_t)n * dl, &dl2));
    REID_TRY(dbg_output(ctx, "dbgp.out", no, &dout));
    REID_TRY(launch_descriptor(ctx, d1, dl1, d2, dl2, n, de, dl, dout));
    REID_TRY(dbg_download(ctx, out, dout, no));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// flip_w_nchw_kernel through launch_flip_w_nchw (the mirrored view of the 256 x 128 descriptor entries), on host operands: x [rows][w] ->
// y [(rows + 1) w]: the mirrored rows and ONE guard row behind them, preset to 0xff bytes with the rest.
extern "C" int reid_debug_flip_w(reid_ctx* ctx, const float* x, long long rows, int w, float* y) {
    ARG_CHECK(ctx && x && y && rows >= 1 && w >= 1);
    CTX_ENTER(ctx);
    const size_t nx = (size_t)rows * w;
    float *dx, *dy;
    REID_TRY(dbg_upload(ctx, "dbgp.x", x, nx, &dx));
    REID_TRY(dbg_output(ctx, "dbgp.y", nx + w, &dy));
    REID_TRY(launch_flip_w_nchw(ctx, dx, rows, w, dy));
    REID_TRY(dbg_download(ctx, y, dy, nx + w));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// ------------------------------------------------------------------------------------------------ evaluation links (tests/test_gpu_eval_links.py)
// shift_mirror_nchw_kernel through launch_shift_mirror (the second view of the reid_descriptor_*_shift entries), on host operands:
// x [m][3][h][w], shift_tl int32 [m][2] -> y [m 3 h w + w]: the view and ONE guard row behind it, preset to 0xff bytes with the rest.
extern "C" int reid_debug_shift_mirror(reid_ctx* ctx, const float* x, int m, int h, int w, const int32_t* shift_tl, int pad,
                                       const float* fill3, float* y) {
    ARG_CHECK(ctx && x && shift_tl && fill3 && y && m >= 1 && h >= 1 && w >= 1 && pad >= 0);
    for (int i = 0; i < 2 * m; ++i) ARG_CHECK(shift_tl[i] >= 0 && shift_tl[i] <= 2 * pad);
    CTX_ENTER(ctx);
    const size_t nx = (size_t)m * 3 * h * w;
    float *dx, *dy;
    int32_t* dtl;
    REID_TRY(dbg_upload(ctx, "dbgl.x", x, nx, &dx));
    REID_TRY(dbg_upload(ctx, "dbgl.tl", shift_tl, (size_t)2 * m, &dtl));
    REID_TRY(dbg_output(ctx, "dbgl.y", nx + w, &dy));
    REID_TRY(launch_shift_mirror(ctx, dx, m, h, w, dtl, pad, fill3, dy));
    REID_TRY(dbg_download(ctx, y, dy, nx + w));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// dist_add_l2_kernel through launch_dist_add_l2 (reid_distmat_add_l2*), on host operands: a [n][d], inout [n n + n] - the matrix, updated
// in place, and ONE guard row behind it, preset to 0xff bytes here.
extern "C" int reid_debug_dist_add_l2(reid_ctx* ctx, const float* a, int n, int d, float* inout) {
    ARG_CHECK(ctx && a && inout && n >= 1 && d >= 1 && d <= 32);
    CTX_ENTER(ctx);
    const size_t nn = (size_t)n * n;
    float *da, *dio;
    REID_TRY(dbg_upload(ctx, "dbgl.a", a, (size_t)n * d, &da));
    REID_TRY(dbg_output(ctx, "dbgl.io", nn + n, &dio));
    HIP_TRY(hipMemcpyAsync(dio, inout, nn * 4, hipMemcpyHostToDevice, ctx->stream));
    REID_TRY(launch_dist_add_l2(ctx, da, n, d, dio));
    REID_TRY(dbg_download(ctx, inout, dio, nn + n));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}
