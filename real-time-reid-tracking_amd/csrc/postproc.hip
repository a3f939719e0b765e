// Post-processing of the reference's evaluation script on the device:
//   * flip test-time augmentation + retrieval descriptor, image_reid_inference.py:112-123,252-253,267-268:
//         d(x) = cat(normalize(emb(x)), normalize(logits(x)));  descriptor = normalize((d(x) + d(hflip(x))) / 2)
//   * camera de-biasing, inference_utils.py:5-15 (`diminish_camera_bias`): per camera c with rows X_c,
//         P = inverse(X_c^T X_c + n_c * la * I);   X_c <- normalize_rows((X_c - mean(X_c)) P^T)
//     The reference inverts a 1263 x 1263 matrix per camera with LAPACK on the CPU.  Here everything stays a GEMM on the
//     fp32 MFMA kernel: the Gram matrix, then Newton-Schulz  X <- X (2I - A X)  from X0 = I / ||A||_inf (A is symmetric
//     positive definite with eigenvalues in [n la, ||A||_inf], so the iteration converges quadratically from the first step
//     and every iterate is a polynomial in A, i.e. symmetric: no transposes), then the projection GEMM and two rounds of
//     residual correction on the projected rows (4 more GEMMs of n_c x d x d), which hold the result to an fp32 LAPACK
//     inverse's accuracy up to condition number 3e4 (tests/test_gpu_postproc.py).
#include "reid_internal.h"
#include "pil_launch.h"
#include "eval_links.h"
#include <string.h>
#include <stdio.h>
#include <stdlib.h>

namespace {

__global__ void flip_w_nchw_kernel(const float* __restrict__ x, long long rows, int w, float* __restrict__ y) {
    const long long total = rows * w;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / w;
        const int c = (int)(i - r * w);
        y[i] = x[r * w + (w - 1 - c)];
    }
}

__device__ __forceinline__ float block_sum(float v, float* sh) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// one block (256 threads) per row: F.normalize semantics (x / max(||x||, 1e-12))
__global__ __launch_bounds__(256) void descriptor_kernel(const float* __restrict__ e1, const float* __restrict__ l1,
                                                         const float* __restrict__ e2, const float* __restrict__ l2, int de,
                                                         int dl, float* __restrict__ out) {
    __shared__ float sh[4];
    const int r = blockIdx.x, tid = threadIdx.x, d = de + dl;
    auto sq = [&](const float* p, int n) {
        float a = 0.f;
        for (int k = tid; k < n; k += 256) a += p[k] * p[k];
        return fmaxf(sqrtf(block_sum(a, sh)), 1e-12f);
    };
    const float ne1 = sq(e1 + (long long)r * de, de), nl1 = sq(l1 + (long long)r * dl, dl);
    float ne2 = 1.f, nl2 = 1.f;
    if (e2) {
        ne2 = sq(e2 + (long long)r * de, de);
        nl2 = sq(l2 + (long long)r * dl, dl);
    }
    float* o = out + (long long)r * d;
    float acc = 0.f;
    for (int k = tid; k < d; k += 256) {
        float v = k < de ? e1[(long long)r * de + k] / ne1 : l1[(long long)r * dl + k - de] / nl1;
        if (e2) {
            const float u = k < de ? e2[(long long)r * de + k] / ne2 : l2[(long long)r * dl + k - de] / nl2;
            v = (v + u) / 2.0f;
        }
        o[k] = v;
        acc += v * v;
    }
    if (!e2) return;   // a single view is already the concatenation of two unit vectors: the reference does not renormalise it
    const float nrm = fmaxf(sqrtf(block_sum(acc, sh)), 1e-12f);
    for (int k = tid; k < d; k += 256) o[k] = o[k] / nrm;
}

// gather rows idx[i] of x [.][d] into cur [ni][dp] (zero padded) and accumulate the column mean
__global__ void gather_rows_kernel(const float* __restrict__ x, const int32_t* __restrict__ idx, int ni, int d, int dp,
                                   float* __restrict__ cur) {
    const long long total = (long long)ni * dp;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(i / dp), c = (int)(i - (long long)r * dp);
        cur[i] = c < d ? x[(long long)idx[r] * d + c] : 0.f;
    }
}
// column means of cur [ni][dp]: one thread per column, rows in order (the reference's mean(dim=0) sums rows sequentially)
__global__ void col_mean_kernel(const float* __restrict__ cur, int ni, int dp, float* __restrict__ mean) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= dp) return;
    float a = 0.f;
    for (int r = 0; r < ni; ++r) a += cur[(long long)r * dp + c];
    mean[c] = a / (float)ni;
}
__global__ void center_kernel(const float* __restrict__ cur, const float* __restrict__ mean, long long total, int dp,
                              float* __restrict__ out) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        out[i] = cur[i] - mean[i % dp];
}
// cur [ni][dp] -> curT [dp][nip] (zero padded columns)
__global__ void transpose_kernel(const float* __restrict__ cur, int ni, int dp, int nip, float* __restrict__ curT) {
    const long long total = (long long)dp * nip;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i / nip), r = (int)(i - (long long)c * nip);
        curT[i] = r < ni ? cur[(long long)r * dp + c] : 0.f;
    }
}
// A = G + ridge * I on the real d x d block, ridge * I on the padding; row_abs[r] = sum |A[r][:]|
__global__ void ridge_rowsum_kernel(float* __restrict__ a, int d, int dp, float ridge, float* __restrict__ row_abs) {
    __shared__ float sh[4];
    const int r = blockIdx.x;
    float s = 0.f;
    for (int c = threadIdx.x; c < dp; c += 256) {
        float v = a[(long long)r * dp + c];
        if (r >= d || c >= d) v = 0.f;
        if (r == c) v = r < d ? v + ridge : ridge;   // padding: any positive value inside the spectrum (never read back)
        a[(long long)r * dp + c] = v;
        s += fabsf(v);
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0) row_abs[r] = s;
}
__global__ void max_kernel(const float* __restrict__ v, int n, float* __restrict__ out) {
    __shared__ float sh[4];
    float m = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, v[i]);
    for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}
__global__ void scaled_identity_kernel(const float* __restrict__ alpha, int dp, float* __restrict__ x) {
    const long long total = (long long)dp * dp;
    const float inv = 1.0f / alpha[0];
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        x[i] = (i / dp == i % dp) ? inv : 0.f;
}
// tt <- (2I - t)^T, and res += ||I - t||_F^2 of t = A X (the residual of the current iterate).  The transposed copy makes
// the second product of the step, computed as X . tt^T by the A.B^T GEMM, exactly X (2I - A X).
__global__ void two_i_minus_t_kernel(const float* __restrict__ t, int dp, float* __restrict__ tt, float* __restrict__ res) {
    const long long total = (long long)dp * dp;
    float acc = 0.f;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(i / dp), c = (int)(i - (long long)r * dp);
        const float eye = r == c ? 1.0f : 0.0f;
        const float v = t[i];
        acc += (eye - v) * (eye - v);
        tt[(long long)c * dp + r] = 2.0f * eye - v;
    }
    for (int o = 32; o; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(res, acc);
}
// x <- (x + x^T) / 2: keeps every iterate exactly symmetric, so that A . x^T (what the GEMM computes) is A x
__global__ void symmetrize_kernel(float* __restrict__ x, int dp) {
    const long long total = (long long)dp * dp;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(i / dp), c = (int)(i - (long long)r * dp);
        if (c <= r) continue;
        const float m = 0.5f * (x[i] + x[(long long)c * dp + r]);
        x[i] = m;
        x[(long long)c * dp + r] = m;
    }
}
// out = a + s * b (s = -1: the residual C - Y A of the projected rows; s = 1: the correction added to them); out may be a or b
__global__ void add_scaled_kernel(const float* a, const float* b, float s, long long total, float* out) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        out[i] = a[i] + s * b[i];
}
// out rows (normalised with torch.norm semantics: plain division) scattered back to x[idx[r]][:d]
__global__ __launch_bounds__(256) void normalize_scatter_kernel(const float* __restrict__ y, const int32_t* __restrict__ idx,
                                                                int d, int dp, float* __restrict__ x) {
    __shared__ float sh[4];
    const int r = blockIdx.x;
    float a = 0.f;
    for (int c = threadIdx.x; c < d; c += 256) a += y[(long long)r * dp + c] * y[(long long)r * dp + c];
    const float nrm = sqrtf(block_sum(a, sh));
    float* o = x + (long long)idx[r] * d;
    for (int c = threadIdx.x; c < d; c += 256) o[c] = y[(long long)r * dp + c] / nrm;
}

inline int grid_for(long long work) {
    long long g = (work + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

int gemm_nt_dev(reid_ctx* ctx, const float* a, int m, const float* b, int n, int k, float* c) {
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.A = a; p.lda = k;
    p.B = b; p.ldb = k;
    p.M = m; p.N = n; p.K = k;
    p.C = c; p.ldc = n;
    return launch_gemm_f32(ctx, A_DENSE, E_BIAS, p, REID_K_DIST_GEMM, 2.0 * m * n * k, 4.0 * ((double)m * k + (double)n * k + (double)m * n));
}

}  // namespace

// descriptor_kernel, one block per row: e1 / e2 [n][de], l1 / l2 [n][dl] (e2 and l2 both nullptr: a single view) -> out [n][de + dl]
int launch_descriptor(reid_ctx* ctx, const float* e1, const float* l1, const float* e2, const float* l2, int n, int de, int dl, float* out) {
    prof_begin(ctx, REID_K_ELEMENTWISE, 0, (double)n * (de + dl) * 4.0 * (e2 ? 3 : 2));
    hipLaunchKernelGGL(descriptor_kernel, dim3(n), dim3(256), 0, ctx->stream, e1, l1, e2, l2, de, dl, out);
    prof_end(ctx);
    LAUNCH_CHECK();
    return REID_OK;
}

// flip_w_nchw_kernel: y [rows][w] = x [rows][w] with its columns reversed
int launch_flip_w_nchw(reid_ctx* ctx, const float* x, long long rows, int w, float* y) {
    hipLaunchKernelGGL(flip_w_nchw_kernel, dim3(grid_for(rows * w)), dim3(256), 0, ctx->stream, x, rows, w, y);
    LAUNCH_CHECK();
    return REID_OK;
}

// ---- libreid_hip_eval_links.so (eval_links.h), opened on the first call that needs it: the shifted mirrored view of the
// reid_descriptor_*_shift entries and reid_distmat_add_l2*.
static struct EvalLinksLib : SideLib {
    EvalLinksLib() : SideLib("libreid_hip_eval_links.so", "the shifted mirrored view (reid_descriptor_*_shift) and reid_distmat_add_l2 need") {}
    SIDE_FN(shift_mirror, eval_links_shift_mirror);
    SIDE_FN(dist_add_l2, eval_links_dist_add_l2);
} eval_links;

// shift_mirror_nchw_kernel: y = crop(pad(mirror(x))) of x [m][3][h][w], (top, left) per image from d_shift_tl (device int32 [m][2])
int launch_shift_mirror(reid_ctx* ctx, const float* x, int m, int h, int w, const int32_t* d_shift_tl, int pad, const float* fill3, float* y) {
    REID_TRY(eval_links.open());
    prof_begin(ctx, REID_K_ELEMENTWISE, 0, 8.0 * m * 3 * h * w);
    const hipError_t e = eval_links.shift_mirror(ctx->stream, x, m, h, w, d_shift_tl, pad, fill3, y);
    prof_end(ctx);
    return eval_links.status(e, eval_links.shift_mirror);
}

// dist_add_l2_kernel: d_inout [n][n] += euclidean_dist(a, a), a [n][d]
int launch_dist_add_l2(reid_ctx* ctx, const float* a, int n, int d, float* d_inout) {
    REID_TRY(eval_links.open());
    prof_begin(ctx, REID_K_ELEMENTWISE, 2.0 * n * n * d, 8.0 * n * n);
    const hipError_t e = eval_links.dist_add_l2(ctx->stream, a, n, d, d_inout);
    prof_end(ctx);
    return eval_links.status(e, eval_links.dist_add_l2);
}

// The second view of the reid_descriptor_*_shift entries (strong_inference, reid/data_transforms.py:130-191): the mirror shifted by
// (top - pad, left - pad) over a border of `fill`.  d_tl: device int32 [n][2] of the call's images (descriptor_dev's n).
struct ShiftView {
    const int32_t* d_tl;
    int pad;
    float fill[3];
};

// pad in 0 .. 32 and every (top, left) in [0, 2 pad]: REID_ERR_ARG naming the image otherwise
static int shift_check(const char* who, const int32_t* shift_tl, int n, int pad) {
    if (pad < 0 || pad > 32) {
        reid_set_error("%s: pad %d outside 0 .. 32", who, pad);
        return REID_ERR_ARG;
    }
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 2; ++k)
            if (shift_tl[2 * i + k] < 0 || shift_tl[2 * i + k] > 2 * pad) {
                reid_set_error("%s: shift_tl of image %d: %s %d outside [0, 2 pad = %d]", who, i, k ? "left" : "top", shift_tl[2 * i + k],
                               2 * pad);
                return REID_ERR_ARG;
            }
    return REID_OK;
}

// x: [n][3][256][128] fp32 already normalised by the caller's transform (the evaluation script uses ImageNet mean/std,
// data_transforms.py:56-130); out: [n][512 + num_class].  flip_tta != 0 averages the descriptor of the mirrored image.
// before_view(v, i, m) runs before the forward of images [i, i + m) of view v (0 plain, 1 mirrored): nothing for the float entries,
// the side indices of the pass for reid_descriptor_images_u8.
// h x w other than 256 x 128 (or the debug switch anysize_force): the any-size forward of api.hip in passes of se_any_pass images, the
// mirrored view read with reversed columns by its layout kernel (no flipped copy of the batch).
// sv != nullptr (the *_shift entries, flip_tta on): the second view is the SHIFTED mirror - at 256 x 128 shift_mirror_nchw_kernel writes
// pp.flip in place of flip_w_nchw_kernel, at another size it writes a shifted copy of the pass (pp.shift) and the any-size forward runs
// on it with mirror = 0.  Everything else is the same call.
template <class BeforeView>
static int descriptor_dev(reid_ctx* ctx, const float* d_x, int n, int h, int w, int flip_tta, float* d_out, BeforeView before_view,
                          const ShiftView* sv = nullptr) {
    ARG_CHECK(ctx && d_x && d_out && n >= 0);
    REID_TRY(se_any_ready(ctx, h, w, "reid_descriptor_*_hw"));
    CTX_ENTER(ctx);
    if (n == 0) return REID_OK;
    int de = 0, nc = 0;
    REID_TRY(reid_seres18_dims(ctx, &de, &nc));
    if (nc <= 0) {
        reid_set_error("reid_descriptor_*: the loaded weights have no classifier (cls.w), the descriptor needs the logits");
        return REID_ERR_STATE;
    }
    const size_t img = (size_t)3 * h * w;
    float *e1, *l1, *e2 = nullptr, *l2 = nullptr, *xf = nullptr;
    REID_TRY(ctx_ws(ctx, "pp.e1", (size_t)n * de * 4, (void**)&e1));
    REID_TRY(ctx_ws(ctx, "pp.l1", (size_t)n * nc * 4 + 16, (void**)&l1));
    REID_TRY(before_view(0, 0, n));
    if (se_any_routes(ctx, h, w)) {
        REID_TRY(reid_embed_f32_nchw_hw_dev(ctx, d_x, n, h, w, e1, l1));
        if (flip_tta) {
            REID_TRY(ctx_ws(ctx, "pp.e2", (size_t)n * de * 4, (void**)&e2));
            REID_TRY(ctx_ws(ctx, "pp.l2", (size_t)n * nc * 4 + 16, (void**)&l2));
            const int pass = se_any_pass(ctx, h, w);
            for (int i = 0; i < n; i += pass) {
                const int m = n - i < pass ? n - i : pass;
                if (sv) {
                    if (!xf) REID_TRY(ctx_ws(ctx, "pp.shift", (size_t)(n < pass ? n : pass) * img * 4, (void**)&xf));
                    REID_TRY(launch_shift_mirror(ctx, d_x + (size_t)i * img, m, h, w, sv->d_tl + 2 * (size_t)i, sv->pad, sv->fill, xf));
                }
                REID_TRY(before_view(1, i, m));
                REID_TRY(se_any_run_nchw(ctx, sv ? xf : d_x + (size_t)i * img, m, h, w, sv ? 0 : 1, e2 + (size_t)i * de, l2 + (size_t)i * nc));
            }
        }
        return launch_descriptor(ctx, e1, l1, e2, l2, n, de, nc, d_out);
    }
    REID_TRY(reid_embed_f32_nchw_dev(ctx, d_x, n, e1, l1));
    if (flip_tta) {
        REID_TRY(ctx_ws(ctx, "pp.e2", (size_t)n * de * 4, (void**)&e2));
        REID_TRY(ctx_ws(ctx, "pp.l2", (size_t)n * nc * 4 + 16, (void**)&l2));
        const int chunk = ctx->chunk;
        REID_TRY(ctx_ws(ctx, "pp.flip", (size_t)chunk * img * 4, (void**)&xf));
        for (int i = 0; i < n; i += chunk) {
            const int m = n - i < chunk ? n - i : chunk;
            const long long rows = (long long)m * 3 * 256;
            if (sv) REID_TRY(launch_shift_mirror(ctx, d_x + (size_t)i * img, m, 256, 128, sv->d_tl + 2 * (size_t)i, sv->pad, sv->fill, xf));
            else REID_TRY(launch_flip_w_nchw(ctx, d_x + (size_t)i * img, rows, 128, xf));
            REID_TRY(before_view(1, i, m));
            REID_TRY(reid_embed_f32_nchw_dev(ctx, xf, m, e2 + (size_t)i * de, l2 + (size_t)i * nc));
        }
    }
    return launch_descriptor(ctx, e1, l1, e2, l2, n, de, nc, d_out);
}

// the debug switch anysize_force belongs to the reid_*_hw entries: the entries without a size keep the 256 x 128 forward whatever it says
struct ForceOff {
    reid_ctx* ctx;
    int saved;
    explicit ForceOff(reid_ctx* c) : ctx(c), saved(c ? c->anysize_force : 0) {
        if (ctx) ctx->anysize_force = 0;
    }
    ~ForceOff() {
        if (ctx) ctx->anysize_force = saved;
    }
};

extern "C" int reid_descriptor_f32_nchw_hw_dev(reid_ctx* ctx, const float* d_x, int n, int h, int w, int flip_tta, float* d_out) {
    return descriptor_dev(ctx, d_x, n, h, w, flip_tta, d_out, [](int, int, int) -> int { return REID_OK; });
}

extern "C" int reid_descriptor_f32_nchw_dev(reid_ctx* ctx, const float* d_x, int n, int flip_tta, float* d_out) {
    ForceOff off(ctx);
    return descriptor_dev(ctx, d_x, n, 256, 128, flip_tta, d_out, [](int, int, int) -> int { return REID_OK; });
}

extern "C" int reid_descriptor_f32_nchw_hw(reid_ctx* ctx, const float* x, int n, int h, int w, int flip_tta, float* out) {
    ARG_CHECK(ctx && x && out && n >= 0);
    REID_TRY(se_any_ready(ctx, h, w, "reid_descriptor_f32_nchw_hw"));
    CTX_ENTER(ctx);
    if (n == 0) return REID_OK;
    int de = 0, nc = 0;
    REID_TRY(reid_seres18_dims(ctx, &de, &nc));
    const size_t img = (size_t)3 * h * w;
    float *dx, *dout;
    REID_TRY(ctx_ws(ctx, "pp.x", (size_t)n * img * 4, (void**)&dx));
    REID_TRY(ctx_ws(ctx, "pp.out", (size_t)n * (de + (nc > 0 ? nc : 0)) * 4 + 16, (void**)&dout));
    HIP_TRY(hipMemcpyAsync(dx, x, (size_t)n * img * 4, hipMemcpyHostToDevice, ctx->stream));
    REID_TRY(reid_descriptor_f32_nchw_hw_dev(ctx, dx, n, h, w, flip_tta, dout));
    HIP_TRY(hipMemcpyAsync(out, dout, (size_t)n * (de + nc) * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

extern "C" int reid_descriptor_f32_nchw(reid_ctx* ctx, const float* x, int n, int flip_tta, float* out) {
    ForceOff off(ctx);
    return reid_descriptor_f32_nchw_hw(ctx, x, n, 256, 128, flip_tta, out);
}

// reid_descriptor_f32_nchw_hw* with flip_tta = 1 and the SHIFTED mirror as the second view.  What is refused, with nothing queued: the
// arguments of the shift (REID_ERR_ARG), what reid_descriptor_f32_nchw_hw* refuses, a missing libreid_hip_eval_links.so (REID_ERR_STATE).
static int shift_entry_ready(reid_ctx* ctx, const char* who, int n, int h, int w, const int32_t* shift_tl, int pad, const float* fill3) {
    ARG_CHECK(ctx && shift_tl && n >= 0);
    if (!fill3) {
        reid_set_error("%s: fill3 is NULL (the border of the shifted view, e.g. (0 - mean) / std per channel)", who);
        return REID_ERR_ARG;
    }
    REID_TRY(shift_check(who, shift_tl, n, pad));
    REID_TRY(se_any_ready(ctx, h, w, who));
    return eval_links.open();
}

extern "C" int reid_descriptor_f32_nchw_shift_dev(reid_ctx* ctx, const float* d_x, int n, int h, int w, const int32_t* shift_tl, int pad,
                                                  const float* fill3, float* d_out) {
    ARG_CHECK(ctx && d_x && d_out);
    REID_TRY(shift_entry_ready(ctx, "reid_descriptor_f32_nchw_shift_dev", n, h, w, shift_tl, pad, fill3));
    CTX_ENTER(ctx);
    if (n == 0) return REID_OK;
    ShiftView sv{nullptr, pad, {fill3[0], fill3[1], fill3[2]}};
    REID_TRY(ctx_ws(ctx, "pp.tl", (size_t)n * 8, (void**)&sv.d_tl));
    HIP_TRY(hipMemcpyAsync((void*)sv.d_tl, shift_tl, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));   // shift_tl is the caller's: not read after this call returns
    return descriptor_dev(ctx, d_x, n, h, w, 1, d_out, [](int, int, int) -> int { return REID_OK; }, &sv);
}

extern "C" int reid_descriptor_f32_nchw_shift(reid_ctx* ctx, const float* x, int n, int h, int w, const int32_t* shift_tl, int pad,
                                              const float* fill3, float* out) {
    ARG_CHECK(ctx && x && out);
    REID_TRY(shift_entry_ready(ctx, "reid_descriptor_f32_nchw_shift", n, h, w, shift_tl, pad, fill3));
    CTX_ENTER(ctx);
    if (n == 0) return REID_OK;
    int de = 0, nc = 0;
    REID_TRY(reid_seres18_dims(ctx, &de, &nc));
    const size_t img = (size_t)3 * h * w;
    float *dx, *dout;
    REID_TRY(ctx_ws(ctx, "pp.x", (size_t)n * img * 4, (void**)&dx));
    REID_TRY(ctx_ws(ctx, "pp.out", (size_t)n * (de + (nc > 0 ? nc : 0)) * 4 + 16, (void**)&dout));
    HIP_TRY(hipMemcpyAsync(dx, x, (size_t)n * img * 4, hipMemcpyHostToDevice, ctx->stream));
    REID_TRY(reid_descriptor_f32_nchw_shift_dev(ctx, dx, n, h, w, shift_tl, pad, fill3, dout));
    HIP_TRY(hipMemcpyAsync(out, dout, (size_t)n * (de + nc) * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

// uint8 images of any sizes in: transforms.Resize((256, 128)) as PIL computes it -> ToTensor -> Normalize on the device (PilPlan,
// libreid_hip_pil_resize.so), then per pass of `chunk` images what reid_descriptor_f32_nchw_dev runs on that pass - the same passes, the
// same kernels, so the same bits as reid_descriptor_f32_nchw on the images preprocessed on the host.  n pending side indices serve the
// plain and the mirrored view of an image, as the script's model(img, cam.repeat(2)) and as reid_swin_descriptor_*; the float entry
// computes the same when it is given the indices twice (its plain passes take the first n, its mirrored passes the next n).  None stays
// pending.
// shift_tl != nullptr (reid_descriptor_images_u8_shift): the second view is the shifted mirror over a border of the table's entry for
// pixel value 0 - Pad(fill = 0) on the 8-bit image, then ToTensor + Normalize.
static int descriptor_images_u8(reid_ctx* ctx, const char* who, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n,
                                int out_h, int out_w, const float* mean_std6, int flip_tta, const int32_t* shift_tl, int pad, float* out) {
    ARG_CHECK(ctx);
    struct SideDrop {
        reid_ctx* ctx;
        ~SideDrop() {
            ctx->side_idx.clear();
            ctx->side_cursor = 0;
        }
    } drop{ctx};
    ARG_CHECK(packed && offsets && hw && out && n >= 0);
    REID_TRY(pil_mean_std(&mean_std6));
    RaggedSrc src{packed, offsets, hw, n};
    REID_TRY(src.check());
    if (shift_tl) REID_TRY(shift_check(who, shift_tl, n, pad));
    REID_TRY(se_any_ready(ctx, out_h, out_w, who));
    if (shift_tl) REID_TRY(eval_links.open());
    CTX_ENTER(ctx);
    if (n == 0) return REID_OK;
    int de = 0, nc = 0;
    REID_TRY(reid_seres18_dims(ctx, &de, &nc));
    if (nc <= 0) {
        reid_set_error("reid_descriptor_*: the loaded weights have no classifier (cls.w), the descriptor needs the logits");
        return REID_ERR_STATE;
    }
    const int pass = se_any_routes(ctx, out_h, out_w) ? se_any_pass(ctx, out_h, out_w) : ctx->chunk;
    PilPlan plan;
    REID_TRY(plan.build(src, out_h, out_w, mean_std6, pass));
    std::vector<int32_t> side;
    if (!ctx->side_idx.empty()) {
        side.assign(ctx->side_idx.begin() + ctx->side_cursor, ctx->side_idx.end());
        if (side.size() != (size_t)n) {
            reid_set_error("reid_descriptor_images_u8: %d images but %zu side indices are pending", n, side.size());
            return REID_ERR_ARG;
        }
    }
    EmbedOut o{out, nullptr, de + nc, 0};
    REID_TRY(src.alloc(ctx, "io"));
    REID_TRY(o.alloc(ctx, "ppd", n, 0, false));
    REID_TRY(plan.alloc(ctx, "io"));
    ShiftView sv{nullptr, pad, {plan.table[0], plan.table[256], plan.table[512]}};
    if (shift_tl) REID_TRY(ctx_ws(ctx, "pp.tl", (size_t)n * 8, (void**)&sv.d_tl));
    return embed_host(
        ctx, n, pass,
        [&](int i, int m, hipStream_t s) -> int {
            REID_TRY(src.up(i, m, s));
            if (i == 0 && shift_tl) HIP_TRY(hipMemcpyAsync((void*)sv.d_tl, shift_tl, (size_t)n * 8, hipMemcpyHostToDevice, s));
            return i == 0 ? plan.up(s) : REID_OK;
        },
        [&](int i, int m, float* d_row, float*) -> int {
            REID_TRY(plan.launch(ctx, src, i, m, nullptr, plan.d_f32));
            const ShiftView pass_sv{sv.d_tl + 2 * (size_t)i, sv.pad, {sv.fill[0], sv.fill[1], sv.fill[2]}};
            return descriptor_dev(
                ctx, plan.d_f32, m, out_h, out_w, flip_tta, d_row,
                [&](int, int, int) -> int {
                    if (!side.empty()) {
                        ctx->side_idx.assign(side.begin() + i, side.begin() + i + m);
                        ctx->side_cursor = 0;
                    }
                    return REID_OK;
                },
                shift_tl ? &pass_sv : nullptr);
        },
        o);
}

extern "C" int reid_descriptor_images_u8_hw(reid_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n, int out_h,
                                            int out_w, const float* mean_std6, int flip_tta, float* out) {
    return descriptor_images_u8(ctx, "reid_descriptor_images_u8_hw", packed, offsets, hw, n, out_h, out_w, mean_std6, flip_tta, nullptr, 0, out);
}

extern "C" int reid_descriptor_images_u8_shift(reid_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n,
                                               int out_h, int out_w, const float* mean_std6, const int32_t* shift_tl, int pad, float* out) {
    if (ctx && !shift_tl) {   // the pending side indices are dropped as on every other refusal of this entry
        ctx->side_idx.clear();
        ctx->side_cursor = 0;
    }
    ARG_CHECK(ctx && shift_tl);
    return descriptor_images_u8(ctx, "reid_descriptor_images_u8_shift", packed, offsets, hw, n, out_h, out_w, mean_std6, 1, shift_tl, pad, out);
}

// d_inout [n][n] += euclidean_dist(a, a) (reid/losses/utils.py:21-35), a [n][d] - the attribute term the evaluation script adds to the
// Jaccard matrix (image_reid_inference.py:276-289) - in place, one read and one write of the matrix (dist_add_l2_kernel, eval_links.h).
extern "C" int reid_distmat_add_l2_dev(reid_ctx* ctx, const float* d_a, int n, int d, float* d_inout) {
    ARG_CHECK(ctx && n >= 0);
    if (d < 1 || d > 32) {
        reid_set_error("reid_distmat_add_l2: d = %d outside 1 .. 32", d);
        return REID_ERR_ARG;
    }
    if (n == 0) return REID_OK;
    ARG_CHECK(d_a && d_inout && ((uintptr_t)d_inout & 15) == 0);
    REID_TRY(eval_links.open());
    CTX_ENTER(ctx);
    return launch_dist_add_l2(ctx, d_a, n, d, d_inout);
}

extern "C" int reid_distmat_add_l2(reid_ctx* ctx, const float* a, int n, int d, float* inout) {
    ARG_CHECK(ctx && n >= 0);
    if (d < 1 || d > 32) {
        reid_set_error("reid_distmat_add_l2: d = %d outside 1 .. 32", d);
        return REID_ERR_ARG;
    }
    if (n == 0) return REID_OK;
    ARG_CHECK(a && inout);
    REID_TRY(eval_links.open());
    CTX_ENTER(ctx);
    float *da, *dio;
    REID_TRY(ctx_ws(ctx, "addl2.a", (size_t)n * d * 4, (void**)&da));
    REID_TRY(ctx_ws(ctx, "addl2.io", (size_t)n * n * 4, (void**)&dio));
    HIP_TRY(hipMemcpyAsync(da, a, (size_t)n * d * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(dio, inout, (size_t)n * n * 4, hipMemcpyHostToDevice, ctx->stream));
    REID_TRY(launch_dist_add_l2(ctx, da, n, d, dio));
    HIP_TRY(hipMemcpyAsync(inout, dio, (size_t)n * n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ctx_fault_status(ctx);
}

extern "C" int reid_descriptor_images_u8(reid_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n,
                                         const float* mean_std6, int flip_tta, float* out) {
    ForceOff off(ctx);
    return reid_descriptor_images_u8_hw(ctx, packed, offsets, hw, n, 256, 128, mean_std6, flip_tta, out);
}

// d_x [n][d] is updated in place; cams is a HOST array of camera ids >= 0 (ids without rows are skipped: the reference's
// torch.inverse of an all-zero matrix would raise).  iters <= 0 selects the default number of Newton-Schulz steps.
extern "C" int reid_cam_debias_dev(reid_ctx* ctx, float* d_x, const int32_t* cams, int n, int d, float la, int iters) {
    ARG_CHECK(ctx && d_x && cams && n >= 1 && d >= 1 && la > 0.f);
    CTX_GUARD(ctx);
    if (iters <= 0) iters = 40;   // upper bound; the residual rule below stops after ~8-14 steps
    int ncam = 0;
    for (int i = 0; i < n; ++i) {
        ARG_CHECK(cams[i] >= 0);
        if (cams[i] + 1 > ncam) ncam = cams[i] + 1;
    }
    const int dp = (d + 3) / 4 * 4;
    std::vector<std::vector<int32_t>> rows(ncam);
    for (int i = 0; i < n; ++i) rows[cams[i]].push_back(i);
    size_t max_ni = 0;
    for (auto& r : rows) max_ni = r.size() > max_ni ? r.size() : max_ni;
    const int max_nip = (int)((max_ni + 3) / 4 * 4);
    int32_t* d_idx;
    float *cur, *cen, *curT, *mean, *A, *X, *T, *T2, *X2, *rowabs, *alpha;
    REID_TRY(ctx_ws(ctx, "cd.idx", (size_t)n * 4, (void**)&d_idx));
    REID_TRY(ctx_ws(ctx, "cd.cur", max_ni * dp * 4, (void**)&cur));
    REID_TRY(ctx_ws(ctx, "cd.cen", max_ni * dp * 4, (void**)&cen));
    REID_TRY(ctx_ws(ctx, "cd.curT", (size_t)dp * max_nip * 4, (void**)&curT));
    REID_TRY(ctx_ws(ctx, "cd.mean", (size_t)dp * 4, (void**)&mean));
    REID_TRY(ctx_ws(ctx, "cd.A", (size_t)dp * dp * 4, (void**)&A));
    REID_TRY(ctx_ws(ctx, "cd.X", (size_t)dp * dp * 4, (void**)&X));
    REID_TRY(ctx_ws(ctx, "cd.T", (size_t)dp * dp * 4, (void**)&T));
    REID_TRY(ctx_ws(ctx, "cd.T2", (size_t)dp * dp * 4, (void**)&T2));
    REID_TRY(ctx_ws(ctx, "cd.X2", (size_t)dp * dp * 4, (void**)&X2));
    REID_TRY(ctx_ws(ctx, "cd.rowabs", (size_t)dp * 4, (void**)&rowabs));
    REID_TRY(ctx_ws(ctx, "cd.alpha", 16, (void**)&alpha));
    float *res, *corr;
    REID_TRY(ctx_ws(ctx, "cd.res", max_ni * dp * 4, (void**)&res));
    REID_TRY(ctx_ws(ctx, "cd.corr", max_ni * dp * 4, (void**)&corr));
    hipStream_t st = ctx->stream;
    size_t off = 0;
    std::vector<int32_t> flat;
    flat.reserve(n);
    for (auto& r : rows) flat.insert(flat.end(), r.begin(), r.end());
    HIP_TRY(hipMemcpyAsync(d_idx, flat.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int c = 0; c < ncam; ++c) {
        const int ni = (int)rows[c].size();
        if (ni == 0) continue;
        const int nip = (ni + 3) / 4 * 4;
        const int32_t* idx = d_idx + off;
        off += ni;
        const long long tot = (long long)ni * dp;
        hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for(tot)), dim3(256), 0, st, d_x, idx, ni, d, dp, cur);
        hipLaunchKernelGGL(col_mean_kernel, dim3((dp + 255) / 256), dim3(256), 0, st, cur, ni, dp, mean);
        hipLaunchKernelGGL(center_kernel, dim3(grid_for(tot)), dim3(256), 0, st, cur, mean, tot, dp, cen);
        hipLaunchKernelGGL(transpose_kernel, dim3(grid_for((long long)dp * nip)), dim3(256), 0, st, cur, ni, dp, nip, curT);
        LAUNCH_CHECK();
        REID_TRY(gemm_nt_dev(ctx, curT, dp, curT, dp, nip, A));                      // G = X_c^T X_c (uncentred, as the reference)
        hipLaunchKernelGGL(ridge_rowsum_kernel, dim3(dp), dim3(256), 0, st, A, d, dp, (float)ni * la, rowabs);
        hipLaunchKernelGGL(max_kernel, dim3(1), dim3(256), 0, st, rowabs, dp, alpha);
        hipLaunchKernelGGL(scaled_identity_kernel, dim3(grid_for((long long)dp * dp)), dim3(256), 0, st, alpha, dp, X);
        LAUNCH_CHECK();
        // Newton-Schulz with a stopping rule: the residual ||I - A X||_F squares every step until it reaches the fp32 noise
        // floor; iterating past that point lets rounding errors (which do not commute with A) grow, so stop as soon as
        // the residual no longer halves and keep the better of the last two iterates.
        float *xa = X, *xb = X2;
        float r_prev = INFINITY;
        bool stopped = false;   // the rule below ended the iteration: xa is the inverse to fp32 accuracy (not when `iters` ran out first)
        for (int it = 0; it < iters; ++it) {
            REID_TRY(gemm_nt_dev(ctx, A, dp, xa, dp, dp, T));                        // T = A X   (X symmetric)
            HIP_TRY(hipMemsetAsync(alpha + 1, 0, 4, st));
            hipLaunchKernelGGL(two_i_minus_t_kernel, dim3(grid_for((long long)dp * dp)), dim3(256), 0, st, T, dp, T2, alpha + 1);
            LAUNCH_CHECK();
            float r2 = 0.f;
            HIP_TRY(hipMemcpyAsync(&r2, alpha + 1, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            const float r = sqrtf(r2);
            if (it == 0 && !(r < INFINITY)) {   // NaN / inf in the input rows: there is no previous iterate to fall back to
                reid_set_error("reid_cam_debias: non-finite residual for camera %d (NaN or inf in its rows?)", c);
                return REID_ERR_ARG;
            }
            if (!(r < r_prev)) {            // got worse (or NaN): the previous iterate is the answer
                float* t = xa; xa = xb; xb = t;
                stopped = true;
                break;
            }
            // quadratic phase (r_prev < 1e-2 would square to < 1e-4) but no longer halving: noise floor, keep the current iterate
            if ((r_prev < 1e-2f && r > 0.5f * r_prev) || r < 1e-6f) {
                stopped = true;
                break;
            }
            r_prev = r;
            REID_TRY(gemm_nt_dev(ctx, xa, dp, T2, dp, dp, xb));                      // X' = X (2I - A X)
            hipLaunchKernelGGL(symmetrize_kernel, dim3(grid_for((long long)dp * dp)), dim3(256), 0, st, xb, dp);
            LAUNCH_CHECK();
            float* t = xa; xa = xb; xb = t;
        }
        REID_TRY(gemm_nt_dev(ctx, cen, ni, xa, dp, dp, cur));                        // Y = (X_c - mean) P^T, P symmetric
        // Two rounds of residual correction on the projected rows, Y <- Y + (C - Y A) X with C the centred rows.  X carries entries of
        // size 1 / (n la) while C lies mostly in the well-conditioned subspace of A, so C X alone loses kappa^2 eps to cancellation; the
        // residual C - Y A is small and computed from A itself, which brings Y to what an fp32 LAPACK inverse gives (kappa eps).  Only
        // behind a finished inverse: on an iterate cut short by `iters` a round would be one more Newton-Schulz step in disguise.
        for (int round = 0; stopped && round < 2; ++round) {
            REID_TRY(gemm_nt_dev(ctx, cur, ni, A, dp, dp, res));                     // Y A   (A symmetric)
            hipLaunchKernelGGL(add_scaled_kernel, dim3(grid_for(tot)), dim3(256), 0, st, cen, res, -1.0f, tot, res);
            LAUNCH_CHECK();
            REID_TRY(gemm_nt_dev(ctx, res, ni, xa, dp, dp, corr));                   // (C - Y A) X
            hipLaunchKernelGGL(add_scaled_kernel, dim3(grid_for(tot)), dim3(256), 0, st, cur, corr, 1.0f, tot, cur);
            LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(normalize_scatter_kernel, dim3(ni), dim3(256), 0, st, cur, idx, d, dp, d_x);
        LAUNCH_CHECK();
    }
    return REID_OK;
}

extern "C" int reid_cam_debias(reid_ctx* ctx, float* x, const int32_t* cams, int n, int d, float la, int iters) {
    ARG_CHECK(ctx && x && cams && n >= 1 && d >= 1 && la > 0.f);
    CTX_GUARD(ctx);
    float* dx;
    REID_TRY(ctx_ws(ctx, "cd.x", (size_t)n * d * 4, (void**)&dx));
    HIP_TRY(hipMemcpyAsync(dx, x, (size_t)n * d * 4, hipMemcpyHostToDevice, ctx->stream));
    REID_TRY(reid_cam_debias_dev(ctx, dx, cams, n, d, la, iters));
    HIP_TRY(hipMemcpyAsync(x, dx, (size_t)n * d * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return REID_OK;
}

// ---- smooth_tracklets, reid/inference_utils.py:18-27: every valid row of a tracklet (rows with the same sequence id) becomes
// keep * row + (1 - keep) * mean(valid rows of the tracklet), keep = 0.1 in the reference.  Rows are grouped on the host (CSR
// of row indices per tracklet); one block column-slice per tracklet: a thread owns a column, sums it over the tracklet's rows
// in row order (coalesced across the 256 columns of the slice), then rewrites the rows.
__global__ __launch_bounds__(256) void smooth_tracklets_kernel(float* __restrict__ x, const int32_t* __restrict__ rows,
                                                               const int32_t* __restrict__ start, int d, float keep) {
    const int g = blockIdx.x, col = blockIdx.y * 256 + threadIdx.x;
    if (col >= d) return;
    const int b = start[g], e = start[g + 1];
    float acc = 0.f;
    for (int i = b; i < e; ++i) acc += x[(long long)rows[i] * d + col];
    const float avg = acc / (float)(e - b);
    for (int i = b; i < e; ++i) {
        float* p = x + (long long)rows[i] * d + col;
        *p = *p * keep + avg * (1.0f - keep);
    }
}

extern "C" int reid_smooth_tracklets_dev(reid_ctx* ctx, float* d_x, const int32_t* seqs, const uint8_t* valid, int n, int d,
                                         float keep) {
    ARG_CHECK(ctx && d_x && seqs && n >= 0 && d >= 1);
    CTX_GUARD(ctx);
    if (n == 0) return REID_OK;
    std::map<int32_t, std::vector<int32_t>> groups;   // ordered like np.unique(seqs)
    for (int i = 0; i < n; ++i)
        if (!valid || valid[i]) groups[seqs[i]].push_back(i);
    if (groups.empty()) return REID_OK;
    std::vector<int32_t> rows, start(1, 0);
    for (auto& kv : groups) {
        rows.insert(rows.end(), kv.second.begin(), kv.second.end());
        start.push_back((int32_t)rows.size());
    }
    int32_t *d_rows, *d_start;
    REID_TRY(ctx_ws(ctx, "st.rows", rows.size() * 4, (void**)&d_rows));
    REID_TRY(ctx_ws(ctx, "st.start", start.size() * 4, (void**)&d_start));
    HIP_TRY(hipMemcpyAsync(d_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_start, start.data(), start.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(smooth_tracklets_kernel, dim3((unsigned)groups.size(), (d + 255) / 256), dim3(256), 0, ctx->stream, d_x, d_rows,
                       d_start, d, keep);
    LAUNCH_CHECK();
    HIP_TRY(hipStreamSynchronize(ctx->stream));   // rows / start are locals
    return REID_OK;
}

extern "C" int reid_smooth_tracklets(reid_ctx* ctx, float* x, const int32_t* seqs, const uint8_t* valid, int n, int d, float keep) {
    ARG_CHECK(ctx && x && seqs && n >= 0 && d >= 1);
    CTX_GUARD(ctx);
    if (n == 0) return REID_OK;
    float* dx;
    REID_TRY(ctx_ws(ctx, "cd.x", (size_t)n * d * 4, (void**)&dx));
    HIP_TRY(hipMemcpyAsync(dx, x, (size_t)n * d * 4, hipMemcpyHostToDevice, ctx->stream));
    REID_TRY(reid_smooth_tracklets_dev(ctx, dx, seqs, valid, n, d, keep));
    HIP_TRY(hipMemcpyAsync(x, dx, (size_t)n * d * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return REID_OK;
}
