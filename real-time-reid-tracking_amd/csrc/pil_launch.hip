// Host side of the *_images_u8 entry points: the coefficient tables of one call and the launcher of libreid_hip_pil_resize.so's two
// kernels (pil_resize.h).  No kernel lives here: the product library's kernel list stays what it was.
#include "pil_launch.h"
#include <map>
#include <cmath>

namespace {
// libreid_hip_pil_resize.so, opened beside this library on the first *_images_u8 call (or reid_debug_pil_resize): a process that never
// hands over uint8 images for the evaluation chain never opens it.  Missing library or symbol: REID_ERR_STATE naming the file.
struct PilLib : SideLib {
    PilLib() : SideLib("libreid_hip_pil_resize.so", "the *_images_u8 entry points need") {}
    SIDE_FN(max_side, pil_resize_max_side);
    SIDE_FN(max_out, pil_resize_max_out);
    SIDE_FN(coeffs, pil_resize_coeffs);
    SIDE_FN(norm_table, pil_resize_norm_table);
    SIDE_FN(launch, pil_resize_launch);
} pil;

const float kImagenet[6] = {0.485f, 0.456f, 0.406f, 0.229f, 0.224f, 0.225f};
}  // namespace

int pil_mean_std(const float** mean_std6) {
    if (!*mean_std6) *mean_std6 = kImagenet;
    const float* ms = *mean_std6;
    for (int c = 0; c < 3; ++c)
        if (!(ms[3 + c] > 0.f) || !std::isfinite(ms[3 + c]) || !std::isfinite(ms[c])) {
            reid_set_error("*_images_u8: mean must be finite and std positive (channel %d: mean %g, std %g)", c, ms[c], ms[3 + c]);
            return REID_ERR_ARG;
        }
    return REID_OK;
}

int PilPlan::build(const RaggedSrc& src, int oh, int ow, const float* mean_std6, int pass_) {
    REID_TRY(pil.open());
    const int lim = pil.max_side(), lim_out = pil.max_out();
    if (oh < 1 || ow < 1 || oh > lim_out || ow > lim_out) {
        reid_set_error("PIL resize: output size %d x %d, each side must be in [1, %d]", oh, ow, lim_out);
        return REID_ERR_ARG;
    }
    if (src.pitch || pass_ < 1 || !mean_std6) {
        reid_set_error("PIL resize: packed images, a pass size and mean / std are needed");
        return REID_ERR_ARG;
    }
    for (int i = 0; i < src.n; ++i)
        if (src.hw[2 * i] > lim || src.hw[2 * i + 1] > lim) {
            reid_set_error("PIL resize: image %d is %d x %d, a source side may be %d at most", i, src.hw[2 * i], src.hw[2 * i + 1], lim);
            return REID_ERR_ARG;
        }
    out_h = oh;
    out_w = ow;
    n = src.n;
    pass = pass_;
    pil.norm_table(mean_std6, table);
    tables.clear();
    images.resize(n);
    mid_bytes = 0;
    std::map<std::pair<int, int>, std::pair<int, int>> seen;   // (in, out) -> (start in `tables`, ksize)
    auto table_of = [&](int in, int out, int* start, int* ksize) -> int {
        auto it = seen.find({in, out});
        if (it == seen.end()) {
            int ks = 0;
            if (pil.coeffs(in, out, nullptr, nullptr, &ks) != 0) return REID_ERR_ARG;
            const size_t at = tables.size();
            tables.resize(at + (size_t)out * (2 + ks));
            if (pil.coeffs(in, out, tables.data() + at + 2 * (size_t)out, tables.data() + at, &ks) != 0) {
                reid_set_error("PIL resize: no coefficients for %d -> %d", in, out);
                return REID_ERR_ARG;
            }
            it = seen.emplace(std::make_pair(in, out), std::make_pair((int)at, ks)).first;
        }
        *start = it->second.first;
        *ksize = it->second.second;
        return REID_OK;
    };
    size_t at = 0;
    for (int i = 0; i < n; ++i) {
        if (i % pass == 0) at = 0;
        PilImage& im = images[i];
        REID_TRY(table_of(src.hw[2 * i + 1], ow, &im.h_tab, &im.h_ksize));
        REID_TRY(table_of(src.hw[2 * i], oh, &im.v_tab, &im.v_ksize));
        im.mid = (long long)at;
        at += (size_t)src.hw[2 * i] * ow * 3;
        if (at > mid_bytes) mid_bytes = at;
    }
    return REID_OK;
}

int PilPlan::alloc(reid_ctx* ctx, const char* tag) {
    const std::string t(tag);
    const int m = n < pass ? n : pass;
    REID_TRY(ctx_ws(ctx, (t + ".pil.tab").c_str(), tables.size() * 4, (void**)&d_tables));
    REID_TRY(ctx_ws(ctx, (t + ".pil.img").c_str(), images.size() * sizeof(PilImage), (void**)&d_images));
    REID_TRY(ctx_ws(ctx, (t + ".pil.lut").c_str(), sizeof(table), (void**)&d_table));
    REID_TRY(ctx_ws(ctx, (t + ".pil.mid").c_str(), mid_bytes, (void**)&d_mid));
    REID_TRY(ctx_ws(ctx, (t + ".pil.f32").c_str(), (size_t)m * 3 * out_h * out_w * 4, (void**)&d_f32));
    return REID_OK;
}

int PilPlan::up(hipStream_t s) const {
    HIP_TRY(hipMemcpyAsync(d_tables, tables.data(), tables.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_images, images.data(), images.size() * sizeof(PilImage), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_table, table, sizeof(table), hipMemcpyHostToDevice, s));
    return REID_OK;
}

int PilPlan::launch(reid_ctx* ctx, const RaggedSrc& src, int i, int m, uint8_t* d_u8, float* d_out) const {
    REID_TRY(pil.open());
    if (i < 0 || m < 1 || m > pass || i % pass || i + m > n || src.n != n || !src.d_src || !d_tables || !d_mid || !d_out) {
        reid_set_error("PIL resize: bad launch (images [%d, %d) of %d, passes of %d)", i, i + m, n, pass);
        return REID_ERR_ARG;
    }
    int max_h = 1;
    double bytes = 0;
    for (int j = i; j < i + m; ++j) {
        if (src.hw[2 * j] > max_h) max_h = src.hw[2 * j];
        bytes += 3.0 * src.hw[2 * j] * (src.hw[2 * j + 1] + 2.0 * out_w) + (double)out_h * out_w * (d_u8 ? 15 : 12);
    }
    prof_begin(ctx, REID_K_ELEMENTWISE, 0, bytes);
    const hipError_t e =
        pil.launch(ctx->stream, src.d_src, src.d_off + i, src.d_hw + 2 * i, m, max_h, out_h, out_w, d_tables, d_images + i, d_table, d_mid, d_u8, d_out);
    prof_end(ctx);
    HIP_TRY(e);
    return REID_OK;
}
