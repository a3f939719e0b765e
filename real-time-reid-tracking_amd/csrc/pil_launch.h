// The host side of the *_images_u8 entry points (pil_launch.hip, part of libreid_hip.so): one call's coefficient tables and the launcher
// of the two kernels of libreid_hip_pil_resize.so (pil_resize.h).  Used by reid_descriptor_images_u8 (postproc.hip),
// reid_swin_descriptor_images_u8 (swin.hip) and the harness reid_debug_pil_resize (debug.hip).
#pragma once
#include "reid_internal.h"
#include "pil_resize.h"
#include <vector>

// mean_std6 == NULL -> ImageNet (the evaluation script's Normalize); mean finite and std positive, REID_ERR_ARG otherwise
int pil_mean_std(const float** mean_std6);

// Everything a call's resize needs beside the pixels.  build() is pure host work and refuses, with nothing queued: a missing side library
// (REID_ERR_STATE naming the file), an output side outside [1, pil_resize_max_out()] or a source side above pil_resize_max_side()
// (REID_ERR_ARG naming the limit).  The tables are computed once per distinct (in, out) pair and shared between images of equal size; the
// intermediate of a pass of `pass` images is laid out from byte 0 again, so <tag>.pil.mid holds the largest pass, not the call.
struct PilPlan {
    int out_h = 0, out_w = 0, n = 0, pass = 0;
    std::vector<int32_t> tables;
    std::vector<PilImage> images;
    float table[768];
    size_t mid_bytes = 0;
    int32_t* d_tables = nullptr;
    PilImage* d_images = nullptr;
    float* d_table = nullptr;
    uint8_t* d_mid = nullptr;
    float* d_f32 = nullptr;   // [min(pass, n)][3][out_h][out_w], the pass's normalised images
    int build(const RaggedSrc& src, int out_h, int out_w, const float* mean_std6, int pass);
    int alloc(reid_ctx* ctx, const char* tag);
    int up(hipStream_t s) const;   // queues the upload of tables, image records and the normalisation table
    // images [i, i + m) of the uploaded `src` (i a multiple of pass, m <= pass) -> d_f32 (and d_u8 [m][out_h][out_w][3] when not null)
    int launch(reid_ctx* ctx, const RaggedSrc& src, int i, int m, uint8_t* d_u8, float* d_out) const;
};
