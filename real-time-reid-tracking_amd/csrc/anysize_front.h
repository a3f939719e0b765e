// libreid_hip_anysize_front.so (anysize_front.hip): the front end of the any-size ResNet18-IBN-SE forward from uint8 crops in ONE kernel -
// cv2-style bilinear resize + Normalize, conv 7x7 s2 p3 (3 -> 64) + folded BatchNorm, MaxPool2d(3, 2, 1) - bit for bit what
// anysize_resize_norm, the generic GEMM's stem (gemm_f32.hip, A_STEM_F32) and maxpool3s2_kernel give in three launches.  libreid_hip.so
// does not link it: api.hip opens it from its own directory with dlopen on the first reid_frame_submit_hw / reid_embed_frame_u8_hw at a
// size other than 256 x 128.  Without the file that call is REID_ERR_STATE naming it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// How any_front_kernel cuts an H x W input (each side 32 .. 512): a function of H and W only, so an image's result never depends on
// the batch.  H1 x W1 is the stem map ((H - 1) / 2 + 1), H2 x W2 the pooled map ((H1 - 1) / 2 + 1).
//   band b      : pooled rows [2 b, 2 b + 2) (the last band of an odd H2 has one).  It needs stem rows 4 b - 1 .. 4 b + 3 (those inside the
//                 map) and stages the 15 input rows 8 b - 5 .. 8 b + 9 (those outside the image as zeros: the convolution's padding).
//   column tile : pooled columns [q0, q0 + nq): 16 in tile 0, 15 in every later one, so that the stem columns it needs,
//                 x0 = max(0, 2 q0 - 1) .. min(W1, 2 (q0 + nq)) - 1, are at most 32 - one row of an MFMA tile.  It stages input pixels
//                 2 x0 - 3 .. 2 x0 - 3 + 2 ncol + 4.
//   block       : one image, one column tile, bands_per_block consecutive bands (a strip); the weights stay in LDS for all of them.
enum {
    ANYSIZE_FRONT_BAND_ROWS = 2,     // pooled rows of a band
    ANYSIZE_FRONT_STEM_ROWS = 5,     // stem rows of a band (2 * BAND_ROWS + 1)
    ANYSIZE_FRONT_IN_ROWS = 15,      // input rows staged for a band (4 * BAND_ROWS + 7)
    ANYSIZE_FRONT_MAX_NCOL = 32,     // stem columns of a column tile, at most
    ANYSIZE_FRONT_IN_PITCH = 210,    // floats of a staged input row: 70 pixels (2 * 32 + 5 = 69 and one of slack for the padded taps)
    ANYSIZE_FRONT_WP = 172,          // floats of a weight row in LDS (7 x 24 + 4)
    ANYSIZE_FRONT_LDS_BYTES = (64 * ANYSIZE_FRONT_WP + ANYSIZE_FRONT_IN_ROWS * ANYSIZE_FRONT_IN_PITCH + 3 * ANYSIZE_FRONT_MAX_NCOL * 64) * 4
};

struct anysize_front_geom {
    int32_t H1, W1, H2, W2;
    int32_t nbands, bands_per_block, nstrips, ncoltiles;
    int32_t lds_bytes;       // what the kernel declares
    int32_t in_rows, in_pitch, max_ncol;
};
struct anysize_front_band {
    int32_t p0, np;          // pooled rows [p0, p0 + np)
    int32_t y_lo;            // stem row of local row 0 (may be -1); local row j is stem row y_lo + j, j < 5
    int32_t iy_lo;           // input row of staged row 0 (may be negative); staged row i is input row iy_lo + i, i < 15
};
struct anysize_front_coltile {
    int32_t q0, nq;          // pooled columns [q0, q0 + nq)
    int32_t x0, ncol;        // stem columns [x0, x0 + ncol), all inside the map
    int32_t ix_lo, npx;      // staged pixel 0 is input pixel ix_lo (may be negative); npx pixels are staged
};

extern "C" {
// the cut of an H x W input; hipErrorInvalidValue for a side outside 32 .. 512 (host code only: no device call)
hipError_t anysize_front_plan(int H, int W, anysize_front_geom* geom);
hipError_t anysize_front_plan_band(int H, int W, int band, anysize_front_band* out);
hipError_t anysize_front_plan_coltile(int H, int W, int tile, anysize_front_coltile* out);
// packed / offsets / hw / pitch as anysize_resize_norm takes them (device pointers; pitch 0 = packed crops, else the frame's width in pixels),
// mean_std6_host on the host; stem_w [64][192] (k = r * 24 + s * 3 + c, zero padded), scale / shift [64] on the device.
// out [n][H2][W2][64] fp32 NHWC.
hipError_t anysize_front(hipStream_t stream, const uint8_t* packed, const long long* offsets, const int* hw, int n, int H, int W, int pitch,
                         const float* mean_std6_host, const float* stem_w, const float* scale, const float* shift, float* out);
}
