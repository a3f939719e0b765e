// libreid_hip_eval_links.so (eval_links.hip): the two links of the evaluation script's chain beside the forward and the re-ranking - the
// shifted mirrored view of `strong_inference` (reid/data_transforms.py:130-191) and the Market-1501 attribute distance added to the
// Jaccard matrix (reid/image_reid_inference.py:276-289, reid/losses/utils.py:21-35).  libreid_hip.so does not link it: postproc.hip opens
// it from its own directory with dlopen on the first reid_descriptor_*_shift / reid_distmat_add_l2* call (or a harness of its launchers).
// Without the file those calls are REID_ERR_STATE naming it.  The callers check the arguments; every pointer is a device pointer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// shift_mirror_nchw_kernel: crop(pad(mirror(x))) of fp32 NCHW x [m][3][h][w] -> y of the same shape,
//     sy = oy + top - pad;  sx = ox + left - pad;   y[i][c][oy][ox] = (0 <= sy < h && 0 <= sx < w) ? x[i][c][sy][w - 1 - sx] : fill[c]
// with (top, left) = shift_tl[2 i], shift_tl[2 i + 1] (int32 on the device).  (top, left) == (pad, pad) is the plain mirror.  Pure data
// movement.  w % 4 == 0 and y 16-byte aligned: one 16-byte store per thread and four pixels; scalar stores otherwise.  At most
// eval_links_grid_cap() blocks of 256 threads, which stride over the rest.  x and y must not overlap.
hipError_t eval_links_shift_mirror(hipStream_t stream, const float* x, int m, int h, int w, const int32_t* shift_tl, int pad, const float* fill3,
                                   float* y);
int eval_links_grid_cap(void);   // 4096
// dist_add_l2_kernel: d_inout [n][n] += sqrt(max(s_i + s_j - 2 a_i.a_j, 1e-12)) in place, a fp32 [n][d], 1 <= d <= eval_links_max_d(),
// s_i the squared norm of row i.  Tiles of eval_links_tile() rows and columns, both row panels in LDS padded with zeros to 32 columns; the
// dot product and the norms are ascending-k fp32 FMA chains from 0 and s_i + s_j is one fp32 add, so an all-zero d_inout becomes
// symmetric bit for bit.  A NaN in `a` (or in d_inout) stays a NaN.  One 16-byte load and store per four elements of the matrix, whatever
// n: the tile's columns start at a 16-byte boundary of each ROW (d_inout itself 16-byte aligned); quads that straddle a row end are
// finished with scalar accesses.
hipError_t eval_links_dist_add_l2(hipStream_t stream, const float* a, int n, int d, float* d_inout);
int eval_links_tile(void);    // 64
int eval_links_max_d(void);   // 32
}
