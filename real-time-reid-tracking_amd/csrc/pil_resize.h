// libreid_hip_pil_resize.so (pil_resize.hip): the first link of the evaluation script's chain on the device - transforms.Resize((H, W)) on
// an RGB PIL image, i.e. Pillow's 8-bit Image.resize((W, H), BILINEAR) (Resample.c), then ToTensor and Normalize
// (reid/data_transforms.py:56-127) - for the *_images_u8 entry points.  libreid_hip.so does not link it: pil_launch.hip opens it from its own
// directory with dlopen on the first *_images_u8 call (or reid_debug_pil_resize), so every other caller needs what it needed before.  Such a
// call without this library is REID_ERR_STATE naming the file.  It needs nothing from the product library and loads without a GPU: the
// coefficient and table functions are plain host code (tests/test_pil_resize_host.py calls them through ctypes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// The largest source side and the largest output side pil_resize_launch takes (4096 and 1024).
int pil_resize_max_side(void);
int pil_resize_max_out(void);
// Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter, one axis, in_size -> out_size, in IEEE double without
// contraction: *ksize = 2 * ceil(max(in / out, 1)) + 1; bounds [out_size][2] = (xmin, xmax); k [out_size][*ksize] 22-bit fixed point, zero
// beyond xmax.  k and bounds may both be NULL (only *ksize is wanted).  Returns 0, or -1 for a size below 1.
int pil_resize_coeffs(int in_size, int out_size, int32_t* k, int32_t* bounds, int* ksize);
// table [3][256] = (v / 255 - mean[c]) / std[c] in float32 with two true divisions, the bits of torch's
// to(float32).div(255).sub_(mean).div_(std); mean_std6 = mean[3] | std[3]
void pil_resize_norm_table(const float* mean_std6, float* table);

// One image of a launch.  h_tab / v_tab: where the image's horizontal (w -> out_w) and vertical (h -> out_h) tables start in `tables`,
// in int32 units; a table is bounds [out][2] followed by k [out][ksize].  mid: byte offset of the image's [h][out_w][3] intermediate.
struct PilImage {
    int h_tab, h_ksize, v_tab, v_ksize;
    long long mid;
};
// n ragged uint8 RGB HWC images (image i: hw[2i] x hw[2i + 1] pixels at byte offsets[i] of src, rows one after the other) -> two launches:
// pil_resize_h_kernel writes the horizontally resized uint8 image [h][out_w][3] of every image into mid, pil_resize_v_kernel resizes that
// vertically and writes u8_out [n][out_h][out_w][3] (when not NULL) and f32_out [n][3][out_h][out_w] = table[c][value].  max_h: the tallest
// image of the launch (grid size only).  Every pointer is a device pointer; images[i] and the tables must describe hw[2i], hw[2i + 1].
hipError_t pil_resize_launch(hipStream_t stream, const uint8_t* src, const long long* offsets, const int* hw, int n, int max_h, int out_h,
                             int out_w, const int32_t* tables, const PilImage* images, const float* table, uint8_t* mid, uint8_t* u8_out,
                             float* f32_out);
}
