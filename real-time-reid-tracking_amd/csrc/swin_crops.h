// libreid_hip_swin_crops.so (swin_crops.hip): the front end of the Swin uint8 entry points (reid_swin_embed_ragged_u8 /
// reid_swin_embed_frame_u8) as one launch on a stream.  libreid_hip.so does not link it: swin.hip opens it from its own directory with
// dlopen on the first crops call (as it opens libreid_hip_swin_v2.so for v2 weights), so a caller that only hands over float images needs
// libreid_hip.so alone, as before.  A crops call without this library is REID_ERR_STATE naming the file.  The caller is
// launch_swin_crop_front in swin.hip, which checks the arguments.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// n uint8 HxWx3 windows -> the output of ShadowFeatureExtraction's first convolution, c1_out fp32 [n][H / 2][W / 2][12] (NHWC12, what
// sfe_conv1_kernel writes from a normalised NCHW image): window i = hw[2i] x hw[2i + 1] pixels at byte offsets[i] of src, rows `pitch`
// pixels apart (0: the window's own width), bilinear to H x W with resize_norm_kernel's taps, (v - mean[c]) / std[c], conv 2x2 stride 2.
// src / offsets / hw / c1_w [12][(kh, kw, c)] / c1_b [12] / c1_out are device pointers, c1_out 16-byte aligned; mean_std6 is a HOST
// pointer to mean[3] then std[3] (passed to the kernel by value).  H, W even; (W / 2) * 48 bytes per row keeps every pixel 16-byte aligned.
hipError_t swin_crops_front(hipStream_t stream, const uint8_t* src, const long long* offsets, const int* hw, int n, int H, int W, int pitch,
                            const float* mean_std6, const float* c1_w, const float* c1_b, float* c1_out);
}
