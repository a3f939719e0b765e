// libreid_hip_swin_eval.so (swin_eval.hip): what the Swin descriptor entry points (reid_swin_descriptor_*) launch beyond the forward of
// reid_swin_embed_* - the two stems of the mirrored view and the descriptor itself.  libreid_hip.so does not link it: swin.hip opens it from
// its own directory with dlopen on the first descriptor call (as it opens libreid_hip_swin_crops.so on the first crops call), so a caller
// that only embeds needs what it needed before.  A descriptor call without this library is REID_ERR_STATE naming the file.  The callers
// are launch_sfe_conv1_mirror, launch_swin_crop_front_mirror and launch_swin_descriptor in swin.hip, which check the arguments.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// sfe_conv1_kernel (swin.hip) of the horizontally mirrored image, without a mirrored copy: x fp32 NCHW [n][3][h][w] ->
// c1_out [n][h / 2][w / 2][12], output pixel (oy, ox) from input columns w - 1 - (2 ox + kw).  The same products in the same order as
// sfe_conv1_kernel on a host-flipped x, so the same bits.  h, w even; all device pointers.
hipError_t swin_eval_conv1_mirror(hipStream_t stream, const float* x, int n, int h, int w, const float* c1_w, const float* c1_b,
                                  float* c1_out);
// swin_crops_front (swin_crops.h) with the RESIZED image's columns reversed - the mirror after the resize, the order of the reference's
// transforms (Resize -> flip -> ToTensor -> Normalize): the same arguments, the same bits as sfe_conv1_kernel on the crops resized,
// normalised and then flipped on the host.
hipError_t swin_eval_crop_front_mirror(hipStream_t stream, const uint8_t* src, const long long* offsets, const int* hw, int n, int H, int W,
                                       int pitch, const float* mean_std6, const float* c1_w, const float* c1_b, float* c1_out);
// The retrieval descriptor of the evaluation script for a Swin (reid/image_reid_inference.py:117-123,252-253 with
// swin_transformer.py:422-423, which returns (logits, x_norm)): one block per image,
//     d(e) = cat(normalize(cls_w e), normalize(e));   e2 == NULL: out = d(e1);   else out = normalize((d(e1) + d(e2)) / 2),
// normalize = F.normalize (v / max(||v||, 1e-12)).  e1, e2 [n][96] (x_norm of the plain and of the mirrored view), cls_w [num_class][96],
// out rows of num_class + 96 floats, `ld` floats apart (ld >= num_class + 96); device pointers, e1 / e2 / cls_w 16-byte aligned.  The
// classifier runs here in exact fp32, k = 0 .. 95 in order, one FMA each; the logits live in LDS only.  1 <= num_class <= the limit below.
hipError_t swin_eval_descriptor(hipStream_t stream, const float* e1, const float* e2, const float* cls_w, int n, int num_class, long long ld,
                                float* out);
int swin_eval_max_classes(void);   // 4096: both views' logits of one image are held in 32 KB of LDS
}
