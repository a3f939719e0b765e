// libreid_hip_swin_v2.so (swin_v2.hip): the two kernels of the Swin "v2" blocks as launches on a stream.  libreid_hip.so does not link
// it: swin.hip opens it from its own directory with dlopen when a v2 checkpoint is loaded (as comm.hip opens librccl on first use), so a
// caller that never loads v2 weights needs libreid_hip.so alone, as before.  A v2 checkpoint without this library is an error of
// reid_swin_load.  The callers are launch_window_attn_cos / launch_post_norm in swin.hip, which check the arguments.
#pragma once
#include <hip/hip_runtime.h>

extern "C" {
// mode 0: fp32 qkv [tokens][ldq] -> fp32 out [tokens][C]; 2: fp32 qkv -> [oh | ol'] f16 out [tokens][2C]; 1: f16 qkv -> f16 out.
// bias_t: [heads][49 keys][64 queries] (queries 49 .. 63 zero), scale: [heads], both on the device.  fault: reid_ctx.fault or null.
hipError_t swin_v2_window_attn_cos(hipStream_t stream, int mode, const void* qkv, int ldq, int n_img, int H, int W, int heads, int shifted,
                                   const float* bias_t, const float* scale, void* out, int* fault);
// out = x + (LayerNorm(y) g + b), eps 1e-5, rows of C <= 768 channels (C % 4 == 0); out may be x.  side_mode 0: no side output; 1: f16
// copy of out [T][C]; 2: [oh | ol'] f16 [T][2C] (+ the range guard on fault).
hipError_t swin_v2_post_norm(hipStream_t stream, int side_mode, const float* x, const float* y, long long T, int C, const float* g,
                             const float* b, float* out, _Float16* side, int* fault);
}
