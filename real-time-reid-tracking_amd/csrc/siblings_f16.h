// libreid_hip_siblings_f16.so (siblings_f16.hip): the attention tails of CARes18_IBN and EMARes18_IBN for the fp16-storage mode, as
// launches on a stream.  libreid_hip.so does not link it: api.hip opens it from its own directory with dlopen the first time a
// sibling checkpoint runs in mode 1 (as swin.hip opens libreid_hip_swin_v2.so), so a caller that never does needs libreid_hip.so
// alone, as before.  A sibling in mode 1 without this library is an error of the embed call.
// Activations are _Float16 NHWC [n][H][W][C]; parameters stay fp32 (the layouts of attention_f32.hip).  out must not alias y or sc.
// A shape a launcher cannot run returns hipErrorInvalidValue before anything is launched.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

extern "C" {
// out = relu(1/3 (y s_hw[h,w] + y s_cw[c,w] + y s_hc[h,c]) + sc).  wts: [3 gates: cw, hc, hw][100] = conv weight [2][7][7], BN scale,
// BN shift.  C in {8, 16, ..., 512} with C / 8 a power of two, W * C <= 32768, H a multiple of the slice rows (siblings_f16.hip).
// workspace: siblings_f16_ta_workspace_bytes(n, H, W, C) bytes, 16-byte aligned.
size_t siblings_f16_ta_workspace_bytes(int n, int H, int W, int C);
hipError_t siblings_f16_ta_tail(hipStream_t stream, const _Float16* y, const _Float16* sc, int n, int H, int W, int C, const float* wts,
                                void* workspace, _Float16* out);
// out = relu(EMA(y) + sc), 32 channel groups of C / 32 in {2, 4, 8, 16} channels, W in {8, 16, 32, 64}.  prm = conv1x1 w [cg][cg], b [cg] |
// conv3x3 w [cg][cg][3][3], b [cg] | GroupNorm weight [cg], bias [cg].  Needs no workspace (the query returns 0).
size_t siblings_f16_ema_workspace_bytes(int n, int H, int W, int C);
hipError_t siblings_f16_ema_tail(hipStream_t stream, const _Float16* y, const _Float16* sc, int n, int H, int W, int C, const float* prm,
                                 _Float16* out);
}
