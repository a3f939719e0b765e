// libreid_hip_anysize_ca.so (anysize_ca.hip): the TripletAttention block tail of CARes18-IBN (reid/backbones/triplet_attention.py:46-101,
// CARes18.py:145-157) for any map size - what the any-size forward (api.hip, seres18_trunk_any) launches behind conv2 when the loaded
// architecture is cares18_ibn and reid_ctx_set_hw_siblings is 1.  libreid_hip.so does not link it: api.hip opens it from its own directory
// with dlopen on the first such call, and a call without the file is REID_ERR_STATE naming it.  Everything here is a device pointer.
//
//   out = relu(1/3 * ((y * s_hw[h, w] + y * s_cw[c, w]) + y * s_hc[h, c]) + shortcut)       y, shortcut, out: NHWC fp32 [n][H][W][C]
//   s_g = sigmoid(scale_g * conv7x7_pad3(ZPool_g(y)) + shift_g),  ZPool channel 0 = unbiased std (torch.std), channel 1 = mean, over
//   C for the (H, W) plane of gate hw, over H for the (C, W) plane of gate cw, over W for the (H, C) plane of gate hc.
//
// Arithmetic: sum and sum of squares of a line in fp64 in an order fixed by (H, W, C) alone (a product of two floats is exact there),
// mean = s1 / n, var = max((s2 - s1 * mean) / (n - 1), 0), std = sqrt(var), both rounded ONCE to fp32; the convolution is 98 fused
// multiply-adds in fp32 in (channel, row, column) order over the taps inside the plane, then fmaf(acc, scale, shift) and
// 1 / (1 + expf(-a)); the combine rounds every product and sum of the formula above on its own (no contraction).  No atomics and no
// partial result crosses a block: an image's bits depend on neither n, its position in the batch nor the launch.
//
// Workspace of a call, per = H W + C W + H C floats per image:
//   maps  [n][2 per]   hw [2][H][W] | cw [2][C][W] | hc [2][H][C]        (channel 0 std, channel 1 mean)
//   gates [n][per]     hw [H][W]    | cw [W][C]    | hc [H][C]           (cw transposed: the apply kernel reads 16 bytes along C)
// maps start at ws, gates at (float*)ws + n * 2 * per.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

extern "C" {
// bytes of ws for a call of anysize_ca_tail with these arguments; 0 for a shape outside the range
size_t anysize_ca_workspace_bytes(int n, int H, int W, int C);
// prm: [3 gates: cw, hc, hw][100] = conv weight [2][7][7], folded BN scale, shift (Se18Block::ta).  2 <= H, W <= 128, C in {64, 128, 256,
// 512}, 1 <= n <= 65535; anything else is hipErrorInvalidValue with nothing launched.  out must not alias y or shortcut.
hipError_t anysize_ca_tail(hipStream_t stream, const float* y, const float* shortcut, int n, int H, int W, int C, const float* prm, void* ws,
                           float* out);
}
