// libreid_hip_anysize_ema.so (anysize_ema.hip): the EMA block tail of EMARes18-IBN (reid/backbones/EMA_Res18.py:23-38, 79-86) for any map
// size - what the any-size forward (api.hip, seres18_trunk_any) launches behind conv2 when the loaded architecture is emares18_ibn and
// reid_ctx_set_hw_ema is 1.  libreid_hip.so does not link it: api.hip opens it from its own directory with dlopen on the first such call,
// and a call without the file is REID_ERR_STATE naming it.  Everything here is a device pointer.
//
//   out = relu(y * sigmoid(wt[h, w]) + shortcut)                      y, shortcut, out: NHWC fp32 [n][H][W][C]
// per group g of cg = C / 32 CONSECUTIVE channels (c = g cg + k; the parameters are shared by the groups):
//   sig_h[h][c] = sigmoid(b1[k] + sum_ci w1[k][ci] mean_w(y)[h][g cg + ci]),  sig_w[w][c] likewise on mean_h(y)
//   x1pre = (y * sig_h) * sig_w,   x1 = (x1pre - mu[c]) * rstd[c] * gw[k] + gb[k]       (GroupNorm of one channel per group over the map:
//                                                                                        biased variance, eps 1e-5)
//   x2    = b3[k] + sum_{ci, r, s} w3[k][ci][r][s] y[h + r - 1][w + s - 1][g cg + ci]    (zero padding)
//   s1    = softmax_k(agp(x1)) = softmax_k(gb),   s2 = softmax_k(mean over the map of x2)
//   wt    = sum_k s1[k] x2[k] + s2[k] x1[k]
// agp(x1): the mean of a GroupNorm output over the extent it was normalised on IS the GroupNorm bias in exact arithmetic, so s1 is
// softmax(gb) and no pass measures it (the float64 oracle of tests/anysize_ema_ref.py computes it the long way; the difference is its
// rounding).
//
// Arithmetic.  Sums over a line or over the map are fp64 sums of fp32 values (a product of two floats is exact there) in an order fixed by
// (H, W, C) alone, rounded ONCE: mean = s / n; mu = S1 / hw, var = max((S2 - S1 mu) / hw, 0), rstd = 1 / sqrt(var + 1e-5), agp(x2) =
// S3 / hw, each rounded to fp32.  The 1x1 convolution is cg fused multiply-adds on the bias in ci order; the 3 x 3 convolution is fused
// multiply-adds on the bias in (quad of four ci, tap r s, ci within the quad) order - for cg <= 4 that is (tap, ci) - and a tap outside
// the map adds nothing; the sigmoids are 1 / (1 + expf(-a)); the softmaxes subtract the maximum, sum expf in k order and divide; x1pre
// rounds both products, x1 = fmaf((x1pre - mu) * rstd, gw, gb); wt accumulates fmaf(s1, x2, .) then fmaf(s2, x1, .) per channel in k
// order within a lane's four channels and adds the lanes of a group pairwise (cg 8: one add, cg 16: (a + b) + (c + d)); the product
// y * gate and the sum with the shortcut round on their own.  The statistics pass and the apply pass form x1pre and x2 with the same code,
// so they see the same bits.  No atomics: where an image's sums are split over row slabs, the slabs' fp64 partials are added in slab order.
// An image's bits depend on neither n, its position in the batch nor the launch.
//
// Launches: (1) any_ema_lines_kernel, grid (H + W, n): a block owns one row or one column, reduces it per channel and applies the 1x1
// convolution and sigmoid to its H + W vector entry.  (2) any_ema_pass_kernel<cg, false>, grid (slabs, n): S1, S2, S3 of a row slab per
// channel.  (3) any_ema_finish_kernel, grid (n): mu, rstd, s1, s2.  (4) any_ema_pass_kernel<cg, true>, grid (slabs, n): the apply pass,
// the same walk and the same code for x1pre and x2.  No kernel keeps a slab of the map in
// LDS; a lane owns four consecutive channels, reads and writes 16 bytes along C, and takes the 3 x 3 neighbourhood from L1 in the same
// 16-byte pieces.  x2 is formed again in (4) rather than stored: a stored x2 would add a write and a read of the whole map.
//
// Workspace of a call (anysize_ema_slabs(H, W, C) = S row slabs per image):
//   part  [n][S][3][C] double   S1 | S2 | S3 of a slab                   at ws
//   sig   [n][H + W][C] float   sig_h rows [0, H), sig_w rows [H, H + W)  at (float*)((double*)ws + n S 3 C)
//   small [n][4][C] float       mu | rstd | s1 | s2                       behind sig
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// row slabs per image: about 1024 16-byte pieces per block - one trip of four pieces per thread, so that a pass of a few images spreads
// over the device and no thread walks a chain of dependent trips - in whole rows, a function of (H, W, C) alone
static inline int anysize_ema_rows(int H, int W, int C) {
    int slabs = (H * W * (C / 4) + 1023) / 1024;
    if (slabs > H) slabs = H;
    return (H + slabs - 1) / slabs;
}
static inline int anysize_ema_slabs(int H, int W, int C) {
    const int rows = anysize_ema_rows(H, W, C);
    return (H + rows - 1) / rows;
}

extern "C" {
// bytes of ws for a call of anysize_ema_tail with these arguments; 0 for a shape outside the range
size_t anysize_ema_workspace_bytes(int n, int H, int W, int C);
// prm (cg = C / 32): conv1x1 w [cg][cg], b [cg] | conv3x3 w [cg][cg][3][3], b [cg] | GroupNorm weight [cg], bias [cg] (Se18Block::ema).
// 2 <= H, W <= 128, C in {64, 128, 256, 512}, 1 <= n <= 65535; anything else is hipErrorInvalidValue with nothing launched.  out must not
// alias y or shortcut.
hipError_t anysize_ema_tail(hipStream_t stream, const float* y, const float* shortcut, int n, int H, int W, int C, const float* prm, void* ws,
                            float* out);
}
