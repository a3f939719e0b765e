// libreid_hip_anysize_sib_f16.so (anysize_sib_f16.hip): the block tails of CARes18-IBN (TripletAttention, reid/backbones/
// triplet_attention.py:46-101, CARes18.py:145-157) and EMARes18-IBN (EMA, reid/backbones/EMA_Res18.py:23-38, 79-86) for any map size on
// f16 maps - what the any-size forward (api.hip, seres18_trunk_any) launches behind conv2 when such an architecture is loaded and
// reid_ctx_set_hw_sib_f16 is 1.  The stem, max-pool, convolutions, IBN finish and GeM neck of that forward are libreid_hip_anysize_f16.so's.
// libreid_hip.so does not link this file: api.hip opens it from its own directory with dlopen on the first such call, and a call without
// the file is REID_ERR_STATE naming it.  Everything here is a device pointer.
//
// y, shortcut, out: NHWC _Float16 [n][H][W][C].  The formulas are those of anysize_ca.h and anysize_ema.h, and so is the arithmetic, on
// inputs that happen to be f16 values (the contract anysize_f16.h states for its SE tail): sums over a line, a slab or the map are fp64 sums
// in an order fixed by (H, W, C) alone, every statistic is rounded ONCE to fp32; convolutions, sigmoids, softmaxes, GroupNorm and the combine
// run in fp32 in the orders anysize_ca.h / anysize_ema.h give - the 3 x 3 convolution in (quad of four ci, tap r s, ci within the quad)
// order, wt per quad of channels in k order and the quads of a group pairwise (cg 8: one add, cg 16: (a + b) + (c + d)), the combine of the
// TripletAttention tail with every product and sum rounded on its own - and the result is rounded to f16 exactly once, at the store (the
// conversion any_se_tail_f16_kernel stores with: round to nearest even, a value beyond f16's range becomes infinity).  No atomics; no
// partial result crosses a block but the EMA tail's fp64 slab partials, added in slab order.  An image's bits depend on neither n, its
// position in the batch nor the launch.
//
// A lane's 16 bytes are EIGHT channels.  EMA, cg = C / 32 consecutive channels per group: a lane holds four groups at cg 2, two at cg 4,
// one at cg 8, half a group at cg 16; the 3 x 3 neighbourhood comes from L1 in 16-byte pieces (a piece is read once per quad of input
// channels it feeds), no slab lies in LDS.  The launches are those of the fp32 tails: TripletAttention (1) any_sib_ca_stats_kernel, grid
// (H + W, n), a block per image row / column, (2) any_sib_ca_gate_kernel, a thread per gate element, (3) any_sib_ca_apply_kernel, grid
// (row slabs, n); EMA (1) any_sib_ema_lines_kernel, grid (H + W, n), (2) any_sib_ema_pass_kernel<cg, false>, grid (slabs, n), (3)
// any_sib_ema_finish_kernel, grid (n), (4) any_sib_ema_pass_kernel<cg, true>.
//
// The workspaces keep the fp32 / fp64 layouts - and the byte counts - of the fp32 tails:
//   TripletAttention (anysize_ca.h):  maps [n][2 per] | gates [n][per],  per = H W + C W + H C floats
//   EMA (anysize_ema.h):              part [n][S][3][C] double | sig [n][H + W][C] float | small [n][4][C] float,  S = anysize_ema_slabs(H, W, C)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "anysize_ema.h"   // anysize_ema_rows / anysize_ema_slabs: the EMA tail's row slabs are the fp32 tail's

extern "C" {
// bytes of ws for a call of the tail with these arguments (anysize_ca_workspace_bytes / anysize_ema_workspace_bytes of the same shape);
// 0 for a shape outside the range
size_t anysize_sib_f16_ca_workspace_bytes(int n, int H, int W, int C);
size_t anysize_sib_f16_ema_workspace_bytes(int n, int H, int W, int C);
// prm as anysize_ca_tail / anysize_ema_tail take it (fp32: Se18Block::ta, Se18Block::ema).  2 <= H, W <= 128, C in {64, 128, 256, 512},
// 1 <= n <= 65535; anything else is hipErrorInvalidValue with nothing launched.  out must not alias y or shortcut.
hipError_t anysize_sib_f16_ca_tail(hipStream_t stream, const _Float16* y, const _Float16* shortcut, int n, int H, int W, int C, const float* prm,
                                   void* ws, _Float16* out);
hipError_t anysize_sib_f16_ema_tail(hipStream_t stream, const _Float16* y, const _Float16* shortcut, int n, int H, int W, int C, const float* prm,
                                    void* ws, _Float16* out);
}
