// libreid_hip_distmat_x3.so (distmat_x3.hip): the m x n distance matrix of reid_distmat_x3* in the fp32-class arithmetic -
// fp32 x [m][ld] and y [n][ld] in, fp32 out [m][n], both operands split to f16 parts by the loader on their way into LDS (no packed copy of
// either lives in HBM).  libreid_hip.so does not link it: api.hip opens it from its own directory with dlopen on the first reid_distmat_x3*
// call.  Without the file that call is REID_ERR_STATE naming it.  The caller checks the arguments; every pointer is a device pointer except
// fault, the context's sticky fault word in mapped host memory (may be NULL).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// out[i][j] = metric(dot, xx[i], yy[j]) with dot = 2^-11 sum_k (xh yq + xl' yh + xh yl')[i][j]: xh = f16_rn(x), xl' = f16_rn((x - xh) 2^11),
// yh = f16_rn(y), yq = f16(yh 2^11), yl' = f16_rn((y - yh) 2^11); per step of 32 columns the three products go into ONE fp32 accumulator
// in that order.  ld % 32 == 0, rows 16-byte aligned and zero-padded from the true width on (the caller's pad_rows_to(.., 32)).
// xx [m] / yy [n]: squared row norms (launch_row_sqnorm), NULL for REID_METRIC_DOT.  The metric formulas are gemm_f32_dma.hip's.
// No launch splits K and the k order of an element depends on ld alone: out[i][j] has the same bits whatever m, n or its position.
// Domain: |x| < 65504 and |y| 2^11 < 65504 (|y| < 31.98); a value outside it, or a non-finite one, raises fault[0].  For L2 and L2SQR
// the metric is symmetric, so the caller may put the larger-ranged set on the x side.
// form_out (may be NULL): the tile form launched, DISTMAT_X3_FORM_*; it depends on n only: 128 x 64 tiles for n <= 64, 128 x 128 above.
hipError_t distmat_x3(hipStream_t stream, const float* x, int m, const float* y, int n, int ld, const float* xx, const float* yy, int metric,
                      float* out, int* fault, int* form_out);
}
enum { DISTMAT_X3_FORM_128x64 = 1, DISTMAT_X3_FORM_128x128 = 2 };
