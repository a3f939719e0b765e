// libreid_hip_select_x3.so (select_x3.hip): the k smallest distances of every row of x to the rows of y - reid_argmin_rows_x3* (k = 1, any
// metric) and reid_knn_x3* (squared L2, k <= 24) - with the candidates from the fp32-class arithmetic of dist_x3_kernel (distmat_x3.h; the
// selection runs in that kernel's epilogue, no m x n matrix is written) and the ANSWER in exact fp32: the bits of reid_argmin_rows* /
// reid_knn*, indices and values.  libreid_hip.so does not link it: api.hip opens it from its own directory with dlopen on the first
// reid_*_x3 selection call.  Without the file that call is REID_ERR_STATE naming it.  The caller checks the arguments; every pointer is a
// device pointer except fault, the context's sticky fault word in mapped host memory (may be NULL).
// A tile list holds 32 keys: of more keys below the row's threshold it keeps the 32 smallest, and their last bounds the rest of the tile.
// The 32 smallest values of a row are therefore candidates whatever the order of y's rows, and so is the proof: a row whose k-th and
// (k + 8)-th values lie further apart than twice the error bound is never recomputed.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

extern "C" {
// Bytes of workspace select_x3 wants for an m x n problem: every row's lists, or - from SELECT_X3_WS_CAP on - as many rows' as fit the cap
// (select_x3 then walks the rows in chunks; never fewer than 128 rows).
size_t select_x3_ws_bytes(int m, int n);
// The row's error bound B as refine_kernel evaluates it (the same function, compiled for the host): tests only.
float select_x3_bound(int metric, int ld, float xx, float ymax, float ymin);
// D [m][k] / I [m][k]: the k smallest of metric(x[i], y[j]) over j by (value, j), ascending; a row with n < k is padded with (+inf, -1).
// D may be NULL.  x [m][ld], y [n][ld]: ld % 32 == 0, rows 16-byte aligned and zero-padded (pad_rows_to(.., 32)); xx [m] / yy [n]:
// squared row norms (launch_row_sqnorm) - needed under EVERY metric, REID_METRIC_DOT included: the error bound of the proof is a closed
// form of them.  1 <= k <= SELECT_X3_KMAX.
// flags [m] (device, required): 1 where the row was recomputed by the exact-row kernel (not proven, or forced), else 0.
// force_every > 0 (tests): every row whose index is a multiple of it takes the exact-row kernel whatever the proof says.
// form_out (may be NULL): SELECT_X3_FORM_*, a rule of n alone - the rule of distmat_x3.h.
// Launches are ordered by the stream alone; nothing here waits for another block.
hipError_t select_x3(hipStream_t stream, const float* x, int m, const float* y, int n, int ld, const float* xx, const float* yy, int metric,
                     int k, float* D, int32_t* I, void* ws, size_t ws_bytes, int* fault, int force_every, int* flags, int* form_out);
}
enum { SELECT_X3_FORM_128x64 = 1, SELECT_X3_FORM_128x128 = 2 };
enum { SELECT_X3_KMAX = 24, SELECT_X3_KK = 32, SELECT_X3_SAMPLE = 512 };
#define SELECT_X3_WS_CAP ((size_t)256 << 20)
