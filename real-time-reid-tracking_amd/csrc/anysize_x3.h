// libreid_hip_anysize_x3.so (anysize_x3.hip): the trunk convolutions of ResNet18-IBN-SE for any map size in the fp32-class arithmetic
//  - fp32 NHWC in, fp32 NHWC out, the activations split to [xh | xl'] f16 by the loader on their way into LDS, the
// weights in the [wh 2^11 | wh | wl'] form the 256 x 128 forward caches (launch_split_weights).  libreid_hip.so does not link it: api.hip
// opens it from its own directory with dlopen on the first convolution of the any-size forward at reid_ctx_set_hw_precision(ctx, 2).
// Without the file that call is REID_ERR_STATE naming it.  The caller checks the arguments; every pointer is a device pointer except fault,
// the context's sticky fault word in mapped host memory (may be NULL).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// out[m][co] = relu?( (sum_k x.w)[m][co] * scale[co] + shift[co] (+ residual[m][co]) ), m = (image, oy, ox) of n Ho Wo output pixels,
// k = (tap, channel) with padding taps read as zero.  r = 3 (pad 1) or 1 (pad 0), stride 1 or 2, cin % 32 == 0, cout % 64 == 0.
// w16 [cout][r r][terms cin] f16 with [wh 2^11 | wh | wl'] in the first 3 cin columns of a tap.  ReLU (relu != 0) from column relu_from on.
// No launch splits K: an output element is summed in one fixed order whatever tile it falls into.
// form_out (may be NULL): the tile form launched, ANYSIZE_X3_FORM_*; it depends on the geometry only, never on n.
hipError_t anysize_x3_conv(hipStream_t stream, const float* x, int n, int h, int w, int cin, const _Float16* w16, int terms, int cout, int r,
                           int stride, int pad, const float* scale, const float* shift, const float* residual, int relu, int relu_from,
                           float* out, int* fault, int* form_out);
}
enum { ANYSIZE_X3_FORM_128x64 = 1, ANYSIZE_X3_FORM_128x128 = 2 };
