// libreid_hip_bank96.so (bank96.hip): the cost stage of the frame pipeline for 96-wide feature banks - the Swin-T embedding - as one
// launch on a stream.  libreid_hip.so does not link it: bank.hip opens it from its own directory with dlopen on the first
// reid_frame_submit_swin (as swin.hip opens libreid_hip_swin_crops.so on the first crops call), so a ResNet tracker needs libreid_hip.so
// alone, as before.  A Swin frame without this library is REID_ERR_STATE naming the file.  The caller is bank_cost_launch in bank.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// out[t][m] = min over the samples of track slots[i] of metric(sample, dets[j]), bank_cost512_kernel's arguments and result rules
// (bank.hip) for d = 96: feat [.][budget][96], sq [.][budget] squared norms, count [.] samples held (<= budget), slots [t], dets [m][96],
// all device pointers, feat and dets 16-byte aligned.  metric 0 cosine, 1 squared euclidean; gate < 0: raw costs.  t, m >= 1.
hipError_t bank96_cost(hipStream_t stream, const float* feat, const float* sq, const int32_t* count, int budget, const int32_t* slots, int t,
                       const float* dets, int m, int metric, float gate, float* out);
}
