// Cost stage of the frame pipeline for 96-wide feature banks (the Swin-T embedding; bank.hip has the metric, the bank and the d = 512
// kernel this one is modelled on).  What it replaces: NearestNeighborDistanceMetric.distance ([external] deep_sort/sort/nn_matching.py)
// for the reference's swin_transformer tracker model (modification_tracking/models/__init__.py:80).
//
// bank_cost_kernel (bank.hip, any d) gives a 96-element row to a whole wave: one and a half loads' worth of lanes carry data, a sample
// costs 32 LDS reads and 96 shuffles.  Here a wave is four groups of 16 lanes and each group streams a DIFFERENT sample of the track, so
// a wave handles four samples per step with all 64 lanes loading:
//   * lane l of a group keeps six elements of each of the block's 16 detections in 96 registers: elements 4l .. 4l + 3 and 64 + 2l,
//     64 + 2l + 1.  A sample row is then one 16-byte and one 8-byte load per lane, both naturally aligned (rows are 384 bytes) and both
//     contiguous over the group (the split 6l .. 6l + 5 would put every other lane's 16-byte load on an 8-byte boundary);
//   * per step a lane does 96 FMAs and a four-level butterfly - the first four levels of butterfly16 - leaves dot(sample g, detection
//     j(l)) one per lane: 15 shuffles per FOUR samples;
//   * the minimum over samples stays in a register and is reduced over the four groups (xor 16, xor 32) at the end, then over the
//     block's waves through LDS;
//   * the next step's rows are in flight during the arithmetic.  No scratch.
// Result rules are bank_cost512_kernel's: fminf drops NaN costs, the euclidean clamp lets NaN through, a track without samples gives inf
// (raw) or gate + 1e-5, a gated entry above the gate becomes gate + 1e-5.  The summation order differs from bank_cost_kernel's (6
// products per lane + 4 levels against 2 products + 6 levels), so the two agree to rounding, not bit for bit.
//
// Built as a library of its own, libreid_hip_bank96.so (bank96.h): libreid_hip.so, its dependencies and its kernel list
// (tests/golden/kernels.json) stay what they were; this library's kernel is held to tests/golden/kernels_bank96.json.
#include "bank96.h"
#include <math.h>

namespace {

constexpr int DT = 16;     // detections per block
constexpr int NW96 = 8;    // waves per block: 4 NW96 = 32 samples of the track per step
constexpr int D = 96;

__device__ __forceinline__ float clamp0(float c) { return c < 0.f ? 0.f : c; }

// after step s the lane holds 16 >> s sums over 2^s lanes of its group; detection index j(lane) = 8 b0 + 4 b1 + 2 b2 + b3
__device__ __forceinline__ float butterfly_group(float (&v)[16], int lane) {
    float r8[8], r4[4], r2[2];
    const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4, b3 = lane & 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) r8[i] = (b0 ? v[i + 8] : v[i]) + __shfl_xor(b0 ? v[i] : v[i + 8], 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) r4[i] = (b1 ? r8[i + 4] : r8[i]) + __shfl_xor(b1 ? r8[i] : r8[i + 4], 2);
#pragma unroll
    for (int i = 0; i < 2; ++i) r2[i] = (b2 ? r4[i + 2] : r4[i]) + __shfl_xor(b2 ? r4[i] : r4[i + 2], 4);
    return (b3 ? r2[1] : r2[0]) + __shfl_xor(b3 ? r2[0] : r2[1], 8);
}

// Reads: dets rows j0 .. j0 + nj - 1 < m; bank rows s < cnt = count[slot] <= budget of track slot = slots[t] (the host checks the slots
// against the bank).  Writes: out[t][j0 .. j0 + nj - 1].
__global__ __launch_bounds__(NW96 * 64) void bank_cost96_kernel(const float* __restrict__ feat, const float* __restrict__ sq,
                                                                const int32_t* __restrict__ count, int budget,
                                                                const int32_t* __restrict__ slots, const float* __restrict__ dets, int m,
                                                                int metric, float gate, float* __restrict__ out) {
    __shared__ float best_sh[NW96][DT];
    const int t = blockIdx.x, j0 = blockIdx.y * DT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l = lane & 15, g = lane >> 4;   // lane of the group, group of the wave
    const int nj = m - j0 < DT ? m - j0 : DT;
    const int jl = ((l & 1) << 3) | ((l & 2) << 1) | ((l & 4) >> 1) | ((l & 8) >> 3);   // this lane's detection
    float dv[DT][6];
    float tmp[16];
#pragma unroll
    for (int j = 0; j < DT; ++j) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        float2 c = make_float2(0.f, 0.f);
        if (j < nj) {
            a = *(const float4*)(dets + (long long)(j0 + j) * D + l * 4);
            c = *(const float2*)(dets + (long long)(j0 + j) * D + 64 + l * 2);
        }
        dv[j][0] = a.x; dv[j][1] = a.y; dv[j][2] = a.z; dv[j][3] = a.w;
        dv[j][4] = c.x; dv[j][5] = c.y;
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 6; ++e) s += dv[j][e] * dv[j][e];
        tmp[j] = s;
    }
    const float dsq = butterfly_group(tmp, lane);   // |det jl|^2
    const int slot = slots[t];
    const int cnt = count[slot];
    const float* base = feat + (long long)slot * budget * D;
    float best = INFINITY;
    float4 ra = make_float4(0.f, 0.f, 0.f, 0.f);
    float2 rb = make_float2(0.f, 0.f);
    if (wave * 4 + g < cnt) {
        ra = *(const float4*)(base + (long long)(wave * 4 + g) * D + l * 4);
        rb = *(const float2*)(base + (long long)(wave * 4 + g) * D + 64 + l * 2);
    }
    for (int s0 = wave * 4; s0 < cnt; s0 += NW96 * 4) {   // the trip count is the wave's: every lane takes part in the shuffles
        const int s = s0 + g;
        const bool live = s < cnt;                        // a group past the track's last sample computes on stale rows, unused
        const float rv[6] = {ra.x, ra.y, ra.z, ra.w, rb.x, rb.y};
        const float ssq = live ? sq[(long long)slot * budget + s] : 1.f;
        if (s + NW96 * 4 < cnt) {                         // next step's row is in flight during this one's arithmetic
            ra = *(const float4*)(base + (long long)(s + NW96 * 4) * D + l * 4);
            rb = *(const float2*)(base + (long long)(s + NW96 * 4) * D + 64 + l * 2);
        }
#pragma unroll
        for (int j = 0; j < DT; ++j) {
            float a = 0.f;
#pragma unroll
            for (int e = 0; e < 6; ++e) a += rv[e] * dv[j][e];
            tmp[j] = a;
        }
        const float dot = butterfly_group(tmp, lane);
        float c;
        if (metric == 0) c = 1.f - dot / (sqrtf(ssq) * sqrtf(dsq));
        else c = clamp0(ssq + dsq - 2.f * dot);
        if (live) best = fminf(best, c);
    }
    best = fminf(best, __shfl_xor(best, 16));
    best = fminf(best, __shfl_xor(best, 32));
    if (lane < 16) best_sh[wave][jl] = best;
    __syncthreads();
    if (tid < nj) {
        float c = best_sh[0][tid];
#pragma unroll
        for (int w = 1; w < NW96; ++w) c = fminf(c, best_sh[w][tid]);
        if (cnt == 0) c = gate >= 0.f ? gate + 1e-5f : INFINITY;   // a track without samples matches nothing
        else if (gate >= 0.f && c > gate) c = gate + 1e-5f;
        out[(long long)t * m + j0 + tid] = c;
    }
}

}  // namespace

extern "C" hipError_t bank96_cost(hipStream_t stream, const float* feat, const float* sq, const int32_t* count, int budget,
                                  const int32_t* slots, int t, const float* dets, int m, int metric, float gate, float* out) {
    if (!feat || !sq || !count || !slots || !dets || !out || budget < 1 || t < 1 || m < 1 || (metric != 0 && metric != 1) ||
        ((uintptr_t)feat & 15) || ((uintptr_t)dets & 15))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(bank_cost96_kernel, dim3(t, (m + DT - 1) / DT), dim3(NW96 * 64), 0, stream, feat, sq, count, budget, slots, dets, m,
                       metric, gate, out);
    return hipGetLastError();
}
