// What the four WPE kernels share (dereverb_kernels.hip, dereverb_mc_kernels.hip, dereverb_stream_kernels.hip,
// dereverb_mc_stream_kernels.hip): the arithmetic rules of adn.h, each written once, and the launchers of the single-channel
// kernels, which only the joint launchers of adn_internal.h call (C = 1 runs the single-channel kernel: that choice is made there,
// once per launcher).  Measured: profiles/wpe_family.md.
#pragma once
#include "adn_internal.h"

namespace adn {

// max(x, c) of adn.h: a NaN x stays NaN
__device__ __forceinline__ float max_keep_nan(float x, float c) { return x < c ? c : x; }

// Complex multiply-adds, two fmaf per component.  The ORDER of the two products is part of the result, and the offline and the
// recursive definitions order the imaginary part differently, so there are two conjugate forms: do not fold one into the other.
//   cfma           acc + a b            re: a.x b.x, then -a.y b.y        im: a.x b.y, then a.y b.x
//   cfma_conj      acc + a conj(b)      re: a.x b.x, then  a.y b.y        im: -a.x b.y, then a.y b.x    ("dereverb stream")
//   cfma_conj_yx   acc + a conj(b)      re: a.x b.x, then  a.y b.y        im: a.y b.x, then -a.x b.y    ("dereverb")
//   cfms_conj      acc - conj(a) b      re: -a.x b.x, then -a.y b.y       im: -a.x b.y, then a.y b.x    ("dereverb": the filter)
__device__ __forceinline__ float2 cfma(float2 a, float2 b, float2 acc)
{
    return make_float2(fmaf(-a.y, b.y, fmaf(a.x, b.x, acc.x)), fmaf(a.y, b.x, fmaf(a.x, b.y, acc.y)));
}
__device__ __forceinline__ float2 cfma_conj(float2 a, float2 b, float2 acc)
{
    return make_float2(fmaf(a.y, b.y, fmaf(a.x, b.x, acc.x)), fmaf(a.y, b.x, fmaf(-a.x, b.y, acc.y)));
}
__device__ __forceinline__ float2 cfma_conj_yx(float2 a, float2 b, float2 acc)
{
    return make_float2(fmaf(a.y, b.y, fmaf(a.x, b.x, acc.x)), fmaf(-a.x, b.y, fmaf(a.y, b.x, acc.y)));
}
__device__ __forceinline__ float2 cfms_conj(float2 a, float2 b, float2 acc)
{
    return make_float2(fmaf(-a.y, b.y, fmaf(-a.x, b.x, acc.x)), fmaf(a.y, b.x, fmaf(-a.x, b.y, acc.y)));
}

// ---- the single-channel kernels behind the joint launchers (adn_internal.h) at C = 1 -----------------------------------------
long wpe_grid_1ch(int n_clips, int F, int K);
hipError_t launch_wpe_1ch(const void *spec, int n_clips, int T, int F, const WpeConsts &k, void *spec_out, float *mag_out, int width,
                          hipStream_t st);
hipError_t launch_wpe_online_1ch(const void *spec, int n_rows, int T, int F, int first_frame, const WpeStreamConsts &c, float *wstate,
                                 void *spec_out, float *mag_out, int width, int col0, hipStream_t st);
hipError_t launch_wpe_stream_1ch(float *state, float *y, int n_streams, const StreamGeom &g, const StreamCall &call,
                                 const WpeStreamConsts &c, float *wstate, hipStream_t st);

}  // namespace adn
