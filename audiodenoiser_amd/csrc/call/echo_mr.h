// Multi-reference echo cancellation (echo_mr_kernels.hip; include/adn_call.h, "echo stream multireference"): the launchers behind
// the adn_aec_mr_* entry points of call_api.hip.  AecMrConsts: the parameters, Q = refs and K the taps PER CHANNEL (N = Q K <= 32
// stacked unknowns), and p0 = 1 / loading, derived once per call on the host in fp32.  astate: aec_mr_record_floats(Q, K, D) =
// 2 N^2 + 4 N + 2 Q D floats per (slot, bin) -- P, h and Q rings of the last D + K far-end frames -- [slot][bin] consecutive, group
// i = slot i; a group that starts at frame 0 reads none of it.  The launches differ in where the frames are: frame-major spectrograms
// mic / spec_out [row][frame][F] and far [row][ref][frame][F]; or the X rings of a lockstep stream state whose streams g (Q + 1) ...
// g (Q + 1) + Q are the microphone and the Q far ends of group g (e_t over the microphone's ring cells, M_t into columns [W - B, W)
// of its windows of y, nothing of a far-end stream written).  Q = 1 is NOT launched from here: the entry points forward to
// launch_aec_online / launch_aec_stream of adn_internal.h.  Not part of any public ABI.
#pragma once
#include "../adn_internal.h"

namespace adn {

struct AecMrConsts {
    int Q, K, D;
    float alpha, p0, quiet;
};
long aec_mr_record_floats(int Q, int K, int D);
long aec_mr_grid(long n_groups, int F, int N);
hipError_t launch_aec_mr_online(const void *mic, const void *far, int n_rows, int T, int F, int first_frame, const AecMrConsts &c,
                                float *astate, void *spec_out, float *mag_out, int width, int col0, hipStream_t st);
hipError_t launch_aec_mr_stream(float *state, float *y, int n_streams, const StreamGeom &g, const StreamCall &call, const AecMrConsts &c,
                                float *astate, hipStream_t st);

}  // namespace adn
