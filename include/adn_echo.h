/* adn_echo.h -- acoustic echo cancellation on the MI355X (gfx950): the C ABI of libadn_echo.so.  See adn.h for the conventions. */
#ifndef ADN_ECHO_H
#define ADN_ECHO_H
#include "adn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- echo stream: acoustic echo cancellation, a per-bin RLS filter from the far-end reference to the microphone ---------------------
 * A header and a library of their own.  libadn.so exports exactly the functions adn.h declares, and that table is closed; the
 * four functions below are the ONLY symbols libadn_echo.so exports (same build: -fvisibility=hidden and the version script
 * csrc/libadn_echo.map).  libadn_echo.so is linked from the objects of libadn.so plus the operator's own two files
 * (csrc/echo_stream_kernels.hip, csrc/echo/echo_api.hip), which libadn.so does not hold; so it needs nothing of libadn.so at run time, and the stream state it works on is the adn_stream_* state of adn.h, byte for byte: a caller
 * loads both libraries and hands the state of one to the other.  The conventions are adn.h's (status codes, device pointers, the
 * caller's stream, no allocation, no blocking); the one difference is the message of a failed call, which each library keeps for
 * itself: after an adn_aec_* call it is read with adn_aec_last_error, not adn_last_error.
 *
 * No reference counterpart and no checkpoint.  The library DEFINES the operator below (float64 restatement: tests/echo_ref.py); it
 * is UNPINNED against any package.  It removes from a microphone what a known second signal -- the far end, what the loudspeaker
 * played -- left in it: plain exponentially forgetting RLS per (pair, bin), with the Hermitian update of "dereverb stream" as part
 * of the definition.  It is causal.  There is NO variance weighting, on purpose: on the host prototype (profiles/bench_echo.md) the
 * lam_t of "dereverb stream" and three smoothed variants cancelled 2 ... 5 dB in single talk against 16 dB for lam = 1.
 * Not validated: the defaults are the values of that host prototype; they were not tuned by ear.
 *
 * A pair is one microphone and its far end; every (pair, bin) is independent.  Y_t is the microphone and R_t the far end, complex
 * STFT values, both zero for t < 0.  In fp32, with the rounding rules of "dereverb stream" (a complex multiply-add is two fmaf per
 * component, the real-part product first; sums start at +0; divisions and the square root correctly rounded, componentwise; no fp
 * contraction):
 *   first frame (t = 0):  h = 0 (K taps),  P = (1 / delta) I (K x K)          (1 / delta: once per call, in fp32)
 *   x~_j  = R_{t-D-j},  j = 0 ... K-1              (D >= 0: with D = 0, x~_0 is the CURRENT far-end frame)
 *   e_t   = Y_t - sum_j conj(h_j) x~_j             (j ascending; the OUTPUT)
 *   r     = sum_j fmaf(re_j, re_j, im_j * im_j)    (j ascending, from +0; re_j, im_j of x~_j)
 *   if not (r <= quiet):                           (a NaN r adapts, and poisons its own row only)
 *       u_j  = sum_k P_jk x~_k                     (k ascending)
 *       q    = sum_j Re(conj(x~_j) u_j)            (j ascending)
 *       den  = alpha + q
 *       k_j  = u_j / den
 *       P_jk <- (P_jk - k_j conj(u_k)) / alpha   for j >= k;  Im P_jj := 0;  P_kj := conj(P_jk)
 *       h_j  <- h_j + k_j conj(e_t)
 *   optional M_t = sqrtf(fmaf(e.re, e.re, e.im * e.im))
 * The gate: a frame whose stacked far-end power r is at most `quiet` leaves P and h untouched, bit for bit; e_t is still produced,
 * from the frozen filter.  A silent far end is the normal state of a call, and without the gate P grows by 1 / alpha per silent
 * frame and overflows fp32 after about ln(3e38 delta) / -ln(alpha) frames: 18 000 frames, 290 s at hop 128 and 8 kHz, at the defaults.
 * Parameters (adn_aec_params; NULL = the defaults): taps K 8, delay D 0, forget alpha 0.995, loading delta 10, quiet 1e-8.  Legal
 * (ADN_ERR_INVALID otherwise, before any launch, the message starts with the function's name and names the field; a NaN is
 * illegal): 1 <= taps <= 32; 0 <= delay <= 8; 0.95 <= forget <= 1; 1e-3 <= loading <= 1e6; 0 <= quiet <= 1; and
 * 2 taps (1 - forget) <= 1, evaluated in double on the fp32 value of forget as in "dereverb stream multichannel": below it the
 * window 1 / (1 - forget) holds fewer frames than twice the unknowns.
 * loading and quiet are ABSOLUTE powers, as the delta of "dereverb stream" is: the operator is NOT scale invariant.  The defaults
 * suit spectra of audio at a peak of about 0.5 with n_fft 512 (loading = 0.01 raised the fp32 floor of the test cases from 8e-6 to 5e-3).
 * Consequences: with R = 0 the output is Y, bit for bit; with Y = 0 the output is zero; a non-finite value is confined to its own
 * (pair, bin); a row whose first frame of the call is frame 0 starts fresh whatever the state holds: no reset, no sentinel; with
 * alpha = 1 and no gated frame, h after T frames solves (delta I + sum_t x~_t x~_t^H) h = sum_t x~_t conj(Y_t).
 * Quality on the host (tests/test_echo_host.py, tests/echo_cases.py; float64 restatement, defaults, a 640-tap room at 8 kHz, far-end
 * single talk for 2 s and double talk after): the figures are in profiles/bench_echo.md and README.md, and both are asserted with 10 dB.
 *
 * What is pinned.  The result is bounded per (pair, bin) against the float64 restatement (tests/test_gpu_echo.py: E <= 4 floor, the
 * floor the largest E of the fp32 restatement of the same case in its two arithmetics, never below 2^-23, capped at 1e-4).  Pinned
 * bit for bit: two calls give the same result; any cut of a row's frames into calls; a row alone or in any batch, in whatever
 * slot; a bin whichever other bins share the call; mag_out against sqrtf(fmaf(re, re, im * im)) of spec_out; a lockstep pair
 * (adn_aec_stream) against adn_aec_online on the same ring spectrograms.  NOT pinned: the bits against numpy.  Deterministic: no
 * atomics, no reduction across lanes.
 *
 * State (adn_aec_stream_state_bytes(n_slots, n_bins, params), caller-owned, opaque, 8-byte aligned; host-only, and it validates
 * everything about the parameters): per (slot, bin) P, h and a ring of the last D + K far-end frames indexed by frame number,
 * 2 K^2 + 4 K + 2 D floats.  The history lives in the state and not in a stream's X ring: that ring's depth is the stream plan's,
 * and frame-major callers cut a row into calls.  Every byte of a row's record is written on store.
 *
 * Two entry points, one step function:
 *   adn_aec_online: mic_spec, far_spec and spec_out (n_rows, n_frames, n_bins, 2), the frames first_frame ... first_frame +
 *     n_frames - 1 of every row; mag_out (n_rows, 1, n_bins, width), may be NULL, columns [col0, col0 + n_frames) written.  Row i
 *     uses slot i.  It writes those columns, all of spec_out, the state of its rows, and not one byte else.  spec_out may overlap
 *     neither input.
 *   adn_aec_stream: between adn_stream_analyze and adn_stream_emit, for an adn_stream_* state whose streams 2 g and 2 g + 1 are the
 *     microphone and the far end of pair g (n_streams even; lookahead must be 0).  It reads both X rings for the frames the steps
 *     emit and writes e_t into stream 2 g's ring cells and M_t into columns [window - block, window) of window row 2 g of y, and
 *     not one byte of stream 2 g + 1's ring or windows; nothing for frames at and past the end of a finished stream.  aec_state
 *     has n_streams / 2 slots, pair g uses slot g.  adn_stream_emit is unchanged: it emits all streams and the host keeps row 2 g.
 * Cost: one launch, n_rows x ceil(n_bins / (256 / G)) workgroups of 256 threads, G = 8, 16 or 32 lanes per (row, bin), the smallest
 * that holds taps; P stays in registers for the whole call; per row-frame 8 K^2 + 12 K fp32 FMAs (4 K^2 for u, 4 K^2 for the update of all K^2 entries, 12 K for e, r, q and h), and 8 K^2 + 16 K + 8 D bytes of
 * state per row read and written per call.  No workspace, no atomics, no constant table (a capture may hold a first call); nothing
 * blocks or allocates.  A call's time is the per-frame chain of a workgroup, three workgroup barriers a frame: profiles/bench_echo.md.
 * Limits (ADN_ERR_INVALID before any launch; a refused call writes nothing): NULL or misaligned pointers (spectra and state 8-byte,
 * mag_out and y 4-byte); counts below 1; n_bins, n_slots <= 2^20; n_rows <= n_slots; first_frame >= 0 and first_frame + n_frames <
 * 2^31; col0 >= 0 and col0 + n_frames <= width when a mag_out is given; spec_out overlapping an input; a grid of 2^31 workgroups or
 * more; for adn_aec_stream what adn_wpe_stream refuses about the stream state and the steps, and an odd n_streams.
 * ADN_ERR_WORKSPACE: a state below adn_aec_stream_state_bytes.  Element offsets are 64-bit.
 * The pool form -- calls of one or several microphones that share a far end, each on its own clock, the same recursion on a pool
 * state -- is declared in adn_call.h and exported by libadn_call.so: this library's table is closed at the four functions below.  It
 * sizes its state with adn_aec_stream_state_bytes, which stays here.
 * Not here: more than one reference channel (stereo and surround far ends are "echo stream multireference" of adn_call.h, the
 * same recursion on the stacked references, exported by libadn_call.so); partitioned time-domain filters;
 * double-talk detectors; non-linear echo; any tuning by ear. */
typedef struct adn_aec_params { int taps, delay; float forget, loading, quiet; } adn_aec_params;
ADN_API const char *adn_aec_last_error(void);   /* the message of this thread's last failed adn_aec_* call; "" before any */
ADN_API int adn_aec_stream_state_bytes(int n_slots, int n_bins, const adn_aec_params *params, size_t *bytes);
ADN_API int adn_aec_online(const float *mic_spec, const float *far_spec, int n_rows, int n_frames, int n_bins, long first_frame,
                           const adn_aec_params *params, void *state, size_t state_bytes, int n_slots, float *spec_out,
                           float *mag_out, int width, int col0, void *stream);
ADN_API int adn_aec_stream(void *stream_state, size_t stream_state_bytes, float *y, int n_streams, long first_step, int n_steps,
                           long final_length, int n_fft, int hop, int window, int block, int lookahead, int max_steps,
                           const adn_aec_params *params, void *aec_state, size_t aec_state_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ADN_ECHO_H */
