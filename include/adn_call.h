/* adn_call.h -- operators of a two-way call on the MI355X (gfx950): the C ABI of libadn_call.so.  See adn.h for the conventions. */
#ifndef ADN_CALL_H
#define ADN_CALL_H
#include "adn.h"
#include "adn_echo.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- call: operators of a two-way call that the two closed tables cannot take ---------------------------------------------------------
 * A third header and a third library.  libadn.so exports exactly what adn.h declares and libadn_echo.so exactly the four functions
 * of adn_echo.h; both tables are closed.  This one is OPEN: the next operator of a call is declared here and named in
 * csrc/libadn_call.map.  libadn_call.so exports the functions declared below and nothing else (-fvisibility=hidden and that
 * version script, which lists them name by name).  It is linked from the objects of libadn.so, the echo kernel file
 * (csrc/echo_stream_kernels.hip), csrc/echo/echo_api.hip for the argument checks it shares, and csrc/call/ (call_api.hip and the
 * multi-reference kernel file echo_mr_kernels.hip, which no other library holds); the four
 * functions of adn_echo.h are in it and stay local.  It needs neither other library at run time.  The states it works on are
 * theirs, byte for byte: the pool state of adn.h ("stream pool") and the echo state of adn_echo.h, sized by
 * adn_aec_stream_state_bytes of libadn_echo.so, which stays there; both are plain device memory, so a caller loads the libraries
 * side by side and hands the buffers of one to the other.  The conventions are adn.h's (status codes, device pointers, the caller's
 * stream, no allocation, no blocking); the message of a failed call is this library's own and is read with adn_call_last_error,
 * and a refused call leaves the other two libraries' messages as they were.
 *
 * ---- echo stream pool: the operator "echo stream" of adn_echo.h for calls that open, stall and hang up on their own clocks
 * No new arithmetic: every (microphone, bin) row is the recursion of "echo stream", statement for statement, from the same step
 * function of the same kernel file.  What is new is where a row's frames come from and which frames it walks.
 *
 * A CALL is M = mics microphones that share ONE far end (a device with several microphones has one loudspeaker): M + 1 streams of
 * a pool state, the microphones in order and the far end last.  Call r owns stream slots r (M + 1) ... r (M + 1) + M of the pool
 * state (n_slots a multiple of M + 1) and slots r M ... r M + M - 1 of the echo state, one per microphone; aec_state holds
 * n_slots / (M + 1) * M slots of n_fft / 2 + 1 bins.  One mics per pool state.  With mics = 1 a call is the pair of adn_aec_stream.
 *
 * adn_aec_stream_pool runs between adn_stream_pool_analyze and adn_stream_pool_emit on the same row table: n_rows = n_calls (M + 1)
 * rows of (slot, step, final_length), call i of the table in rows i (M + 1) ... i (M + 1) + M, which must name the M + 1 slots of one
 * call in order with one step and one final_length.  y is the windows buffer of the analyze call, (n_rows, 1, n_bins, window).
 * Pair g of the launch is microphone m = g % M of table call i = g / M:
 *   frames, step and ring slot:   table row i (M + 1) + m
 *   far-end ring slot:            table row i (M + 1) + M
 *   window row in y:              the microphone's table row index, i (M + 1) + m
 *   echo-state slot:              (slot of table row i (M + 1)) / (M + 1) * M + m
 * It reads both X rings for the frames the row's step emits, [step block, step block + block - 1], cut at the last frame of a
 * finished call; it writes e_t into the microphone slot's ring cells, M_t into columns [window - block, window) of the
 * microphone's window row of y, and the state records of the named pairs.  It writes not one byte else: nothing of a far-end slot
 * or of its window row; nothing of a slot the table does not name; nothing for frames at and past the end of a finished call.  So
 * the far-end rows need no resynthesis: a caller hands adn_stream_pool_emit the microphone rows alone (a row table is what that
 * call takes), and nothing of the far-end slot's overlap-add section ever changes.
 * A pair whose step is 0 starts fresh whatever its state slot holds: no reset, no sentinel, and a slot is reusable as it is.
 *
 * What is pinned, bit for bit (tests/test_gpu_echo_pool.py): the ring cells, window columns and state records against
 * adn_aec_stream on the same cells, for mics 1, 2, 4 and 7, in whatever slots and table order; calls at different steps in one
 * launch against each alone; every microphone of a pool's call against a solo lockstep pair fed that microphone and the far end.
 * Against float64 it is bounded as "echo stream" is, by that bound.
 *
 * Cost: one launch, n_calls M x ceil(n_bins / (256 / G)) workgroups of 256 threads, G = 8, 16 or 32 the smallest that holds taps.
 * A workgroup is one pair and 256 / G consecutive bins, so all its groups walk the same frames and its three barriers per frame are
 * uniform; the frames differ between workgroups.  The row table travels by value in the kernel arguments.  No workspace, no
 * atomics, no constant table; nothing blocks or allocates.
 * Limits (ADN_ERR_INVALID before any launch, the message starts with the function's name; a refused call writes nothing): mics
 * outside 1 ... ADN_CALL_MAX_MICS; what adn_wpe_mc_stream_pool refuses with channels = mics + 1 -- the pool plan and state, n_rows
 * below 1, above ADN_STREAM_POOL_MAX_ROWS or no multiple of mics + 1, a slot outside [0, n_slots), a slot named twice, a call
 * whose rows are not its mics + 1 slots in order or disagree in step or final_length, n_slots no multiple of mics + 1, a step
 * outside the stream section's limits; lookahead other than 0; NULL or misaligned pointers (states 8-byte, y 4-byte); parameters
 * outside the ranges of adn_echo.h.  ADN_ERR_WORKSPACE: a pool state below adn_stream_pool_state_bytes or an echo state below
 * adn_aec_stream_state_bytes of n_slots / (mics + 1) * mics slots.
 * Not here: pools that mix mics; more than one far-end channel PER CALL OF A POOL (the frame-major and lockstep forms with several
 * are "echo stream multireference" below); a lockstep form with several microphones; double-talk detectors; graph capture of a tick;
 * any tuning by ear. */
#define ADN_CALL_MAX_MICS 7
ADN_API const char *adn_call_last_error(void);   /* the message of this thread's last failed call into this library; "" before any */
ADN_API int adn_aec_stream_pool(void *pool_state, size_t pool_state_bytes, int n_slots, int mics, int n_fft, int hop, int window,
                                int block, int lookahead, long ring_samples, const adn_stream_pool_row *rows, int n_rows, float *y,
                                const adn_aec_params *params, void *aec_state, size_t aec_state_bytes, void *stream);

/* ---- echo stream multireference: "echo stream" of adn_echo.h on the stacked vector of Q far-end channels ------------------------------
 * A stereo or surround far end: the microphone hears the sum of Q = refs loudspeaker signals through Q rooms, and no single
 * reference models that sum.  ONE filter of N = Q K taps over all Q references does (float64 restatement: tests/echo_mr_ref.py;
 * kernel: csrc/call/echo_mr_kernels.hip).  1 <= refs <= ADN_CALL_MAX_REFS (8), taps K is PER CHANNEL, and N = refs taps <= 32.
 * A group is one microphone Y and its Q far ends R_{.,q}; every (group, bin) is independent.  The definition is "echo stream" with
 *   x~_r = R_{t-D-j, q}   at r = q K + j,  q = 0 ... Q-1,  j = 0 ... K-1       (channel-major, the lag ascending: the order of
 *                                                                               "dereverb multichannel" of adn.h)
 * h of N taps, P N x N with P = (1 / delta) I at the first frame, and every statement of "echo stream" read as written with K -> N:
 * e_t, r, u, q, den, k, the Hermitian update, the gate, the optional M_t; the sums ascend in r; the fp32 rounding rules are the same.
 * The gate is on the STACKED power r of all channels: a frame adapts unless the last D + K frames of every channel are quiet together.
 * Parameters: adn_aec_params of adn_echo.h, unchanged.  params = NULL: taps = 8 for refs = 1 and 16 / refs (integer division: 8, 5,
 * 4, 3, 2, 2, 2) for refs >= 2, the other fields the defaults of adn_echo.h.  The default does NOT fill the stacked size: at forget
 * 0.995 a filter of 32 unknowns misadjusts in double talk (profiles/bench_echo_mr.md: 2 x 16 loses 13 dB of SI-SDR against 2 x 8).
 * It is a design value from that table and was not tuned by ear.  Legal: the ranges of adn_echo.h, and refs taps <= 32, and
 * 2 N (1 - forget) <= 1 evaluated as there (in double, on the fp32 value of forget).
 * Consequences: those of "echo stream" -- all references zero gives Y bit for bit, Y = 0 gives zero, a non-finite value stays in its
 * (group, bin), a row whose first frame is frame 0 starts fresh whatever the state holds -- and with alpha = 1 and no gated frame
 * h solves the stacked normal equations (delta I + sum_t x~_t x~_t^H) h = sum_t x~_t conj(Y_t).  With refs = 1 every entry point
 * below forwards to the launcher of adn_aec_online / adn_aec_stream and returns their bits, the state included.
 * One limit, stated and NOT guarded: a reference channel that stays digitally silent while another plays is not protected by the
 * gate (the stacked power is not quiet), its block of P grows by 1 / alpha per adapted frame and overflows fp32 after about
 * ln(3e38 delta) / -ln(alpha) such frames, as adn_echo.h derives for ungated silence: 18 000 frames at the defaults.  A caller with a
 * mono signal passes refs = 1, not the same signal twice and not a silent second channel.
 *
 * State (adn_aec_mr_state_bytes, host-only, validates everything about the parameters; caller-owned, opaque, 8-byte aligned): per
 * (slot, bin) P, then h, then Q rings of the last D + K far-end frames indexed by frame number, 2 N^2 + 4 N + 2 Q D floats.  With
 * Q = 1 the record is adn_echo.h's byte for byte.  Every byte of a row's record is written on store.
 *
 * Two entry points, one step function:
 *   adn_aec_mr_online: adn_aec_online's contract with far_spec (n_rows, refs, n_frames, n_bins, 2): the Q references of row i follow
 *     each other.  mic_spec, spec_out (n_rows, n_frames, n_bins, 2); mag_out (n_rows, 1, n_bins, width) or NULL, columns [col0, col0 +
 *     n_frames).  Row i uses slot i.  It writes those columns, spec_out, the state of its rows, and not one byte else.
 *   adn_aec_mr_stream: adn_aec_stream's contract with n_streams a multiple of refs + 1: group g is streams g (Q + 1) ... g (Q + 1) + Q
 *     of an adn_stream_* state, the microphone first and the Q far ends after it (lookahead must be 0).  It reads all Q + 1 X rings
 *     for the frames the steps emit and writes e_t into the microphone stream's ring cells, M_t into columns [window - block, window)
 *     of the microphone's window row of y, and the operator state (n_streams / (Q + 1) slots, group g uses slot g); not one byte of a
 *     far-end stream's ring or windows or of anything else; nothing for frames at and past the end of a finished stream.
 * What is pinned (tests/test_gpu_echo_mr.py): per (row, bin) against float64 as "echo stream" is, E <= 4 floor, the floor measured
 * from the float32 restatement of the same case, capped at 1e-4; bit for bit: refs = 1 against adn_aec_online and adn_aec_stream,
 * outputs and state bytes; two calls; any cut of a row's frames into calls; a row alone or in a batch, in any slot; a bin whichever
 * bins share the call; mag_out against spec_out; the lockstep group against adn_aec_mr_online on the same ring spectrograms.
 * Cost: one launch, n_groups x ceil(n_bins / (256 / G)) workgroups of 256 threads, G = 8, 16 or 32 lanes per (group, bin), the
 * smallest that holds N; P stays in registers for the whole call, u, k, h and the Q rings in LDS; per row-frame 8 N^2 + 12 N fp32
 * FMAs and Q + 1 loaded values; 8 N^2 + 16 N + 8 Q D bytes of state per row read and written per call.  No workspace, no atomics, no
 * reduction across lanes, no constant table; three workgroup barriers a frame: profiles/bench_echo_mr.md.
 * Limits (ADN_ERR_INVALID before any launch, the message starts with the function's name and names the field; a refused call
 * writes nothing): what adn_aec_online and adn_aec_stream refuse, by the same code (csrc/echo/echo_checks.h); refs outside 1 ... 8;
 * refs taps > 32; 2 refs taps (1 - forget) > 1; an n_streams that is no multiple of refs + 1; spec_out overlapping mic_spec or any
 * of far_spec's refs spectrograms per row.  ADN_ERR_WORKSPACE: a state below adn_aec_mr_state_bytes.
 * Not here: the pool form, mics x refs calls on their own clocks (the kernel's frame source is a template argument left for it); a
 * guard against the wind-up of a reference that stays silent while others play; N > 32; double-talk detectors; non-linear echo; any
 * tuning by ear. */
#define ADN_CALL_MAX_REFS 8
ADN_API int adn_aec_mr_state_bytes(int n_slots, int n_bins, int refs, const adn_aec_params *params, size_t *bytes);
ADN_API int adn_aec_mr_online(const float *mic_spec, const float *far_spec, int n_rows, int refs, int n_frames, int n_bins,
                              long first_frame, const adn_aec_params *params, void *state, size_t state_bytes, int n_slots,
                              float *spec_out, float *mag_out, int width, int col0, void *stream);
ADN_API int adn_aec_mr_stream(void *stream_state, size_t stream_state_bytes, float *y, int n_streams, int refs, long first_step,
                              int n_steps, long final_length, int n_fft, int hop, int window, int block, int lookahead, int max_steps,
                              const adn_aec_params *params, void *aec_state, size_t aec_state_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ADN_CALL_H */
