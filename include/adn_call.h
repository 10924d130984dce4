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
 * (csrc/echo_stream_kernels.hip), csrc/echo/echo_api.hip for the argument checks it shares, and csrc/call/call_api.hip; the four
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
 * Not here: pools that mix mics; more than one far-end channel; a lockstep form with several microphones; double-talk detectors;
 * graph capture of a tick; any tuning by ear. */
#define ADN_CALL_MAX_MICS 7
ADN_API const char *adn_call_last_error(void);   /* the message of this thread's last failed call into this library; "" before any */
ADN_API int adn_aec_stream_pool(void *pool_state, size_t pool_state_bytes, int n_slots, int mics, int n_fft, int hop, int window,
                                int block, int lookahead, long ring_samples, const adn_stream_pool_row *rows, int n_rows, float *y,
                                const adn_aec_params *params, void *aec_state, size_t aec_state_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ADN_CALL_H */
