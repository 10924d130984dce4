// C ABI of libadn_call.so (include/adn_call.h): operators of a two-way call that the closed tables of libadn.so and libadn_echo.so
// cannot take.  The exported functions, their argument checks and their launches.  The checks are the ones the other two libraries
// make, by the same code: pool_state, pool_rows and pool_recordings of adn_api.hip (adn_host.h), aec_consts and aec_state_check of
// echo/echo_api.hip (echo/echo_checks.h).  Their objects are linked into this library too; csrc/libadn_call.map keeps every name
// but the ones adn_call.h declares local, adn_echo.h's four included.  The multi-reference forms (adn_aec_mr_*) launch
// call/echo_mr_kernels.hip (echo_mr.h), and at refs = 1 the launchers of echo_stream_kernels.hip.
#include "../echo/echo_checks.h"
#include "echo_mr.h"
#include "../../../include/adn_call.h"

#include <string>

using adn::aligned_to;
using adn::fail;
using adn::fail_hip;
using adn::fail_launch;

extern "C" {

const char *adn_call_last_error(void) { return adn::g_err.c_str(); }

// A call is a recording of mics + 1 channels, the far end the last one: the table checks are adn_wpe_mc_stream_pool's.
int adn_aec_stream_pool(void *pstate, size_t pstate_bytes, int n_slots, int mics, int n_fft, int hop, int window, int block,
                        int lookahead, long ring_samples, const adn_stream_pool_row *rows, int n_rows, float *y,
                        const adn_aec_params *params, void *aec_state, size_t aec_state_bytes, void *stream)
{
    const char *who = "adn_aec_stream_pool";
    const std::string w(who);
    PoolState p;
    adn::StreamPoolRows t = {};
    adn::AecConsts k;
    int max_new, max_span;
    long max_out;
    if (mics < 1 || mics > ADN_CALL_MAX_MICS) return fail(ADN_ERR_INVALID, w + ": need 1 <= mics <= 7 (a call is mics + 1 <= 8 streams)");
    const int channels = mics + 1;
    ADN_TRY(pool_state(who, pstate, pstate_bytes, n_slots, n_fft, hop, window, block, lookahead, ring_samples, &p));
    if (lookahead != 0) return fail(ADN_ERR_INVALID, w + ": the operator is causal: lookahead must be 0");
    if (!y) return fail(ADN_ERR_INVALID, w + ": null pointer");
    if (!aligned_to(y, 4)) return fail(ADN_ERR_INVALID, w + ": y must be 4-byte aligned");
    ADN_TRY(pool_rows(who, p, n_slots, rows, n_rows, &t, &max_new, &max_span, &max_out));
    ADN_TRY(aec_consts(who, params, &k));
    ADN_TRY(pool_recordings(who, n_slots, channels, rows, n_rows));
    ADN_TRY(aec_state_check(w, aec_state, aec_state_bytes, n_slots / channels * mics, n_fft / 2 + 1, k));
    ADN_LAUNCH(adn::launch_aec_stream_pool(static_cast<float *>(pstate), y, mics, p.g, t, k, static_cast<float *>(aec_state),
                                           static_cast<hipStream_t>(stream)), who);
    return ADN_OK;
}

// ---- echo stream multireference ---------------------------------------------------------------------------------------------------
// The parameters of a call with `refs` reference channels: adn_echo.h's ranges by adn_echo.h's code (aec_consts), then the two rules
// on the stacked size N = refs taps.  k: the parent's constants (what the forwarded refs = 1 launch takes); m: the kernel's.
static int aec_mr_consts(const char *who, int refs, const adn_aec_params *params, adn::AecConsts *k, adn::AecMrConsts *m)
{
    const std::string w(who);
    if (refs < 1 || refs > ADN_CALL_MAX_REFS) return fail(ADN_ERR_INVALID, w + ": need 1 <= refs <= 8");
    const adn_aec_params defaults = {refs == 1 ? 8 : 16 / refs, 0, 0.995f, 10.f, 1e-8f};
    const adn_aec_params p = params ? *params : defaults;
    ADN_TRY(aec_consts(who, &p, k));
    if (refs * p.taps > 32) return fail(ADN_ERR_INVALID, w + ": need refs taps <= 32 (taps is per reference channel)");
    // the window 1 / (1 - forget) must hold twice the N unknowns; in double, on the fp32 value the kernel uses
    if (!(2.0 * (double)(refs * p.taps) * (1.0 - (double)p.forget) <= 1.0))
        return fail(ADN_ERR_INVALID, w + ": need 2 refs taps (1 - forget) <= 1 (forget too low for this many stacked taps)");
    *m = adn::AecMrConsts{refs, k->K, k->D, k->alpha, k->p0, k->quiet};
    return ADN_OK;
}

// The record of (refs, taps, delay) is the parent's record of (N, refs delay): 2 N^2 + 4 N + 2 refs delay floats, so the parent's
// state check holds it.
static adn::AecConsts aec_mr_record(const adn::AecMrConsts &m) { return adn::AecConsts{m.Q * m.K, m.Q * m.D, m.alpha, m.p0, m.quiet}; }

int adn_aec_mr_state_bytes(int n_slots, int n_bins, int refs, const adn_aec_params *params, size_t *bytes)
{
    const char *who = "adn_aec_mr_state_bytes";
    const std::string w(who);
    adn::AecConsts k;
    adn::AecMrConsts m;
    if (!bytes) return fail(ADN_ERR_INVALID, w + ": null pointer");
    if (n_slots < 1 || n_slots > (1 << 20) || n_bins < 1 || n_bins > (1 << 20))
        return fail(ADN_ERR_INVALID, w + ": need 1 <= n_slots <= 2^20 and 1 <= n_bins <= 2^20");
    ADN_TRY(aec_mr_consts(who, refs, params, &k, &m));
    *bytes = (size_t)n_slots * (size_t)n_bins * (size_t)adn::aec_mr_record_floats(m.Q, m.K, m.D) * sizeof(float);
    return ADN_OK;
}

int adn_aec_mr_online(const float *mic_spec, const float *far_spec, int n_rows, int refs, int n_frames, int n_bins, long first_frame,
                      const adn_aec_params *params, void *state, size_t state_bytes, int n_slots, float *spec_out, float *mag_out,
                      int width, int col0, void *stream)
{
    const char *who = "adn_aec_mr_online";
    const std::string w(who);
    adn::AecConsts k;
    adn::AecMrConsts m;
    ADN_TRY(aec_online_counts(w, mic_spec, far_spec, spec_out, n_rows, n_frames, n_bins, first_frame));
    ADN_TRY(aec_mr_consts(who, refs, params, &k, &m));
    ADN_TRY(aec_state_check(w, state, state_bytes, n_slots, n_bins, aec_mr_record(m), "adn_aec_mr_state_bytes"));
    ADN_TRY(aec_online_buffers(w, mic_spec, far_spec, refs, n_rows, n_slots, n_frames, n_bins, spec_out, mag_out, width, col0));
    if (adn::aec_mr_grid(n_rows, n_bins, m.Q * m.K) > 0x7fffffffL)
        return fail(ADN_ERR_INVALID, w + ": grid too large (n_rows x ceil(n_bins / bins per workgroup) >= 2^31)");
    if (refs == 1)                                       // the operator of adn_echo.h, by its own launcher: its bits, the state included
        ADN_LAUNCH(adn::launch_aec_online(mic_spec, far_spec, n_rows, n_frames, n_bins, (int)first_frame, k, static_cast<float *>(state),
                                          spec_out, mag_out, width, col0, static_cast<hipStream_t>(stream)), who);
    else
        ADN_LAUNCH(adn::launch_aec_mr_online(mic_spec, far_spec, n_rows, n_frames, n_bins, (int)first_frame, m, static_cast<float *>(state),
                                             spec_out, mag_out, width, col0, static_cast<hipStream_t>(stream)), who);
    return ADN_OK;
}

int adn_aec_mr_stream(void *sstate, size_t sstate_bytes, float *y, int n_streams, int refs, long first_step, int n_steps,
                      long final_length, int n_fft, int hop, int window, int block, int lookahead, int max_steps,
                      const adn_aec_params *params, void *aec_state, size_t aec_state_bytes, void *stream)
{
    const char *who = "adn_aec_mr_stream";
    const std::string w(who);
    adn::StreamGeom g;
    adn::StreamCall call;
    adn::AecConsts k;
    adn::AecMrConsts m;
    ADN_TRY(aec_stream_args(who, sstate, sstate_bytes, y, n_streams, first_step, n_steps, final_length, n_fft, hop, window, block,
                            lookahead, max_steps, &g, &call));
    ADN_TRY(aec_mr_consts(who, refs, params, &k, &m));
    if (n_streams % (refs + 1))
        return fail(ADN_ERR_INVALID, w + ": n_streams must be a multiple of refs + 1 (the microphone first, its refs far ends after it)");
    const int groups = n_streams / (refs + 1);
    ADN_TRY(aec_state_check(w, aec_state, aec_state_bytes, groups, n_fft / 2 + 1, aec_mr_record(m), "adn_aec_mr_state_bytes"));
    if (adn::aec_mr_grid(groups, n_fft / 2 + 1, m.Q * m.K) > 0x7fffffffL)
        return fail(ADN_ERR_INVALID, w + ": grid too large (groups x ceil(n_bins / bins per workgroup) >= 2^31)");
    if (refs == 1)
        ADN_LAUNCH(adn::launch_aec_stream(static_cast<float *>(sstate), y, n_streams, g, call, k, static_cast<float *>(aec_state),
                                          static_cast<hipStream_t>(stream)), who);
    else
        ADN_LAUNCH(adn::launch_aec_mr_stream(static_cast<float *>(sstate), y, n_streams, g, call, m, static_cast<float *>(aec_state),
                                             static_cast<hipStream_t>(stream)), who);
    return ADN_OK;
}

}  // extern "C"
