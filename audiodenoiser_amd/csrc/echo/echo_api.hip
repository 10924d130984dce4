// C ABI of libadn_echo.so (include/adn_echo.h, "echo stream"): per-bin RLS from the far-end reference to the microphone.  The four
// exported functions, their argument checks and the launches of echo_stream_kernels.hip.  This file and that kernel file are linked
// into libadn_echo.so only: libadn.so holds nothing of the operator and its symbol table stays the one adn.h declares.  The checks of
// the stream state and of the steps are adn_api.hip's own (stream_state, stream_call), the ones in front of adn_wpe_stream.
#include "../adn_host.h"
#include "../../../include/adn_echo.h"
#include "echo_checks.h"

#include <string>

using adn::aligned_to;
using adn::fail;
using adn::fail_hip;
using adn::fail_launch;

extern "C" {

const char *adn_aec_last_error(void) { return adn::g_err.c_str(); }

// The parameters of a call (NULL = the defaults), refused outside their legal ranges.  (Not static, nor the other checks below:
// echo_checks.h, for csrc/call/call_api.hip.)
int aec_consts(const char *who, const adn_aec_params *params, adn::AecConsts *k)
{
    const std::string w(who);
    const adn_aec_params defaults = {8, 0, 0.995f, 10.f, 1e-8f};
    const adn_aec_params p = params ? *params : defaults;
    if (p.taps < 1 || p.taps > 32) return fail(ADN_ERR_INVALID, w + ": need 1 <= taps <= 32");
    if (p.delay < 0 || p.delay > 8) return fail(ADN_ERR_INVALID, w + ": need 0 <= delay <= 8");
    // written so that a NaN fails every test
    if (!(p.forget >= 0.95f && p.forget <= 1.f)) return fail(ADN_ERR_INVALID, w + ": need 0.95 <= forget <= 1");
    if (!(p.loading >= 1e-3f && p.loading <= 1e6f)) return fail(ADN_ERR_INVALID, w + ": need 1e-3 <= loading <= 1e6");
    if (!(p.quiet >= 0.f && p.quiet <= 1.f)) return fail(ADN_ERR_INVALID, w + ": need 0 <= quiet <= 1");
    // the window 1 / (1 - forget) must hold twice the K unknowns (adn_echo.h); in double, on the fp32 value the kernel uses
    if (!(2.0 * (double)p.taps * (1.0 - (double)p.forget) <= 1.0))
        return fail(ADN_ERR_INVALID, w + ": need 2 taps (1 - forget) <= 1 (forget too low for this many taps)");
    k->K = p.taps;
    k->D = p.delay;
    k->alpha = p.forget;
    k->p0 = 1.f / p.loading;
    k->quiet = p.quiet;
    return ADN_OK;
}

static size_t aec_bytes(int n_slots, int n_bins, const adn::AecConsts &k)
{
    return (size_t)n_slots * (size_t)n_bins * (size_t)adn::aec_record_floats(k.K, k.D) * sizeof(float);
}

int aec_state_check(const std::string &w, const void *state, size_t state_bytes, int n_slots, int n_bins, const adn::AecConsts &k,
                    const char *sizer)
{
    if (!state) return fail(ADN_ERR_INVALID, w + ": null pointer (the echo state)");
    if (n_slots < 1 || n_slots > (1 << 20) || n_bins < 1 || n_bins > (1 << 20))
        return fail(ADN_ERR_INVALID, w + ": need 1 <= n_slots <= 2^20 and 1 <= n_bins <= 2^20");
    if (state_bytes < aec_bytes(n_slots, n_bins, k))
        return fail(ADN_ERR_WORKSPACE, w + ": the echo state is smaller than " + sizer);
    if (!aligned_to(state, 8)) return fail(ADN_ERR_INVALID, w + ": the echo state must be 8-byte aligned");
    return ADN_OK;
}

// What adn_aec_online refuses about its counts and its buffers, in two parts because the parameters and the state are checked
// between them.  far_channels: far_spec holds that many spectrograms per row (1 here; adn_aec_mr_online of adn_call.h: refs).
int aec_online_counts(const std::string &w, const void *mic_spec, const void *far_spec, const void *spec_out, int n_rows, int n_frames,
                      int n_bins, long first_frame)
{
    if (!mic_spec || !far_spec || !spec_out) return fail(ADN_ERR_INVALID, w + ": null pointer (mic_spec, far_spec, spec_out)");
    if (n_rows < 1 || n_frames < 1 || n_bins < 1) return fail(ADN_ERR_INVALID, w + ": n_rows, n_frames and n_bins must be >= 1");
    if (first_frame < 0 || first_frame + n_frames >= (1L << 31))
        return fail(ADN_ERR_INVALID, w + ": need first_frame >= 0 and first_frame + n_frames < 2^31");
    return ADN_OK;
}

int aec_online_buffers(const std::string &w, const float *mic_spec, const float *far_spec, int far_channels, int n_rows, int n_slots,
                       int n_frames, int n_bins, const float *spec_out, const float *mag_out, int width, int col0)
{
    if (n_rows > n_slots) return fail(ADN_ERR_INVALID, w + ": row i uses slot i: need n_rows <= n_slots");
    if (mag_out && (col0 < 0 || width < 1 || (long)col0 + n_frames > width))
        return fail(ADN_ERR_INVALID, w + ": need col0 >= 0 and col0 + n_frames <= width");
    if (!aligned_to(mic_spec, 8) || !aligned_to(far_spec, 8) || !aligned_to(spec_out, 8) || !aligned_to(mag_out, 4))
        return fail(ADN_ERR_INVALID, w + ": mic_spec, far_spec and spec_out must be 8-byte aligned, mag_out 4-byte aligned");
    const size_t span = (size_t)n_rows * (size_t)n_frames * (size_t)n_bins * 2 * sizeof(float);
    const char *o = reinterpret_cast<const char *>(spec_out);
    const char *m = reinterpret_cast<const char *>(mic_spec), *f = reinterpret_cast<const char *>(far_spec);
    if ((m < o + span && o < m + span) || (f < o + span && o < f + span * (size_t)far_channels))
        return fail(ADN_ERR_INVALID, w + ": spec_out may not overlap mic_spec or far_spec");
    return ADN_OK;
}

// What adn_aec_stream refuses about the stream state, y and the steps: adn_wpe_stream's checks, and the causal plan
int aec_stream_args(const char *who, void *sstate, size_t sstate_bytes, const float *y, int n_streams, long first_step, int n_steps,
                    long final_length, int n_fft, int hop, int window, int block, int lookahead, int max_steps, adn::StreamGeom *g,
                    adn::StreamCall *call)
{
    const std::string w(who);
    ADN_TRY(stream_state(who, sstate, sstate_bytes, n_streams, n_fft, hop, window, block, lookahead, max_steps, g));
    if (lookahead != 0) return fail(ADN_ERR_INVALID, w + ": the operator is causal: lookahead must be 0");
    if (!y) return fail(ADN_ERR_INVALID, w + ": null pointer");
    if (!aligned_to(y, 4)) return fail(ADN_ERR_INVALID, w + ": y must be 4-byte aligned");
    return stream_call(who, *g, first_step, n_steps, final_length, call);
}

int adn_aec_stream_state_bytes(int n_slots, int n_bins, const adn_aec_params *params, size_t *bytes)
{
    const std::string w("adn_aec_stream_state_bytes");
    adn::AecConsts k;
    if (!bytes) return fail(ADN_ERR_INVALID, w + ": null pointer");
    if (n_slots < 1 || n_slots > (1 << 20) || n_bins < 1 || n_bins > (1 << 20))
        return fail(ADN_ERR_INVALID, w + ": need 1 <= n_slots <= 2^20 and 1 <= n_bins <= 2^20");
    ADN_TRY(aec_consts("adn_aec_stream_state_bytes", params, &k));
    *bytes = aec_bytes(n_slots, n_bins, k);
    return ADN_OK;
}

int adn_aec_online(const float *mic_spec, const float *far_spec, int n_rows, int n_frames, int n_bins, long first_frame,
                   const adn_aec_params *params, void *state, size_t state_bytes, int n_slots, float *spec_out, float *mag_out,
                   int width, int col0, void *stream)
{
    const std::string w("adn_aec_online");
    adn::AecConsts k;
    ADN_TRY(aec_online_counts(w, mic_spec, far_spec, spec_out, n_rows, n_frames, n_bins, first_frame));
    ADN_TRY(aec_consts("adn_aec_online", params, &k));
    ADN_TRY(aec_state_check(w, state, state_bytes, n_slots, n_bins, k));
    ADN_TRY(aec_online_buffers(w, mic_spec, far_spec, 1, n_rows, n_slots, n_frames, n_bins, spec_out, mag_out, width, col0));
    if (adn::aec_stream_grid(n_rows, n_bins, k.K) > 0x7fffffffL)
        return fail(ADN_ERR_INVALID, w + ": grid too large (n_rows x ceil(n_bins / bins per workgroup) >= 2^31)");
    ADN_LAUNCH(adn::launch_aec_online(mic_spec, far_spec, n_rows, n_frames, n_bins, (int)first_frame, k, static_cast<float *>(state),
                                      spec_out, mag_out, width, col0, static_cast<hipStream_t>(stream)), "adn_aec_online");
    return ADN_OK;
}

int adn_aec_stream(void *sstate, size_t sstate_bytes, float *y, int n_streams, long first_step, int n_steps, long final_length,
                   int n_fft, int hop, int window, int block, int lookahead, int max_steps, const adn_aec_params *params,
                   void *aec_state, size_t aec_state_bytes, void *stream)
{
    const std::string w("adn_aec_stream");
    adn::StreamGeom g;
    adn::StreamCall call;
    adn::AecConsts k;
    ADN_TRY(aec_stream_args("adn_aec_stream", sstate, sstate_bytes, y, n_streams, first_step, n_steps, final_length, n_fft, hop, window,
                            block, lookahead, max_steps, &g, &call));
    ADN_TRY(aec_consts("adn_aec_stream", params, &k));
    if (n_streams % 2) return fail(ADN_ERR_INVALID, w + ": n_streams must be even (stream 2 g the microphone, 2 g + 1 the far end)");
    ADN_TRY(aec_state_check(w, aec_state, aec_state_bytes, n_streams / 2, n_fft / 2 + 1, k));
    if (adn::aec_stream_grid(n_streams / 2, n_fft / 2 + 1, k.K) > 0x7fffffffL)
        return fail(ADN_ERR_INVALID, w + ": grid too large (pairs x ceil(n_bins / bins per workgroup) >= 2^31)");
    ADN_LAUNCH(adn::launch_aec_stream(static_cast<float *>(sstate), y, n_streams, g, call, k, static_cast<float *>(aec_state),
                                      static_cast<hipStream_t>(stream)), "adn_aec_stream");
    return ADN_OK;
}

}  // extern "C"
