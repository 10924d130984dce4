// C ABI of libadn_call.so (include/adn_call.h): operators of a two-way call that the closed tables of libadn.so and libadn_echo.so
// cannot take.  The exported functions, their argument checks and their launches.  The checks are the ones the other two libraries
// make, by the same code: pool_state, pool_rows and pool_recordings of adn_api.hip (adn_host.h), aec_consts and aec_state_check of
// echo/echo_api.hip (echo/echo_checks.h).  Their objects are linked into this library too; csrc/libadn_call.map keeps every name
// but the ones adn_call.h declares local, adn_echo.h's four included.
#include "../echo/echo_checks.h"
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

}  // extern "C"
