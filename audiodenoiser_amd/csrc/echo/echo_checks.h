// The checks every echo entry point makes (echo_api.hip defines them): the parameters of a call against the legal ranges of
// include/adn_echo.h, the operator state against its size, and what adn_aec_online and adn_aec_stream refuse about their other
// arguments.  Declared for csrc/call/call_api.hip, whose forms of the operator (include/adn_call.h) refuse what adn_aec_online and
// adn_aec_stream refuse, by the same code.  Not part of any public ABI: both libraries' version scripts keep the names local.
#pragma once
#include "../adn_host.h"
#include "../../../include/adn_echo.h"

#include <string>

extern "C" {
// params NULL = the defaults; the message starts with `who` and names the field
int aec_consts(const char *who, const adn_aec_params *params, adn::AecConsts *k);
// ADN_ERR_WORKSPACE for a state below n_slots x n_bins records of aec_record_floats(k.K, k.D) floats (the message names `sizer`, the
// function that gives the size), ADN_ERR_INVALID for a null or misaligned one and for counts outside [1, 2^20]
int aec_state_check(const std::string &w, const void *state, size_t state_bytes, int n_slots, int n_bins, const adn::AecConsts &k,
                    const char *sizer = "adn_aec_stream_state_bytes");
// adn_aec_online's own refusals, in the order it makes them: the counts before the parameters and the state, the buffers after.
// far_spec holds far_channels spectrograms per row.
int aec_online_counts(const std::string &w, const void *mic_spec, const void *far_spec, const void *spec_out, int n_rows, int n_frames,
                      int n_bins, long first_frame);
int aec_online_buffers(const std::string &w, const float *mic_spec, const float *far_spec, int far_channels, int n_rows, int n_slots,
                       int n_frames, int n_bins, const float *spec_out, const float *mag_out, int width, int col0);
// adn_aec_stream's: the stream state against its plan, lookahead 0, y, the steps
int aec_stream_args(const char *who, void *sstate, size_t sstate_bytes, const float *y, int n_streams, long first_step, int n_steps,
                    long final_length, int n_fft, int hop, int window, int block, int lookahead, int max_steps, adn::StreamGeom *g,
                    adn::StreamCall *call);
}
