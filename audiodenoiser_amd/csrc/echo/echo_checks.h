// The two checks every echo entry point makes (echo_api.hip defines them): the parameters of a call against the legal ranges of
// include/adn_echo.h, and the operator state against adn_aec_stream_state_bytes.  Declared for csrc/call/call_api.hip, whose pool form
// of the operator (include/adn_call.h) refuses what adn_aec_stream refuses, by the same code.  Not part of any public ABI: both
// libraries' version scripts keep the names local.
#pragma once
#include "../adn_host.h"
#include "../../../include/adn_echo.h"

#include <string>

extern "C" {
// params NULL = the defaults; the message starts with `who` and names the field
int aec_consts(const char *who, const adn_aec_params *params, adn::AecConsts *k);
// ADN_ERR_WORKSPACE for a state below n_slots x n_bins records, ADN_ERR_INVALID for a null or misaligned one and for counts outside [1, 2^20]
int aec_state_check(const std::string &w, const void *state, size_t state_bytes, int n_slots, int n_bins, const adn::AecConsts &k);
}
