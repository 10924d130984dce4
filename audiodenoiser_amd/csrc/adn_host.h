// Helpers shared by the translation units that implement the C ABI of include/adn.h (adn_api.hip, unet.hip): the last-error
// string, the status-returning wrappers around HIP calls, and the device guard.  Not part of the public ABI.
#pragma once
#include "../../include/adn.h"
#include "adn_internal.h"

#include <string>

namespace adn {

extern thread_local std::string g_err;          // what adn_last_error() returns; defined in adn_api.hip

inline int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}
inline int fail_hip(hipError_t e, const char *what)
{
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    return ADN_ERR_HIP;
}
#define ADN_HIP(call)                                   \
    do {                                                \
        hipError_t e_ = (call);                         \
        if (e_ != hipSuccess) return adn::fail_hip(e_, #call); \
    } while (0)
// a check that has set the message itself: its code goes on to the caller
#define ADN_TRY(call)                                   \
    do {                                                \
        const int rc_ = (call);                         \
        if (rc_ != ADN_OK) return rc_;                  \
    } while (0)
// launches that may need a constant table: a cold lookup on a capturing stream is the CALLER's error (adn.h, Conventions)
inline int fail_launch(hipError_t e, const char *what)
{
    if (e == ADN_COLD_IN_CAPTURE)
        return fail(ADN_ERR_INVALID, std::string(what) + ": first use of this (device, n_fft) on a stream that is being captured -- the "
                    "constant tables are built with a blocking upload; call adn_prepare(device, n_fft) before the capture");
    return fail_hip(e, what);
}
#define ADN_LAUNCH(call, what)                          \
    do {                                                \
        hipError_t e_ = (call);                         \
        if (e_ != hipSuccess) return adn::fail_launch(e_, what); \
    } while (0)

// Switches the calling thread to `device` for the lifetime of the guard and restores the caller's device on every
// exit path: no entry point leaves a hidden side effect on the caller's HIP state (adn.h, Conventions).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device)
    {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) {
            err = hipSetDevice(device);
            switched = err == hipSuccess;
        }
    }
    ~DeviceGuard()
    {
        if (switched) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

inline bool aligned_to(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace adn

// The two checks that stand in front of every entry point working on an adn_stream_* state (adn_api.hip): the state against its
// plan, and the steps of a call.  Declared for csrc/echo/echo_api.hip, which puts them in front of adn_aec_stream.
extern "C" {
int stream_state(const char *who, void *state, size_t state_bytes, int n_streams, int n_fft, int hop, int window, int block,
                 int lookahead, int max_steps, adn::StreamGeom *g);
int stream_call(const char *who, const adn::StreamGeom &g, long first, int n_steps, long final_length, adn::StreamCall *c);
}

// The same for a pool state (adn_api.hip): the state against its plan, the row table of a call, and the rows of a call on recordings
// of `channels` streams.  Declared for csrc/call/call_api.hip, which puts them in front of the pool operators of libadn_call.so.
struct PoolState {
    adn::StreamGeom g;
    long ring_off, total, R;
};
extern "C" {
int pool_state(const char *who, void *state, size_t state_bytes, int n_slots, int n_fft, int hop, int window, int block,
               int lookahead, long ring, PoolState *p);
int pool_rows(const char *who, const PoolState &p, int n_slots, const adn_stream_pool_row *rows, int n_rows,
              adn::StreamPoolRows *t, int *max_new, int *max_span, long *max_out);
int pool_recordings(const char *who, int n_slots, int channels, const adn_stream_pool_row *rows, int n_rows);
}
