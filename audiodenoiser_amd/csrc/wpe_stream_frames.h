// What the two recursive WPE kernels share (dereverb_stream_kernels.hip, dereverb_mc_stream_kernels.hip): the grid, the store of a
// record's P rows and the places a row's frames come from (the rounding rules are wpe_common.h's).  One definition, so that a joint
// stream of one recording and C single-channel streams read and write the same cells by the same arithmetic.  Everything is in an unnamed
// namespace on purpose: each of the two translation units instantiates its own kernels on these types, and the single-channel
// kernels keep the symbols and the code they had when this text stood in their file (tools/kernel_isa_digest.py).
#pragma once
#include "wpe_common.h"

namespace adn {
namespace {

constexpr int WS_G = 32;                             // lanes per group = the most taps
constexpr int WS_GROUPS = 8;                         // groups (bins) per workgroup
constexpr int WS_HMAX = 40;                          // D + K at most

// workgroups per row (or group of rows) of a launch: WS_GROUPS bins each
inline long ws_tiles(int F) { return ((long)F + WS_GROUPS - 1) / WS_GROUPS; }

// Lane r holds row r of P in Pr; a record keeps element (r, s) at s N + r.  (The load of that row, u = P x~, q and the Hermitian
// update are the same statements in both kernels too, but stay written out in each: as shared functions they moved the kernels'
// instructions and five of fifteen rows of the timing tables past the parent's spread -- profiles/wpe_family.md.)
__device__ __forceinline__ void store_P_row(const float2 (&Pr)[WS_G], float2 *stP, int r, int N)
{
#pragma unroll
    for (int k = 0; k < WS_G; ++k)
        if (k < N && r < N) stP[k * N + r] = Pr[k];
}

// ---------------------------------------------------------------------------------------------- where the frames are
struct FrameMajor {
    const float2 *spec;
    float2 *out;
    float *mag;                          // may be null
    int T, width, col0, first_frame;
};

template <class Rows>
struct InRing {
    float *state;                        // the adn_stream_* / pool state
    float *y;                            // the windows buffer
    StreamGeom g;
    Rows rows;
};

__device__ __forceinline__ StreamCall call_of(const StreamCall &c, const StreamGeom &, long) { return c; }
__device__ __forceinline__ StreamCall call_of(const StreamPoolRows &t, const StreamGeom &g, long row)
{
    return stream_call_of(g, t.row[row].step, 1, t.row[row].final_length);
}
__device__ __forceinline__ long slot_of(const StreamCall &, long row) { return row; }
__device__ __forceinline__ long slot_of(const StreamPoolRows &t, long row) { return t.row[row].slot; }

// What a group needs to know about its row: the state slot, the frames [t0, t1], and the addresses of frame t
struct RowFrames {
    long slot;
    int t0, t1;
};

__device__ __forceinline__ RowFrames frames_of(const FrameMajor &s, long row, int, StreamCall &)
{
    return RowFrames{row, s.first_frame, s.first_frame + s.T - 1};
}
template <class Rows>
__device__ __forceinline__ RowFrames frames_of(const InRing<Rows> &s, long row, int, StreamCall &c)
{
    c = call_of(s.rows, s.g, row);
    return RowFrames{slot_of(s.rows, row), c.f_first, c.f_last};
}

__device__ __forceinline__ float2 load_frame(const FrameMajor &s, const RowFrames &, const StreamCall &, long row, int F, int bin, int t)
{
    return s.spec[(row * s.T + (t - s.first_frame)) * (long)F + bin];
}
__device__ __forceinline__ void store_frame(const FrameMajor &s, const RowFrames &, const StreamCall &, long row, int F, int bin, int t,
                                            float2 d, float m)
{
    const long i = t - s.first_frame;
    s.out[(row * s.T + i) * (long)F + bin] = d;
    if (s.mag) s.mag[(row * F + bin) * (long)s.width + s.col0 + i] = m;
}
template <class Rows>
__device__ __forceinline__ float2 *ring_cell(const InRing<Rows> &s, const RowFrames &r, int F, int bin, int t)
{
    return reinterpret_cast<float2 *>(s.state + s.g.x_off) + (r.slot * s.g.RX + t % s.g.RX) * (long)F + bin;
}
template <class Rows>
__device__ __forceinline__ float2 load_frame(const InRing<Rows> &s, const RowFrames &r, const StreamCall &, long, int F, int bin, int t)
{
    return *ring_cell(s, r, F, bin, t);
}
template <class Rows>
__device__ __forceinline__ void store_frame(const InRing<Rows> &s, const RowFrames &r, const StreamCall &c, long row, int F, int bin, int t,
                                            float2 d, float m)
{
    *ring_cell(s, r, F, bin, t) = d;
    // frame t is local frame W - B + t mod B of step t / B (look-ahead 0), window (row n_steps + step - first) of the buffer
    const int st = t / s.g.B;
    s.y[((row * c.n_steps + (st - c.first)) * (long)F + bin) * s.g.W + (s.g.W - s.g.B) + (t - st * s.g.B)] = m;
}

// ---------------------------------------------------------------------------------------------- frames that come with a magnitude
// The streaming beamformer (beamform_stream_kernels.hip) reads C rows per group, each frame with a magnitude estimate M_t, and
// writes ONE row per group.  Added beside the sources above, which keep their layout and their code:
//   FrameMajorMasked      FrameMajor whose `out` / `mag` rows are GROUPS, plus mag_in [group C + c][F][mag_width] at mag_col0
//   InRing<StreamCall>    M_t is read where store_frame above writes it (columns [W - B, W) of the row's windows); the output row of
//                         group g is its first stream, g C
struct FrameMajorMasked {
    FrameMajor f;
    const float *mag_in;
    int mag_width, mag_col0;
};

__device__ __forceinline__ RowFrames frames_of(const FrameMajorMasked &s, long row, int F, StreamCall &c) { return frames_of(s.f, row, F, c); }
__device__ __forceinline__ float2 load_frame(const FrameMajorMasked &s, const RowFrames &r, const StreamCall &c, long row, int F, int bin, int t)
{
    return load_frame(s.f, r, c, row, F, bin, t);
}
__device__ __forceinline__ void store_frame(const FrameMajorMasked &s, const RowFrames &r, const StreamCall &c, long row, int F, int bin, int t,
                                            float2 d, float m)
{
    store_frame(s.f, r, c, row, F, bin, t, d, m);
}
__device__ __forceinline__ float load_mag(const FrameMajorMasked &s, const RowFrames &, const StreamCall &, long row, int F, int bin, int t)
{
    return s.mag_in[(row * F + bin) * (long)s.mag_width + s.mag_col0 + (t - s.f.first_frame)];
}
template <class Rows>
__device__ __forceinline__ float load_mag(const InRing<Rows> &s, const RowFrames &, const StreamCall &c, long row, int F, int bin, int t)
{
    const int st = t / s.g.B;
    return s.y[((row * c.n_steps + (st - c.first)) * (long)F + bin) * s.g.W + (s.g.W - s.g.B) + (t - st * s.g.B)];
}
// the row group g's result goes to, of C rows per group
__device__ __forceinline__ long out_row_of(const FrameMajorMasked &, long g, int) { return g; }
template <class Rows>
__device__ __forceinline__ long out_row_of(const InRing<Rows> &, long g, int C) { return g * C; }

// ---------------------------------------------------------------------------------------------- groups of C rows
// The joint kernels (dereverb_mc_stream_kernels.hip, beamform_stream_kernels.hip) work on GROUPS of C consecutive rows and keep
// one operator-state slot per group.  Two lookups say where a group's things are; overloads on the source, so that the frame-major
// and the lockstep instantiations stay the code they were (row = ring slot, group = state slot):
//   chan_slot_of    the ring slot of row `row` (= g C + c)
//   group_slot_of   the operator-state slot of group g
// A pool's rows name their slots: a recording r owns the stream slots r C ... r C + C - 1 in channel order (the entry points refuse
// every other table), so its channel c is slot_of(rows, g C + c) and its operator-state slot is slot_of(rows, g C) / C.  The
// window row in y stays the row index in every source.
__device__ __forceinline__ long chan_slot_of(const FrameMajor &, long row) { return row; }
__device__ __forceinline__ long chan_slot_of(const FrameMajorMasked &, long row) { return row; }
template <class Rows>
__device__ __forceinline__ long chan_slot_of(const InRing<Rows> &s, long row) { return slot_of(s.rows, row); }
__device__ __forceinline__ long group_slot_of(const FrameMajor &, long g, int) { return g; }
__device__ __forceinline__ long group_slot_of(const FrameMajorMasked &, long g, int) { return g; }
__device__ __forceinline__ long group_slot_of(const InRing<StreamCall> &, long g, int) { return g; }
__device__ __forceinline__ long group_slot_of(const InRing<StreamPoolRows> &s, long g, int C) { return slot_of(s.rows, g * C) / C; }

}  // namespace
}  // namespace adn
