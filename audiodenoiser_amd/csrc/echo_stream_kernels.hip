// Acoustic echo cancellation for gfx950: exponentially forgetting RLS from the far-end reference to the microphone, one update per
// frame and (pair, bin) row.  Definition: include/adn_echo.h, "echo stream"; float64 restatement: tests/echo_ref.py.
//
// State of a (slot, bin) row (adn_aec_stream_state_bytes; REC = 2 K^2 + 4 K + 2 D floats, rows [slot][bin] consecutive):
//   P     [k][j] float2   the K x K inverse correlation matrix, element (j, k) at k K + j: lane j's loads are consecutive in j
//   h     [j]    float2   the K taps
//   hist  [i]    float2   the last far-end frames, frame t at t mod H, H = D + K
// A row whose first frame of the call is frame 0 reads none of it, and every byte of a row's record is written on store.
//
// Shape of the work.  A row is a recurrence over its frames, rows are independent.  A GROUP of G lanes owns one row, G in
// {8, 16, 32} the smallest that holds K (the default K = 8 fills its group; the 32 lanes of the WPE kernel would idle 24).  Lane j
// holds row j of P in registers (G float2), and u, k, h and the far-end ring of the group live in LDS.  A workgroup is 256 threads:
// 256 / G groups, the same pair of the launch for 256 / G consecutive bins, so every group of a workgroup walks the same frames and
// the barriers are uniform.  Per frame:
//   1  lane 0 puts R_t into the ring (x~_i = R_{t-D-i} is read out of the ring where it lies, no gathered copy)      barrier
//   2  every lane forms e_t and r (K steps, tap order, LDS broadcasts); lane j forms u_j                             barrier
//   3  every lane forms q and den (tap order); lane j forms k_j                                                      barrier
//   4  unless the row is gated: lane j updates its row of P and h_j.  Lane 0 stores e_t and M_t.
// Three barriers, not the WPE kernel's four.  Every ring read of frame t is in steps 2 and 3, that is before the barrier after
// step 3 (the oldest tap x~_{K-1} = R_{t+1-H} lies in the very cell that step 1 of frame t + 1 overwrites, so this matters); step
// 4 reads u and k only and writes h_j and registers only.  A wave that runs ahead into step 1 of frame t + 1 has passed that
// barrier, so every wave has finished its ring reads of frame t, and u, k and h are next written after the barrier of that step 1,
// which no wave passes before all have finished step 4.  A ring read moved into step 4 would need the fourth barrier back.  The
// barriers are workgroup barriers (__syncthreads) although a group never leaves its wave: see DESIGN.md, "Echo cancellation".
// The gate (r <= quiet) is uniform per group but not per workgroup, so it guards the stores of step 4 only and
// no barrier stands inside it.
// No value crosses lanes through a reduction: every lane computes e, r, q and den itself, in tap order, so nothing depends on G or
// on neighbours.  The Hermitian update is the WPE kernel's: lane j computes P_jk for k <= j as written in adn_echo.h and takes its k > j
// entries as the conjugate of the SAME statement evaluated for (k, j) on conj(P_jk).
//
// Where the frames come from is the template argument:
//   EchoFrameMajor        mic / far / spec_out [row][frame][F] float2, mag_out [row][F][width] at col0; continues at first_frame
//   InRing<StreamCall>    pair g is streams 2 g (microphone) and 2 g + 1 (far end) of an adn_stream_* state: both X rings are read
//                         for frames f_first .. f_last, e_t goes into stream 2 g's ring cells, M_t into columns [W - B, W) of window
//                         row 2 g of y; nothing of stream 2 g + 1 is written.  Operator-state slot g.
//   EchoPoolCalls         InRing<StreamPoolRows> and M: the row table holds CALLS of M microphones and one far end, M + 1 rows each,
//                         the microphones first (include/adn_call.h).  Pair g is microphone m = g % M of call i = g / M: its frames,
//                         its step and its ring slot are table row i (M + 1) + m's, its far-end ring slot table row i (M + 1) + M's,
//                         its window row in y the microphone's table row, its operator-state slot
//                         (slot of the call's first row / (M + 1)) M + m.  Nothing of a far-end slot is written.  Every row
//                         derives its own frames [t0, t1] from its step, so they differ BETWEEN workgroups; a workgroup is still one
//                         pair, so its groups walk the same frames and the barriers stay uniform.
// The step itself is one function, compiled with fp contraction off, every multiply-add an explicit fmaf.
//
// Cost (derived): per row-frame 8 K^2 + 12 K fp32 FMAs -- 4 K^2 for u, 4 K^2 for the update (a lane evaluates all K entries of its
// row of P, not a triangle), 4 K each for e and h, 2 K each for r and q -- not counting that every lane repeats e, r and q; the state is
// 8 K^2 + 16 K + 8 D bytes per row read and written per call.  No atomics, no workspace, no constant table.
#include "wpe_stream_frames.h"

namespace adn {
namespace {

constexpr int AEC_THREADS = 256;
constexpr int AEC_HMAX = 40;                          // D + K at most

// The LDS of one group
template <int G>
struct EchoLds {
    float2 ring[AEC_HMAX];
    float2 u[G], k[G], h[G];
};

struct EchoFrameMajor {
    FrameMajor f;                                     // spec = the microphone
    const float2 *far;
};

struct EchoPoolCalls {
    InRing<StreamPoolRows> r;
    int M;                                            // microphones per call
};

// ---- where a pair's frames are: the microphone row / slot, the far-end row / slot, the operator-state slot
struct PairRows {
    RowFrames mic, far;                               // .slot: the ring slot (InRing) or the row (frame-major)
    long out_row, state_slot;
};
__device__ __forceinline__ PairRows pair_of(const EchoFrameMajor &s, long g, int F, StreamCall &c)
{
    const RowFrames r = frames_of(s.f, g, F, c);
    return PairRows{r, r, g, g};
}
__device__ __forceinline__ PairRows pair_of(const InRing<StreamCall> &s, long g, int F, StreamCall &c)
{
    const RowFrames m = frames_of(s, 2 * g, F, c);
    return PairRows{m, RowFrames{2 * g + 1, m.t0, m.t1}, 2 * g, g};
}
__device__ __forceinline__ PairRows pair_of(const EchoPoolCalls &s, long g, int F, StreamCall &c)
{
    const long i = g / s.M, first = i * (s.M + 1), row = first + (g - i * s.M);
    const RowFrames m = frames_of(s.r, row, F, c);
    return PairRows{m, RowFrames{slot_of(s.r.rows, first + s.M), m.t0, m.t1}, row, group_slot_of(s.r, i, s.M + 1) * s.M + (g - i * s.M)};
}
__device__ __forceinline__ float2 load_far(const EchoFrameMajor &s, const PairRows &p, const StreamCall &, int F, int bin, int t)
{
    return s.far[(p.far.slot * s.f.T + (t - s.f.first_frame)) * (long)F + bin];
}
__device__ __forceinline__ float2 load_far(const InRing<StreamCall> &s, const PairRows &p, const StreamCall &c, int F, int bin, int t)
{
    return load_frame(s, p.far, c, p.far.slot, F, bin, t);
}
__device__ __forceinline__ float2 load_far(const EchoPoolCalls &s, const PairRows &p, const StreamCall &c, int F, int bin, int t)
{
    return load_frame(s.r, p.far, c, p.far.slot, F, bin, t);
}
__device__ __forceinline__ float2 load_mic(const EchoFrameMajor &s, const PairRows &p, const StreamCall &c, int F, int bin, int t)
{
    return load_frame(s.f, p.mic, c, p.out_row, F, bin, t);
}
__device__ __forceinline__ float2 load_mic(const InRing<StreamCall> &s, const PairRows &p, const StreamCall &c, int F, int bin, int t)
{
    return load_frame(s, p.mic, c, p.out_row, F, bin, t);
}
__device__ __forceinline__ float2 load_mic(const EchoPoolCalls &s, const PairRows &p, const StreamCall &c, int F, int bin, int t)
{
    return load_frame(s.r, p.mic, c, p.out_row, F, bin, t);
}
__device__ __forceinline__ void store_out(const EchoFrameMajor &s, const PairRows &p, const StreamCall &c, int F, int bin, int t, float2 e,
                                          float m)
{
    store_frame(s.f, p.mic, c, p.out_row, F, bin, t, e, m);
}
__device__ __forceinline__ void store_out(const InRing<StreamCall> &s, const PairRows &p, const StreamCall &c, int F, int bin, int t,
                                          float2 e, float m)
{
    store_frame(s, p.mic, c, p.out_row, F, bin, t, e, m);
}

__device__ __forceinline__ void store_out(const EchoPoolCalls &s, const PairRows &p, const StreamCall &c, int F, int bin, int t,
                                          float2 e, float m)
{
    store_frame(s.r, p.mic, c, p.out_row, F, bin, t, e, m);
}

// One frame of one row, as lane j of its group sees it.  y, r_t: the microphone and the far-end value; Pr: row j of P; pos = t mod H.
// Returns e_t.
template <int G>
__device__ __forceinline__ float2 step(float2 y, float2 r_t, float2 (&Pr)[G], EchoLds<G> &l, int j, int pos, const AecConsts &c)
{
#pragma clang fp contract(off)
    const int K = c.K, H = c.D + K;
    // 1: the ring holds R_t too before anything reads it (D = 0: x~_0 is the current frame)
    if (j == 0) l.ring[pos] = r_t;
    __syncthreads();
    // 2: x~_i = ring[(pos - D - i) mod H]; the ring of a fresh row is zero, which is R_t for t < 0
    int first = pos - c.D;
    if (first < 0) first += H;
    float2 pred = make_float2(0.f, 0.f), u = make_float2(0.f, 0.f);
    float r = 0.f;
    int at = first;
#pragma unroll
    for (int i = 0; i < G; ++i) {
        if (i < K) {
            const float2 xi = l.ring[at];
            pred = cfma_conj(xi, l.h[i], pred);                           // + conj(h_i) x~_i
            r = r + fmaf(xi.x, xi.x, xi.y * xi.y);
            u = cfma(Pr[i], xi, u);                                       // lane j: + P_ji x~_i
            at = at == 0 ? H - 1 : at - 1;
        }
    }
    const float2 e = make_float2(y.x - pred.x, y.y - pred.y);            // the sum starts at +0: Y_t - (+0) is Y_t, signed zeros too
    l.u[j] = u;
    __syncthreads();
    // 3
    float q = 0.f;
    at = first;
#pragma unroll 4
    for (int i = 0; i < K; ++i) {
        const float2 xi = l.ring[at], ui = l.u[i];
        q = fmaf(xi.y, ui.y, fmaf(xi.x, ui.x, q));                        // + Re(conj(x~_i) u_i)
        at = at == 0 ? H - 1 : at - 1;
    }
    const float den = c.alpha + q;
    const float2 kj = make_float2(u.x / den, u.y / den);
    l.k[j] = kj;
    __syncthreads();
    // 4: the gate.  A NaN r adapts.  P_jk <- (P_jk - k_j conj(u_k)) / alpha for k <= j; for k > j the conjugate of that statement
    // for (k, j)
    if (!(r <= c.quiet)) {
        const float2 nkj = make_float2(-kj.x, -kj.y);
#pragma unroll
        for (int k = 0; k < G; ++k) {
            if (k < K) {
                float2 v;
                if (k <= j) {
                    v = cfma_conj(nkj, l.u[k], Pr[k]);
                } else {
                    const float2 kk = l.k[k];
                    v = cfma_conj(make_float2(-kk.x, -kk.y), u, make_float2(Pr[k].x, -Pr[k].y));
                }
                v.x = v.x / c.alpha;
                v.y = v.y / c.alpha;
                if (k == j) v.y = 0.f;
                if (k > j) v.y = -v.y;
                Pr[k] = v;
            }
        }
        if (j < K) l.h[j] = cfma_conj(kj, e, l.h[j]);                     // h_j + k_j conj(e)
    }
    return e;
}

template <int G, class Src>
__global__ __launch_bounds__(AEC_THREADS) void aec_stream_kernel(Src src, AecConsts c, float *__restrict__ astate, int F, int tilesF)
{
    constexpr int GROUPS = AEC_THREADS / G;
    __shared__ EchoLds<G> lds[GROUPS];
    const int j = threadIdx.x & (G - 1), grp = threadIdx.x / G;
    const long pair = blockIdx.x / (unsigned)tilesF;
    const int bin = (int)(blockIdx.x - pair * tilesF) * GROUPS + grp;
    const bool live = bin < F;                                   // a group past the last bin walks zeros and stores nothing
    EchoLds<G> &l = lds[grp];
    const int K = c.K, H = c.D + K;

    StreamCall call;
    const PairRows p = pair_of(src, pair, F, call);
    const int t0 = p.mic.t0, t1 = p.mic.t1;
    const long rec = 2L * K * K + 4L * K + 2L * c.D;             // aec_record_floats(K, D)
    float *st = astate + (p.state_slot * F + (live ? bin : 0)) * rec;
    float2 *stP = reinterpret_cast<float2 *>(st), *stH = stP + K * K, *stR = stH + K;

    float2 Pr[G];
    const bool carried = live && t0 != 0;
#pragma unroll
    for (int k = 0; k < G; ++k) {
        Pr[k] = make_float2(0.f, 0.f);
        if (k < K && j < K) Pr[k] = carried ? stP[k * K + j] : make_float2(k == j ? c.p0 : 0.f, 0.f);
    }
    l.h[j] = (carried && j < K) ? stH[j] : make_float2(0.f, 0.f);
    for (int i = j; i < H; i += G) l.ring[i] = carried ? stR[i] : make_float2(0.f, 0.f);
    __syncthreads();                                             // before lane 0 puts the first frame into a cell another lane cleared

    int pos = t0 % H;
    for (int t = t0; t <= t1; ++t) {
        float2 y = make_float2(0.f, 0.f), r = y;
        if (live) {
            y = load_mic(src, p, call, F, bin, t);
            r = load_far(src, p, call, F, bin, t);
        }
        const float2 e = step<G>(y, r, Pr, l, j, pos, c);
        if (live && j == 0) {
#pragma clang fp contract(off)
            store_out(src, p, call, F, bin, t, e, sqrtf(fmaf(e.x, e.x, e.y * e.y)));
        }
        pos = pos + 1 == H ? 0 : pos + 1;
    }
    __syncthreads();                                             // lane 0's last ring cell and every h_j, before other lanes store them

    if (live) {
#pragma unroll
        for (int k = 0; k < G; ++k)
            if (k < K && j < K) stP[k * K + j] = Pr[k];
        if (j < K) stH[j] = l.h[j];
        for (int i = j; i < H; i += G) stR[i] = l.ring[i];
    }
}

inline long aec_tiles(int F, int G) { return ((long)F + AEC_THREADS / G - 1) / (AEC_THREADS / G); }
inline int aec_lanes(int K) { return K <= 8 ? 8 : K <= 16 ? 16 : 32; }

template <class Src>
hipError_t launch(const Src &src, long n_pairs, int F, const AecConsts &c, float *astate, hipStream_t st)
{
    const int G = aec_lanes(c.K);
    const long tiles = aec_tiles(F, G), grid = n_pairs * tiles;
    if (grid > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 g((unsigned)grid), b(AEC_THREADS);
    if (G == 8)
        hipLaunchKernelGGL((aec_stream_kernel<8, Src>), g, b, 0, st, src, c, astate, F, (int)tiles);
    else if (G == 16)
        hipLaunchKernelGGL((aec_stream_kernel<16, Src>), g, b, 0, st, src, c, astate, F, (int)tiles);
    else
        hipLaunchKernelGGL((aec_stream_kernel<32, Src>), g, b, 0, st, src, c, astate, F, (int)tiles);
    return hipGetLastError();
}

}  // namespace

long aec_record_floats(int K, int D) { return 2L * K * K + 4L * K + 2L * D; }

long aec_stream_grid(long n_pairs, int F, int K) { return n_pairs * aec_tiles(F, aec_lanes(K)); }

hipError_t launch_aec_online(const void *mic, const void *far, int n_rows, int T, int F, int first_frame, const AecConsts &c, float *astate,
                             void *spec_out, float *mag_out, int width, int col0, hipStream_t st)
{
    EchoFrameMajor src{FrameMajor{static_cast<const float2 *>(mic), static_cast<float2 *>(spec_out), mag_out, T, width, col0, first_frame},
                       static_cast<const float2 *>(far)};
    return launch(src, n_rows, F, c, astate, st);
}

hipError_t launch_aec_stream(float *state, float *y, int n_streams, const StreamGeom &g, const StreamCall &call, const AecConsts &c,
                             float *astate, hipStream_t st)
{
    if (call.f_last < call.f_first) return hipSuccess;
    InRing<StreamCall> src{state, y, g, call};
    return launch(src, n_streams / 2, g.n_fft / 2 + 1, c, astate, st);
}

// rows: whole calls of `mics` microphones and a far end, mics + 1 rows each (the entry point has checked the table)
hipError_t launch_aec_stream_pool(float *state, float *y, int mics, const StreamGeom &g, const StreamPoolRows &rows, const AecConsts &c,
                                  float *astate, hipStream_t st)
{
    if (mics < 1 || rows.n < mics + 1 || rows.n % (mics + 1)) return hipErrorInvalidValue;
    EchoPoolCalls src{InRing<StreamPoolRows>{state, y, g, rows}, mics};
    return launch(src, (long)(rows.n / (mics + 1)) * mics, g.n_fft / 2 + 1, c, astate, st);
}

}  // namespace adn
