// Multi-reference acoustic echo cancellation for gfx950: the RLS of echo_stream_kernels.hip on the STACKED vector of Q far-end
// channels, one update per frame and (group, bin) row.  Definition: include/adn_call.h, "echo stream multireference"; float64
// restatement: tests/echo_mr_ref.py.  A stereo or surround loudspeaker set reaches the microphone through Q rooms, and one filter of
// N = Q K taps over all Q references models their sum; Q filters run one after the other do not.
//
// State of a (slot, bin) row (adn_aec_mr_state_bytes; REC = 2 N^2 + 4 N + 2 Q D floats, rows [slot][bin] consecutive):
//   P     [s][r] float2   the N x N inverse correlation matrix, element (r, s) at s N + r: lane r's loads are consecutive in r
//   h     [r]    float2   the N taps, r = q K + j: channel-major, the lag ascending
//   hist  [q][i] float2   Q rings of the last far-end frames, frame t of channel q at q H + t mod H, H = D + K
// With Q = 1 this is the record of echo_stream_kernels.hip byte for byte.  A row whose first frame of the call is frame 0 reads none of
// it, and every byte of a row's record is written on store.
//
// Shape of the work: the parent's.  A GROUP of G lanes owns one row, G in {8, 16, 32} the smallest that holds N; lane r holds row r
// of P in registers (G float2), and u, k, h and the Q rings of the group live in LDS (Q (D + K) = Q D + N <= 64 + G float2).  A
// workgroup is 256 threads: 256 / G groups, the same group of the launch for 256 / G consecutive bins, so every group of a workgroup
// walks the same frames and the barriers are uniform.  Per frame:
//   1  lane q < Q puts R_{t,q} into ring q (x~_r = R_{t-D-j,q} is read out of the rings where it lies, no gathered copy);
//      lane r < N puts the ring cell x~_r lies in this frame into the group's cell table                                    barrier
//   2  every lane forms e_t and r (N steps, stacked order, LDS broadcasts); lane r forms u_r                                 barrier
//   3  every lane forms q and den (stacked order); lane r forms k_r                                                         barrier
//   4  unless the row is gated: lane r updates its row of P and h_r.  Lane 0 stores e_t and M_t.
// Three barriers, and the argument that three suffice is the parent's, ring by ring: every ring read of frame t is in steps 2 and 3,
// before the barrier after step 3, and the cell step 1 of frame t + 1 overwrites in ring q is the one x~_{q K + K - 1} of frame t lay
// in; step 4 reads u and k only and writes h_r and registers only.  Q <= N <= G, so the Q loads of step 1 are one load per lane.
// No value crosses lanes through a reduction: every lane computes e, r, q and den itself, in stacked order, so nothing depends on G
// or on neighbours.  Where x~_r lies -- ring q = r / K, cell (t - D - j) mod H -- is not walked in the loops of steps 2 and 3: a
// scalar walk with the channel boundary and the wrap in it cost 10 ... 24 % over the parent's kernel at equal N
// (profiles/bench_echo_mr.md).  Lane r knows its own (q, j) once per call, forms its cell in two integer operations per frame and
// writes it into cell[r] beside its ring write, before the first barrier; the loops read cell[i] at a compile-time offset and then
// the ring at that cell, both broadcasts of one address per group.  The table is rewritten in step 1 of frame t + 1, after the
// barrier that ends the ring reads of frame t, so the three barriers hold it as they hold the rings.
//
// Where the frames come from is the template argument, and a pool source can be added beside these two as EchoPoolCalls stands
// beside InRing<StreamCall> in the parent:
//   MrFrameMajor          mic / spec_out [row][frame][F] float2, far [row][q][frame][F], mag_out [row][F][width] at col0
//   MrRing                group g is streams g (Q + 1) (microphone) and g (Q + 1) + 1 + q (far end q) of an adn_stream_* state: all
//                         Q + 1 X rings are read for frames f_first .. f_last, e_t goes into the microphone's ring cells, M_t into
//                         columns [W - B, W) of window row g (Q + 1) of y; nothing of a far-end stream is written.  State slot g.
// The step is one function, compiled with fp contraction off, every multiply-add an explicit fmaf.
//
// Cost (derived): per row-frame 8 N^2 + 12 N fp32 FMAs, the parent's at K = N; the state is 8 N^2 + 16 N + 8 Q D bytes per row read
// and written per call.  No atomics, no workspace, no constant table.
#include "echo_mr.h"
#include "../wpe_stream_frames.h"

namespace adn {
namespace {

constexpr int MR_THREADS = 256;

// The LDS of one group: Q D + N <= 8 * 8 + G cells of rings
template <int G>
struct MrLds {
    float2 ring[64 + G];
    float2 u[G], k[G], h[G];
    int cell[G];                                      // cell[r]: where x~_r lies in `ring` this frame
};

struct MrFrameMajor {
    FrameMajor f;                                     // spec = the microphone
    const float2 *far;                                // [row][q][frame][F]
    int Q;
};

struct MrRing {
    InRing<StreamCall> r;
    int Q;
};

// ---- where a group's frames are: the microphone row / slot, the first far-end row / slot, the window row, the operator-state slot
struct GroupRows {
    RowFrames mic;
    long far0, out_row, state_slot;
};
__device__ __forceinline__ GroupRows group_of(const MrFrameMajor &s, long g, int F, StreamCall &c)
{
    return GroupRows{frames_of(s.f, g, F, c), g * s.Q, g, g};
}
__device__ __forceinline__ GroupRows group_of(const MrRing &s, long g, int F, StreamCall &c)
{
    const long first = g * (s.Q + 1);
    return GroupRows{frames_of(s.r, first, F, c), first + 1, first, g};
}
__device__ __forceinline__ float2 load_mic(const MrFrameMajor &s, const GroupRows &p, const StreamCall &c, int F, int bin, int t)
{
    return load_frame(s.f, p.mic, c, p.out_row, F, bin, t);
}
__device__ __forceinline__ float2 load_mic(const MrRing &s, const GroupRows &p, const StreamCall &c, int F, int bin, int t)
{
    return load_frame(s.r, p.mic, c, p.out_row, F, bin, t);
}
__device__ __forceinline__ float2 load_far(const MrFrameMajor &s, const GroupRows &p, const StreamCall &, int F, int bin, int t, int q)
{
    return s.far[((p.far0 + q) * s.f.T + (t - s.f.first_frame)) * (long)F + bin];
}
__device__ __forceinline__ float2 load_far(const MrRing &s, const GroupRows &p, const StreamCall &c, int F, int bin, int t, int q)
{
    return load_frame(s.r, RowFrames{p.far0 + q, p.mic.t0, p.mic.t1}, c, p.far0 + q, F, bin, t);
}
__device__ __forceinline__ void store_out(const MrFrameMajor &s, const GroupRows &p, const StreamCall &c, int F, int bin, int t, float2 e,
                                          float m)
{
    store_frame(s.f, p.mic, c, p.out_row, F, bin, t, e, m);
}
__device__ __forceinline__ void store_out(const MrRing &s, const GroupRows &p, const StreamCall &c, int F, int bin, int t, float2 e, float m)
{
    store_frame(s.r, p.mic, c, p.out_row, F, bin, t, e, m);
}

// One frame of one row, as lane j of its group sees it.  y: the microphone value; r_t: far-end channel j's value (lanes j < Q); Pr:
// row j of P; pos = t mod H; ring0, lag: the first cell of the ring x~_j lies in, (j / K) H, and its lag j % K.  Returns e_t.
template <int G>
__device__ __forceinline__ float2 step(float2 y, float2 r_t, float2 (&Pr)[G], MrLds<G> &l, int j, int pos, int ring0, int lag,
                                       const AecMrConsts &c)
{
#pragma clang fp contract(off)
    const int K = c.K, H = c.D + K, N = c.Q * K;
    // 1: the rings hold R_t too before anything reads them (D = 0: x~_{q K} is the current frame of channel q); x~_j = R_{t-D-lag}
    // lies at (pos - D - lag) mod H of its ring, and pos - D - lag > -H
    if (j < c.Q) l.ring[j * H + pos] = r_t;
    int at = pos - c.D - lag;
    if (at < 0) at += H;
    l.cell[j] = ring0 + at;                                               // lanes j >= N: never read
    __syncthreads();
    // 2: the rings of a fresh row are zero, which is R_t for t < 0
    float2 pred = make_float2(0.f, 0.f), u = make_float2(0.f, 0.f);
    float r = 0.f;
#pragma unroll
    for (int i = 0; i < G; ++i) {
        if (i < N) {
            const float2 xi = l.ring[l.cell[i]];
            pred = cfma_conj(xi, l.h[i], pred);                           // + conj(h_i) x~_i
            r = r + fmaf(xi.x, xi.x, xi.y * xi.y);
            u = cfma(Pr[i], xi, u);                                       // lane j: + P_ji x~_i
        }
    }
    const float2 e = make_float2(y.x - pred.x, y.y - pred.y);            // the sum starts at +0: Y_t - (+0) is Y_t, signed zeros too
    l.u[j] = u;
    __syncthreads();
    // 3
    float q = 0.f;
#pragma unroll 4
    for (int i = 0; i < N; ++i) {
        const float2 xi = l.ring[l.cell[i]], ui = l.u[i];
        q = fmaf(xi.y, ui.y, fmaf(xi.x, ui.x, q));                        // + Re(conj(x~_i) u_i)
    }
    const float den = c.alpha + q;
    const float2 kj = make_float2(u.x / den, u.y / den);
    l.k[j] = kj;
    __syncthreads();
    // 4: the gate, on the stacked power of all channels.  A NaN r adapts.  P_jk <- (P_jk - k_j conj(u_k)) / alpha for k <= j; for
    // k > j the conjugate of that statement for (k, j)
    if (!(r <= c.quiet)) {
        const float2 nkj = make_float2(-kj.x, -kj.y);
#pragma unroll
        for (int k = 0; k < G; ++k) {
            if (k < N) {
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
        if (j < N) l.h[j] = cfma_conj(kj, e, l.h[j]);                     // h_j + k_j conj(e)
    }
    return e;
}

// The occupancy the parent's kernel has at the same G (6, 5 and 4 waves per SIMD: 80, 96 and 128 VGPRs) is asked for by name: left
// alone, the compiler keeps the cell table's reads in flight over a few registers more and loses a wave at every G.
template <int G, class Src>
__global__ __launch_bounds__(MR_THREADS) __attribute__((amdgpu_waves_per_eu(G == 8 ? 6 : G == 16 ? 5 : 4)))
void aec_mr_kernel(Src src, AecMrConsts c, float *__restrict__ astate, int F, int tilesF)
{
    constexpr int GROUPS = MR_THREADS / G;
    __shared__ MrLds<G> lds[GROUPS];
    const int j = threadIdx.x & (G - 1), grp = threadIdx.x / G;
    const long group = blockIdx.x / (unsigned)tilesF;
    const int bin = (int)(blockIdx.x - group * tilesF) * GROUPS + grp;
    const bool live = bin < F;                                   // a group past the last bin walks zeros and stores nothing
    MrLds<G> &l = lds[grp];
    const int K = c.K, H = c.D + K, N = c.Q * K, cells = c.Q * H;

    StreamCall call;
    const GroupRows p = group_of(src, group, F, call);
    const int t0 = p.mic.t0, t1 = p.mic.t1;
    const long rec = 2L * N * N + 4L * N + 2L * c.Q * c.D;       // aec_mr_record_floats(Q, K, D)
    float *st = astate + (p.state_slot * F + (live ? bin : 0)) * rec;
    float2 *stP = reinterpret_cast<float2 *>(st), *stH = stP + N * N, *stR = stH + N;

    float2 Pr[G];
    const bool carried = live && t0 != 0;
#pragma unroll
    for (int k = 0; k < G; ++k) {
        Pr[k] = make_float2(0.f, 0.f);
        if (k < N && j < N) Pr[k] = carried ? stP[k * N + j] : make_float2(k == j ? c.p0 : 0.f, 0.f);
    }
    l.h[j] = (carried && j < N) ? stH[j] : make_float2(0.f, 0.f);
    for (int i = j; i < cells; i += G) l.ring[i] = carried ? stR[i] : make_float2(0.f, 0.f);
    __syncthreads();                                             // before lane q puts the first frame into a cell another lane cleared

    // lane j's place in the stack: j = q K + lag.  A lane past the stack (j >= N) gets a cell nobody reads; its ring0 is kept
    // inside the rings so that the table never holds an index outside them.
    const int jq = j < N ? j / K : 0, lag = j - jq * K < K ? j - jq * K : 0, ring0 = jq * H;
    int pos = t0 % H;
    for (int t = t0; t <= t1; ++t) {
        float2 y = make_float2(0.f, 0.f), r = y;
        if (live) {
            y = load_mic(src, p, call, F, bin, t);
            if (j < c.Q) r = load_far(src, p, call, F, bin, t, j);
        }
        const float2 e = step<G>(y, r, Pr, l, j, pos, ring0, lag, c);
        if (live && j == 0) {
#pragma clang fp contract(off)
            store_out(src, p, call, F, bin, t, e, sqrtf(fmaf(e.x, e.x, e.y * e.y)));
        }
        pos = pos + 1 == H ? 0 : pos + 1;
    }
    __syncthreads();                                             // the last ring cells and every h_j, before other lanes store them

    if (live) {
#pragma unroll
        for (int k = 0; k < G; ++k)
            if (k < N && j < N) stP[k * N + j] = Pr[k];
        if (j < N) stH[j] = l.h[j];
        for (int i = j; i < cells; i += G) stR[i] = l.ring[i];
    }
}

inline long mr_tiles(int F, int G) { return ((long)F + MR_THREADS / G - 1) / (MR_THREADS / G); }
inline int mr_lanes(int N) { return N <= 8 ? 8 : N <= 16 ? 16 : 32; }

template <class Src>
hipError_t launch(const Src &src, long n_groups, int F, const AecMrConsts &c, float *astate, hipStream_t st)
{
    const int N = c.Q * c.K;
    if (c.Q < 1 || c.Q > 8 || c.K < 1 || N > 32 || c.D < 0 || c.D > 8) return hipErrorInvalidValue;   // the LDS of a group holds no more
    const int G = mr_lanes(N);
    const long tiles = mr_tiles(F, G), grid = n_groups * tiles;
    if (grid > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 g((unsigned)grid), b(MR_THREADS);
    if (G == 8)
        hipLaunchKernelGGL((aec_mr_kernel<8, Src>), g, b, 0, st, src, c, astate, F, (int)tiles);
    else if (G == 16)
        hipLaunchKernelGGL((aec_mr_kernel<16, Src>), g, b, 0, st, src, c, astate, F, (int)tiles);
    else
        hipLaunchKernelGGL((aec_mr_kernel<32, Src>), g, b, 0, st, src, c, astate, F, (int)tiles);
    return hipGetLastError();
}

}  // namespace

long aec_mr_record_floats(int Q, int K, int D)
{
    const long N = (long)Q * K;
    return 2L * N * N + 4L * N + 2L * Q * D;
}

long aec_mr_grid(long n_groups, int F, int N) { return n_groups * mr_tiles(F, mr_lanes(N)); }

hipError_t launch_aec_mr_online(const void *mic, const void *far, int n_rows, int T, int F, int first_frame, const AecMrConsts &c,
                                float *astate, void *spec_out, float *mag_out, int width, int col0, hipStream_t st)
{
    MrFrameMajor src{FrameMajor{static_cast<const float2 *>(mic), static_cast<float2 *>(spec_out), mag_out, T, width, col0, first_frame},
                     static_cast<const float2 *>(far), c.Q};
    return launch(src, n_rows, F, c, astate, st);
}

hipError_t launch_aec_mr_stream(float *state, float *y, int n_streams, const StreamGeom &g, const StreamCall &call, const AecMrConsts &c,
                                float *astate, hipStream_t st)
{
    if (call.f_last < call.f_first) return hipSuccess;
    if (n_streams < c.Q + 1 || n_streams % (c.Q + 1)) return hipErrorInvalidValue;
    MrRing src{InRing<StreamCall>{state, y, g, call}, c.Q};
    return launch(src, n_streams / (c.Q + 1), g.n_fft / 2 + 1, c, astate, st);
}

}  // namespace adn
