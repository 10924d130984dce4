// Streaming dereverberation for gfx950: recursive (RLS) WPE, one update per frame and (slot, bin) row.
// Definition: include/adn.h, "dereverb stream"; float64 restatement: tests/dereverb_stream_ref.py.
//
// State of a (slot, bin) row (adn_wpe_stream_state_bytes; REC = 2 K^2 + 4 K + 2 D + 2 floats, rows [slot][bin] consecutive):
//   P     [k][j] float2   the K x K inverse correlation matrix, element (j, k) at k K + j: lane j's loads are consecutive in j
//   g     [j]    float2   the K taps
//   hist  [h]    float2   the last raw frames, frame t at t mod H, H = D + K
//   s     1 float (+ 1 pad)
// A row whose first frame of the call is frame 0 reads none of it.
//
// Shape of the work.  A row is a recurrence over its frames, rows are independent.  A GROUP of 32 lanes owns one row: lane j holds
// row j of P in registers (up to 32 float2), and x~, u, k, g and the history ring of the group live in LDS.  A workgroup is 8
// groups, the same row of the launch for 8 consecutive bins, so every group of a workgroup walks the same frames and the barriers
// are uniform.  Per frame:
//   1  lane k gathers x~_k = X_{t-D-k} out of the ring                                    barrier
//   2  every lane forms e_t (K steps, tap order, LDS broadcasts); lane j forms u_j        barrier
//   3  every lane forms q and den (tap order); lane j forms k_j                           barrier
//   4  lane j updates its row of P and g_j; lane 0 stores d_t, M_t and X_t into the ring  barrier
// No value crosses lanes through a reduction: every lane computes e, q and den itself, in tap order, so nothing depends on the
// lane count or on neighbours.  Lane j computes P_jk for k <= j as written in adn.h and takes its k > j entries as the conjugate
// of the SAME statement evaluated for (k, j) on conj(P_jk) -- the old P is exactly Hermitian, so this is bit for bit what lane k
// computes for P_kj, and P stays exactly Hermitian with no exchange.  With K < 32 the lanes j >= K idle (K = 20: 12 of 32).
// The state is loaded once per call and stored once; lanes past the last bin load nothing and store nothing.
//
// Where the frames come from is the template argument (the pattern of stream_kernels.hip and baseline_kernels.hip):
//   FrameMajor            spec / spec_out [row][frame][F] float2, mag_out [row][F][width] at col0; the call continues at first_frame
//   InRing<StreamCall>    the X ring of an adn_stream_* state, frames f_first .. f_last of the call, in place; M_t into columns
//                         [W - B, W) of the windows buffer.  Row = slot = stream.
//   InRing<StreamPoolRows> the same for a table of (slot, step, final_length) rows, one step each.
// The step itself is one function, compiled with fp contraction off, every multiply-add an explicit fmaf: its arithmetic is the
// statements as written whichever instantiation inlines it, so a pooled stream equals a lockstep one bit for bit.
//
// Cost (derived; what was measured is in profiles/bench_dereverb_stream.md): per row-frame 4 K^2 FMAs for u, 2 K (K + 1) for the
// update, 8 K for e and g -- 2.6 k at K = 20, against 257 x 62.5 row-frames a second for one 8 kHz feed: negligible.  The state is
// 8 K^2 + 16 K + 8 D + 8 bytes per row read and written (3.5 KB at the defaults, 0.9 MB per feed and direction).  Measured on the
// MI355X, those bytes do not bind: a step of four frames is 32 us for one feed and 334 us for 256 feeds, 0.17 of the byte bound.
// What binds is the per-frame chain of one workgroup, 8 us: 2 K correctly rounded divisions by alpha per lane (the definition
// divides), both sides of the divergent k <= j branch, three passes of K LDS broadcasts, four barriers.  No atomics, no
// workspace, no constant table.
#include "wpe_stream_frames.h"                        // the frame sources: shared with dereverb_mc_stream_kernels.hip

#include <type_traits>

namespace adn {
namespace {

// The LDS of one group
struct GroupLds {
    float2 ring[WS_HMAX];
    float2 xt[WS_G], u[WS_G], k[WS_G], g[WS_G];
};

// One frame of one row, as lane j of its group sees it.  Pr: row j of P.  Returns e_t; `s` is the running power.
__device__ __forceinline__ float2 step(float2 x, bool first, float &s, float2 (&Pr)[WS_G], GroupLds &l, int j, int pos,
                                       const WpeStreamConsts &c)
{
#pragma clang fp contract(off)
    const int K = c.K;
    // 1: x~_k = X_{t-D-k}; the ring of a fresh row is zero, which is X_t for t < 0
    if (j < K) {
        int at = pos - c.D - j;
        if (at < 0) at += c.D + K;
        l.xt[j] = l.ring[at];
    }
    __syncthreads();
    // 2
    const float p = fmaf(x.x, x.x, x.y * x.y);
    s = first ? p : c.beta * s + c.one_minus_beta * p;
    const float phi = max_keep_nan(c.rho * s, 1e-30f);
    float2 pred = make_float2(0.f, 0.f);
#pragma unroll 4
    for (int i = 0; i < K; ++i) pred = cfma_conj(l.xt[i], l.g[i], pred);  // + conj(g_i) x~_i
    const float2 e = make_float2(x.x - pred.x, x.y - pred.y);            // the sum starts at +0: X_t - (+0) is X_t, signed zeros too
    float2 u = make_float2(0.f, 0.f);
#pragma unroll
    for (int k = 0; k < WS_G; ++k)
        if (k < K) u = cfma(Pr[k], l.xt[k], u);
    l.u[j] = u;
    __syncthreads();
    // 3
    const float lam = max_keep_nan(fmaf(e.x, e.x, e.y * e.y), phi);
    float q = 0.f;
#pragma unroll 4
    for (int i = 0; i < K; ++i) {
        const float2 xi = l.xt[i], ui = l.u[i];
        q = fmaf(xi.y, ui.y, fmaf(xi.x, ui.x, q));                        // + Re(conj(x~_i) u_i)
    }
    const float den = c.alpha * lam + q;
    const float2 kj = make_float2(u.x / den, u.y / den);
    l.k[j] = kj;
    __syncthreads();
    // 4: P_jk <- (P_jk - k_j conj(u_k)) / alpha for k <= j; for k > j the conjugate of that statement for (k, j)
    const float2 nkj = make_float2(-kj.x, -kj.y);
#pragma unroll
    for (int k = 0; k < WS_G; ++k) {
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
    if (j < K) l.g[j] = cfma_conj(kj, e, l.g[j]);                         // g_j + k_j conj(e)
    if (j == 0) l.ring[pos] = x;
    __syncthreads();
    return e;
}

template <class Src>
__global__ __launch_bounds__(WS_G * WS_GROUPS) void wpe_stream_kernel(Src src, WpeStreamConsts c, float *__restrict__ wstate, int F,
                                                                     int groupsF)
{
    __shared__ GroupLds lds[WS_GROUPS];
    const int j = threadIdx.x & (WS_G - 1), grp = threadIdx.x / WS_G;
    const long row = blockIdx.x / (unsigned)groupsF;
    const int bin = (int)(blockIdx.x - row * groupsF) * WS_GROUPS + grp;
    const bool live = bin < F;                                   // a group past the last bin walks zeros and stores nothing
    GroupLds &l = lds[grp];
    const int K = c.K, H = c.D + K;

    StreamCall call;
    const RowFrames r = frames_of(src, row, F, call);
    const bool fresh = r.t0 == 0;
    const long rec = 2L * K * K + 4L * K + 2L * c.D + 2;         // wpe_stream_record_floats(1, K, D)
    float *st = wstate + (r.slot * F + (live ? bin : 0)) * rec;
    float2 *stP = reinterpret_cast<float2 *>(st), *stG = stP + K * K, *stH = stG + K;
    float *stS = reinterpret_cast<float *>(stH + H);

    float2 Pr[WS_G];
    float s = 0.f;
    const bool carried = live && !fresh;
#pragma unroll
    for (int k = 0; k < WS_G; ++k) {
        Pr[k] = make_float2(0.f, 0.f);
        if (k < K && j < K) Pr[k] = carried ? stP[k * K + j] : make_float2(k == j ? c.p0 : 0.f, 0.f);
    }
    l.g[j] = (carried && j < K) ? stG[j] : make_float2(0.f, 0.f);
    for (int h = j; h < H; h += WS_G) l.ring[h] = carried ? stH[h] : make_float2(0.f, 0.f);
    if (carried) s = stS[0];
    __syncthreads();

    int pos = r.t0 % H;
    for (int t = r.t0; t <= r.t1; ++t) {
        const float2 x = live ? load_frame(src, r, call, row, F, bin, t) : make_float2(0.f, 0.f);
        const float2 e = step(x, t == 0, s, Pr, l, j, pos, c);
        if (live && j == 0) {
#pragma clang fp contract(off)
            store_frame(src, r, call, row, F, bin, t, e, sqrtf(fmaf(e.x, e.x, e.y * e.y)));
        }
        pos = pos + 1 == H ? 0 : pos + 1;
    }

    if (live) {
        store_P_row(Pr, stP, j, K);
        if (j < K) stG[j] = l.g[j];
        for (int h = j; h < H; h += WS_G) stH[h] = l.ring[h];
        if (j == 0) {
            stS[0] = s;
            stS[1] = 0.f;                                        // the pad: every byte of a row's record is written
        }
    }
}

template <class Src>
hipError_t launch(const Src &src, long n_rows, int F, const WpeStreamConsts &c, float *wstate, hipStream_t st)
{
    const long groupsF = ws_tiles(F), grid = wpe_stream_grid(n_rows, F);
    if (grid > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wpe_stream_kernel<Src>, dim3((unsigned)grid), dim3(WS_G * WS_GROUPS), 0, st, src, c, wstate, F, (int)groupsF);
    return hipGetLastError();
}

}  // namespace

long wpe_stream_grid(long n_rows, int F) { return n_rows * ws_tiles(F); }

hipError_t launch_wpe_online_1ch(const void *spec, int n_rows, int T, int F, int first_frame, const WpeStreamConsts &c, float *wstate,
                                 void *spec_out, float *mag_out, int width, int col0, hipStream_t st)
{
    FrameMajor src{static_cast<const float2 *>(spec), static_cast<float2 *>(spec_out), mag_out, T, width, col0, first_frame};
    return launch(src, n_rows, F, c, wstate, st);
}

hipError_t launch_wpe_stream_1ch(float *state, float *y, int n_streams, const StreamGeom &g, const StreamCall &call,
                                 const WpeStreamConsts &c, float *wstate, hipStream_t st)
{
    if (call.f_last < call.f_first) return hipSuccess;
    InRing<StreamCall> src{state, y, g, call};
    return launch(src, n_streams, g.n_fft / 2 + 1, c, wstate, st);
}

// the pool's rows are single-channel streams: C is fixed at 1 here (a pool of recordings is launch_wpe_mc_stream_pool of
// dereverb_mc_stream_kernels.hip on the same source)
hipError_t launch_wpe_stream_pool(float *state, float *y, const StreamGeom &g, const StreamPoolRows &rows, const WpeStreamConsts &c,
                                  float *wstate, hipStream_t st)
{
    InRing<StreamPoolRows> src{state, y, g, rows};
    return launch(src, rows.n, g.n_fft / 2 + 1, c, wstate, st);
}

}  // namespace adn
