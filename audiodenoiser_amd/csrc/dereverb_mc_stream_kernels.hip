// Streaming multichannel dereverberation for gfx950: recursive (RLS) joint WPE of the C channels of a recording, one update per
// frame and (group, bin).  Definition: include/adn.h, "dereverb stream multichannel"; float64 restatement:
// tests/dereverb_mc_stream_ref.py.  C = 1 runs the kernel of dereverb_stream_kernels.hip: the launchers at the end choose.
//
// State of a (slot, bin) (adn_wpe_mc_stream_state_bytes; REC = 2 N^2 + 2 N C + 2 C (D + K) + 2 floats, N = C K, records [slot][bin]
// consecutive; at C = 1 this is the single-channel record):
//   P     [s][r] float2   the N x N inverse correlation matrix, element (r, s) at s N + r: lane r's loads are consecutive in r
//   G     [c][r] float2   the N x C taps, column c (the filter that predicts channel c) at c N
//   hist  [c][h] float2   the last raw frames of channel c, frame t at t mod H, H = D + K
//   s     1 float (+ 1 pad)
// A group whose first frame of the call is frame 0 reads none of it.
//
// Shape of the work: that of the single-channel kernel.  A GROUP of 32 lanes owns one (group of channels, bin): lane r holds row r
// of P in registers (up to 32 float2 = 64 VGPRs), and x~, u, k, G, the C rings, the C inputs and the C errors live in LDS (3.7 KB
// per group, whatever (C, K)).  A workgroup is 8 groups, 8 consecutive bins of the same recording, so every group of a workgroup
// walks the same frames and the barriers are uniform.  Per frame:
//   1  lane r gathers x~_r = X_{t-D-j, c}, r = c K + j, out of ring c; lane c < C posts X_{t,c}                barrier
//   2  lane r forms u_r; lane c < C forms e_c = X_{t,c} - sum_r conj(G_rc) x~_r and posts it                   barrier
//   3  every lane forms p, s, phi, lam (channel order), q and den (r order); lane r forms k_r                  barrier
//   4  lane r updates its row of P and row r of G (C entries); lane c < C stores d, M and X_{t,c} into ring c  barrier
// No value crosses lanes through a reduction: every sum the definition orders is formed by ONE lane in that order.  The Hermitian
// update is the single-channel kernel's: lane r computes P_rs for s <= r as written and takes s > r as the conjugate of the same
// statement evaluated for (s, r) on conj(P_rs), bit for bit what lane s computes, so P stays exactly Hermitian with no exchange.
//
// How the C errors are formed, and why.  Two ways were open.  (a) Every lane forms all C errors itself: no lane waits for another,
// but each lane pays C N complex FMAs a frame -- 256 at (8, 4), 64 at (2, 16) -- in front of the 32 of its row of u, and the
// parent measured that exactly this per-frame dependent chain is the kernel's time.  (b) Lane c forms e_c alone, in r order, and
// posts it in LDS.  Chosen: (b).  The errors are not needed before lam_t, and lam_t already waits behind the barrier that
// publishes u (q needs every u_r), so the broadcast rides on a barrier the frame has anyway: the "one more barrier" of the naive
// form of (b) is not paid.  The cost is the divergence inside the half-wave: lanes c < C run N FMAs for e_c beside the N of u_r,
// so the chain of stage 2 is 2 N FMAs whatever C is, against (C + 1) N for (a).  G is stored column-major with a pitch of 33
// cells, so that the C lanes reading G_ic for the same i hit C different banks, and lane r's update of G_rc is conflict-free.
//
// Where the frames come from is the template argument, the parent's pattern and the parent's structs (wpe_stream_frames.h):
//   FrameMajor            spec / spec_out [group C + c][frame][F] float2, mag_out [group C + c][F][width] at col0
//   InRing<StreamCall>    the X rings of an adn_stream_* state whose streams g C ... g C + C - 1 are group g, in place; M_t into
//                         columns [W - B, W) of each channel's windows.  Slot = group.
//   InRing<StreamPoolRows> the same for a table of (slot, step, final_length) rows, C consecutive rows a recording: channel c of
//                         group g is ring slot rows[g C + c].slot, the state slot is rows[g C].slot / C, the windows of y are row
//                         g C + c.  The entry point has checked that a group's slots are r C ... r C + C - 1 in this order and
//                         that its rows agree in step and final_length, so the frames of the first row are every channel's.
// A channel of a group is a row of those structs, so a joint stream and C single-channel ones address the same cells.  The step
// is one function, compiled with fp contraction off, every multiply-add an explicit fmaf: a lockstep stream equals
// adn_wpe_mc_online on the same spectrogram bit for bit.
//
// Cost (derived; what was measured is in profiles/bench_dereverb_mc_stream.md): per frame 4 N^2 FMAs for u, 2 N (N + 1) for P,
// 4 N C for e and as many for G, and per lane the chain N (u) + N (e, lanes c < C) + N (q) + 2 N (both sides of the s <= r branch)
// + C (G) FMAs, 2 N + 2 divisions, four barriers: at N = 32 1.6 times the single-channel chain at K = 20.  No atomics, no
// workspace, no constant table.
#include "wpe_stream_frames.h"

namespace adn {
namespace {

constexpr int MS_CMAX = 8;                           // channels at most
constexpr int MS_RING = 96;                          // C (D + K) = C D + N <= 8 x 8 + 32 cells
constexpr int MS_GP = WS_G + 1;                      // pitch of a column of G in LDS

// The LDS of one group
struct McGroupLds {
    float2 ring[MS_RING];                            // channel c's ring at c H
    float2 xt[WS_G], u[WS_G], k[WS_G];
    float2 G[MS_CMAX * MS_GP];                       // G_rc at c MS_GP + r
    float2 x[MS_CMAX], e[MS_CMAX];
};

// One frame of one group, as lane r sees it.  Pr: row r of P.  x: X_{t,r} for r < C.  Returns e_r for r < C; `s` is the running
// power, the same in every lane.
__device__ __forceinline__ float2 mc_step(float2 x, bool first, float &s, float2 (&Pr)[WS_G], McGroupLds &l, int r, int pos, int C,
                                          float fC, const WpeStreamConsts &c)
{
#pragma clang fp contract(off)
    const int K = c.K, N = C * K, H = c.D + K;
    // 1: x~_r = X_{t-D-j, ch}; the rings of a fresh group are zero, which is X_t for t < 0
    if (r < N) {
        const int ch = r / K, j = r - ch * K;
        int at = pos - c.D - j;
        if (at < 0) at += H;
        l.xt[r] = l.ring[ch * H + at];
    }
    if (r < C) l.x[r] = x;
    __syncthreads();
    // 2
    float2 u = make_float2(0.f, 0.f);
#pragma unroll
    for (int k = 0; k < WS_G; ++k)
        if (k < N) u = cfma(Pr[k], l.xt[k], u);
    l.u[r] = u;
    float2 e = make_float2(0.f, 0.f);
    if (r < C) {
        const float2 *Gc = l.G + r * MS_GP;
        float2 pred = make_float2(0.f, 0.f);
#pragma unroll 4
        for (int i = 0; i < N; ++i) pred = cfma_conj(l.xt[i], Gc[i], pred);  // + conj(G_ic) x~_i
        e = make_float2(x.x - pred.x, x.y - pred.y);                        // the sum starts at +0: the first D frames are X_t itself
        l.e[r] = e;
    }
    __syncthreads();
    // 3
    float p = 0.f, ee = 0.f;
    for (int ch = 0; ch < C; ++ch) {
        const float2 xc = l.x[ch], ec = l.e[ch];
        p = p + fmaf(xc.x, xc.x, xc.y * xc.y);
        ee = ee + fmaf(ec.x, ec.x, ec.y * ec.y);
    }
    p = p / fC;
    s = first ? p : c.beta * s + c.one_minus_beta * p;
    const float phi = max_keep_nan(c.rho * s, 1e-30f);
    const float lam = max_keep_nan(ee / fC, phi);
    float q = 0.f;
#pragma unroll 4
    for (int i = 0; i < N; ++i) {
        const float2 xi = l.xt[i], ui = l.u[i];
        q = fmaf(xi.y, ui.y, fmaf(xi.x, ui.x, q));                          // + Re(conj(x~_i) u_i)
    }
    const float den = c.alpha * lam + q;
    const float2 kr = make_float2(u.x / den, u.y / den);
    l.k[r] = kr;
    __syncthreads();
    // 4: P_rs <- (P_rs - k_r conj(u_s)) / alpha for s <= r; for s > r the conjugate of that statement for (s, r)
    const float2 nkr = make_float2(-kr.x, -kr.y);
#pragma unroll
    for (int k = 0; k < WS_G; ++k) {
        if (k < N) {
            float2 v;
            if (k <= r) {
                v = cfma_conj(nkr, l.u[k], Pr[k]);
            } else {
                const float2 kk = l.k[k];
                v = cfma_conj(make_float2(-kk.x, -kk.y), u, make_float2(Pr[k].x, -Pr[k].y));
            }
            v.x = v.x / c.alpha;
            v.y = v.y / c.alpha;
            if (k == r) v.y = 0.f;
            if (k > r) v.y = -v.y;
            Pr[k] = v;
        }
    }
    if (r < N)
        for (int ch = 0; ch < C; ++ch) l.G[ch * MS_GP + r] = cfma_conj(kr, l.e[ch], l.G[ch * MS_GP + r]);    // G_rc + k_r conj(e_c)
    if (r < C) l.ring[r * H + pos] = x;
    __syncthreads();
    return e;
}

template <class Src>
__global__ __launch_bounds__(WS_G * WS_GROUPS) void wpe_mc_stream_kernel(Src src, WpeStreamConsts c, int C, float *__restrict__ wstate,
                                                                        int F, int groupsF)
{
    __shared__ McGroupLds lds[WS_GROUPS];
    const int r = threadIdx.x & (WS_G - 1), grp = threadIdx.x / WS_G;
    const long g = blockIdx.x / (unsigned)groupsF;
    const int bin = (int)(blockIdx.x - g * groupsF) * WS_GROUPS + grp;
    const bool live = bin < F;                                   // a group past the last bin walks zeros and stores nothing
    McGroupLds &l = lds[grp];
    const int K = c.K, N = C * K, H = c.D + K;

    // every channel of a group covers the same frames: those of its first one.  Lane r < C speaks for channel r, row g C + r of
    // the frame source; where its ring slot and the group's state slot are is the source's to say (wpe_stream_frames.h).
    StreamCall call;
    const RowFrames r0 = frames_of(src, g * C, F, call);
    const long chan = g * C + (r < C ? r : 0);
    const RowFrames rc{chan_slot_of(src, chan), r0.t0, r0.t1};
    const bool mine = live && r < C;
    const bool fresh = r0.t0 == 0;
    const long rec = 2L * N * N + 2L * N * C + 2L * C * H + 2;   // wpe_stream_record_floats(C, K, D)
    float *st = wstate + (group_slot_of(src, g, C) * F + (live ? bin : 0)) * rec;
    float2 *stP = reinterpret_cast<float2 *>(st), *stG = stP + N * N, *stH = stG + N * C;
    float *stS = reinterpret_cast<float *>(stH + C * H);

    float2 Pr[WS_G];
    float s = 0.f;
    const bool carried = live && !fresh;
#pragma unroll
    for (int k = 0; k < WS_G; ++k) {
        Pr[k] = make_float2(0.f, 0.f);
        if (k < N && r < N) Pr[k] = carried ? stP[k * N + r] : make_float2(k == r ? c.p0 : 0.f, 0.f);
    }
    for (int ch = 0; ch < C; ++ch) l.G[ch * MS_GP + r] = (carried && r < N) ? stG[ch * N + r] : make_float2(0.f, 0.f);
    for (int h = r; h < C * H; h += WS_G) l.ring[h] = carried ? stH[h] : make_float2(0.f, 0.f);
    if (carried) s = stS[0];
    __syncthreads();

    const float fC = (float)C;
    int pos = r0.t0 % H;
    for (int t = r0.t0; t <= r0.t1; ++t) {
        const float2 x = mine ? load_frame(src, rc, call, chan, F, bin, t) : make_float2(0.f, 0.f);
        const float2 e = mc_step(x, t == 0, s, Pr, l, r, pos, C, fC, c);
        if (mine) {
#pragma clang fp contract(off)
            store_frame(src, rc, call, chan, F, bin, t, e, sqrtf(fmaf(e.x, e.x, e.y * e.y)));
        }
        pos = pos + 1 == H ? 0 : pos + 1;
    }

    if (live) {
        store_P_row(Pr, stP, r, N);
        if (r < N)
            for (int ch = 0; ch < C; ++ch) stG[ch * N + r] = l.G[ch * MS_GP + r];
        for (int h = r; h < C * H; h += WS_G) stH[h] = l.ring[h];
        if (r == 0) {
            stS[0] = s;
            stS[1] = 0.f;                                        // the pad: every byte of a record is written
        }
    }
}

template <class Src>
hipError_t launch(const Src &src, long n_groups, int C, int F, const WpeStreamConsts &c, float *wstate, hipStream_t st)
{
    const long groupsF = ws_tiles(F), grid = wpe_stream_grid(n_groups, F);
    if (grid > 0x7fffffffL || C < 2 || C > MS_CMAX || C * c.K > WS_G || C * (c.D + c.K) > MS_RING) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wpe_mc_stream_kernel<Src>, dim3((unsigned)grid), dim3(WS_G * WS_GROUPS), 0, st, src, c, C, wstate, F, (int)groupsF);
    return hipGetLastError();
}

}  // namespace

// P (N x N), G (N x C), C rings of D + K frames, s and a pad, N = C K: what the kernels above and of dereverb_stream_kernels.hip lay out
long wpe_stream_record_floats(int C, int K, int D) { return 2L * C * K * C * K + 2L * C * K * C + 2L * C * (D + K) + 2; }

// every statement of one channel is "dereverb stream": C = 1 runs the single-channel kernel, its bits
hipError_t launch_wpe_online(const void *spec, int n_groups, int C, int T, int F, int first_frame, const WpeStreamConsts &c,
                             float *wstate, void *spec_out, float *mag_out, int width, int col0, hipStream_t st)
{
    if (C == 1) return launch_wpe_online_1ch(spec, n_groups, T, F, first_frame, c, wstate, spec_out, mag_out, width, col0, st);
    FrameMajor src{static_cast<const float2 *>(spec), static_cast<float2 *>(spec_out), mag_out, T, width, col0, first_frame};
    return launch(src, n_groups, C, F, c, wstate, st);
}

hipError_t launch_wpe_stream(float *state, float *y, int n_streams, int C, const StreamGeom &g, const StreamCall &call,
                             const WpeStreamConsts &c, float *wstate, hipStream_t st)
{
    if (C == 1) return launch_wpe_stream_1ch(state, y, n_streams, g, call, c, wstate, st);
    if (C < 1) return hipErrorInvalidValue;
    if (call.f_last < call.f_first) return hipSuccess;
    InRing<StreamCall> src{state, y, g, call};
    return launch(src, n_streams / C, C, g.n_fft / 2 + 1, c, wstate, st);
}

// rows.n / C recordings of C consecutive rows each; C = 1 is the single-channel pool's kernel, its bits
hipError_t launch_wpe_mc_stream_pool(float *state, float *y, int C, const StreamGeom &g, const StreamPoolRows &rows,
                                     const WpeStreamConsts &c, float *wstate, hipStream_t st)
{
    if (C == 1) return launch_wpe_stream_pool(state, y, g, rows, c, wstate, st);
    if (C < 1 || rows.n < C || rows.n % C) return hipErrorInvalidValue;
    InRing<StreamPoolRows> src{state, y, g, rows};
    return launch(src, rows.n / C, C, g.n_fft / 2 + 1, c, wstate, st);
}

}  // namespace adn
