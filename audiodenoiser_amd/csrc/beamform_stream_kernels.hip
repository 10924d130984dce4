// Streaming mask-driven MVDR beamformer for gfx950: the C channels of a live recording (1 <= C <= 8) to one channel, the two spatial
// covariances carried on the device and updated once per frame, one filter per refresh.  Definition: include/adn.h, "beamform
// stream"; float64 restatement: tests/beamform_stream_ref.py.  The shape is mvdr_kernel's (beamform_kernels.hip), the Cholesky solve
// is the same code (wpe_solve.h) with K = C and C right-hand sides, the frame sources are the recursive WPE kernels'
// (wpe_stream_frames.h).
//
// State of a slot (adn_mvdr_stream_state_bytes; a slot is a GROUP; (2 E + C) F float2, E = C (C + 1) / 2), entry-major over the bins:
//   Phi_s  [e][F] float2    the packed lower triangle, entry e = r (r + 1) / 2 + k, k <= r; the diagonal keeps its imaginary part
//   Phi_n  [e][F] float2    likewise
//   w      [c][F] float2    the filter of the last refresh
// so the lanes that own neighbouring bins read and write neighbouring addresses.  A group whose first frame of the call is frame 0
// reads none of it.
//
// Shape of the work.  A workgroup of ONE wave owns BINS neighbouring bins of one group, LPB = 64 / BINS lanes per (group, bin): 4
// lanes (16 bins) up to C = 4, 8 lanes (8 bins) beyond.  Lane gl of a bin carries the SAME EPL = ceil(E / LPB) entries of Phi_s and
// of Phi_n in registers for the whole call: loaded from the state once, stored once.  Per frame:
//   1  lane i < C BINS posts cell X_{t,c} and magnitude M_{t,c} of (channel, bin) = (i / BINS, i % BINS) in LDS; it has had them in
//      registers since the frame before (the loads of frame t + 1 are issued before frame t is worked on)                  barrier
//   2  every lane of a bin forms s_t, q_t, m_t and n_t for itself from the C posted cells, channels ascending: no lane waits
//   3  every lane updates its entries: (m_t X_r) conj(X_k) + alpha (.) Phi, the product by alpha rounded once
//   4  on a refresh frame (t % R == 0, uniform over the workgroup) the triangle of Phi_n and the C columns of Phi_s go to LDS,
//      wpe_solve factors once and lanes 0 ... C - 1 substitute a column each, lane 0 forms tau and w and posts w       barriers
//   5  lane b < BINS forms Y_t of bin b from the posted cells and w, and stores it and |Y_t|                              barrier
// Vector FMAs, not MFMA: the sums are fp32 FMAs in a stated order, and a C x C outer product per frame is far below an MFMA tile
// (the head of beamform_kernels.hip).  Every barrier is the wave's own.
// In place (the ring source): the lanes that read the cells and the magnitudes of a (group, bin, frame) belong to the workgroup
// that writes Y_t and |Y_t| over channel 0's, behind the barrier of stage 1; frame t + 1, fetched early, lives in other cells.
// A pool's recordings (InRing<StreamPoolRows>): the C rows of group g name the stream slots r C ... r C + C - 1, which the entry
// point has checked; the ring cells are those slots', the state slot is r, the windows of y are the rows' (wpe_stream_frames.h,
// "groups of C rows").  Y_t and |Y_t| go over the group's first row only, as in lockstep.
// Bit guarantees (adn.h).  Everything of a (group, bin) is computed by its own lanes from LDS cells addressed by the bin's slot in
// the tile only as an offset: no value depends on the slot, on the tile's other bins or on the group's place in the batch.  Lanes
// past the last bin walk the last bin again and store nothing.  No atomics, no workspace, no constant table.
// Cost: one launch of n_groups x ceil(F / BINS) workgroups; per (group, bin) and frame 8 E + 4 C FMAs and, on a refresh frame, the
// solve's chain (C^3 / 3 for the factor, 2 C^2 per column) run by at most C lanes.  Measured: profiles/bench_beamform_stream.md.
#include "wpe_solve.h"
#include "wpe_stream_frames.h"

namespace adn {
namespace {

constexpr int MS_THREADS = 64;                        // one wave

constexpr int mvdr_stream_lanes_per_bin(int C) { return C <= 4 ? 4 : 8; }

template <int C, class Src>
__global__ __launch_bounds__(MS_THREADS) void mvdr_stream_kernel(Src src, MvdrStreamConsts k, float2 *__restrict__ state, int F, int tiles)
{
#pragma clang fp contract(off)
    constexpr int LPB = mvdr_stream_lanes_per_bin(C);
    constexpr int BINS = MS_THREADS / LPB;               // bins of a tile
    constexpr int E = C * (C + 1) / 2;                   // entries of a packed lower triangle
    constexpr int EPL = (E + LPB - 1) / LPB;             // entries a lane carries, of Phi_s and of Phi_n
    constexpr int CS = BINS + 32 / LPB;                  // cells between two channels of the staged frame (mvdr_kernel's pitch)
    static_assert(C * BINS <= MS_THREADS, "a lane stages at most one cell of a frame");
    static_assert(C <= LPB, "wpe_solve substitutes one column per lane");
    __shared__ float2 Xs[C * CS];                        // X_{t,c} of bin b at c * CS + b
    __shared__ float Ms[C * BINS];                       // M_{t,c} of bin b at c * BINS + b
    __shared__ float2 Tri[BINS * E];                     // Phi_n / A / L of bin b at b * E, packed lower triangle
    __shared__ float2 G[BINS * C * C];                   // column c of bin b at (b * C + c) * C
    __shared__ float2 Wl[C * BINS];                      // w_c of bin b at c * BINS + b: carried from refresh to refresh

    const int tid = threadIdx.x;
    const long grp = blockIdx.x / (unsigned)tiles;
    const int b0 = (int)(blockIdx.x - grp * tiles) * BINS;
    // every channel of a group covers the same frames: those of its first row
    StreamCall call;
    const RowFrames r0 = frames_of(src, grp * C, F, call);
    const int t0 = r0.t0, t1 = r0.t1;
    const bool fresh = t0 == 0;
    // the lane that stages (channel sc, bin sb), and later the filter entry of the same place
    const bool stager = tid < C * BINS;
    const int sc = stager ? tid / BINS : 0, sb = tid % BINS;
    const int sbin = b0 + sb < F ? b0 + sb : F - 1;
    const long srow = grp * C + sc;
    const RowFrames rs{chan_slot_of(src, srow), t0, t1};
    // the lane that forms Y_t of bin ib
    const int ib = tid % BINS;
    const bool writer = tid < BINS && b0 + ib < F;
    const long orow = out_row_of(src, grp, C);
    const RowFrames ro{chan_slot_of(src, orow), t0, t1};
    // one group of LPB lanes per bin: bin gb; lane gl has entries gl, gl + LPB, ... of the packed triangle, (row r, column k <= r)
    const int gb = tid / LPB, gl = tid % LPB;
    const bool live = b0 + gb < F;
    const int gbin = live ? b0 + gb : F - 1;
    int er[EPL], ek[EPL];
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        const int e = gl + j * LPB;                      // an entry past the last one walks entry 0 again and is not kept
        er[j] = ek[j] = 0;
        if (e < E) wpe_tri_block(e, er[j], ek[j]);
    }

    float2 *st = state + group_slot_of(src, grp, C) * (long)(2 * E + C) * F;
    float2 as[EPL], an[EPL];
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        const int e = gl + j * LPB;
        as[j] = an[j] = make_float2(0.f, 0.f);
        if (!fresh && e < E) {
            as[j] = st[(long)e * F + gbin];
            an[j] = st[(long)(E + e) * F + gbin];
        }
    }
    if (stager) Wl[sc * BINS + sb] = fresh ? make_float2(0.f, 0.f) : st[(long)(2 * E + sc) * F + sbin];

    float2 xn = make_float2(0.f, 0.f);
    float mn = 0.f;
    if (stager) {
        xn = load_frame(src, rs, call, srow, F, sbin, t0);
        mn = load_mag(src, rs, call, srow, F, sbin, t0);
    }
    int phase = t0 % k.R;                                // t % R, carried
    for (int t = t0; t <= t1; ++t) {
        // 1
        if (stager) {
            Xs[sc * CS + sb] = xn;
            Ms[sc * BINS + sb] = mn;
        }
        __syncthreads();
        if (stager && t < t1) {
            xn = load_frame(src, rs, call, srow, F, sbin, t + 1);
            mn = load_mag(src, rs, call, srow, F, sbin, t + 1);
        }
        // 2: m_t = s_t / q_t inside [rho, 1 - rho]
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float mg = Ms[c * BINS + gb];
            const float2 v = Xs[c * CS + gb];
            s = s + mg * mg;
            q = q + fmaf(v.x, v.x, v.y * v.y);
        }
        float m = k.m.rho;
        if (q > 0.f) {
            m = max_keep_nan(s / q, k.m.rho);
            m = m > k.m.one_minus_rho ? k.m.one_minus_rho : m;
        }
        const float n = 1.f - m;
        // 3
#pragma unroll
        for (int j = 0; j < EPL; ++j) {
            const float2 xr = Xs[er[j] * CS + gb], xk = Xs[ek[j] * CS + gb];
            as[j] = cfma_conj_yx(make_float2(m * xr.x, m * xr.y), xk, make_float2(k.alpha * as[j].x, k.alpha * as[j].y));
            an[j] = cfma_conj_yx(make_float2(n * xr.x, n * xr.y), xk, make_float2(k.alpha * an[j].x, k.alpha * an[j].y));
        }
        // 4
        if (phase == 0) {
            // Phi_n as the packed triangle, Phi_s as C full columns: the upper triangle is the conjugate, the diagonal is real
#pragma unroll
            for (int j = 0; j < EPL; ++j) {
                const int e = gl + j * LPB;
                if (e < E) {
                    const int r = er[j], c = ek[j];
                    Tri[gb * E + e] = an[j];
                    float2 *g = G + gb * C * C;
                    if (r == c) {
                        g[c * C + r] = make_float2(as[j].x, 0.f);
                    } else {
                        g[c * C + r] = as[j];
                        g[r * C + c] = make_float2(as[j].x, -as[j].y);
                    }
                }
            }
            __syncthreads();
            wpe_solve<LPB>(Tri + gb * E, G + gb * C * C, C, k.m.loading, gl, C, C);
            if (gl == 0) {                               // tau = max(sum_c Re G_cc, 1e-30), w_c = G[c][ref] / tau
                const float2 *g = G + gb * C * C;
                float tau = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) tau = tau + g[c * C + c].x;
                tau = max_keep_nan(tau, 1e-30f);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float2 v = g[k.m.ref * C + c];
                    Wl[c * BINS + gb] = make_float2(v.x / tau, v.y / tau);
                }
            }
            __syncthreads();
        }
        phase = phase + 1 == k.R ? 0 : phase + 1;
        // 5: Y_t = sum_c conj(w_c) X_{t,c}
        if (tid < BINS) {
            float2 y = make_float2(0.f, 0.f);
#pragma unroll
            for (int c = 0; c < C; ++c) y = cfma_conj(Xs[c * CS + ib], Wl[c * BINS + ib], y);
            if (writer) store_frame(src, ro, call, orow, F, b0 + ib, t, y, sqrtf(fmaf(y.x, y.x, y.y * y.y)));
        }
        __syncthreads();
    }

    if (live) {
#pragma unroll
        for (int j = 0; j < EPL; ++j) {
            const int e = gl + j * LPB;
            if (e < E) {
                st[(long)e * F + gbin] = as[j];
                st[(long)(E + e) * F + gbin] = an[j];
            }
        }
    }
    if (stager && b0 + sb < F) st[(long)(2 * E + sc) * F + sbin] = Wl[sc * BINS + sb];
}

template <int C, class Src>
hipError_t launch_c(const Src &src, long n_groups, int F, const MvdrStreamConsts &k, float *state, hipStream_t st)
{
    const long grid = mvdr_stream_grid(n_groups, C, F);
    if (grid > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL((mvdr_stream_kernel<C, Src>), dim3((unsigned)grid), dim3(MS_THREADS), 0, st, src, k, reinterpret_cast<float2 *>(state),
                       F, (int)(grid / n_groups));
    return hipGetLastError();
}

template <class Src>
hipError_t launch(const Src &src, long n_groups, int C, int F, const MvdrStreamConsts &k, float *state, hipStream_t st)
{
    if (k.m.ref < 0 || k.m.ref >= C || k.R < 1 || n_groups < 1) return hipErrorInvalidValue;
    switch (C) {
    case 1: return launch_c<1>(src, n_groups, F, k, state, st);
    case 2: return launch_c<2>(src, n_groups, F, k, state, st);
    case 3: return launch_c<3>(src, n_groups, F, k, state, st);
    case 4: return launch_c<4>(src, n_groups, F, k, state, st);
    case 5: return launch_c<5>(src, n_groups, F, k, state, st);
    case 6: return launch_c<6>(src, n_groups, F, k, state, st);
    case 7: return launch_c<7>(src, n_groups, F, k, state, st);
    case 8: return launch_c<8>(src, n_groups, F, k, state, st);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

long mvdr_stream_grid(long n_groups, int C, int F)
{
    const long bins = MS_THREADS / mvdr_stream_lanes_per_bin(C);
    return (((long)F + bins - 1) / bins) * n_groups;
}

// the two packed triangles and the filter of a (slot, bin)
long mvdr_stream_record_floats(int C) { return 2L * (C * (C + 1) + C); }

hipError_t launch_mvdr_online(const void *spec, const float *mag, int mag_width, int mag_col0, int n_groups, int C, int T, int F,
                              int first_frame, const MvdrStreamConsts &k, float *state, void *spec_out, float *mag_out, int width,
                              int col0, hipStream_t st)
{
    FrameMajorMasked src{{static_cast<const float2 *>(spec), static_cast<float2 *>(spec_out), mag_out, T, width, col0, first_frame},
                         mag, mag_width, mag_col0};
    return launch(src, n_groups, C, F, k, state, st);
}

hipError_t launch_mvdr_stream(float *sstate, float *y, int n_streams, int C, const StreamGeom &g, const StreamCall &call,
                              const MvdrStreamConsts &k, float *state, hipStream_t st)
{
    if (C < 1 || n_streams % C) return hipErrorInvalidValue;
    if (call.f_last < call.f_first) return hipSuccess;
    InRing<StreamCall> src{sstate, y, g, call};
    return launch(src, n_streams / C, C, g.n_fft / 2 + 1, k, state, st);
}

// rows.n / C recordings of C consecutive rows each (wpe_stream_frames.h, "groups of C rows")
hipError_t launch_mvdr_stream_pool(float *sstate, float *y, int C, const StreamGeom &g, const StreamPoolRows &rows,
                                   const MvdrStreamConsts &k, float *state, hipStream_t st)
{
    if (C < 1 || rows.n < C || rows.n % C) return hipErrorInvalidValue;
    InRing<StreamPoolRows> src{sstate, y, g, rows};
    return launch(src, rows.n / C, C, g.n_fft / 2 + 1, k, state, st);
}

}  // namespace adn
