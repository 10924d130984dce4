// Mask-driven MVDR beamformer for gfx950: the C channels of a recording (1 <= C <= 8) to one channel, everything of a (group, bin)
// in one launch.  Definition: include/adn.h, "beamform"; float64 restatement: tests/beamform_ref.py.  The shape is that of the
// offline WPE kernels (dereverb_mc_kernels.hip); the Cholesky solve is the same code (wpe_solve.h) with K = C and C right-hand sides.
//
// Layouts: X is FRAME-major [group * C + channel][frame][F] float2 (adn_stft_complex of an (n_groups C, L) batch), the mask
// magnitudes are bin-major [group * C + channel][F][mag_width] with the frame fastest; the result is [group][frame][F] float2 and the
// optional magnitudes [group][F][width].
//
// Shape of the work.  A workgroup of ONE wave owns BINS neighbouring bins of one group, LPB = 64 / BINS lanes per (group, bin),
// chosen from C alone: 4 lanes (16 bins) up to C = 4, 8 lanes (8 bins) beyond.  The sums over t are sequential by definition, so
// the launch has only (group, bin) to spread over the chip: an hour of two-channel audio at n_fft 512 is 30 x 257 of them, and
// tiles of 64 bins made 150 workgroups for 256 CUs, each waiting on its own loads (measured: 3.1 ms; profiles/bench_beamform.md).
// One-wave tiles give 510 workgroups, several per CU, and make every barrier a wave's own.  LPB must hold the C lanes that substitute a
// column each in wpe_solve, and the E = C (C + 1) / 2 entries of a packed lower triangle are dealt to the lanes round-robin,
// EPL = ceil(E / LPB) each (1, 1, 2, 3 | 2, 3, 4, 5): a lane carries the SAME entries of Phi_s and Phi_n, so the two cells X_r and
// X_k it reads per entry and frame feed both sums (eight FMAs and four multiplies per two 8-byte LDS reads).  More lanes per bin
// would idle more of them (at C = 8, 36 entries fill 90 % of 8 x 5 slots, 56 % of 64 x 1) and would narrow the tile's run of
// bins, which is what the frame-major X is read along: 16 bins are 128 contiguous bytes per (channel, frame), 8 bins 64.
//   frames   come through LDS in chunks of TC = 32, all C channels of the tile's bins per frame row, so no limit on n_frames comes
//            from LDS.  A lane issues all its loads of a chunk (up to 32 cells of X and as many magnitudes) before it stores the
//            first to LDS: with a load, a wait and a store per cell the launch was bound by one memory latency per cell.  A channel's cells of a row are CS = BINS + 32 / LPB apart: the lanes of one bin read different channels
//            of the same bin, and at a pitch of BINS they would all sit on one bank; with CS the 32 lanes of a half wave
//            (32 / LPB bins x LPB lanes) read 32 different banks or share an address.
//   mask     the magnitudes of a chunk are read along the frame (32 frames = 128 contiguous bytes per (channel, bin)) into a
//            tile of odd pitch; one lane per (frame, bin) forms s_t, q_t and m_t and writes m_t to LDS.
//   products every lane walks the chunk's frames in order: the sum over t is sequential from frame 0 in every lane alike.
//   solve    the entries go to LDS over the frame tile, which is dead by then: Phi_n as the packed lower triangle, Phi_s as C full
//            columns (the upper triangle the conjugate, the diagonal real); wpe_solve factors once and lanes 0 ... C-1 substitute
//            one column each; lane 0 forms tau and w.
//   output   a second pass stages the frames again; one lane per (frame, bin) forms Y_t with w in registers, stores it along the
//            bins, and |Y_t| goes through the odd-pitch tile to be stored along the frames.
// Vector FMAs, not MFMA: the sums are fp32 FMAs in a stated order, and a C x C outer product per frame is far below an MFMA tile.
// Bit guarantees (adn.h).  Everything of a (group, bin) is computed by its own lanes from LDS cells addressed by the bin's slot in the
// tile only as an offset: no value depends on the slot, on the tile's other bins or on the group's place in the batch.  Lanes past
// the last bin walk the last bin again and store nothing.  No atomics, no workspace, no constant table.
// Cost: one launch of n_groups x ceil(F / BINS) workgroups; per (group, bin) 4 T (C (C + 1) + C) FMAs and X read twice.  Measured
// times: profiles/bench_beamform.md.
#include "adn_internal.h"
#include "wpe_solve.h"

namespace adn {
namespace {

constexpr int MVDR_THREADS = 64;                      // one wave: see the head of the file
constexpr int MVDR_TC = 32;                          // frames per staged chunk

constexpr int mvdr_lanes_per_bin(int C) { return C <= 4 ? 4 : 8; }

template <int C>
__global__ __launch_bounds__(MVDR_THREADS) void mvdr_kernel(const float2 *__restrict__ X, const float *__restrict__ Min, int mag_width,
                                                            float2 *__restrict__ Y, float *__restrict__ Mout, int T, int F, int tiles,
                                                            int width, MvdrConsts k)
{
#pragma clang fp contract(off)
    constexpr int LPB = mvdr_lanes_per_bin(C);
    constexpr int BINS = MVDR_THREADS / LPB;             // bins of a tile
    constexpr int E = C * (C + 1) / 2;                   // entries of a packed lower triangle
    constexpr int EPL = (E + LPB - 1) / LPB;             // entries a lane carries, of Phi_s and of Phi_n
    constexpr int CS = BINS + 32 / LPB;                  // cells between two channels of a staged frame row
    constexpr int PITCH = C * CS;                        // cells of a staged frame row
    constexpr int MP = MVDR_TC + 1;                      // pitch of the magnitude tile: odd
    constexpr int OP = BINS + 1;                         // pitch of the output magnitude tile: odd
    constexpr int NLD = MVDR_TC * C * BINS / MVDR_THREADS;   // cells of a chunk a lane stages, of X and of the magnitudes
    static_assert(NLD * MVDR_THREADS == MVDR_TC * C * BINS, "the lanes stage a chunk in whole rounds");
    static_assert(C <= LPB, "wpe_solve substitutes one column per lane");
    static_assert(BINS * (E + C * C) <= MVDR_TC * PITCH, "the triangle and the columns lie over the frame tile");
    __shared__ float2 Xs[MVDR_TC * PITCH];               // row: frame t0 + row; cell: channel * CS + bin.  After the sums: Tri, G
    constexpr int MS = C * BINS * MP > MVDR_TC * OP ? C * BINS * MP : MVDR_TC * OP;
    __shared__ float Ms[MS];                             // [(channel * BINS + bin)][frame]; the output pass: |Y| as [frame][OP]
    __shared__ float Wm[MVDR_TC * BINS];                 // m_t of [frame][bin]
    __shared__ float2 Wl[BINS * C];                      // w of [channel][bin]
    float2 *Tri = Xs;                                    // Phi_n / A / L of bin b at b * E, packed lower triangle
    float2 *G = Xs + BINS * E;                           // column c of bin b at (b * C + c) * C

    const int tid = threadIdx.x;
    const long grp = blockIdx.x / (unsigned)tiles;
    const int b0 = (int)(blockIdx.x - grp * tiles) * BINS;
    const float2 *x = X + grp * C * (long)T * F;
    const float *mg = Min + grp * C * (long)F * mag_width;
    // one lane per (frame, bin) of a chunk: bin ib, frames iq, iq + LPB, ...
    const int ib = tid % BINS, iq = tid / BINS;
    const bool live = b0 + ib < F;
    // one group of LPB lanes per bin: bin gb; lane gl has entries gl, gl + LPB, ... of the packed triangle, (row r, column k <= r)
    const int gb = tid / LPB, gl = tid % LPB;
    int offr[EPL], offk[EPL];
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        const int e = gl + j * LPB;                      // an entry past the last one walks entry 0 again and is not kept
        int r = 0, c = 0;
        if (e < E) wpe_tri_block(e, r, c);
        offr[j] = r * CS + gb;
        offk[j] = c * CS + gb;
    }

    float2 as[EPL], an[EPL];
#pragma unroll
    for (int j = 0; j < EPL; ++j) as[j] = an[j] = make_float2(0.f, 0.f);

    for (long t0 = 0; t0 < T; t0 += MVDR_TC) {
        const int left = T - t0 < MVDR_TC ? (int)(T - t0) : MVDR_TC;
        float2 xv[NLD];
        float mv[NLD];
#pragma unroll
        for (int u = 0; u < NLD; ++u) {                                         // X along the bins: every load of the chunk in flight
            const int i = tid + u * MVDR_THREADS, b = i % BINS, c = (i / BINS) % C, f = i / (BINS * C);
            const int bin = b0 + b < F ? b0 + b : F - 1;
            xv[u] = x[((long)c * T + (f < left ? t0 + f : T - 1)) * F + bin];   // a frame past the end reads the last one: dropped below
        }
#pragma unroll
        for (int u = 0; u < NLD; ++u) {                                         // the magnitudes along the frames, likewise
            const int i = tid + u * MVDR_THREADS, f = i % MVDR_TC, cell = i / MVDR_TC, b = cell % BINS, c = cell / BINS;
            const int bin = b0 + b < F ? b0 + b : F - 1;
            mv[u] = mg[((long)c * F + bin) * mag_width + (f < left ? t0 + f : T - 1)];
        }
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int i = tid + u * MVDR_THREADS, b = i % BINS, c = (i / BINS) % C, f = i / (BINS * C);
            Xs[f * PITCH + c * CS + b] = f < left ? xv[u] : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int i = tid + u * MVDR_THREADS, f = i % MVDR_TC, cell = i / MVDR_TC;
            Ms[cell * MP + f] = f < left ? mv[u] : 0.f;
        }
        __syncthreads();
        for (int f = iq; f < left; f += LPB) {                                  // m_t: s_t / q_t inside [rho, 1 - rho]
            float s = 0.f, q = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float m = Ms[(c * BINS + ib) * MP + f];
                const float2 v = Xs[f * PITCH + c * CS + ib];
                s = s + m * m;
                q = q + fmaf(v.x, v.x, v.y * v.y);
            }
            float m = k.rho;
            if (q > 0.f) {
                m = max_keep_nan(s / q, k.rho);
                m = m > k.one_minus_rho ? k.one_minus_rho : m;
            }
            Wm[f * BINS + ib] = m;
        }
        __syncthreads();
#pragma unroll 4
        for (int f = 0; f < left; ++f) {                                        // the sums over t, frame after frame
            const float m = Wm[f * BINS + gb];
            const float n = 1.f - m;
            const float2 *row = Xs + f * PITCH;
#pragma unroll
            for (int j = 0; j < EPL; ++j) {
                const float2 xr = row[offr[j]], xk = row[offk[j]];
                as[j] = cfma_conj_yx(make_float2(m * xr.x, m * xr.y), xk, as[j]);
                an[j] = cfma_conj_yx(make_float2(n * xr.x, n * xr.y), xk, an[j]);
            }
        }
        __syncthreads();
    }

    // Phi_n as the packed triangle, Phi_s as C full columns: the upper triangle is the conjugate, the diagonal is real
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        const int e = gl + j * LPB;
        if (e < E) {
            int r, c;
            wpe_tri_block(e, r, c);
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
    wpe_solve<LPB>(Tri + gb * E, G + gb * C * C, C, k.loading, gl, C, C);
    if (gl == 0) {                                                              // tau = max(sum_c Re G_cc, 1e-30), w_c = G[c][ref] / tau
        const float2 *g = G + gb * C * C;
        float tau = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) tau = tau + g[c * C + c].x;
        tau = max_keep_nan(tau, 1e-30f);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float2 v = g[k.ref * C + c];
            Wl[c * BINS + gb] = make_float2(v.x / tau, v.y / tau);
        }
    }
    __syncthreads();
    float2 w[C];
#pragma unroll
    for (int c = 0; c < C; ++c) w[c] = Wl[c * BINS + ib];

    for (long t0 = 0; t0 < T; t0 += MVDR_TC) {                                  // Y_t = sum_c conj(w_c) X_{t,c}
        const int left = T - t0 < MVDR_TC ? (int)(T - t0) : MVDR_TC;
        float2 xv[NLD];
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int i = tid + u * MVDR_THREADS, b = i % BINS, c = (i / BINS) % C, f = i / (BINS * C);
            const int bin = b0 + b < F ? b0 + b : F - 1;
            xv[u] = x[((long)c * T + (f < left ? t0 + f : T - 1)) * F + bin];
        }
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int i = tid + u * MVDR_THREADS, b = i % BINS, c = (i / BINS) % C, f = i / (BINS * C);
            Xs[f * PITCH + c * CS + b] = f < left ? xv[u] : make_float2(0.f, 0.f);
        }
        __syncthreads();
        for (int f = iq; f < left; f += LPB) {
            float2 y = make_float2(0.f, 0.f);
#pragma unroll
            for (int c = 0; c < C; ++c) y = cfma_conj(Xs[f * PITCH + c * CS + ib], w[c], y);
            if (live) Y[(grp * T + t0 + f) * F + b0 + ib] = y;
            Ms[f * OP + ib] = sqrtf(fmaf(y.x, y.x, y.y * y.y));
        }
        __syncthreads();
        if (Mout) {
            for (int i = tid; i < MVDR_TC * BINS; i += MVDR_THREADS) {
                const int f = i % MVDR_TC, b = i / MVDR_TC;
                if (f < left && b0 + b < F) Mout[(grp * F + b0 + b) * width + t0 + f] = Ms[f * OP + b];
            }
            __syncthreads();
        }
    }
}

template <int C>
hipError_t launch(const void *spec, const float *mag, int mag_width, int n_groups, int T, int F, const MvdrConsts &k, void *spec_out,
                  float *mag_out, int width, hipStream_t st)
{
    const long grid = mvdr_grid(n_groups, C, F);
    if (grid > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL((mvdr_kernel<C>), dim3((unsigned)grid), dim3(MVDR_THREADS), 0, st, static_cast<const float2 *>(spec), mag,
                       mag_width, static_cast<float2 *>(spec_out), mag_out, T, F, (int)(grid / n_groups), width, k);
    return hipGetLastError();
}

}  // namespace

long mvdr_grid(int n_groups, int C, int F)
{
    const long bins = MVDR_THREADS / mvdr_lanes_per_bin(C);
    return (((long)F + bins - 1) / bins) * n_groups;
}

hipError_t launch_mvdr(const void *spec, const float *mag, int mag_width, int n_groups, int C, int T, int F, const MvdrConsts &k,
                       void *spec_out, float *mag_out, int width, hipStream_t st)
{
    if (k.ref < 0 || k.ref >= C) return hipErrorInvalidValue;
    switch (C) {
    case 1: return launch<1>(spec, mag, mag_width, n_groups, T, F, k, spec_out, mag_out, width, st);
    case 2: return launch<2>(spec, mag, mag_width, n_groups, T, F, k, spec_out, mag_out, width, st);
    case 3: return launch<3>(spec, mag, mag_width, n_groups, T, F, k, spec_out, mag_out, width, st);
    case 4: return launch<4>(spec, mag, mag_width, n_groups, T, F, k, spec_out, mag_out, width, st);
    case 5: return launch<5>(spec, mag, mag_width, n_groups, T, F, k, spec_out, mag_out, width, st);
    case 6: return launch<6>(spec, mag, mag_width, n_groups, T, F, k, spec_out, mag_out, width, st);
    case 7: return launch<7>(spec, mag, mag_width, n_groups, T, F, k, spec_out, mag_out, width, st);
    case 8: return launch<8>(spec, mag, mag_width, n_groups, T, F, k, spec_out, mag_out, width, st);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace adn
