// Dereverberation baseline for gfx950: single-channel WPE (weighted prediction error, delayed linear prediction per frequency bin),
// all iterations of a (clip, bin) row in one launch.  Definition: include/adn.h, "dereverb"; float64 restatement: tests/dereverb_ref.py.
//
// Layouts: X and the result are FRAME-major [clip][frame][F] float2 (adn_stft_complex); the optional magnitudes are the network-output
// layout adn_denoise_resynth reads, bin-major [clip][F][width] with the frame fastest.
//
// Shape of the work.  A row's iteration is a weighted correlation of its past frames (R: K x K Hermitian, P: K), a Cholesky solve
// and a filter pass; rows are independent.  One lane cannot hold R (K (K + 1) / 2 + K, up to 560 complex accumulators), so the lower
// triangle of R is cut into 4 x 4 blocks and a row's blocks are spread over a GROUP of LPB lanes of one wave: nb = ceil(K / 4),
// nb (nb + 1) / 2 blocks, LPB = 16 up to K = 20 (15 blocks), 32 up to K = 28 (28 blocks), 64 beyond (36 blocks).  A lane holds the 16
// complex accumulators of its block, and the four of P when its block sits in column 0.  A workgroup is 256 lanes = 256 / LPB
// neighbouring bins of one clip: 16 bins at the defaults, so a frame of the tile is one 128-byte segment of the frame-major input.
//   frames   come through LDS in chunks of TC = 64 with the H = D + 4 nb - 1 frames before them (zeros before frame 0), so no limit
//            on n_frames comes from LDS; the history is read again per chunk and comes from L2.
//   weights  after a chunk is staged, one lane per (frame, bin) runs the previous iteration's filter (K complex FMAs) and writes
//            w_t = 1 / lam_t to LDS; d^(i-1) is never stored in memory.
//   products frames go four at a time: a block at (rb, cb) needs X at the seven lags around 4 rb and the seven around 4 cb for four
//            frames (14 LDS reads of 8 bytes, 4 weights, 4 X_t for P) and does 4 x (16 + 4) complex multiply-adds on them: about 350
//            vector operations per 22 LDS reads.  The sum over t is sequential from frame 0, in every lane alike.
//   solve    the blocks go to LDS as the packed lower triangle; the group's lanes share the rows of a column of the Cholesky
//            factor (inner sums sequential in k, so the bits do not depend on LPB), then lane 0 substitutes forward and back.
//   output   pass I + 1 runs the same filter with the last g and stores d; the magnitudes go through LDS transposed, so that a
//            wave stores 64 consecutive frames of one bin.
// Vector FMAs, not the exact-fp32 MFMA: the correlation as Z^H Z would divide by sqrt(lam) twice where the definition weights once
// by 1 / lam, and the 4 x 4 register blocks already keep the LDS reads an order below the FMAs.  ("dereverb".)
//
// Bit guarantees (adn.h).  Everything of a row is computed by its own group, from LDS cells addressed by the bin's slot in the
// tile only as an offset: no value depends on the slot, on the tile's other bins or on the clip's place in the batch.  Lanes past
// the last bin walk the last bin again and store nothing.  No atomics, no workspace.
// Cost: one launch of n_clips x ceil(F / (256 / LPB)) workgroups; per row and iteration 4 T (K (K + 1) / 2 + K) FMAs for the
// correlation (the 4 x 4 blocks compute 4 T 16 nb (nb + 1) / 2, 1.04 x that at K = 20) and 4 T K for the filter, the solve K^3 / 6.
// Measured times: profiles/bench_dereverb.md.
#include "adn_internal.h"
#include "wpe_solve.h"                               // the grid, the block decode, wpe_solve: shared with dereverb_mc_kernels.hip

namespace adn {
namespace {

constexpr int WPE_THREADS = 256;
constexpr int WPE_TC = 64;                           // frames per staged chunk
constexpr int WPE_HMAX = 8 + 32 - 1;                 // most history frames: D + 4 nb - 1

// lanes that share a row: the smallest of 16, 32, 64 that holds the nb (nb + 1) / 2 blocks of its lower triangle
inline int wpe_lanes_per_bin(int K) { return K <= 20 ? 16 : K <= 28 ? 32 : 64; }

// d_t = X_t - sum_j conj(g_j) X_{t-D-j}, j ascending over the n taps whose frame exists (adn.h, "dereverb").  xs points at X_t of
// the row in the staged chunk, earlier frames `pitch` cells before each other.
__device__ __forceinline__ float2 wpe_filter(const float2 *xs, int pitch, const float2 *g, int n, int D)
{
#pragma clang fp contract(off)
    float2 d = xs[0];
    const float2 *p = xs - (long)D * pitch;
    for (int j = 0; j < n; ++j, p -= pitch) d = cfms_conj(g[j], *p, d);
    return d;
}

template <int LPB>
__global__ __launch_bounds__(WPE_THREADS) void wpe_kernel(const float2 *__restrict__ X, float2 *__restrict__ Y, float *__restrict__ M,
                                                          int T, int F, int tiles, int width, WpeConsts k)
{
    constexpr int BINS = WPE_THREADS / LPB;              // bins of a tile
    constexpr int KMAX = LPB == 16 ? 20 : LPB == 32 ? 28 : 32;
    constexpr int TRI = KMAX * (KMAX + 1) / 2;
    constexpr int WP = BINS + 1;                         // pitch of the weight / magnitude tile: odd
    __shared__ float2 Xs[(WPE_TC + WPE_HMAX) * BINS];    // row r: frame t0 - H + r of the tile's bins
    __shared__ float Ws[WPE_TC * WP];
    __shared__ float2 Tri[BINS * TRI];
    __shared__ float2 G[BINS * KMAX];
    __shared__ float part[WPE_THREADS];
    __shared__ float phis[BINS];

    const int tid = threadIdx.x;
    const long clip = blockIdx.x / (unsigned)tiles;
    const int b0 = (int)(blockIdx.x - clip * tiles) * BINS;
    const float2 *x = X + clip * (long)T * F;
    const int K = k.K, D = k.D;
    const int nb = (K + 3) >> 2, H = D + 4 * nb - 1;
    // one lane per (frame, bin) of a chunk: bin ib, frames iq, iq + LPB, ...
    const int ib = tid % BINS, iq = tid / BINS;
    const bool live = b0 + ib < F;
    // one group of LPB lanes per bin: bin gb, block (rb, cb) of the lower triangle, rb >= cb
    const int gb = tid / LPB, gl = tid % LPB;
    int rb, cb;
    wpe_tri_block(gl, rb, cb);
    const bool owner = rb < nb;                          // lanes past the last block compute block (0, 0) again and keep nothing
    if (!owner) rb = cb = 0;

    const auto stage = [&](long t0) {
        for (int i = tid; i < (H + WPE_TC) * BINS; i += WPE_THREADS) {
            const long t = t0 - H + i / BINS;
            const int b = b0 + i % BINS;
            Xs[i] = t >= 0 && t < T ? x[t * F + (b < F ? b : F - 1)] : make_float2(0.f, 0.f);
        }
    };

    // phi = max(rho (sum_t p_t) / T, 1e-30): LPB partial sums per bin, each over its frames in order, added in order
    {
        float acc = 0.f;
        for (long t0 = 0; t0 < T; t0 += WPE_TC) {
            stage(t0);
            __syncthreads();
            for (int f = iq; f < WPE_TC && t0 + f < T; f += LPB) {
                const float2 v = Xs[(H + f) * BINS + ib];
                acc += fmaf(v.x, v.x, v.y * v.y);
            }
            __syncthreads();
        }
        part[tid] = acc;
        __syncthreads();
        if (tid < BINS) {
            float s = 0.f;
            for (int q = 0; q < LPB; ++q) s += part[q * BINS + tid];
            phis[tid] = max_keep_nan((k.rho * s) / (float)T, 1e-30f);
        }
        __syncthreads();
    }
    const float phi = phis[ib];

    for (int it = 0; it <= k.I; ++it) {                  // it < I: iteration it + 1; it == I: the output pass
        float2 acc[4][4], accP[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            accP[a] = make_float2(0.f, 0.f);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[a][c] = make_float2(0.f, 0.f);
        }
        for (long t0 = 0; t0 < T; t0 += WPE_TC) {
            stage(t0);
            __syncthreads();
            for (int f = iq; f < WPE_TC; f += LPB) {
                const long t = t0 + f;
                float w = 0.f;
                if (t < T) {
                    const long avail = t - D + 1;        // taps whose frame exists
                    const int n = it == 0 || avail <= 0 ? 0 : avail < K ? (int)avail : K;
                    const float2 d = wpe_filter(Xs + (H + f) * BINS + ib, BINS, G + ib * KMAX, n, D);
                    const float p = fmaf(d.x, d.x, d.y * d.y);
                    if (it == k.I) {
                        if (live) Y[(clip * T + t) * F + b0 + ib] = d;
                        w = sqrtf(p);
                    } else {
                        w = 1.f / max_keep_nan(p, phi);
                    }
                }
                Ws[f * WP + ib] = w;
            }
            __syncthreads();
            if (it == k.I) {
                if (M) {
                    for (int i = tid; i < WPE_TC * BINS; i += WPE_THREADS) {
                        const int f = i % WPE_TC, b = i / WPE_TC;
                        if (t0 + f < T && b0 + b < F) M[(clip * F + b0 + b) * width + t0 + f] = Ws[f * WP + b];
                    }
                }
            } else {
                const int left = T - t0 < WPE_TC ? (int)(T - t0) : WPE_TC;
                for (int f4 = 0; f4 < left; f4 += 4) {   // frames t0 + f4 .. + 3; past T the weights and the frames are zero
                    float2 xr[7], xc[7], xt[4];
                    float w[4];
                    const int row = f4 + 4 * nb - 4;     // row of lag 4 rb + 3 of the first frame: f4 + H - D - 4 rb - 3
#pragma unroll
                    for (int i = 0; i < 7; ++i) {
                        xr[i] = Xs[(row - 4 * rb + i) * BINS + gb];
                        xc[i] = Xs[(row - 4 * cb + i) * BINS + gb];
                    }
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        w[s] = Ws[(f4 + s) * WP + gb];
                        xt[s] = Xs[(f4 + H + s) * BINS + gb];
                    }
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
#pragma unroll
                        for (int a = 0; a < 4; ++a) {    // lag 4 rb + a of frame s sits at xr[s - a + 3]
                            const float2 u = make_float2(w[s] * xr[s - a + 3].x, w[s] * xr[s - a + 3].y);
#pragma unroll
                            for (int c = 0; c < 4; ++c) acc[a][c] = cfma_conj_yx(u, xc[s - c + 3], acc[a][c]);
                            accP[a] = cfma_conj_yx(u, xt[s], accP[a]);
                        }
                    }
                }
            }
            __syncthreads();
        }
        if (it == k.I) break;
        if (owner) {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int r = 4 * rb + a;
                if (r >= K) continue;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int col = 4 * cb + c;
                    if (col <= r) Tri[gb * TRI + r * (r + 1) / 2 + col] = acc[a][c];
                }
                if (cb == 0) G[gb * KMAX + r] = accP[a];
            }
        }
        __syncthreads();
        wpe_solve<LPB>(Tri + gb * TRI, G + gb * KMAX, K, k.loading, gl);
    }
}

template <int LPB>
hipError_t launch(const void *spec, int n_clips, int T, int F, const WpeConsts &k, void *spec_out, float *mag_out, int width,
                  hipStream_t st)
{
    const long grid = wpe_grid_1ch(n_clips, F, k.K);
    if (grid > 0x7fffffffL) return hipErrorInvalidValue;
    const int tiles = (int)(grid / n_clips);
    hipLaunchKernelGGL(wpe_kernel<LPB>, dim3((unsigned)grid), dim3(WPE_THREADS), 0, st, static_cast<const float2 *>(spec),
                       static_cast<float2 *>(spec_out), mag_out, T, F, tiles, width, k);
    return hipGetLastError();
}

}  // namespace

long wpe_grid_1ch(int n_clips, int F, int K) { return wpe_tile_grid(n_clips, F, wpe_lanes_per_bin(K)); }

hipError_t launch_wpe_1ch(const void *spec, int n_clips, int T, int F, const WpeConsts &k, void *spec_out, float *mag_out, int width,
                          hipStream_t st)
{
    switch (wpe_lanes_per_bin(k.K)) {
    case 16: return launch<16>(spec, n_clips, T, F, k, spec_out, mag_out, width, st);
    case 32: return launch<32>(spec, n_clips, T, F, k, spec_out, mag_out, width, st);
    default: return launch<64>(spec, n_clips, T, F, k, spec_out, mag_out, width, st);
    }
}

}  // namespace adn
