// Multichannel dereverberation for gfx950: joint WPE of the C channels of a recording (2 <= C <= 8; C = 1 is adn_wpe itself and is
// forwarded to its kernel by launch_wpe below), all iterations of a (group, bin) in one launch.  Definition: include/adn.h,
// "dereverb multichannel"; float64 restatement: tests/dereverb_mc_ref.py.  The single-channel sibling is dereverb_kernels.hip,
// whose shape this file keeps; the Cholesky solve is the same code (wpe_solve.h) with C right-hand sides.
//
// Layouts: X and the result are FRAME-major [group * C + channel][frame][F] float2 (adn_stft_complex of an (n_groups C, L) batch);
// the optional magnitudes are bin-major [group * C + channel][F][width] with the frame fastest.
//
// Shape of the work.  The stacked vector of a (group, bin) at frame t has N = C K entries, x~_t[r] = X_{t-D-j, c} at r = c K + j.
// An iteration is R = sum_t w_t x~ x~^H (N x N Hermitian), P = sum_t w_t x~ X_t^H (N x C), one factorisation, C substitutions, and
// a filter pass over all channels.  The lower triangle of R is cut into 4 x 4 blocks ON THE STACKED INDEX, nb = ceil(N / 4) block
// rows, and P into nb x ceil(C / 4) blocks of four rows by four channels: a P block is an R block whose four "columns" are the
// current frame of four channels.  Every block is one lane's 16 complex accumulators, so every lane of a group does the same 64
// complex multiply-adds per frame -- no lane carries P on top of its block, which at C = 8 would have tripled its work.  A group
// of LPB lanes owns a (group, bin): the smallest of 16 / 32 / 64 that holds nb (nb + 1) / 2 + nb ceil(C / 4) blocks, doubled until
// the workgroup's 256 / LPB bins times C channels are at most 32 cells per staged frame (wpe_mc_lanes_per_bin): 16 lanes up to
// N = 16 at C = 2; 32 up to N = 24 at C <= 4; 64 beyond.
//   frames   come through LDS in chunks of TC = 64 with the H = D + K - 1 frames before them (zeros before frame 0), all C channels
//            of the tile's bins per frame row, so no limit on n_frames comes from LDS.
//   weights  after a chunk is staged, one lane per (frame, bin) runs the previous iteration's filter for all C channels (N C
//            complex FMAs, a staged cell read once for the C channels it feeds) and writes w_t = 1 / max(sum_c |d_c|^2 / C, phi)
//            to LDS; d^(i-1) is never stored in memory.
//   products frames go four at a time, the sum over t sequential from frame 0 in every lane alike.
//   solve    the blocks go to LDS as the packed lower triangle IN STACKED ORDER and the C columns of P beside it; wpe_solve
//            factors once and lanes 0 ... C-1 substitute one column each.
//   output   pass I + 1 runs the same filter with the last G and stores d; the magnitudes go through LDS transposed.
//
// The block layout when 4 does not divide K.  The single-channel kernel feeds a block from a seven-cell sliding window: its four
// rows are four consecutive lags, so four frames of them are seven cells of one channel.  With r = c K + j that holds for every
// block only when 4 divides K.  Two ways out were weighed.  (a) Pad every channel to a multiple of four rows in the block grid:
// the window always works, but the grid grows to C ceil(K / 4) block rows -- nothing at (3, 7), but (2, 5) becomes 4 block rows
// instead of 3 and (4, 5) 8 instead of 5 (36 + 8 blocks instead of 15 + 5: 64 lanes instead of 32, and 2.2 times the
// multiply-adds), and the packed triangle the solve sees would have to be gathered through a row map.  (b) Keep the
// blocks on the stacked index and give up the window where it does not apply: a lane then reads its four rows and four columns
// per frame (32 LDS reads of 8 bytes per four frames instead of 14) for the same 256 complex multiply-adds.  (b) is what this
// file does: the reads stay a factor four below the FMAs in LDS-array cycles against VALU cycles (2 cycles per ds_read_b64 and
// wave, 4 x 2 per complex multiply-add), no lane computes padding, and the store to the packed triangle is the single-channel
// kernel's.  WINDOW is a template parameter chosen from K % 4 on the host; both forms perform the same FMAs on the same values in
// the same order, so the choice cannot show in the results (tests/test_gpu_dereverb_mc.py compares (3, 8) and (3, 7) against the
// same restatement, and the reads of a P block's columns are the direct form in both).
//
// Vector FMAs, not MFMA, for the reason dereverb_kernels.hip gives.
// Bit guarantees (adn.h).  Everything of a (group, bin) is computed by its own lane group, from LDS cells addressed by the bin's
// slot in the tile only as an offset: no value depends on the slot, on the tile's other bins or on the group's place in the batch.
// Lanes past the last bin walk the last bin again and store nothing.  No atomics, no workspace.
// Cost: one launch of n_groups x ceil(F / (256 / LPB)) workgroups; per (group, bin) and iteration 4 T (N (N + 1) / 2 + N C) FMAs
// for the correlation (the blocks compute 4 T 16 (nb (nb + 1) / 2 + nb ceil(C / 4))) and 4 T N C for the filter; the solve
// N^3 / 6 + C N^2.  Measured times: profiles/bench_dereverb_mc.md.
#include "adn_internal.h"
#include "wpe_solve.h"

namespace adn {
namespace {

constexpr int WPE_MC_THREADS = 256;
constexpr int WPE_MC_TC = 64;                        // frames per staged chunk
constexpr int WPE_MC_HMAX = 8 + 16 - 1;              // most history frames: D + K - 1 at K <= 32 / 2
constexpr int WPE_MC_CELLS = 32;                     // most (channel, bin) cells of a staged frame row: C x BINS
constexpr int WPE_MC_NMAX = 32;                      // pitch of a column of P / G

inline int wpe_mc_blocks(int C, int K)
{
    const int nb = (C * K + 3) / 4;
    return nb * (nb + 1) / 2 + nb * ((C + 3) / 4);
}

inline int wpe_mc_lanes_per_bin(int C, int K)
{
    const int blocks = wpe_mc_blocks(C, K);
    int lanes = blocks <= 16 ? 16 : blocks <= 32 ? 32 : 64;
    while ((WPE_MC_THREADS / lanes) * C > WPE_MC_CELLS) lanes *= 2;
    return lanes;
}

template <int LPB, bool WINDOW>
__global__ __launch_bounds__(WPE_MC_THREADS) void wpe_mc_kernel(const float2 *__restrict__ X, float2 *__restrict__ Y,
                                                                float *__restrict__ M, int C, int T, int F, int tiles, int width,
                                                                WpeConsts k)
{
    constexpr int BINS = WPE_MC_THREADS / LPB;           // bins of a tile
    constexpr int NTOP = LPB == 16 ? 16 : LPB == 32 ? 24 : 32;   // the largest N a group of LPB lanes has blocks for
    constexpr int TRI = NTOP * (NTOP + 1) / 2;
    __shared__ float2 Xs[(WPE_MC_TC + WPE_MC_HMAX) * WPE_MC_CELLS];      // row: frame t0 - H + row; cell: channel * BINS + bin
    __shared__ float Ws[WPE_MC_TC * (WPE_MC_CELLS + 1)];                 // weights in channel 0's cells; the output pass: |d| of all
    __shared__ float2 Tri[BINS * TRI];
    __shared__ float2 G[WPE_MC_CELLS * WPE_MC_NMAX];                     // column c of bin b at ((b C + c) NMAX)
    __shared__ float part[WPE_MC_THREADS];
    __shared__ float phis[BINS];

    const int tid = threadIdx.x;
    const long grp = blockIdx.x / (unsigned)tiles;
    const int b0 = (int)(blockIdx.x - grp * tiles) * BINS;
    const float2 *x = X + grp * C * (long)T * F;
    const int K = k.K, D = k.D, N = C * K;
    const int nb = (N + 3) >> 2, cq = (C + 3) >> 2, H = D + K - 1;
    const int PITCH = C * BINS, WP = PITCH + 1;          // cells of a staged frame row; pitch of the weight tile: odd
    // one lane per (frame, bin) of a chunk: bin ib, frames iq, iq + LPB, ...
    const int ib = tid % BINS, iq = tid / BINS;
    const bool live = b0 + ib < F;
    // one group of LPB lanes per bin: bin gb; lane gl has block (rb, cb) of R's lower triangle, or block (rb, channels 4 q ...) of P
    const int gb = tid / LPB, gl = tid % LPB;
    const int nR = nb * (nb + 1) / 2;
    int rb = 0, cb = 0;
    bool pblock = false;
    if (gl < nR) {
        wpe_tri_block(gl, rb, cb);
    } else if (gl < nR + nb * cq) {
        pblock = true;
        rb = (gl - nR) / cq;
        cb = (gl - nR) % cq;
    }
    const bool owner = gl < nR + nb * cq;                // lanes past the last block compute block (0, 0) again and keep nothing
    // where the lane's four rows and four columns sit in a staged frame row, and how many rows above the frame's own (H + f):
    // stacked index r = c K + j is channel c at lag D + j; a row or channel past the end walks the last one and is not kept
    int offr[4], offc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int r = min(4 * rb + a, N - 1);
        offr[a] = (H - D - r % K) * PITCH + (r / K) * BINS + gb;
        if (pblock) {
            offc[a] = H * PITCH + min(4 * cb + a, C - 1) * BINS + gb;
        } else {
            const int s = min(4 * cb + a, N - 1);
            offc[a] = (H - D - s % K) * PITCH + (s / K) * BINS + gb;
        }
    }

    const auto stage = [&](long t0) {
        for (int i = tid; i < (H + WPE_MC_TC) * PITCH; i += WPE_MC_THREADS) {
            const long t = t0 - H + i / PITCH;
            const int cell = i % PITCH, c = cell / BINS, b = b0 + cell % BINS;
            Xs[i] = t >= 0 && t < T ? x[((long)c * T + t) * F + (b < F ? b : F - 1)] : make_float2(0.f, 0.f);
        }
    };

    // phi = max(rho (sum_c sum_t p_{t,c}) / (T C), 1e-30): per channel LPB partial sums per bin, each over its frames in order,
    // added in order; the channels ascending
    {
        float acc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = 0.f;
        for (long t0 = 0; t0 < T; t0 += WPE_MC_TC) {
            stage(t0);
            __syncthreads();
            for (int f = iq; f < WPE_MC_TC && t0 + f < T; f += LPB) {
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    if (c < C) {
                        const float2 v = Xs[(H + f) * PITCH + c * BINS + ib];
                        acc[c] += fmaf(v.x, v.x, v.y * v.y);
                    }
                }
            }
            __syncthreads();
        }
        float total = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            if (c < C) {                                 // uniform over the workgroup
                part[tid] = acc[c];
                __syncthreads();
                if (tid < BINS) {
                    float s = 0.f;
                    for (int q = 0; q < LPB; ++q) s += part[q * BINS + tid];
                    total += s;
                }
                __syncthreads();
            }
        }
        if (tid < BINS) phis[tid] = max_keep_nan((k.rho * total) / (float)((long)T * C), 1e-30f);
        __syncthreads();
    }
    const float phi = phis[ib];
    const float fC = (float)C;

    for (int it = 0; it <= k.I; ++it) {                  // it < I: iteration it + 1; it == I: the output pass
        float2 acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[a][c] = make_float2(0.f, 0.f);
        }
        for (long t0 = 0; t0 < T; t0 += WPE_MC_TC) {
            stage(t0);
            __syncthreads();
            for (int f = iq; f < WPE_MC_TC; f += LPB) {
                const long t = t0 + f;
                float w = 0.f;
                if (t < T) {
                    // d_{t,c} = X_{t,c} - sum_r conj(G_rc) x~_t[r], r ascending over the entries whose frame exists
                    const float2 *xs = Xs + (H + f) * PITCH + ib;
                    const float2 *g = G + ib * C * WPE_MC_NMAX;
                    const long avail = t - D + 1;        // lags whose frame exists
                    const int n = it == 0 || avail <= 0 ? 0 : avail < K ? (int)avail : K;
                    float2 d[8];
#pragma unroll
                    for (int c = 0; c < 8; ++c) d[c] = c < C ? xs[c * BINS] : make_float2(0.f, 0.f);
                    {
#pragma clang fp contract(off)
                        for (int cp = 0; cp < C; ++cp) {
                            const float2 *p = xs - D * PITCH + cp * BINS;
                            for (int j = 0; j < n; ++j, p -= PITCH) {
                                const float2 v = *p;
                                const float2 *gr = g + cp * K + j;
#pragma unroll
                                for (int c = 0; c < 8; ++c) {
                                    if (c < C) {
                                        // cfms_conj(q, v, d[c]) written out: as a call it moves this kernel's instructions
                                        const float2 q = gr[c * WPE_MC_NMAX];
                                        d[c].x = fmaf(-q.y, v.y, fmaf(-q.x, v.x, d[c].x));
                                        d[c].y = fmaf(q.y, v.x, fmaf(-q.x, v.y, d[c].y));
                                    }
                                }
                            }
                        }
                    }
                    float s = 0.f;
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        if (c < C) {
                            const float p = fmaf(d[c].x, d[c].x, d[c].y * d[c].y);
                            if (it == k.I) {
                                if (live) Y[((grp * C + c) * T + t) * F + b0 + ib] = d[c];
                                Ws[f * WP + c * BINS + ib] = sqrtf(p);
                            } else {
                                s = c == 0 ? p : s + p;
                            }
                        }
                    }
                    w = 1.f / max_keep_nan(s / fC, phi);
                }
                if (it != k.I) Ws[f * WP + ib] = w;
            }
            __syncthreads();
            if (it == k.I) {
                if (M) {
                    for (int i = tid; i < WPE_MC_TC * PITCH; i += WPE_MC_THREADS) {
                        const int f = i % WPE_MC_TC, cell = i / WPE_MC_TC, c = cell / BINS, b = cell % BINS;
                        if (t0 + f < T && b0 + b < F) M[((grp * C + c) * F + b0 + b) * width + t0 + f] = Ws[f * WP + cell];
                    }
                }
            } else {
                const int left = T - t0 < WPE_MC_TC ? (int)(T - t0) : WPE_MC_TC;
                for (int f4 = 0; f4 < left; f4 += 4) {   // frames t0 + f4 .. + 3; past T the weights and the frames are zero
                    float2 xr[4][4], xc[4][4];           // [frame][row], [frame][column]
                    float w[4];
                    const float2 *base = Xs + f4 * PITCH;
                    if (WINDOW) {                        // 4 | K: rows 4 rb .. + 3 are lags j0 .. j0 + 3 of one channel: seven cells
                        float2 win[7];
#pragma unroll
                        for (int i = 0; i < 7; ++i) win[i] = base[offr[0] + (i - 3) * PITCH];
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
#pragma unroll
                            for (int a = 0; a < 4; ++a) xr[s][a] = win[s - a + 3];
                        }
                    } else {
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
#pragma unroll
                            for (int a = 0; a < 4; ++a) xr[s][a] = base[offr[a] + s * PITCH];
                        }
                    }
                    if (WINDOW && !pblock) {
                        float2 win[7];
#pragma unroll
                        for (int i = 0; i < 7; ++i) win[i] = base[offc[0] + (i - 3) * PITCH];
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
#pragma unroll
                            for (int c = 0; c < 4; ++c) xc[s][c] = win[s - c + 3];
                        }
                    } else {
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
#pragma unroll
                            for (int c = 0; c < 4; ++c) xc[s][c] = base[offc[c] + s * PITCH];
                        }
                    }
#pragma unroll
                    for (int s = 0; s < 4; ++s) w[s] = Ws[(f4 + s) * WP + gb];
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
#pragma unroll
                        for (int a = 0; a < 4; ++a) {
                            const float2 u = make_float2(w[s] * xr[s][a].x, w[s] * xr[s][a].y);
#pragma unroll
                            for (int c = 0; c < 4; ++c) {    // += u conj(v): cfma_conj_yx, written out for the same reason
                                const float2 v = xc[s][c];
                                acc[a][c].x = fmaf(u.y, v.y, fmaf(u.x, v.x, acc[a][c].x));
                                acc[a][c].y = fmaf(-u.x, v.y, fmaf(u.y, v.x, acc[a][c].y));
                            }
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
                if (r >= N) continue;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int col = 4 * cb + c;
                    if (pblock) {
                        if (col < C) G[(gb * C + col) * WPE_MC_NMAX + r] = acc[a][c];
                    } else if (col <= r) {
                        Tri[gb * TRI + r * (r + 1) / 2 + col] = acc[a][c];
                    }
                }
            }
        }
        __syncthreads();
        wpe_solve<LPB>(Tri + gb * TRI, G + gb * C * WPE_MC_NMAX, N, k.loading, gl, C, WPE_MC_NMAX);
    }
}

template <int LPB>
hipError_t launch(const void *spec, int n_groups, int C, int T, int F, const WpeConsts &k, void *spec_out, float *mag_out, int width,
                  hipStream_t st)
{
    const long grid = wpe_grid(n_groups, C, F, k.K);
    if (grid > 0x7fffffffL) return hipErrorInvalidValue;
    const int tiles = (int)(grid / n_groups);
    if (k.K % 4 == 0)
        hipLaunchKernelGGL((wpe_mc_kernel<LPB, true>), dim3((unsigned)grid), dim3(WPE_MC_THREADS), 0, st,
                           static_cast<const float2 *>(spec), static_cast<float2 *>(spec_out), mag_out, C, T, F, tiles, width, k);
    else
        hipLaunchKernelGGL((wpe_mc_kernel<LPB, false>), dim3((unsigned)grid), dim3(WPE_MC_THREADS), 0, st,
                           static_cast<const float2 *>(spec), static_cast<float2 *>(spec_out), mag_out, C, T, F, tiles, width, k);
    return hipGetLastError();
}

}  // namespace

long wpe_grid(int n_groups, int C, int F, int K)
{
    return C == 1 ? wpe_grid_1ch(n_groups, F, K) : wpe_tile_grid(n_groups, F, wpe_mc_lanes_per_bin(C, K));
}

hipError_t launch_wpe(const void *spec, int n_groups, int C, int T, int F, const WpeConsts &k, void *spec_out, float *mag_out,
                      int width, hipStream_t st)
{
    // every statement of one channel reduces to "dereverb": the single-channel kernel, its bits
    if (C == 1) return launch_wpe_1ch(spec, n_groups, T, F, k, spec_out, mag_out, width, st);
    if (C < 1 || C > 8 || C * k.K > WPE_MC_NMAX) return hipErrorInvalidValue;
    switch (wpe_mc_lanes_per_bin(C, k.K)) {
    case 16: return launch<16>(spec, n_groups, C, T, F, k, spec_out, mag_out, width, st);
    case 32: return launch<32>(spec, n_groups, C, T, F, k, spec_out, mag_out, width, st);
    default: return launch<64>(spec, n_groups, C, T, F, k, spec_out, mag_out, width, st);
    }
}

}  // namespace adn
