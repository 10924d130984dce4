// Spectral baseline denoiser for gfx950: minimum-tracking noise estimate + decision-directed Wiener gain, frame after frame.
// Definition: include/adn.h, "baseline"; float64 restatement: tests/baseline_ref.py.
//
// Layouts: the complex spectrogram X is FRAME-major [clip][frame][F] float2 (adn_stft_complex); the result is the network-output
// layout that adn_denoise_resynth reads, bin-major [clip][F][width] with the frame index fastest; the state is [clip][3][F].
//
// Shape of the work.  A (clip, bin) row is a recurrence over its frames, rows are independent: one lane owns one row and walks it
// in frame order, a wave owns 64 consecutive bins of one clip, a workgroup is one wave.
//   reads   a frame of the wave is one coalesced 512-byte float2 load.  The loads do not depend on the recurrence: the TF frames
//           of tile k + 1 are issued into a second register image before tile k is computed (program order; the compiler waits
//           for them with counted vmcnt as the first step of the next tile reaches them), so a tile's TF x ~600 clocks of
//           arithmetic cover the next tile's HBM latency many times over.
//   writes  the output's fastest index is the frame, a direct store would be 64 scattered 4-byte writes per frame.  The TF x 64
//           magnitudes of a tile go through LDS, tile[TF][65]: a frame's 64 lanes write consecutive banks; read back transposed,
//           a half-wave holds the 32 frames of one bin at addresses j * 65 + b, bank (j + b) mod 32, all distinct -- and stores
//           them as one 128-byte row segment, two bins per wave-instruction.
//   chain   per frame three divisions and a square root, all correctly rounded (~75 vector instructions, most of them waiting
//           for the one before), and nothing to run beside them: measured 0.253 us per frame on the MI355X, about 600 clocks,
//           for a wave alone on its SIMD (profiles/bench_baseline.md).
// Cost: 12 n T F bytes (8 read, 4 written), and n ceil(F / 64) waves.  One clip at n_fft 512 is five waves on a chip of 1024
// SIMDs: the time is the chain, clocks per frame x T (T = 3751 for 60 s: 0.95 ms), whatever the bytes.  The bytes only set the
// time from some thousands of clips on (60 clips x 60 s: 0.69 GB, 87 us at 8 TB/s, against the same 0.95 ms chain on 300
// waves: 0.09 of the memory bound).  Cutting a row's frames into segments that run side by side would need warm-started state
// and would break the two bit guarantees of adn.h; it is not done.
//
// Bit guarantees (adn.h): every frame goes through the one `step` below, head, body and tail of a call alike, and the step is
// compiled with fp contraction off, so its arithmetic is the statements as written wherever the compiler inlines it: cutting
// the frames into calls elsewhere moves the tile boundaries and nothing else.
#include "adn_internal.h"

namespace adn {
namespace {

constexpr int BL_TF = 32;                            // frames per tile
constexpr int BL_PITCH = 65;                         // floats per tile row: odd, see above

struct RowState {
    float P, Pmin, S;
    bool fresh;
};

// max(x, c) of adn.h ("baseline"): a NaN x stays NaN
__device__ __forceinline__ float max_keep_nan(float x, float c) { return x < c ? c : x; }

// One frame of one row: the rules of adn.h, "baseline", one statement each.  Returns M_t.
__device__ __forceinline__ float step(float2 x, RowState &s, const SpectralConsts &k)
{
#pragma clang fp contract(off)
    const float p = fmaf(x.x, x.x, x.y * x.y);
    const float P = s.fresh ? p : k.smooth * s.P + k.one_minus_smooth * p;
    const float grown = k.gamma * s.Pmin + k.growth * (P - k.beta * s.P);
    const float Pmin = (!s.fresh && s.Pmin < P) ? grown : P;
    const float N = max_keep_nan(k.bias * Pmin, 1e-30f);
    const float Sprev = s.fresh ? 0.f : s.S;
    const float xi = (k.alpha * Sprev) / N + k.one_minus_alpha * max_keep_nan(p / N - 1.f, 0.f);
    const float G = max_keep_nan(xi / (1.f + xi), k.gain_floor);
    s.P = P;
    s.Pmin = Pmin;
    s.S = (G * G) * p;
    s.fresh = false;
    return G * sqrtf(p);
}

__global__ __launch_bounds__(64) void bl_spectral_gain_kernel(const float2 *__restrict__ X, int T, int F, int wavesF,
                                                              SpectralConsts k, const float *state_in, float *state_out,
                                                              float *__restrict__ out, int width, int col0)
{
    __shared__ float tile[BL_TF * BL_PITCH];
    const int lane = threadIdx.x;
    const long clip = blockIdx.x / (unsigned)wavesF;
    const int b0 = (int)(blockIdx.x - clip * wavesF) * 64;
    const bool live = b0 + lane < F;
    const int bin = live ? b0 + lane : F - 1;                    // lanes past the last bin walk it again and store nothing
    const float2 *x = X + clip * (long)T * F + bin;

    RowState s;
    s.P = -1.f;
    s.Pmin = 0.f;
    s.S = 0.f;
    if (state_in) {
        const float *si = state_in + clip * 3L * F + bin;
        s.P = si[0];
        s.Pmin = si[F];
        s.S = si[2L * F];
    }
    s.fresh = s.P < 0.f;                                         // a NaN P is no fresh start: the row stays poisoned

    float2 cur[BL_TF], nxt[BL_TF];
#pragma unroll
    for (int j = 0; j < BL_TF; ++j) cur[j] = x[(long)(j < T ? j : T - 1) * F];

    float *o = out + clip * (long)F * width + col0;
    const int jr = lane & 31, half = lane >> 5;
    for (int t0 = 0; t0 < T; t0 += BL_TF) {
        const int nf = T - t0 < BL_TF ? T - t0 : BL_TF;
        // the next tile's frames (the last frame again past the end: a valid address, never used)
#pragma unroll
        for (int j = 0; j < BL_TF; ++j) {
            const int t = t0 + BL_TF + j;
            nxt[j] = x[(long)(t < T ? t : T - 1) * F];
        }
#pragma unroll
        for (int j = 0; j < BL_TF; ++j)
            if (j < nf) tile[j * BL_PITCH + lane] = step(cur[j], s, k);
        __syncthreads();
        if (jr < nf) {
#pragma unroll 4
            for (int r = 0; r < 32; ++r) {
                const int b = 2 * r + half;
                if (b0 + b < F) o[(long)(b0 + b) * width + t0 + jr] = tile[jr * BL_PITCH + b];
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < BL_TF; ++j) cur[j] = nxt[j];
    }
    if (state_out && live) {
        float *so = state_out + clip * 3L * F + bin;
        so[0] = s.P;
        so[F] = s.Pmin;
        so[2L * F] = s.S;
    }
}

// The magnitude form (adn.h, "baseline", "The magnitude form"): the same rows of work on the layout of the stream classes.
//
// Layouts: windows and y are bin-major [row * n_steps + s][F][W] with the frame fastest -- what adn_stream_analyze writes and
// adn_stream_emit reads; frame t = s * n_cols + j of a row is column col0 + j of its step s.  The state is [slot][3][F], read and
// written in place by the lane that owns the row; the row's slot and its forced fresh start come from the table in the kernel
// arguments (t.n == 0: row i is slot i and continues).
//
// Shape of the work: as above, one lane per (row, bin), a wave is 64 consecutive bins of one row, one wave per workgroup, frames
// in order through the one `step` with X = (m, 0).
//   reads   the input's fastest index is the frame as well: a direct read would be 64 scattered 4-byte loads per frame.  A tile of
//           up to TF frames comes in the way it leaves: a half-wave reads the row segment of one bin (lane & 31 = the frame of the
//           tile: consecutive columns while the tile stays inside a step, and a tile may span steps -- n_cols need not divide 32 --
//           so every lane derives its frame's address from t / n_cols and t mod n_cols, once per tile), two bins per
//           wave-instruction, 32 registers per lane, and writes them into tile[frame][bin] at banks (j + b) mod 32.  The lanes
//           then read tile[j][lane], overwrite it with M, and the transposed store path of the kernel above writes it out: one
//           tile serves both directions.  The 32 loads of tile k + 1 are issued before tile k is computed, as above.
//   alias   y may be windows: every element of a tile is loaded before any store of that tile (the loads of tile k sit in
//           registers since tile k - 1; the loads of tile k + 1, issued before the stores of tile k, are other frames), and a
//           (row, bin) belongs to one lane of one workgroup.
// Lanes past the last bin walk the last bin again and frames past the end of a tile load the last frame again -- valid addresses --
// and store nothing.
// Expected cost, NOT MEASURED for this kernel: chain-bound like its sibling, whose 0.253 us per frame is the only time measured
// so far; carried over from that, about 1 us for a step of four frames.  A single feed at n_fft 512 is five waves and
// launch-bound; a tick of 256 feeds is 1280 waves, still about one wave per SIMD.  What was measured: profiles/bench_baseline_stream.md.
__global__ __launch_bounds__(64) void bl_spectral_gain_windows_kernel(const float *win, float *y, int n_steps, int F, int W, int col0,
                                                                      int n_cols, int T, int wavesF, SpectralConsts k,
                                                                      float *state, SpectralRows t)
{
    __shared__ float tile[BL_TF * BL_PITCH];
    const int lane = threadIdx.x;
    const int row = blockIdx.x / (unsigned)wavesF;
    const int b0 = (int)(blockIdx.x - (unsigned)row * wavesF) * 64;
    const bool live = b0 + lane < F;
    const int bin = live ? b0 + lane : F - 1;
    const long slot = t.n ? t.row[row].slot : row;
    const bool forced = t.n ? t.row[row].fresh != 0 : false;

    RowState s;
    float *sp = state + slot * 3L * F + bin;
    s.P = sp[0];
    s.Pmin = sp[F];
    s.S = sp[2L * F];
    s.fresh = forced || s.P < 0.f;                               // a NaN P is no fresh start unless the row table forces one

    const long FW = (long)F * W;
    const long base = (long)row * n_steps * FW + col0;           // column col0 of bin 0 of the row's step 0
    const int jr = lane & 31, half = lane >> 5;
    // the address of this lane's frame of the tile at t0, bin 0 (the last frame again past the end: valid, never used)
    const auto frame_at = [&](long t0) -> long {
        const int f = (int)(t0 + jr < T ? t0 + jr : T - 1);
        const int st = f / n_cols;
        return base + st * FW + (f - st * n_cols);
    };
    // a lane's 32 loads of a tile: its frame, bins b0 + 2 r + half (the last bin again past it)
    float cur[BL_TF], nxt[BL_TF];
    {
        const long at = frame_at(0);
#pragma unroll
        for (int r = 0; r < BL_TF; ++r) {
            const int b = b0 + 2 * r + half;
            cur[r] = win[at + (long)(b < F ? b : F - 1) * W];
        }
    }
    for (long t0 = 0; t0 < T; t0 += BL_TF) {
        const int nf = T - t0 < BL_TF ? (int)(T - t0) : BL_TF;
        {
            const long at = frame_at(t0 + BL_TF);
#pragma unroll
            for (int r = 0; r < BL_TF; ++r) {
                const int b = b0 + 2 * r + half;
                nxt[r] = win[at + (long)(b < F ? b : F - 1) * W];
            }
        }
#pragma unroll
        for (int r = 0; r < BL_TF; ++r) tile[jr * BL_PITCH + 2 * r + half] = cur[r];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < BL_TF; ++j)
            if (j < nf) tile[j * BL_PITCH + lane] = step(make_float2(tile[j * BL_PITCH + lane], 0.f), s, k);
        __syncthreads();
        if (jr < nf) {
            const long at = frame_at(t0);
#pragma unroll 4
            for (int r = 0; r < 32; ++r) {
                const int b = 2 * r + half;
                if (b0 + b < F) y[at + (long)(b0 + b) * W] = tile[jr * BL_PITCH + b];
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < BL_TF; ++r) cur[r] = nxt[r];
    }
    if (live) {
        sp[0] = s.P;
        sp[F] = s.Pmin;
        sp[2L * F] = s.S;
    }
}

}  // namespace

hipError_t launch_spectral_gain_windows(const float *windows, float *y, int n_rows, int n_steps, int F, int W, int col0, int n_cols,
                                        const SpectralConsts &k, float *state, const SpectralRows &rows, hipStream_t st)
{
    const long wavesF = ((long)F + 63) / 64;
    const long grid = wavesF * n_rows, T = (long)n_steps * n_cols;
    if (grid > 0x7fffffffL || T > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bl_spectral_gain_windows_kernel, dim3((unsigned)grid), dim3(64), 0, st, windows, y, n_steps, F, W, col0,
                       n_cols, (int)T, (int)wavesF, k, state, rows);
    return hipGetLastError();
}

hipError_t launch_spectral_gain(const void *spec, int n_clips, int T, int F, const SpectralConsts &k, const float *state_in,
                                float *state_out, float *out, int width, int col0, hipStream_t st)
{
    const long wavesF = ((long)F + 63) / 64;
    const long grid = wavesF * n_clips;
    if (grid > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bl_spectral_gain_kernel, dim3((unsigned)grid), dim3(64), 0, st, static_cast<const float2 *>(spec), T, F,
                       (int)wavesF, k, state_in, state_out, out, width, col0);
    return hipGetLastError();
}

}  // namespace adn
