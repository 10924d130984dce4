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

}  // namespace

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
