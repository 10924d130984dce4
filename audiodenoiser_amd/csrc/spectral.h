// What the workgroup-synchronous spectral kernels (STFT, inverse STFT, Griffin-Lim, denoise resynthesis, stream) share, stated
// once: the table layout and its LDS view, the forward real-FFT split, the magnitude / phase rules of adn.h, the LDS budget of
// the resynthesis that the denoiser and the stream run on the way back to audio, and the dispatch over n_fft.
// The FFT itself is fft_core.h.  M = n_fft / 2 complex points per frame throughout.
#pragma once
#include "adn_internal.h"
#include "fft_core.h"

#include <type_traits>

namespace adn {
namespace fftcore {

// Tables of one n_fft (stft_tables; fp32, computed in double on the host), in this order: win[N] periodic Hann,
// tw[M] = exp(-2 pi i j / M), tw2[M/2 + 1] = exp(-2 pi i k / N) padded to an even count of floats.
struct SpecTables {
    const float *win;
    const float2 *tw, *tw2;
};

template <int M>
struct SpecCfg {
    static constexpr int N = 2 * M, F = M + 1;
    static constexpr int TPF = M / 8, FB = STFT_THREADS / TPF;          // threads per frame, frames per FFT pass of a workgroup
    static constexpr int TBL = N + 2 * M + (M + 2);                     // floats of the tables
    static constexpr size_t LDS = (size_t)(TBL + 2 * FB * M) * sizeof(float);   // tables + one pass of frames

    // The tables sit at the start of dynamic LDS; the FFT images of a pass ([FB][M] float2) follow them.
    static __device__ __forceinline__ SpecTables view(const float *smem)
    {
        const float2 *tw = reinterpret_cast<const float2 *>(smem + N);
        return {smem, tw, tw + M};
    }
    static __device__ __forceinline__ float2 *frames(float *smem) { return reinterpret_cast<float2 *>(smem + TBL); }
    // Cooperative copy by STFT_THREADS threads.  No barrier: the caller's next one publishes the tables.
    static __device__ __forceinline__ void load(float *smem, const float *__restrict__ tables)
    {
        for (int i = threadIdx.x; i < TBL; i += STFT_THREADS) smem[i] = tables[i];
    }
};

// Calls f(M) with M = n_fft / 2 as a std::integral_constant for the n_fft the library supports.
template <class Fn>
hipError_t dispatch_n_fft(int n_fft, Fn f)
{
    switch (n_fft) {
        case 64: return f(std::integral_constant<int, 32>{});
        case 128: return f(std::integral_constant<int, 64>{});
        case 256: return f(std::integral_constant<int, 128>{});
        case 512: return f(std::integral_constant<int, 256>{});
        case 1024: return f(std::integral_constant<int, 512>{});
        case 2048: return f(std::integral_constant<int, 1024>{});
        case 4096: return f(std::integral_constant<int, 2048>{});
        default: return hipErrorInvalidValue;
    }
}

// ---------------------------------------------------------------------------------------------- real-FFT split
// Forward: Z = FFT of the frame packed as z[n] = x[2n] + i x[2n+1], in `sc`.  With w = exp(-2 pi i / n_fft),
//   X[k] = Ev[k] + w^k Od[k],  X[M-k] = conj(Ev[k] - w^k Od[k]),  Ev = (Z[k] + conj Z[M-k]) / 2,  Od = (Z[k] - conj Z[M-k]) / 2i.
// Lane t of the frame's M/8 handles k = t + b M/8, b = 0..3: pair(k, X[k], X[M-k]) for 0 < k < M/2, and the lane with k = 0
// also gets edges(X[0], X[M], X[M/2]).  (stft_mag_kernel keeps its own copy: see there.)
template <int M, class Pair, class Edges>
__device__ __forceinline__ void forward_split(const float2 *sc, const float2 *tw2, int t, Pair pair, Edges edges)
{
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int k = t + b * (M / 8);                                // 0 .. M/2-1
        if (k == 0) {
            const float2 z0 = sc[0], zh = sc[M / 2];
            edges(make_float2(z0.x + z0.y, 0.f), make_float2(z0.x - z0.y, 0.f), make_float2(zh.x, -zh.y));
        } else {
            const float2 A = sc[k], Bc = sc[M - k];
            const float2 ev = make_float2(0.5f * (A.x + Bc.x), 0.5f * (A.y - Bc.y));
            const float2 d = make_float2(0.5f * (A.x - Bc.x), 0.5f * (A.y + Bc.y));
            const float2 wo = cmul(tw2[k], make_float2(d.y, -d.x));     // w^k * (d / i)
            const float2 xb = csub(ev, wo);
            pair(k, cadd(ev, wo), make_float2(xb.x, -xb.y));
        }
    }
}

// Inverse: X (xk = X[k], xm = X[M-k]; Im X[0] and Im X[M] ignored, as numpy's irfft does) -> point k (0 .. M-1) of conj(Z), Z =
// Ev + i Od the half-size sequence; the inverse transform is then run as conj(FFT(conj Z)) and slot n of its output holds the
// samples x[2n] = Re / M, x[2n+1] = -Im / M.  There is no function for it: its sums of products are left to hipcc's fp
// contraction, which follows the shape of the code, and the outputs are pinned bit for bit (tools/spectral_digest.py) -- the
// text stands where it runs (istft_frames_kernel, dn_resynth_kernel, stream_emit_kernel) and must stay the same text.

// ---------------------------------------------------------------------------------------------- magnitude and phase
// |X| as adn.h fixes it ("denoise", rule 2): one product, one fma, one square root
__device__ __forceinline__ float mag_of(float2 x) { return sqrtf(fmaf(x.x, x.x, __fmul_rn(x.y, x.y))); }

// S^[k] = m * X[k] / |X[k]|, m real where |X| = 0 ("denoise", rule 5)
__device__ __forceinline__ float2 rephase(float2 x, float m)
{
    const float mag = mag_of(x);
    if (mag == 0.f) return make_float2(m, 0.f);
    const float s = m / mag;
    return make_float2(x.x * s, x.y * s);
}

// ---------------------------------------------------------------------------------------------- resynthesis
// Network magnitudes + the input's phase -> audio, without a stitched spectrogram or a frame buffer: the plan that
// dn_resynth_kernel and stream_emit_kernel follow.  Positions are those of the untrimmed signal: frame f covers
// [f hop, f hop + n_fft), output sample n sits at p = n + n_fft/2, and the frames that cover p are
// ceil((p - n_fft + 1) / hop) .. floor(p / hop), clipped to [0, T) once T is known.  A workgroup owns up to SPAN positions, thread
// tid the SPT positions p0 + u * STFT_THREADS, and walks the frames that cover them in STAGES of SB frames: the stage's clamped
// magnitudes are read along the frame axis (the network's fastest) and parked in LDS behind the tables and a pass of frames, at
// tile[slot * PITCH + bin]; then PASSES of FB frames rescale X (rephase), run the inverse real FFT, window the frames in place,
// and every thread gathers its samples from the pass's frames in ascending frame order -- one chain of fp32 adds per sample, no
// atomics -- before the sum is divided by the window sum-of-squares of the covering frames where that exceeds FLT_MIN.
// The two kernels each carry this loop themselves: as one function it cost dn_resynth_kernel 0.2 - 0.4 % of its time on the
// MI355X, in every form tried, and their outputs are pinned bit for bit, so the text of the loop is the same in both and
// must stay so.
template <int M>
struct ResynthCfg {
    using S = SpecCfg<M>;
    static constexpr int SB0 = 16384 / M < 32 ? 16384 / M : 32;
    static constexpr int SB = S::FB > SB0 ? S::FB : SB0;                  // frames per stage: 32 (128-byte runs of y) while the
                                                                          // tile stays near 64 KB: 16 at n_fft 2048, 8 at 4096
    static constexpr int PITCH = M + 1;                                   // odd: lanes along the frame axis hit distinct banks
    static constexpr int SPT = 8, SPAN = STFT_THREADS * SPT;              // positions per thread / per workgroup
    static constexpr size_t LDS = S::LDS + (size_t)SB * PITCH * sizeof(float);   // tables, a pass of frames, the stage's tile
    static_assert(SB % S::FB == 0 && STFT_THREADS % SB == 0 && (SB & (SB - 1)) == 0, "bad stage size");
    static_assert(LDS <= 160 * 1024, "stage does not fit the LDS of a CU");
};

}  // namespace fftcore
}  // namespace adn
