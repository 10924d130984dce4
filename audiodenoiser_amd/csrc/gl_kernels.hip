// Inverse STFT and the reference's Griffin-Lim loop for gfx950.
//
// Replaces /root/reference/code/test.py:29-48 (griffin_lim_reconstruction): librosa.istft + librosa.stft iterated
// from a random-phase start.  Semantics (librosa 0.10 defaults): n_fft = 2(F-1), win_length = n_fft, periodic Hann,
// center=True with zero padding, istft length = hop*(T-1) after trimming n_fft/2 from both ends, overlap-added
// signal divided by the window sum-of-squares where that exceeds FLT_MIN.
//
// Layout: inside the loop the complex spectrogram is FRAME-major, [clip][frame][F] float2 -- a frame's bins are
// contiguous, so both transforms read and write coalesced and no transposition is needed; only the entry kernel
// (magnitude x random phase) reads the reference's [F][T] layout, through an LDS tile.
//
// Kernels (one iteration = istft_frames -> istft_ola -> stft_complex):
//   gl_polar       mag (N,F,T), rnd (N,F,T) in [0,1)  ->  spec (N,T,F) = mag * exp(2 pi i rnd)
//   istft_frames   spec (N,T,F) -> buf (N,T,n_fft) = window * irfft(frame)   (inverse real FFT = forward FFT of the
//                  conjugated half-size complex sequence; DC/Nyquist imaginary parts ignored like numpy's irfft)
//   istft_ola      buf -> audio (N, hop*(T-1)): each sample gathers its n_fft/hop frames (deterministic, no atomics)
//                  and is normalised by the window sum-of-squares computed from the same frame range
//   stft_complex   audio (N,L) -> spec (N,T,F), centred, zero padded (the magnitude kernel's transform, complex out)
// The "S = |Z| * exp(i angle(Z))" step of test.py:46 is the identity on Z up to two roundings; the loop keeps Z.
#include "spectral.h"

#include <cfloat>

namespace adn {
namespace {

using namespace fftcore;

// ---------------------------------------------------------------------------------------------- polar
__global__ __launch_bounds__(256) void gl_polar_kernel(const float *__restrict__ mag, const float *__restrict__ rnd,
                                                       int F, int T, float2 *__restrict__ spec)
{
    __shared__ float2 tile[32][33];
    const long clip = blockIdx.z;
    const int f0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int k = k0 + r, f = f0 + tx;
        float2 v = make_float2(0.f, 0.f);
        if (k < F && f < T) {
            const long i = (clip * F + k) * T + f;
            float s, c;
            sincospif(2.0f * rnd[i], &s, &c);
            const float m = mag[i];
            v = make_float2(m * c, m * s);
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int f = f0 + r, k = k0 + tx;
        if (k < F && f < T) spec[(clip * T + f) * F + k] = tile[tx][r];
    }
}

// ---------------------------------------------------------------------------------------------- inverse frames
template <int M>
__global__ __launch_bounds__(STFT_THREADS) void istft_frames_kernel(const float2 *__restrict__ spec, int T,
                                                                   const float *__restrict__ tables,
                                                                   float *__restrict__ buf)
{
    using C = SpecCfg<M>;
    constexpr int N = C::N, TPF = C::TPF, FB = C::FB, F = C::F;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const SpecTables tb = C::view(smem);
    C::load(smem, tables);
    __syncthreads();

    const int tid = threadIdx.x, fl = tid / TPF, t = tid - fl * TPF;
    const long clip = blockIdx.y;
    const int f = blockIdx.x * FB + fl;
    const bool live = f < T;
    const float2 *X = spec + (clip * T + (live ? f : 0)) * F;
    float2 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int k = t + u * TPF;                               // 0 .. M-1
        float2 xk = X[k], xm = X[M - k];
        if (k == 0) { xk.y = 0.f; xm.y = 0.f; }                  // (the inverse real-FFT split: spectral.h)
        const float2 ev = make_float2(0.5f * (xk.x + xm.x), 0.5f * (xk.y - xm.y));
        const float2 d = make_float2(0.5f * (xk.x - xm.x), 0.5f * (xk.y + xm.y));
        float2 wi;
        if (k <= M / 2) { const float2 w = tb.tw2[k]; wi = make_float2(w.x, -w.y); }
        else { const float2 w = tb.tw2[M - k]; wi = make_float2(-w.x, -w.y); }
        const float2 od = cmul(wi, d);
        const float2 z = make_float2(ev.x - od.y, ev.y + od.x);
        v[u] = live ? make_float2(z.x, -z.y) : make_float2(0.f, 0.f);
    }
    float2 *sc = C::frames(smem) + fl * M;
    fft_frame<M>(sc, tb.tw, t, v);
    if (live) {
        float *o = buf + (clip * T + f) * (long)N;
        const float inv = 1.0f / (float)M;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int n = t + u * TPF;
            const float2 z = sc[n];                              // conj -> x[2n] = Re, x[2n+1] = -Im
            *reinterpret_cast<float2 *>(o + 2 * n) =
                make_float2(tb.win[2 * n] * (z.x * inv), tb.win[2 * n + 1] * (-z.y * inv));
        }
    }
}

// ---------------------------------------------------------------------------------------------- overlap-add
__global__ __launch_bounds__(256) void istft_ola_kernel(const float *__restrict__ buf, int T, int n_fft, int hop,
                                                        long out_len, const float *__restrict__ win,
                                                        float *__restrict__ audio)
{
    const long clip = blockIdx.y;
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= out_len) return;
    const long p = n + n_fft / 2;                                // index in the untrimmed signal
    long f_hi = p / hop;
    if (f_hi > T - 1) f_hi = T - 1;
    long f_lo = (p - n_fft + hop) / hop;                         // ceil((p - n_fft + 1) / hop) for p >= n_fft - hop
    if (p < n_fft) f_lo = 0;
    const float *b = buf + clip * T * (long)n_fft;
    float s = 0.f, wss = 0.f;
    for (long f = f_lo; f <= f_hi; ++f) {
        const int j = (int)(p - f * hop);
        s += b[f * n_fft + j];
        const float w = win[j];
        wss += w * w;
    }
    audio[clip * out_len + n] = wss > FLT_MIN ? s / wss : s;
}

// ---------------------------------------------------------------------------------------------- complex STFT
template <int M>
__global__ __launch_bounds__(STFT_THREADS) void stft_complex_kernel(const float *__restrict__ audio, long L, int hop,
                                                                   int pad, int T, const float *__restrict__ tables,
                                                                   float2 *__restrict__ spec)
{
    using C = SpecCfg<M>;
    constexpr int TPF = C::TPF, FB = C::FB, F = C::F;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const SpecTables tb = C::view(smem);
    C::load(smem, tables);
    __syncthreads();

    const int tid = threadIdx.x, fl = tid / TPF, t = tid - fl * TPF;
    const long clip = blockIdx.y;
    const int f = blockIdx.x * FB + fl;
    const bool live = f < T;
    const float *a = audio + clip * L;
    const long s0 = (long)(live ? f : 0) * hop - pad;
    float2 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int n2 = 2 * (t + u * TPF);
        const long s = s0 + n2;
        const float x0 = (live && s >= 0 && s < L) ? a[s] : 0.f;
        const float x1 = (live && s + 1 >= 0 && s + 1 < L) ? a[s + 1] : 0.f;
        v[u] = make_float2(tb.win[n2] * x0, tb.win[n2 + 1] * x1);
    }
    float2 *sc = C::frames(smem) + fl * M;
    fft_frame<M>(sc, tb.tw, t, v);
    if (live) {
        float2 *o = spec + (clip * T + f) * (long)F;
        forward_split<M>(sc, tb.tw2, t, [&](int k, float2 xa, float2 xb) { o[k] = xa; o[M - k] = xb; },
                         [&](float2 x0, float2 xM, float2 xh) { o[0] = x0; o[M] = xM; o[M / 2] = xh; });
    }
}

template <int M>
hipError_t launch_istft_frames_m(const float2 *spec, int n_clips, int T, const float *tables, float *buf, hipStream_t st)
{
    using C = SpecCfg<M>;
    constexpr auto kern = istft_frames_kernel<M>;
    const hipError_t e = lds_opt_in<kern>(C::LDS);
    if (e != hipSuccess) return e;
    dim3 grid((unsigned)((T + C::FB - 1) / C::FB), (unsigned)n_clips);
    hipLaunchKernelGGL(kern, grid, dim3(STFT_THREADS), C::LDS, st, spec, T, tables, buf);
    return hipGetLastError();
}

template <int M>
hipError_t launch_stft_complex_m(const float *audio, int n_clips, long L, int hop, int pad, int T, const float *tables,
                                 float2 *spec, hipStream_t st)
{
    using C = SpecCfg<M>;
    constexpr auto kern = stft_complex_kernel<M>;
    const hipError_t e = lds_opt_in<kern>(C::LDS);
    if (e != hipSuccess) return e;
    dim3 grid((unsigned)((T + C::FB - 1) / C::FB), (unsigned)n_clips);
    hipLaunchKernelGGL(kern, grid, dim3(STFT_THREADS), C::LDS, st, audio, L, hop, pad, T, tables, spec);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_gl_polar(const float *mag, const float *rnd, int n_clips, int F, int T, void *spec, hipStream_t st)
{
    dim3 grid((unsigned)((T + 31) / 32), (unsigned)((F + 31) / 32), (unsigned)n_clips);
    hipLaunchKernelGGL(gl_polar_kernel, grid, dim3(256), 0, st, mag, rnd, F, T, static_cast<float2 *>(spec));
    return hipGetLastError();
}

hipError_t launch_istft_frames(const void *spec, int n_clips, int T, int n_fft, float *buf, hipStream_t st)
{
    const float *tables = nullptr;
    hipError_t e = stft_tables(n_fft, &tables, st);
    if (e != hipSuccess) return e;
    const float2 *s = static_cast<const float2 *>(spec);
    return dispatch_n_fft(n_fft, [&](auto m) { return launch_istft_frames_m<m()>(s, n_clips, T, tables, buf, st); });
}

hipError_t launch_istft_ola(const float *buf, int n_clips, int T, int n_fft, int hop, float *audio, hipStream_t st)
{
    const float *tables = nullptr;
    hipError_t e = stft_tables(n_fft, &tables, st);
    if (e != hipSuccess) return e;
    const long out_len = (long)hop * (T - 1);
    if (out_len <= 0) return hipErrorInvalidValue;
    dim3 grid((unsigned)((out_len + 255) / 256), (unsigned)n_clips);
    hipLaunchKernelGGL(istft_ola_kernel, grid, dim3(256), 0, st, buf, T, n_fft, hop, out_len, tables, audio);
    return hipGetLastError();
}

hipError_t launch_stft_complex(const float *audio, int n_clips, long L, int n_fft, int hop, int T, void *spec,
                               hipStream_t st)
{
    const float *tables = nullptr;
    hipError_t e = stft_tables(n_fft, &tables, st);
    if (e != hipSuccess) return e;
    float2 *s = static_cast<float2 *>(spec);
    const int pad = n_fft / 2;
    return dispatch_n_fft(n_fft, [&](auto m) { return launch_stft_complex_m<m()>(audio, n_clips, L, hop, pad, T, tables, s, st); });
}

}  // namespace adn
