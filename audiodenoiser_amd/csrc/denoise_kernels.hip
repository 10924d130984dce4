// Long-form denoising for gfx950: spectrogram -> network windows, network windows -> stitched spectrogram, and the fused
// way back to audio (stitch + clamp + noisy phase + inverse STFT of the input's length).  Definition: include/adn.h,
// "denoise"; float64 restatement: tests/denoise_ref.py.
//
// Layouts: the complex spectrogram X is FRAME-major [clip][frame][F] float2 (adn_stft_complex); the network's windows are
// bin-major [clip * K + k][F][Wd] with the window's frame index fastest.  Both directions are transpositions and go
// through LDS so that global reads and writes stay contiguous along the fastest index of their side.
//
// Kernels:
//   dn_windows   X -> |X| cut into K windows per clip (frames >= T zero), 32 x 32 tile through LDS
//   dn_stitch    y (windows) -> Y or max(Y, 0), (clip, F, T): linear cross-fade of the V shared frames, same layout both sides
//   dn_resynth   y, X -> audio (clip, L): resynthesis in stages and passes (ResynthCfg<M>, spectral.h) over the frames that cover a
//                workgroup's span (its own and the n_fft/hop - 1 halo frames of its neighbours, recomputed), fed with the
//                stitched magnitudes; the sums are normalised as the inverse STFT normalises them.  No stitched spectrogram,
//                no workspace.
#include "spectral.h"

#include <cfloat>

namespace adn {
namespace {

using namespace fftcore;

// Cover of frame f by the windows of the plan: the last window that starts at or before f (k_hi, local frame j_hi) and, inside
// a cross-fade, the one before it (local frame j_hi + S).  Weights as adn.h defines them: (j + 1) / (V + 1) rising in the later
// window, (W - j) / (V + 1) = (V - j_hi) / (V + 1) falling in the earlier one; 1 outside the cross-fades.
struct Cover {
    int k_hi, j_hi;
    bool two;
    float a_lo, a_hi;
};
__device__ __forceinline__ Cover cover_of(int f, const DenoiseGeom &g)
{
    Cover c;
    int k = f / g.S;
    if (k > g.K - 1) k = g.K - 1;
    c.k_hi = k;
    c.j_hi = f - k * g.S;
    c.two = k >= 1 && c.j_hi < g.V;
    const float d = (float)(g.V + 1);
    c.a_hi = c.two ? (float)(c.j_hi + 1) / d : 1.f;
    c.a_lo = c.two ? (float)(g.V - c.j_hi) / d : 0.f;
    return c;
}

// Y = a_lo * y_lo + a_hi * y_hi; a frame that one window covers is passed through untouched.  hipcc's __fmul_rn / __fadd_rn are
// the plain operators, so fp contraction may fuse either product, per call site: NOT always two rounded products and a rounded
// sum.  What is pinned: 4 eps sum_k a_k |y_k| for the stitch kernel (test_stitch_against_restatement; a fused product only
// tightens it), TOL between the fused kernel and the composed form (test_resynth), and each kernel's own bits as
// tools/spectral_digest.py records them -- run that tool before reshaping a loop that calls this.
__device__ __forceinline__ float blend(const Cover &c, float lo, float hi)
{
    return __fadd_rn(__fmul_rn(c.a_lo, lo), __fmul_rn(c.a_hi, hi));
}
__device__ __forceinline__ float stitch_at(const float *__restrict__ yc, int bin, int F, const DenoiseGeom &g, const Cover &c)
{
    const float hi = yc[((long)c.k_hi * F + bin) * g.Wd + c.j_hi];
    if (!c.two) return hi;
    const float lo = yc[((long)(c.k_hi - 1) * F + bin) * g.Wd + c.j_hi + g.S];
    return blend(c, lo, hi);
}

// ---------------------------------------------------------------------------------------------- windows
__global__ __launch_bounds__(256) void dn_windows_kernel(const float2 *__restrict__ X, int F, DenoiseGeom g, int tilesJ,
                                                         int tilesF, float *__restrict__ out)
{
    __shared__ float tile[32][33];
    unsigned b = blockIdx.x;
    const int tj = (int)(b % (unsigned)tilesJ);
    b /= (unsigned)tilesJ;
    const int tf = (int)(b % (unsigned)tilesF);
    const long win = b / (unsigned)tilesF;                       // clip * K + k
    const long clip = win / g.K;
    const int k = (int)(win - clip * g.K);
    const int j0 = tj * 32, f0 = tf * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int j = j0 + r, fr = k * g.S + j, bin = f0 + tx;
        float v = 0.f;
        if (j < g.Wd && fr < g.T && bin < F) v = mag_of(X[(clip * g.T + fr) * (long)F + bin]);
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int bin = f0 + r, j = j0 + tx;
        if (bin < F && j < g.Wd) out[(win * F + bin) * (long)g.Wd + j] = tile[tx][r];
    }
}

// ---------------------------------------------------------------------------------------------- stitch
// One thread = 4 consecutive frames of one (clip, bin) row.  VEC: T, Wd, S and V are multiples of 4, so the four frames share
// their cover and every row offset is a multiple of 4 floats: 16-byte loads and stores.
template <bool VEC>
__global__ __launch_bounds__(256) void dn_stitch_kernel(const float *__restrict__ y, int F, DenoiseGeom g, int tb, int clamp,
                                                        float *__restrict__ out)
{
    unsigned b = blockIdx.x;
    const int bx = (int)(b % (unsigned)tb);
    b /= (unsigned)tb;
    const int bin = (int)(b % (unsigned)F);
    const long clip = b / (unsigned)F;
    const long t0 = ((long)bx * 256 + threadIdx.x) * 4;
    if (t0 >= g.T) return;
    const float *yc = y + clip * g.K * (long)F * g.Wd;
    float *o = out + (clip * F + bin) * (long)g.T + t0;
    if (VEC) {
        const Cover c = cover_of((int)t0, g);
        const float4 h4 = *reinterpret_cast<const float4 *>(yc + ((long)c.k_hi * F + bin) * g.Wd + c.j_hi);
        float r[4] = {h4.x, h4.y, h4.z, h4.w};
        if (c.two) {
            const float4 l4 = *reinterpret_cast<const float4 *>(yc + ((long)(c.k_hi - 1) * F + bin) * g.Wd + c.j_hi + g.S);
            const float l[4] = {l4.x, l4.y, l4.z, l4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = blend(cover_of((int)t0 + e, g), l[e], r[e]);
        }
        if (clamp) {
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = relu_nan(r[e]);
        }
        *reinterpret_cast<float4 *>(o) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (t0 + e < g.T) {
                const float v = stitch_at(yc, bin, F, g, cover_of((int)t0 + e, g));
                o[e] = clamp ? relu_nan(v) : v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- fused resynthesis
// at the default n_fft 512 (70 KB of LDS) two workgroups fit a CU: the registers are capped at 128 there (fits without spills)
template <int M>
__global__ __launch_bounds__(STFT_THREADS, (M == 256 ? 4 : 2)) void dn_resynth_kernel(
    const float *__restrict__ y, const float2 *__restrict__ X, long L, int hop, DenoiseGeom g, int span, int nblk,
    const float *__restrict__ tables, float *__restrict__ audio)
{
    using C = ResynthCfg<M>;
    using S = SpecCfg<M>;
    constexpr int N = S::N, TPF = S::TPF, FB = S::FB, SB = C::SB, F = S::F, P = C::PITCH, SPT = C::SPT;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *s_win = smem;
    float2 *s_tw = reinterpret_cast<float2 *>(smem + N);
    float2 *s_tw2 = s_tw + M;                                   // exp(-2 pi i k / N), k = 0 .. M/2
    float2 *s_sc = reinterpret_cast<float2 *>(smem + S::TBL);
    float *s_fr = smem + S::TBL;                                // the same storage once a pass's frames are windowed: [FB][N]
    float *s_tile = smem + S::TBL + 2 * FB * M;                 // [SB][P] stitched, clamped magnitudes of the stage
    const int tid = threadIdx.x;
    for (int i = tid; i < S::TBL; i += STFT_THREADS) smem[i] = tables[i];

    const long clip = blockIdx.x / (unsigned)nblk;
    const int bx = (int)(blockIdx.x - clip * nblk);
    const long n0 = (long)bx * span;
    const long n1 = n0 + span < L ? n0 + span : L;
    const int T = g.T;
    // frames that cover the span: sample n sits at p = n + n_fft/2 of the untrimmed signal, inside frames
    // ceil((p - n_fft + 1) / hop) .. floor(p / hop), clipped to [0, T)
    const int f_begin = n0 + M < N ? 0 : (int)((n0 + M - N + hop) / hop);
    int f_end = (int)((n1 - 1 + M) / hop);
    if (f_end > T - 1) f_end = T - 1;

    // the thread's samples n0 + tid + u * 512 sit at p0 + u * 512 of the untrimmed signal
    const int p0 = (int)(n0 + tid + M);
    float acc[SPT];
#pragma unroll
    for (int u = 0; u < SPT; ++u) acc[u] = 0.f;

    const float *yc = y + clip * g.K * (long)F * g.Wd;
    const float2 *Xc = X + clip * (long)T * F;
    const int fl = tid / TPF, t = tid - fl * TPF;               // FFT role: frame slot, lane inside the frame
    const int jf = tid & (SB - 1), kb = tid / SB;               // staging role: frame of the stage, first bin
    const float inv = 1.0f / (float)M;

    for (int fs = f_begin; fs <= f_end; fs += SB) {
        {
            const int f = fs + jf;
            const bool lv = f <= f_end;
            const Cover c = cover_of(lv ? f : 0, g);
            constexpr int KS = STFT_THREADS / SB;                // bins between a thread's loads; 8 loads in flight per thread
            const float *y_hi = yc + (long)c.k_hi * F * g.Wd + c.j_hi;
            const float *y_lo = yc + (long)(c.two ? c.k_hi - 1 : c.k_hi) * F * g.Wd + c.j_hi + (c.two ? g.S : 0);
            for (int k0 = kb; k0 < F; k0 += 8 * KS) {
                float hi[8], lo[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int k = k0 + e * KS < F ? k0 + e * KS : F - 1;
                    hi[e] = y_hi[(long)k * g.Wd];
                }
                if (c.two) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int k = k0 + e * KS < F ? k0 + e * KS : F - 1;
                        lo[e] = y_lo[(long)k * g.Wd];
                    }
#pragma unroll
                    for (int e = 0; e < 8; ++e) hi[e] = blend(c, lo[e], hi[e]);
                }
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (k0 + e * KS < F) s_tile[jf * P + k0 + e * KS] = lv ? relu_nan(hi[e]) : 0.f;
            }
        }
        __syncthreads();
        for (int fp = fs; fp < fs + SB && fp <= f_end; fp += FB) {
            const int f = fp + fl;
            const bool live = f <= f_end;
            const float2 *Xf = Xc + (long)(live ? f : 0) * F;
            const float *mt = s_tile + (fp - fs + fl) * P;
            float2 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = t + u * TPF;                       // 0 .. M-1
                float2 xk = rephase(Xf[k], mt[k]), xm = rephase(Xf[M - k], mt[M - k]);
                if (k == 0) { xk.y = 0.f; xm.y = 0.f; }          // irfft ignores Im X[0], Im X[M]
                const float2 ev = make_float2(0.5f * (xk.x + xm.x), 0.5f * (xk.y - xm.y));
                const float2 d = make_float2(0.5f * (xk.x - xm.x), 0.5f * (xk.y + xm.y));
                float2 wi;
                if (k <= M / 2) { const float2 w = s_tw2[k]; wi = make_float2(w.x, -w.y); }
                else { const float2 w = s_tw2[M - k]; wi = make_float2(-w.x, -w.y); }
                const float2 od = cmul(wi, d);
                const float2 z = make_float2(ev.x - od.y, ev.y + od.x);
                v[u] = live ? make_float2(z.x, -z.y) : make_float2(0.f, 0.f);
            }
            float2 *sc = s_sc + fl * M;
            fft_frame<M>(sc, s_tw, t, v);
#pragma unroll
            for (int u = 0; u < 8; ++u) {                        // window in place: slot n holds samples 2n, 2n + 1
                const int n = t + u * TPF;
                const float2 z = sc[n];
                sc[n] = make_float2(s_win[2 * n] * (z.x * inv), s_win[2 * n + 1] * (-z.y * inv));
            }
            __syncthreads();
            // gather: frame fr holds the sample at j = p - fr * hop when 0 <= j < n_fft; frames ascend
            const int fr_last = fp + FB - 1 < f_end ? fp + FB - 1 : f_end;
            for (int fr = fp; fr <= fr_last; ++fr) {
                const float *frame = s_fr + (fr - fp) * N;
                const int j0 = p0 - fr * hop;
#pragma unroll
                for (int u = 0; u < SPT; ++u) {
                    const int j = j0 + u * STFT_THREADS;
                    const bool in = (unsigned)j < (unsigned)N;   // (the load is unconditional so that the eight go out together)
                    const float s = frame[in ? j : 0];
                    if (in) acc[u] += s;
                }
            }
            // no barrier here: the next pass overwrites the frames behind fft_frame's first barrier, and a new stage only
            // touches the tile, which every thread has finished reading before that same barrier
        }
    }
#pragma unroll
    for (int u = 0; u < SPT; ++u) {
        const long n = n0 + tid + u * STFT_THREADS;
        if (n >= n1) continue;
        // window sum-of-squares of the frames that cover the sample, the inverse STFT's normalisation
        const int p = p0 + u * STFT_THREADS;
        int f_hi = p / hop;
        if (f_hi > T - 1) f_hi = T - 1;
        const int f_lo = p < N ? 0 : (p - N + hop) / hop;
        float wss = 0.f;
        for (int fr = f_lo; fr <= f_hi; ++fr) {
            const float w = s_win[p - fr * hop];
            wss += w * w;
        }
        audio[clip * L + n] = wss > FLT_MIN ? acc[u] / wss : acc[u];
    }
}

template <int M>
hipError_t launch_resynth_m(const float *y, const float2 *X, int n_clips, long L, int hop, const DenoiseGeom &g,
                            const float *tables, float *audio, hipStream_t st)
{
    using C = ResynthCfg<M>;
    constexpr auto kern = dn_resynth_kernel<M>;
    const hipError_t e = lds_opt_in<kern>(C::LDS);
    if (e != hipSuccess) return e;
    // span: the most samples (<= SPAN) whose frames, halo included, fill whole FFT passes: hop * (k * FB - halo)
    constexpr int FB = SpecCfg<M>::FB;
    const int halo = (2 * M + hop - 1) / hop - 1;
    int span = C::SPAN;
    for (long k = 1; hop * (k * FB - halo) <= C::SPAN; ++k)
        if (k * FB > halo) span = (int)(hop * (k * FB - halo));
    const long nblk = (L + span - 1) / span;
    if (nblk * n_clips > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kern, dim3((unsigned)(nblk * n_clips)), dim3(STFT_THREADS), C::LDS, st, y, X, L, hop, g, span,
                       (int)nblk, tables, audio);
    return hipGetLastError();
}

}  // namespace

bool denoise_geom(int n_frames, int window, int overlap, DenoiseGeom *g)
{
    if (n_frames < 1 || window < 16 || overlap < 0 || overlap > window / 2) return false;
    g->T = n_frames;
    g->V = overlap;
    g->S = window - overlap;
    if (n_frames <= window) {
        g->K = 1;
        g->Wd = n_frames < 16 ? 16 : n_frames;
    } else {
        g->K = 1 + (n_frames - window + g->S - 1) / g->S;
        g->Wd = window;
    }
    return true;
}

hipError_t launch_denoise_windows(const void *spec, int n_clips, int F, const DenoiseGeom &g, float *out, hipStream_t st)
{
    const long tilesJ = (g.Wd + 31) / 32, tilesF = (F + 31) / 32;
    const long grid = tilesJ * tilesF * g.K * (long)n_clips;
    if (grid > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dn_windows_kernel, dim3((unsigned)grid), dim3(256), 0, st, static_cast<const float2 *>(spec), F, g,
                       (int)tilesJ, (int)tilesF, out);
    return hipGetLastError();
}

hipError_t launch_denoise_stitch(const float *y, int n_clips, int F, const DenoiseGeom &g, int clamp, float *out,
                                 hipStream_t st)
{
    const long tb = ((long)g.T + 1023) / 1024;
    const long grid = tb * F * (long)n_clips;
    if (grid > 0x7fffffffL) return hipErrorInvalidValue;
    const bool vec = ((g.T | g.Wd | g.S | g.V) & 3) == 0;
    if (vec)
        hipLaunchKernelGGL(dn_stitch_kernel<true>, dim3((unsigned)grid), dim3(256), 0, st, y, F, g, (int)tb, clamp, out);
    else
        hipLaunchKernelGGL(dn_stitch_kernel<false>, dim3((unsigned)grid), dim3(256), 0, st, y, F, g, (int)tb, clamp, out);
    return hipGetLastError();
}

hipError_t launch_denoise_resynth(const float *y, const void *spec, int n_clips, long L, int n_fft, int hop,
                                  const DenoiseGeom &g, float *audio, hipStream_t st)
{
    const float *tables = nullptr;
    hipError_t e = stft_tables(n_fft, &tables, st);
    if (e != hipSuccess) return e;
    const float2 *X = static_cast<const float2 *>(spec);
    return dispatch_n_fft(n_fft, [&](auto m) { return launch_resynth_m<m()>(y, X, n_clips, L, hop, g, tables, audio, st); });
}

}  // namespace adn
