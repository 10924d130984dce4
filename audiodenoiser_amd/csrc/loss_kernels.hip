// Per-clip CombinedPerceptualLoss on the device — the payload of the multi-GPU all-gather.
//
// Replaces, per clip, the arithmetic of /root/reference/code/loss.py:
//   MultiScaleSTFTLoss (loss.py:6-35): mean over the frequency axis -> a series of T values; for (n_fft, hop) in
//     ((63,16),(32,8),(16,4)): |STFT| with a rectangular window, centred, zero padded; mean |.|-difference; /3
//   MelSpectrogramLoss (loss.py:37-69): torchaudio MelSpectrogram(sr 8000, n_fft 63, hop 16, 64 mels): periodic
//     Hann, centred with reflect padding, power 2, HTK filters (norm None) -> mean |.|-difference
//   CombinedPerceptualLoss (loss.py:71-95): 0.4 stft + 0.4 mel + 0.2 * mean|pred - target|
// Every clip contributes equally many elements to each l1_loss, so the reference's batch values are the means
// over clips of the four numbers written here: out[clip] = {total, stft, mel, l1}.
//
// Two launches: (1) HBM-bound column sums over row slabs (reads both spectrogram batches once, coalesced along
// the frame axis, deterministic partials — no float atomics); (2) one workgroup per clip reduces the partials and
// does the tiny transforms (n_fft <= 63: direct DFT from LDS, 0.12 MFLOP per clip).
#include "adn_internal.h"

#include <cmath>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

namespace adn {
namespace {

constexpr int LOSS_ROWS = 32;      // spectrogram rows per slab workgroup

// partial[clip][slab][0..T) = sum_f pred, [T..2T) = sum_f target, [2T] = sum |pred - target| over the slab's rows
__global__ __launch_bounds__(256) void loss_colsum_kernel(const float *__restrict__ pred, const float *__restrict__ tgt,
                                                          int F, int T, int nslab, float *__restrict__ partial)
{
    __shared__ float red[4];
    const int slab = blockIdx.x % nslab;
    const long clip = blockIdx.x / nslab;
    const int f0 = slab * LOSS_ROWS, f1 = min(f0 + LOSS_ROWS, F);
    const float *p = pred + clip * (long)F * T, *q = tgt + clip * (long)F * T;
    float *out = partial + (clip * nslab + slab) * (long)(2 * T + 1);
    float l1 = 0.f;
    for (int t = threadIdx.x; t < T; t += 256) {
        float sp = 0.f, sq = 0.f;
#pragma unroll 4
        for (int f = f0; f < f1; ++f) {
            const float a = p[(long)f * T + t], b = q[(long)f * T + t];
            sp += a;
            sq += b;
            l1 += fabsf(a - b);
        }
        out[t] = sp;
        out[T + t] = sq;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) l1 += __shfl_down(l1, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = l1;
    __syncthreads();
    if (threadIdx.x == 0) out[2 * T] = red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ float block_sum(float v, float *red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// melfb: [32 freqs][64 mels] fp32 (host, double precision -> float)
// BIG = false (T <= ADN_LOSS_LDS_T): the clip's two frequency-mean series and the mel power spectra of ALL its frames live in the
// CU's LDS.  BIG = true (longer clips: the reference's loss has no length limit, loss.py:23-34,60-66): the series live in
// `series_g` (2 T floats per clip of the workspace, written and read by this workgroup only, L2-resident) and the mel term walks
// the frames in blocks of LOSS_MEL_FB.
constexpr int LOSS_MEL_FB = 256;
template <bool BIG>
__global__ __launch_bounds__(256) void loss_finish_kernel(const float *__restrict__ partial, int F, int T, int nslab,
                                                          const float *__restrict__ melfb, float *series_g, float *__restrict__ out)
{
    extern __shared__ float sm[];
    const long clip = blockIdx.x;
    float *sp = BIG ? series_g + clip * 2 * (long)T : sm, *sq = sp + T;      // frequency-mean series of pred / target
    float *tc = BIG ? sm : sq + T, *ts = tc + 64;  // cos / sin table of the current transform length (<= 63)
    float *specp = ts + 64;                       // mel: |X|^2 [32][frames of a block], pred then target
    __shared__ float red[4];
    const float *pp = partial + clip * nslab * (long)(2 * T + 1);
    const int tid = threadIdx.x;

    float l1 = 0.f;
    for (int t = tid; t < T; t += 256) {
        float a = 0.f, b = 0.f;
        for (int s = 0; s < nslab; ++s) {
            a += pp[(long)s * (2 * T + 1) + t];
            b += pp[(long)s * (2 * T + 1) + T + t];
        }
        sp[t] = a / (float)F;
        sq[t] = b / (float)F;
    }
    for (int s = tid; s < nslab; s += 256) l1 += pp[(long)s * (2 * T + 1) + 2 * T];
    const float l1_mean = block_sum(l1, red) / ((float)F * (float)T);

    // ---- multi-scale |STFT|, rectangular window, centred, zero padded (torch.stft(..., pad_mode="constant")) ----
    float stft_acc = 0.f;
    const int nfft_s[3] = {63, 32, 16}, hop_s[3] = {16, 8, 4};
#pragma unroll 1
    for (int sc = 0; sc < 3; ++sc) {
        const int n = nfft_s[sc], hop = hop_s[sc];
        const int pad = n / 2, nb = n / 2 + 1, nfr = 1 + (T + 2 * pad - n) / hop;   // odd n_fft: 1 + (T-1)/hop
        __syncthreads();
        if (tid < n) {
            float s, c;
            sincospif(2.0f * (float)tid / (float)n, &s, &c);
            tc[tid] = c;
            ts[tid] = -s;
        }
        __syncthreads();
        float acc = 0.f;
        for (int it = tid; it < nb * nfr; it += 256) {
            const int k = it / nfr, fr = it - k * nfr;
            float pr = 0.f, pi = 0.f, qr = 0.f, qi = 0.f;
            int idx = 0;                                              // (k * i) mod n
            for (int i = 0; i < n; ++i) {
                const int s = fr * hop - pad + i;
                if (s >= 0 && s < T) {
                    const float c = tc[idx], sn = ts[idx], a = sp[s], b = sq[s];
                    pr += a * c; pi += a * sn; qr += b * c; qi += b * sn;
                }
                idx += k;
                if (idx >= n) idx -= n;
            }
            acc += fabsf(sqrtf(pr * pr + pi * pi) - sqrtf(qr * qr + qi * qi));
        }
        stft_acc += block_sum(acc, red) / (float)(nb * nfr);
    }
    const float stft_mean = stft_acc / 3.0f;

    // ---- mel: periodic Hann, n_fft 63, hop 16, centred with REFLECT padding, power 2, 32 bins -> 64 mel filters ----
    const int n = 63, hop = 16, pad = 31, nb = 32, nfr = 1 + (T + 2 * pad - n) / hop;
    const int fb = BIG ? LOSS_MEL_FB : nfr;       // frames per block (!BIG: one block holds them all)
    float *specq = specp + nb * fb;
    __syncthreads();
    if (tid < n) {
        float s, c;
        sincospif(2.0f * (float)tid / (float)n, &s, &c);
        tc[tid] = c;
        ts[tid] = -s;
    }
    __syncthreads();
    float macc = 0.f;
    for (int f0 = 0; f0 < nfr; f0 += fb) {
        const int nf = min(fb, nfr - f0);             // frames of this block
        for (int it = tid; it < nb * nf; it += 256) {
            const int k = it / nf, fr = it - k * nf;
            float pr = 0.f, pi = 0.f, qr = 0.f, qi = 0.f;
            int idx = 0;
            for (int i = 0; i < n; ++i) {
                int s = (f0 + fr) * hop - pad + i;
                s = s < 0 ? -s : (s >= T ? 2 * (T - 1) - s : s);          // reflect (no edge repeat)
                const float w = 0.5f - 0.5f * tc[i];                     // periodic Hann: 0.5 - 0.5 cos(2 pi i / n)
                const float c = tc[idx], sn = ts[idx], a = w * sp[s], b = w * sq[s];
                pr += a * c; pi += a * sn; qr += b * c; qi += b * sn;
                idx += k;
                if (idx >= n) idx -= n;
            }
            specp[k * nf + fr] = pr * pr + pi * pi;
            specq[k * nf + fr] = qr * qr + qi * qi;
        }
        __syncthreads();
        for (int it = tid; it < 64 * nf; it += 256) {
            const int m = it / nf, fr = it - m * nf;
            float a = 0.f, b = 0.f;
            for (int f = 0; f < nb; ++f) {
                const float w = melfb[f * 64 + m];
                a += w * specp[f * nf + fr];
                b += w * specq[f * nf + fr];
            }
            macc += fabsf(a - b);
        }
        if (BIG) __syncthreads();                     // the tables are refilled by the next block
    }
    const float mel_mean = block_sum(macc, red) / (float)(64 * nfr);
    if (tid == 0) {
        float *o = out + clip * 4;
        o[0] = 0.4f * stft_mean + 0.4f * mel_mean + 0.2f * l1_mean;
        o[1] = stft_mean;
        o[2] = mel_mean;
        o[3] = l1_mean;
    }
}

std::mutex g_fb_mu;
std::map<int, float *> g_fb;      // device -> mel filterbank

hipError_t get_melfb(const float **out, hipStream_t st)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(g_fb_mu);
    auto it = g_fb.find(dev);
    if (it != g_fb.end()) { *out = it->second; return hipSuccess; }
    if (stream_is_capturing(st)) return ADN_COLD_IN_CAPTURE;      // the upload below blocks: not inside a capture (adn_prepare)
    // torchaudio.functional.melscale_fbanks(n_freqs=32, f_min=0, f_max=4000, n_mels=64, sample_rate=8000,
    // norm=None, mel_scale="htk")
    const int nf = 32, nm = 64;
    const double sr = 8000.0;
    auto hz2mel = [](double f) { return 2595.0 * std::log10(1.0 + f / 700.0); };
    auto mel2hz = [](double m) { return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0); };
    std::vector<double> fpts(nm + 2);
    const double m0 = hz2mel(0.0), m1 = hz2mel(sr / 2.0);
    for (int i = 0; i < nm + 2; ++i) fpts[i] = mel2hz(m0 + (m1 - m0) * i / (nm + 1));
    std::vector<float> fb((size_t)nf * nm);
    for (int f = 0; f < nf; ++f) {
        const double freq = (sr / 2.0) * f / (nf - 1);               // linspace(0, sr//2, n_freqs)
        for (int m = 0; m < nm; ++m) {
            const double down = (freq - fpts[m]) / (fpts[m + 1] - fpts[m]);
            const double up = (fpts[m + 2] - freq) / (fpts[m + 2] - fpts[m + 1]);
            const double v = std::fmax(0.0, std::fmin(down, up));
            fb[(size_t)f * nm + m] = (float)v;
        }
    }
    float *d = nullptr;
    e = hipMalloc(&d, fb.size() * sizeof(float));
    if (e != hipSuccess) return e;
    e = hipMemcpy(d, fb.data(), fb.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); return e; }
    g_fb[dev] = d;
    *out = d;
    return hipSuccess;
}


// ---- backward: d{total, stft, mel, l1}/d{pred, target} (same reference arithmetic, differentiated) ----
//
// Three launches: loss_grad_colsum_kernel gives the row-slab partials of the two series (loss_colsum_kernel's sums, also cut
// along T: one workgroup per clip and slab leaves a long clip on a couple of CUs); loss_grad_series_kernel turns them into
// the series-level gradients gp, gq (one workgroup per clip x tb <= LG_TB series positions, gathering -- no atomics);
// loss_grad_input_kernel broadcasts gp / F + w_l1 sign(pred - target) / (F T) over the F rows (HBM-bound).
constexpr int LG_TB = 256;                     // max series positions per workgroup of loss_grad_series_kernel (one per thread)
constexpr int LG_HALO = 64;                    // series loaded on each side of the block (>= n_fft - 1 = 62)
constexpr int LG_SER = LG_TB + 2 * LG_HALO;
// per scale and block: nf <= (LG_TB + n - 2) / hop + 1 frames -> (16,4) 68, (32,8) 36, (63,16) 20
constexpr int LG_SPEC = 2560;                  // >= nf * nb of every scale (68*9, 36*17, 20*32 = 640), x4 planes -> 4 * 640
constexpr int LG_COEF = 1280;                  // >= nf * n (68*16, 36*32, 20*63) and >= nf * 64 mels (20*64)

// partial[clip][slab][0..T) = sum_f pred, [T..2T) = sum_f target over the slab's rows, in loss_colsum_kernel's order (the series
// are bit-identical to the forward's); grid: clip x slab x 256-column chunk
__global__ __launch_bounds__(256) void loss_grad_colsum_kernel(const float *__restrict__ pred, const float *__restrict__ tgt,
                                                               int F, int T, int nslab, int nchunk, float *__restrict__ partial)
{
    const int chunk = blockIdx.x % nchunk, slab = (blockIdx.x / nchunk) % nslab;
    const long clip = blockIdx.x / ((long)nchunk * nslab);
    const int t = chunk * 256 + threadIdx.x;
    if (t >= T) return;
    const int f0 = slab * LOSS_ROWS, f1 = min(f0 + LOSS_ROWS, F);
    const float *p = pred + clip * (long)F * T, *q = tgt + clip * (long)F * T;
    float sp = 0.f, sq = 0.f;
#pragma unroll 4
    for (int f = f0; f < f1; ++f) {
        sp += p[(long)f * T + t];
        sq += q[(long)f * T + t];
    }
    float *out = partial + (clip * nslab + slab) * (long)(2 * T + 1);
    out[t] = sp;
    out[T + t] = sq;
}

// gp[clip][t] = (1/F) d(w_stft stft + w_mel mel)/dp[t], gq likewise for the target series; w_* from grad_out[clip].
__global__ __launch_bounds__(LG_TB) void loss_grad_series_kernel(const float *__restrict__ partial, int F, int T, int nslab,
                                                                 int tb, int nblk, const float *__restrict__ melfb,
                                                                 const float *__restrict__ gout, float *__restrict__ gp,
                                                                 float *__restrict__ gq)
{
    __shared__ float sp[LG_SER], sq[LG_SER];   // series of pred / target on [lo, hi)
    __shared__ float tc[64], ts[64];
    __shared__ float fb[32 * 64];
    __shared__ float spec[4 * (LG_SPEC / 4)];  // per frame and bin: d/dRe, d/dIm of pred, then of target (mel: Re, Im first)
    __shared__ float coef[2 * LG_COEF];        // per frame and window sample: d/dx of pred, then of target (mel: dM, |X|^2 first)
    const int clip = blockIdx.x / nblk, blk = blockIdx.x - clip * nblk;
    const int tid = threadIdx.x;
    const int t0 = blk * tb, t1 = min(t0 + tb, T);
    const int lo = max(0, t0 - LG_HALO), hi = min(T, t1 + LG_HALO);
    const float *pp = partial + (long)clip * nslab * (2 * (long)T + 1);
    for (int j = tid; j < hi - lo; j += LG_TB) {            // the forward's series: same slab order, same division
        float a = 0.f, b = 0.f;
        for (int s = 0; s < nslab; ++s) {
            a += pp[(long)s * (2 * T + 1) + lo + j];
            b += pp[(long)s * (2 * T + 1) + T + lo + j];
        }
        sp[j] = a / (float)F;
        sq[j] = b / (float)F;
    }
    for (int j = tid; j < 32 * 64; j += LG_TB) fb[j] = melfb[j];
    const float g0 = gout[clip * 4 + 0];
    const float w_stft = 0.4f * g0 + gout[clip * 4 + 1], w_mel = 0.4f * g0 + gout[clip * 4 + 2];
    const int s = t0 + tid;                                 // this thread's series position (valid if s < t1)
    float accp = 0.f, accq = 0.f;
    float *gre_p = spec, *gim_p = spec + LG_SPEC / 4, *gre_q = spec + LG_SPEC / 2, *gim_q = spec + 3 * (LG_SPEC / 4);
    float *cp = coef, *cq = coef + LG_COEF;

    // ---- multi-scale |STFT| (rectangular window, zero padding) ----
    const int nfft_s[3] = {63, 32, 16}, hop_s[3] = {16, 8, 4};
#pragma unroll 1
    for (int sc = 0; sc < 3; ++sc) {
        const int n = nfft_s[sc], hop = hop_s[sc];
        const int pad = n / 2, nb = n / 2 + 1, nfr = 1 + (T + 2 * pad - n) / hop;
        const int a0 = t0 + pad - n + 1;
        const int fr0 = a0 <= 0 ? 0 : (a0 + hop - 1) / hop, fr1 = min(nfr - 1, (t1 - 1 + pad) / hop), nf = fr1 - fr0 + 1;
        const float gs = w_stft / (3.0f * (float)(nb * nfr));
        __syncthreads();
        if (tid < n) {
            float sn, c;
            sincospif(2.0f * (float)tid / (float)n, &sn, &c);
            tc[tid] = c;
            ts[tid] = -sn;
        }
        __syncthreads();
        for (int it = tid; it < nb * nf; it += LG_TB) {
            const int k = it / nf, fr = it - k * nf;
            float pr = 0.f, pi = 0.f, qr = 0.f, qi = 0.f;
            int idx = 0;
            for (int i = 0; i < n; ++i) {
                const int u = (fr0 + fr) * hop - pad + i;
                if (u >= 0 && u < T) {
                    const float c = tc[idx], sn = ts[idx], a = sp[u - lo], b = sq[u - lo];
                    pr += a * c; pi += a * sn; qr += b * c; qi += b * sn;
                }
                idx += k;
                if (idx >= n) idx -= n;
            }
            const float ap = sqrtf(pr * pr + pi * pi), aq = sqrtf(qr * qr + qi * qi);
            const float g = ap > aq ? gs : (ap < aq ? -gs : 0.f);      // d/d|Xp|; d/d|Xq| = -g
            const float hp = ap > 0.f ? g / ap : 0.f, hq = aq > 0.f ? -g / aq : 0.f;   // abs'(z) = z/|z|, 0 at 0
            gre_p[fr * nb + k] = hp * pr; gim_p[fr * nb + k] = hp * pi;
            gre_q[fr * nb + k] = hq * qr; gim_q[fr * nb + k] = hq * qi;
        }
        __syncthreads();
        for (int it = tid; it < nf * n; it += LG_TB) {      // adjoint real DFT of every frame
            const int fr = it / n, i = it - fr * n;
            float a = 0.f, b = 0.f;
            int idx = 0;
            for (int k = 0; k < nb; ++k) {
                a += gre_p[fr * nb + k] * tc[idx] + gim_p[fr * nb + k] * ts[idx];
                b += gre_q[fr * nb + k] * tc[idx] + gim_q[fr * nb + k] * ts[idx];
                idx += i;
                if (idx >= n) idx -= n;
            }
            cp[it] = a;
            cq[it] = b;
        }
        __syncthreads();
        if (s < t1) {                                       // gather the frames covering s (padded positions drop out)
            const int a1 = s + pad - n + 1;
            const int f0 = max(fr0, a1 <= 0 ? 0 : (a1 + hop - 1) / hop), f1 = min(fr1, (s + pad) / hop);
            for (int fr = f0; fr <= f1; ++fr) {
                const int j = (fr - fr0) * n + s - fr * hop + pad;
                accp += cp[j];
                accq += cq[j];
            }
        }
    }

    // ---- mel: periodic Hann, n_fft 63, hop 16, reflect padding 31, power 2, 32 bins x 64 mels ----
    {
        const int n = 63, hop = 16, pad = 31, nb = 32, nfr = 1 + (T + 2 * pad - n) / hop;
        const int a0 = t0 + pad - n + 1;
        const int fr0 = a0 <= 0 ? 0 : (a0 + hop - 1) / hop, fr1 = min(nfr - 1, (t1 - 1 + pad) / hop), nf = fr1 - fr0 + 1;
        const float gm = w_mel / (float)(64 * nfr);
        float *re_p = gre_p, *im_p = gim_p, *re_q = gre_q, *im_q = gim_q, *dm = coef;
        float *pw_p = coef + LG_COEF, *pw_q = pw_p + LG_SPEC / 4;               // |X|^2 (the forward's mel spectra)
        __syncthreads();
        if (tid < n) {
            float sn, c;
            sincospif(2.0f * (float)tid / (float)n, &sn, &c);
            tc[tid] = c;
            ts[tid] = -sn;
        }
        __syncthreads();
        for (int it = tid; it < nb * nf; it += LG_TB) {
            const int k = it / nf, fr = it - k * nf;
            float pr = 0.f, pi = 0.f, qr = 0.f, qi = 0.f;
            int idx = 0;
            for (int i = 0; i < n; ++i) {
                int u = (fr0 + fr) * hop - pad + i;
                u = u < 0 ? -u : (u >= T ? 2 * (T - 1) - u : u);            // reflect (no edge repeat)
                const float w = 0.5f - 0.5f * tc[i];
                const float c = tc[idx], sn = ts[idx], a = w * sp[u - lo], b = w * sq[u - lo];
                pr += a * c; pi += a * sn; qr += b * c; qi += b * sn;
                idx += k;
                if (idx >= n) idx -= n;
            }
            re_p[fr * nb + k] = pr; im_p[fr * nb + k] = pi;
            re_q[fr * nb + k] = qr; im_q[fr * nb + k] = qi;
            pw_p[fr * nb + k] = pr * pr + pi * pi;
            pw_q[fr * nb + k] = qr * qr + qi * qi;
        }
        __syncthreads();
        for (int it = tid; it < 64 * nf; it += LG_TB) {     // dL/dM = gm sign(Mp - Mq)
            const int fr = it / 64, m = it - fr * 64;
            float a = 0.f, b = 0.f;
            for (int f = 0; f < nb; ++f) {
                const float w = fb[f * 64 + m];
                a += w * pw_p[fr * nb + f];
                b += w * pw_q[fr * nb + f];
            }
            dm[it] = a > b ? gm : (a < b ? -gm : 0.f);
        }
        __syncthreads();
        for (int it = tid; it < nb * nf; it += LG_TB) {     // dL/dP[k] = sum_m fb[k,m] dM[m]; dRe = 2 Re dP (target: -dP)
            const int fr = it / nb, k = it - fr * nb;
            float d = 0.f;
            for (int m = 0; m < 64; ++m) d += fb[k * 64 + m] * dm[fr * 64 + m];
            re_p[it] *= 2.f * d; im_p[it] *= 2.f * d;
            re_q[it] *= -2.f * d; im_q[it] *= -2.f * d;
        }
        __syncthreads();
        for (int it = tid; it < nf * n; it += LG_TB) {      // adjoint DFT times the window
            const int fr = it / n, i = it - fr * n;
            float a = 0.f, b = 0.f;
            int idx = 0;
            for (int k = 0; k < nb; ++k) {
                a += re_p[fr * nb + k] * tc[idx] + im_p[fr * nb + k] * ts[idx];
                b += re_q[fr * nb + k] * tc[idx] + im_q[fr * nb + k] * ts[idx];
                idx += i;
                if (idx >= n) idx -= n;
            }
            const float w = 0.5f - 0.5f * tc[i];
            cp[it] = w * a;
            cq[it] = w * b;
        }
        __syncthreads();
        if (s < t1) {
            // padded positions u that read series position s: s itself, -s (left reflection), 2(T-1) - s (right reflection)
            for (int v = 0; v < 3; ++v) {
                if ((v == 1 && (s < 1 || s > pad)) || (v == 2 && (s < T - 1 - pad || s > T - 2))) continue;
                const int u = v == 0 ? s : (v == 1 ? -s : 2 * (T - 1) - s), a1 = u + pad - n + 1;
                const int f0 = max(fr0, a1 <= 0 ? 0 : (a1 + hop - 1) / hop), f1 = min(fr1, (u + pad) / hop);
                for (int fr = f0; fr <= f1; ++fr) {
                    const int j = (fr - fr0) * n + u - fr * hop + pad;
                    accp += cp[j];
                    accq += cq[j];
                }
            }
            gp[(long)clip * T + s] = accp / (float)F;
            gq[(long)clip * T + s] = accq / (float)F;
        }
    }
}

// grad_pred[clip,0,f,t] = gp[clip,t] + c sign(pred - target), grad_target = gq[clip,t] - c sign(...), c = w_l1 / (F T); V = 4:
// float4 along t (T % 4 == 0, 16-byte aligned tensors).  Either output may be null.
template <int V>
__global__ __launch_bounds__(256) void loss_grad_input_kernel(const float *__restrict__ pred, const float *__restrict__ tgt,
                                                              const float *__restrict__ gp, const float *__restrict__ gq,
                                                              const float *__restrict__ gout, int n_clips, int F, int T,
                                                              long items, float *__restrict__ gpred, float *__restrict__ gtgt)
{
    using vec = typename std::conditional<V == 4, float4, float>::type;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;   // vector index inside a clip
    if (i >= items) return;
    const int tv = T / V;
    const int t = (int)(items < 0x7fffffffL ? (int)i % tv : i % tv) * V;
    for (int clip = blockIdx.y; clip < n_clips; clip += gridDim.y) {
        const float c = (0.2f * gout[clip * 4 + 0] + gout[clip * 4 + 3]) / ((float)F * (float)T);
        const long off = (long)clip * items + i;
        const vec a = reinterpret_cast<const vec *>(pred)[off], b = reinterpret_cast<const vec *>(tgt)[off];
        const float *ga = gp + (long)clip * T + t, *gb = gq + (long)clip * T + t;
        const float *pa = reinterpret_cast<const float *>(&a), *pb = reinterpret_cast<const float *>(&b);
        vec ra, rb;
        float *qa = reinterpret_cast<float *>(&ra), *qb = reinterpret_cast<float *>(&rb);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float d = pa[j] - pb[j];
            const float sg = d > 0.f ? c : (d < 0.f ? -c : 0.f);
            qa[j] = ga[j] + sg;
            qb[j] = gb[j] - sg;
        }
        if (gpred) reinterpret_cast<vec *>(gpred)[off] = ra;
        if (gtgt) reinterpret_cast<vec *>(gtgt)[off] = rb;
    }
}

}  // namespace

hipError_t loss_tables(hipStream_t st)
{
    const float *fb = nullptr;
    return get_melfb(&fb, st);
}

// dynamic LDS of loss_finish_kernel<false>: two T-long series, two 64-entry trig tables, 2 x 32 bins x (1 + T/16) mel frames; it
// fits the CU's 160 KiB up to T = ADN_LOSS_LDS_T.  <true>: trig tables + one block of mel frames.
size_t perceptual_loss_lds_bytes(int T)
{
    if (T > ADN_LOSS_LDS_T) return (size_t)(128 + 2 * 32 * LOSS_MEL_FB) * sizeof(float);
    return (size_t)(2 * T + 128 + 2 * 32 * (1 + T / 16)) * sizeof(float);
}

size_t perceptual_loss_workspace_floats(int n_clips, int F, int T)
{
    const int nslab = (F + LOSS_ROWS - 1) / LOSS_ROWS;
    // partial column sums of the row slabs (+ beyond ADN_LOSS_LDS_T frames: the two series of every clip)
    return (size_t)n_clips * nslab * (2 * (size_t)T + 1) + (T > ADN_LOSS_LDS_T ? (size_t)n_clips * 2 * T : 0);
}

hipError_t launch_perceptual_loss(const float *pred, const float *tgt, int n_clips, int F, int T, float *workspace,
                                  float *out, hipStream_t st)
{
    const float *fb = nullptr;
    hipError_t e = get_melfb(&fb, st);
    if (e != hipSuccess) return e;
    const int nslab = (F + LOSS_ROWS - 1) / LOSS_ROWS;
    // everything that can fail is checked BEFORE the first launch (nothing is enqueued on an error)
    const size_t lds = perceptual_loss_lds_bytes(T);
    const bool big = T > ADN_LOSS_LDS_T;
    if (lds > ADN_LOSS_MAX_LDS || (long)n_clips * nslab > 0x7fffffffL) return hipErrorInvalidValue;
    if (lds > 64 * 1024) {
        e = hipFuncSetAttribute(big ? reinterpret_cast<const void *>(loss_finish_kernel<true>) : reinterpret_cast<const void *>(loss_finish_kernel<false>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(loss_colsum_kernel, dim3((unsigned)(n_clips * nslab)), dim3(256), 0, st, pred, tgt, F, T, nslab,
                       workspace);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    float *series = workspace + (size_t)n_clips * nslab * (2 * (size_t)T + 1);
    if (big) hipLaunchKernelGGL(loss_finish_kernel<true>, dim3((unsigned)n_clips), dim3(256), lds, st, workspace, F, T, nslab, fb, series, out);
    else hipLaunchKernelGGL(loss_finish_kernel<false>, dim3((unsigned)n_clips), dim3(256), lds, st, workspace, F, T, nslab, fb, series, out);
    return hipGetLastError();
}

size_t perceptual_loss_backward_workspace_floats(int n_clips, int F, int T)
{
    const int nslab = (F + LOSS_ROWS - 1) / LOSS_ROWS;
    // row-slab partials (rounded to 4 floats: the series gradients behind them are read as float4) + gp and gq
    return ((size_t)n_clips * nslab * (2 * (size_t)T + 1) + 3) / 4 * 4 + 2 * (size_t)n_clips * T;
}

hipError_t launch_perceptual_loss_backward(const float *pred, const float *tgt, int n_clips, int F, int T, const float *grad_out,
                                           float *workspace, float *grad_pred, float *grad_tgt, hipStream_t st)
{
    const float *fb = nullptr;
    hipError_t e = get_melfb(&fb, st);
    if (e != hipSuccess) return e;
    const int nslab = (F + LOSS_ROWS - 1) / LOSS_ROWS, nchunk = (T + 255) / 256;
    // series positions per workgroup: narrower blocks (more frames recomputed per position) until the grid fills the chip
    int tb = LG_TB;
    while (tb > 64 && (long)n_clips * ((T + tb - 1) / tb) < 512) tb /= 2;
    const int nblk = (T + tb - 1) / tb;
    const bool vec = T % 4 == 0 && ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(tgt) |
                                     reinterpret_cast<uintptr_t>(grad_pred) | reinterpret_cast<uintptr_t>(grad_tgt)) & 15) == 0;
    const long items = (long)F * T / (vec ? 4 : 1);        // vectors per clip
    if ((long)n_clips * nslab * nchunk > 0x7fffffffL || (long)n_clips * nblk > 0x7fffffffL || (items + 255) / 256 > 0x7fffffffL)
        return hipErrorInvalidValue;
    float *gp = workspace + ((size_t)n_clips * nslab * (2 * (size_t)T + 1) + 3) / 4 * 4, *gq = gp + (size_t)n_clips * T;
    hipLaunchKernelGGL(loss_grad_colsum_kernel, dim3((unsigned)((long)n_clips * nslab * nchunk)), dim3(256), 0, st, pred, tgt, F, T,
                       nslab, nchunk, workspace);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(loss_grad_series_kernel, dim3((unsigned)(n_clips * nblk)), dim3(LG_TB), 0, st, workspace, F, T, nslab,
                       tb, nblk, fb, grad_out, gp, gq);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((items + 255) / 256), (unsigned)std::min(n_clips, 65535));
    if (vec) hipLaunchKernelGGL(loss_grad_input_kernel<4>, grid, dim3(256), 0, st, pred, tgt, gp, gq, grad_out, n_clips, F, T,
                                items, grad_pred, grad_tgt);
    else hipLaunchKernelGGL(loss_grad_input_kernel<1>, grid, dim3(256), 0, st, pred, tgt, gp, gq, grad_out, n_clips, F, T,
                            items, grad_pred, grad_tgt);
    return hipGetLastError();
}

}  // namespace adn
