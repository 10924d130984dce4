// Objective quality metrics over a batch of clips (adn.h, "quality"): adn_quality -- SNR, SI-SDR and segmental SNR -- and
// adn_stoi, the short-time objective intelligibility measure for audio at 10 kHz.  Every kernel reads a clip up to its own length
// only (`lengths`, read here on the device), adds in one fixed order without atomics, and decides nothing by the batch a clip is
// in: workgroups are laid out by the row pitch, and those beyond a clip's own length write exact zeros that the fixed-order sums
// of the clip pass over unchanged.
#include "spectral.h"

#include <cmath>

// Every fused multiply-add of this file is written as one (fma / fmaf): a product that adn.h rounds before it is subtracted -- alpha r
// in the SI-SDR residual -- must not be contracted into the subtraction, which would turn an exactly zero residual into its rounding
// error (est = alpha ref: +inf by definition).
#pragma clang fp contract(off)

namespace adn {
namespace {

using namespace fftcore;

constexpr int Q_BLK = 8192;             // samples of a clip per workgroup of the two time-domain passes (adn_mix_snr's block)
constexpr int Q_THREADS = 256;

__device__ __forceinline__ long clip_len(const long *lengths, long clip, long L)
{
    if (!lengths) return L;
    const long n = lengths[clip];
    return n < 0 ? 0 : (n > L ? L : n);
}

__device__ __forceinline__ double wave_sum_d(double s)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    return s;
}

// Sum over the Q_THREADS threads of a workgroup in a fixed order: wave trees, then the four wave sums left to right.  Every thread
// returns the sum.  `part`: 4 doubles of LDS; two calls may share it (the leading barrier protects the earlier call's reads).
__device__ __forceinline__ double wg_sum_d(double s, double *part)
{
    s = wave_sum_d(s);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);
}

// Sum of one quantity over the nblk block partials of a clip (`stride` doubles apart): thread t adds blocks t, t + 256, ... in
// ascending order, then wg_sum_d.
__device__ __forceinline__ double clip_sum_d(const double *w, int stride, int nblk, double *part)
{
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += Q_THREADS) s += w[(long)b * stride];
    return wg_sum_d(s, part);
}

// 10 log10(num / den) of one segmental frame, clamped to [-10, 35]; a NaN stays a NaN
__device__ __forceinline__ double seg_value(double srr, double sdd)
{
    const double v = 10.0 * log10((srr + 1e-10) / (sdd + 1e-10));
    return v < -10.0 ? -10.0 : (v > 35.0 ? 35.0 : v);
}

// Pass 1.  ws1[(clip * nblk + blk) * 4 + {0, 1, 2, 3}] = Srr, Ser, Sdd over the block's samples and the sum of the clamped values
// of the segmental frames that START inside the block (a frame may end in the next block: those samples are read twice, the second
// time from the cache).  fp64 throughout: a product of two fp32 values is exact in fp64.
__global__ __launch_bounds__(Q_THREADS) void quality_pass1_kernel(const float *__restrict__ est, const float *__restrict__ ref,
                                                                   const long *__restrict__ lengths, long L, int nblk, int seg,
                                                                   double *__restrict__ ws1)
{
    __shared__ double part[4];
    __shared__ double gsum[16];
    const long clip = blockIdx.x / nblk;
    const int blk = blockIdx.x - (int)(clip * nblk);
    const long len = clip_len(lengths, clip, L);
    const float *e = est + clip * L, *r = ref + clip * L;
    const long beg = (long)blk * Q_BLK;
    const long end = beg + Q_BLK < len ? beg + Q_BLK : len;
    double srr = 0.0, ser = 0.0, sdd = 0.0;
    auto term = [&](long i) {
        const double ev = (double)e[i], rv = (double)r[i], d = ev - rv;
        srr = fma(rv, rv, srr);
        ser = fma(ev, rv, ser);
        sdd = fma(d, d, sdd);
    };
    if (end - beg == Q_BLK) {                             // a whole block: a fixed trip count lets the loads run ahead of the sums
#pragma unroll 8
        for (int k = 0; k < Q_BLK / Q_THREADS; ++k) term(beg + threadIdx.x + k * Q_THREADS);
    } else {
        for (long i = beg + threadIdx.x; i < end; i += Q_THREADS) term(i);
    }
    srr = wg_sum_d(srr, part);
    ser = wg_sum_d(ser, part);
    sdd = wg_sum_d(sdd, part);

    // segmental frames: groups of LPF lanes take the block's frames in turn
    const int lpf = seg >= 64 ? 64 : 16, ng = Q_THREADS / lpf;
    const int g = threadIdx.x / lpf, l = threadIdx.x - g * lpf;
    const long nfr = len / seg;
    long f_lo = (beg + seg - 1) / seg, f_hi = (beg + Q_BLK + seg - 1) / seg;
    if (f_hi > nfr) f_hi = nfr;
    double acc = 0.0;
    for (long f = f_lo + g; f < f_hi; f += ng) {
        const long s0 = f * seg;
        double a = 0.0, b = 0.0;
        for (int i0 = l; i0 < seg; i0 += 4 * lpf) {          // four loads in flight per array; a term beyond the frame is an exact zero
            float ev[4], rv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + u * lpf;
                const bool in = i < seg;
                const float el = e[s0 + (in ? i : 0)], rl = r[s0 + (in ? i : 0)];      // always inside the frame: no branch
                ev[u] = in ? el : 0.f;
                rv[u] = in ? rl : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double d = (double)ev[u] - (double)rv[u];
                a = fma((double)rv[u], (double)rv[u], a);
                b = fma(d, d, b);
            }
        }
        for (int o = lpf >> 1; o > 0; o >>= 1) {
            a += __shfl_xor(a, o, 64);
            b += __shfl_xor(b, o, 64);
        }
        acc += seg_value(a, b);
    }
    if (l == 0) gsum[g] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < ng; ++i) s += gsum[i];
        double *w = ws1 + ((long)clip * nblk + blk) * 4;
        w[0] = srr;
        w[1] = ser;
        w[2] = sdd;
        w[3] = s;
    }
}

// Pass 2, once alpha = Ser / Srr is known (every workgroup adds its clip's partials in the same order):
// ws2[(clip * nblk + blk) * 2 + {0, 1}] = sum of (alpha r)^2 and of (e - alpha r)^2 over the block, from the per-sample differences.
__global__ __launch_bounds__(Q_THREADS) void quality_pass2_kernel(const float *__restrict__ est, const float *__restrict__ ref,
                                                                   const long *__restrict__ lengths, long L, int nblk,
                                                                   const double *__restrict__ ws1, double *__restrict__ ws2)
{
    __shared__ double part[4];
    const long clip = blockIdx.x / nblk;
    const int blk = blockIdx.x - (int)(clip * nblk);
    const long len = clip_len(lengths, clip, L);
    const double *w1 = ws1 + clip * nblk * 4;
    const double srr = clip_sum_d(w1 + 0, 4, nblk, part);
    const double ser = clip_sum_d(w1 + 1, 4, nblk, part);
    const double alpha = ser / srr;
    const float *e = est + clip * L, *r = ref + clip * L;
    const long beg = (long)blk * Q_BLK;
    const long end = beg + Q_BLK < len ? beg + Q_BLK : len;
    double st = 0.0, sres = 0.0;
    auto term = [&](long i) {
        const double t = __dmul_rn(alpha, (double)r[i]), d = (double)e[i] - t;
        st = fma(t, t, st);
        sres = fma(d, d, sres);
    };
    if (end - beg == Q_BLK) {
#pragma unroll 8
        for (int k = 0; k < Q_BLK / Q_THREADS; ++k) term(beg + threadIdx.x + k * Q_THREADS);
    } else {
        for (long i = beg + threadIdx.x; i < end; i += Q_THREADS) term(i);
    }
    st = wg_sum_d(st, part);
    sres = wg_sum_d(sres, part);
    if (threadIdx.x == 0) {
        double *w = ws2 + ((long)clip * nblk + blk) * 2;
        w[0] = st;
        w[1] = sres;
    }
}

// one workgroup per clip: the block partials in a fixed order, then the three values
__global__ __launch_bounds__(Q_THREADS) void quality_finish_kernel(const long *__restrict__ lengths, long L, int nblk, int seg,
                                                                    const double *__restrict__ ws1, const double *__restrict__ ws2,
                                                                    float *__restrict__ out)
{
    __shared__ double part[4];
    const long clip = blockIdx.x;
    const long len = clip_len(lengths, clip, L);
    const double *w1 = ws1 + clip * nblk * 4, *w2 = ws2 + clip * nblk * 2;
    const double srr = clip_sum_d(w1 + 0, 4, nblk, part);
    const double sdd = clip_sum_d(w1 + 2, 4, nblk, part);
    const double sseg = clip_sum_d(w1 + 3, 4, nblk, part);
    const double st = clip_sum_d(w2 + 0, 2, nblk, part);
    const double sres = clip_sum_d(w2 + 1, 2, nblk, part);
    if (threadIdx.x == 0) {
        out[clip * 3 + 0] = (float)(10.0 * log10(srr / sdd));
        out[clip * 3 + 1] = (float)(10.0 * log10(st / sres));
        out[clip * 3 + 2] = (float)(sseg / (double)(len / seg));      // no whole frame: 0 / 0 = NaN
    }
}

// ---- STOI --------------------------------------------------------------------------------------------------------------------
constexpr int ST_N = 256, ST_HOP = 128, ST_M = 256, ST_BANDS = 15, ST_SEG = 30;
constexpr double ST_EPS = 2.220446049250313e-16;                      // 2^-52
constexpr double ST_CLIP = 6.623413251903491;                         // 1 + 10^(15 / 20)
__constant__ int ST_LO[ST_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

// w[n] = numpy.hanning(258)[n + 1], computed in fp64 and rounded once
__device__ __forceinline__ float stoi_window(int n) { return (float)(0.5 - 0.5 * cospi(2.0 * (double)(n + 1) / 257.0)); }

// frames of a signal of len samples: starts range(0, len - 256, 128)
__host__ __device__ __forceinline__ long stoi_frames(long len) { return len > ST_N ? (len - ST_N + ST_HOP - 1) / ST_HOP : 0; }

// norm[clip * nf_max + i] = || w . ref[128 i : 128 i + 256] ||_2: a wave per frame, 64 frames per workgroup
constexpr int ST_EFPW = 64;
__global__ __launch_bounds__(256) void stoi_energy_kernel(const float *__restrict__ ref, const long *__restrict__ lengths, long L,
                                                          long nf_max, int groups, float *__restrict__ norm)
{
    __shared__ float w[ST_N];
    const long clip = blockIdx.x / groups;
    const int grp = blockIdx.x - (int)(clip * groups);
    const long nf = stoi_frames(clip_len(lengths, clip, L));
    const long f0 = (long)grp * ST_EFPW;
    if (f0 >= nf) return;
    w[threadIdx.x] = stoi_window(threadIdx.x);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float *r = ref + clip * L;
    for (long f = f0 + wave; f < f0 + ST_EFPW && f < nf; f += 4) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float x = w[lane + 64 * q] * r[f * ST_HOP + lane + 64 * q];
            s = fmaf(x, x, s);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if (lane == 0) norm[clip * nf_max + f] = sqrtf(s);
    }
}

// One workgroup per clip: the largest frame norm, then the kept frames in order: idx[clip * nf_max + j], j < K, and kept[clip] = K.
// Frame i is kept when 20 log10(n_i + EPS) > 20 log10(n_max + EPS) - 40, i.e. n_i + EPS > (n_max + EPS) / 100, compared in fp64.
__global__ __launch_bounds__(256) void stoi_select_kernel(const float *__restrict__ norm, const long *__restrict__ lengths, long L,
                                                          long nf_max, int *__restrict__ idx, int *__restrict__ kept)
{
    __shared__ float smax[4];
    __shared__ int scount[4];
    const long clip = blockIdx.x;
    const long nf = stoi_frames(clip_len(lengths, clip, L));
    const float *n = norm + clip * nf_max;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float m = 0.f;
    for (long i = threadIdx.x; i < nf; i += 256) m = fmaxf(m, n[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) smax[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    const double thr = ((double)m + ST_EPS) * 0.01;
    int carry = 0;
    for (long base = 0; base < nf; base += 256) {
        const long i = base + threadIdx.x;
        const bool keep = i < nf && (double)n[i] + ST_EPS > thr;
        const unsigned long long mask = __ballot(keep);
        const int below = __popcll(mask & ((1ull << lane) - 1ull));
        __syncthreads();                                  // the previous round's scount has been read
        if (lane == 0) scount[wave] = __popcll(mask);
        __syncthreads();
        int off = carry;
        for (int v = 0; v < wave; ++v) off += scount[v];
        if (keep) idx[clip * nf_max + off + below] = (int)i;
        carry += scount[0] + scount[1] + scount[2] + scount[3];
    }
    if (threadIdx.x == 0) kept[clip] = carry;
}

// Spectra of the compacted signals, which are never stored: frame j of both is built from the source frames idx[j - 1], idx[j] and
// idx[j + 1], windowed again, zero padded to 512 and transformed as 256 packed complex points (fft_frame / forward_split); only the
// 2 x 15 band envelopes leave the kernel: env[(clip * j_max + j) * 30 + sig * 15 + band], sig 0 = ref, 1 = est.
// A workgroup runs 16 transforms side by side -- 8 frames x {ref, est} -- and ST_PASSES such passes.
constexpr int ST_FPP = 8, ST_PASSES = 8, ST_FPW = ST_FPP * ST_PASSES;
constexpr int ST_PW = 260;                                            // pitch of a slot's |X|^2 image (257 bins)
__global__ __launch_bounds__(STFT_THREADS) void stoi_spectra_kernel(const float *__restrict__ est, const float *__restrict__ ref,
                                                                    long L, long nf_max, long j_max, int groups,
                                                                    const int *__restrict__ idx, const int *__restrict__ kept,
                                                                    float *__restrict__ env)
{
    __shared__ float s_w[ST_N];
    __shared__ float2 s_tw[ST_M], s_tw2[ST_M / 2 + 1];
    __shared__ float2 s_sc[2 * ST_FPP * ST_M];
    __shared__ float s_pw[2 * ST_FPP * ST_PW];
    const int tid = threadIdx.x;
    const long clip = blockIdx.x / groups;
    const int grp = blockIdx.x - (int)(clip * groups);
    const int J = kept[clip] - 1;
    const int j0 = grp * ST_FPW;
    if (j0 >= J) return;

    if (tid < ST_N) {
        s_w[tid] = stoi_window(tid);
        double s, c;
        sincospi((double)tid / (double)(ST_M / 2), &s, &c);           // exp(-2 pi i tid / 256)
        s_tw[tid] = make_float2((float)c, (float)-s);
    } else if (tid - ST_N <= ST_M / 2) {
        double s, c;
        sincospi((double)(tid - ST_N) / (double)ST_M, &s, &c);        // exp(-2 pi i k / 512)
        s_tw2[tid - ST_N] = make_float2((float)c, (float)-s);
    }
    __syncthreads();

    const int slot = tid >> 5, t = tid & 31;                          // 32 threads per transform
    const int fr = slot >> 1, sig = slot & 1;
    const float *src = (sig ? est : ref) + clip * L;
    const int *ix = idx + clip * nf_max;
    float2 *sc = s_sc + slot * ST_M;
    float *pw = s_pw + slot * ST_PW;
#pragma unroll 1
    for (int ps = 0; ps < ST_PASSES; ++ps) {
        const int jp = j0 + ps * ST_FPP;
        if (jp >= J) break;                                           // uniform over the workgroup
        const int j = jp + fr;
        float2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = make_float2(0.f, 0.f);
        if (j < J) {
            // c[128 j + p], p < 256: the first half from kept frames j - 1 and j, the second from j and j + 1 (j + 1 <= K - 1)
            const long b1 = (long)ix[j] * ST_HOP, b2 = (long)ix[j + 1] * ST_HOP;
            const long b0 = j > 0 ? (long)ix[j - 1] * ST_HOP : -1;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float x[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int p = 2 * (t + 32 * u) + h;
                    float c;
                    if (u < 2) {
                        const float lo = b0 >= 0 ? s_w[p + ST_HOP] * src[b0 + p + ST_HOP] : 0.f;
                        c = fmaf(s_w[p], src[b1 + p], lo);
                    } else {
                        const float lo = s_w[p] * src[b1 + p];
                        c = fmaf(s_w[p - ST_HOP], src[b2 + p - ST_HOP], lo);
                    }
                    x[h] = s_w[p] * c;
                }
                v[u] = make_float2(x[0], x[1]);
            }
        }
        fft_frame<ST_M>(sc, s_tw, t, v);
        forward_split<ST_M>(
            sc, s_tw2, t,
            [&](int k, float2 xk, float2 xm) {
                pw[k] = fmaf(xk.x, xk.x, xk.y * xk.y);
                pw[ST_M - k] = fmaf(xm.x, xm.x, xm.y * xm.y);
            },
            [&](float2 x0, float2 xM, float2 xh) {
                pw[0] = x0.x * x0.x;
                pw[ST_M] = xM.x * xM.x;
                pw[ST_M / 2] = fmaf(xh.x, xh.x, xh.y * xh.y);
            });
        __syncthreads();
        if (tid < 2 * ST_FPP * ST_BANDS) {
            const int sl = tid / ST_BANDS, b = tid - sl * ST_BANDS;
            const int jj = jp + (sl >> 1);
            if (jj < J) {
                const float *q = s_pw + sl * ST_PW;
                float s = 0.f;
                for (int k = ST_LO[b]; k < ST_LO[b + 1]; ++k) s += q[k];
                env[((long)clip * j_max + jj) * (2 * ST_BANDS) + (sl & 1) * ST_BANDS + b] = sqrtf(s);
            }
        }
        // the next pass writes s_pw only after the barriers of its transform
    }
}

// Step 6 in fp64: a workgroup takes ST_SPW consecutive segments of a clip, stages the envelopes of the frames they cover in LDS and
// gives every (segment, band) to one thread; rho[clip * wgs + wg] = the sum of its correlations in a fixed order.
constexpr int ST_SPW = 64;
__global__ __launch_bounds__(256) void stoi_corr_kernel(const float *__restrict__ env, const int *__restrict__ kept, long j_max,
                                                        int wgs, double *__restrict__ rho)
{
    __shared__ float s_env[(ST_SPW + ST_SEG - 1) * 2 * ST_BANDS];
    __shared__ double part[4];
    const long clip = blockIdx.x / wgs;
    const int wg = blockIdx.x - (int)(clip * wgs);
    const int J = kept[clip] - 1;
    const int nseg = J - (ST_SEG - 1);                                // segments m = 30 .. J
    const int s0 = wg * ST_SPW;
    if (s0 >= nseg) {                                                 // uniform
        if (threadIdx.x == 0) rho[clip * wgs + wg] = 0.0;
        return;
    }
    const int ns = nseg - s0 < ST_SPW ? nseg - s0 : ST_SPW;           // segment s0 + s covers frames [s0 + s, s0 + s + 30)
    const int nfl = (ns + ST_SEG - 1) * 2 * ST_BANDS;
    const float *e = env + ((long)clip * j_max + s0) * (2 * ST_BANDS);
    for (int i = threadIdx.x; i < nfl; i += 256) s_env[i] = e[i];
    __syncthreads();
    double acc = 0.0;
    for (int p = threadIdx.x; p < ns * ST_BANDS; p += 256) {
        const int s = p / ST_BANDS, b = p - s * ST_BANDS;
        const float *x = s_env + s * (2 * ST_BANDS) + b, *y = x + ST_BANDS;
        double xx = 0.0, yy = 0.0;
        for (int i = 0; i < ST_SEG; ++i) {
            const double xv = x[i * 2 * ST_BANDS], yv = y[i * 2 * ST_BANDS];
            xx = fma(xv, xv, xx);
            yy = fma(yv, yv, yy);
        }
        const double a = sqrt(xx) / (sqrt(yy) + ST_EPS);
        double sx = 0.0, sy = 0.0;
        for (int i = 0; i < ST_SEG; ++i) {
            const double xv = x[i * 2 * ST_BANDS], yv = fmin(a * (double)y[i * 2 * ST_BANDS], xv * ST_CLIP);
            sx += xv;
            sy += yv;
        }
        const double mx = sx / ST_SEG, my = sy / ST_SEG;
        double cxx = 0.0, cyy = 0.0, cxy = 0.0;
        for (int i = 0; i < ST_SEG; ++i) {
            const double xv = x[i * 2 * ST_BANDS], yv = fmin(a * (double)y[i * 2 * ST_BANDS], xv * ST_CLIP);
            const double dx = xv - mx, dy = yv - my;
            cxx = fma(dx, dx, cxx);
            cyy = fma(dy, dy, cyy);
            cxy = fma(dx, dy, cxy);
        }
        acc += cxy / ((sqrt(cxx) + ST_EPS) * (sqrt(cyy) + ST_EPS));
    }
    acc = wg_sum_d(acc, part);
    if (threadIdx.x == 0) rho[clip * wgs + wg] = acc;
}

__global__ __launch_bounds__(256) void stoi_finish_kernel(const double *__restrict__ rho, const int *__restrict__ kept, int wgs,
                                                          float *__restrict__ out)
{
    __shared__ double part[4];
    const long clip = blockIdx.x;
    const int J = kept[clip] - 1;
    const double s = clip_sum_d(rho + clip * wgs, 1, wgs, part);
    if (threadIdx.x == 0)
        out[clip] = J < ST_SEG ? __builtin_nanf("") : (float)(s / (double)(ST_BANDS * (J - (ST_SEG - 1))));
}

size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

}  // namespace

long quality_blocks(long L) { return (L + Q_BLK - 1) / Q_BLK; }

size_t quality_workspace_bytes(int n_clips, long L) { return (size_t)n_clips * (size_t)quality_blocks(L) * 6 * sizeof(double); }

hipError_t launch_quality(const float *est, const float *ref, const long *lengths, int n_clips, long L, int seg_frame,
                          void *workspace, float *out, hipStream_t st)
{
    const long nblk = quality_blocks(L);
    if (nblk * n_clips > 0x7fffffffL) return hipErrorInvalidValue;
    double *ws1 = static_cast<double *>(workspace), *ws2 = ws1 + (size_t)n_clips * nblk * 4;
    const dim3 grid((unsigned)(nblk * n_clips)), block(Q_THREADS);
    hipLaunchKernelGGL(quality_pass1_kernel, grid, block, 0, st, est, ref, lengths, L, (int)nblk, seg_frame, ws1);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(quality_pass2_kernel, grid, block, 0, st, est, ref, lengths, L, (int)nblk, ws1, ws2);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(quality_finish_kernel, dim3(n_clips), block, 0, st, lengths, L, (int)nblk, seg_frame, ws1, ws2, out);
    return hipGetLastError();
}

// Sections of the STOI workspace, each 16-byte aligned: frame norms, kept-frame indices, kept counts, envelopes, segment sums.
StoiPlan stoi_plan(int n_clips, long L)
{
    StoiPlan p;
    p.nf_max = stoi_frames(L);
    p.j_max = p.nf_max > 0 ? p.nf_max - 1 : 0;
    const long nseg = p.j_max - (ST_SEG - 1);
    p.wgs = nseg > 0 ? (int)((nseg + ST_SPW - 1) / ST_SPW) : 0;
    size_t o = 0;
    p.norm_off = o;
    o += align16((size_t)n_clips * p.nf_max * sizeof(float));
    p.idx_off = o;
    o += align16((size_t)n_clips * p.nf_max * sizeof(int));
    p.kept_off = o;
    o += align16((size_t)n_clips * sizeof(int));
    p.env_off = o;
    o += align16((size_t)n_clips * p.j_max * 2 * ST_BANDS * sizeof(float));
    p.rho_off = o;
    o += align16((size_t)n_clips * p.wgs * sizeof(double));
    p.total = o;
    return p;
}

hipError_t launch_stoi(const float *est, const float *ref, const long *lengths, int n_clips, long L, void *workspace, float *out,
                       hipStream_t st)
{
    const StoiPlan p = stoi_plan(n_clips, L);
    char *ws = static_cast<char *>(workspace);
    float *norm = reinterpret_cast<float *>(ws + p.norm_off);
    int *idx = reinterpret_cast<int *>(ws + p.idx_off);
    int *kept = reinterpret_cast<int *>(ws + p.kept_off);
    float *env = reinterpret_cast<float *>(ws + p.env_off);
    double *rho = reinterpret_cast<double *>(ws + p.rho_off);
    const long eg = (p.nf_max + ST_EFPW - 1) / ST_EFPW, sg = (p.j_max + ST_FPW - 1) / ST_FPW;
    if (eg * n_clips > 0x7fffffffL) return hipErrorInvalidValue;
    hipError_t e;
    if (eg > 0) {
        hipLaunchKernelGGL(stoi_energy_kernel, dim3((unsigned)(eg * n_clips)), dim3(256), 0, st, ref, lengths, L, p.nf_max, (int)eg, norm);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(stoi_select_kernel, dim3(n_clips), dim3(256), 0, st, norm, lengths, L, p.nf_max, idx, kept);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (sg > 0) {
        hipLaunchKernelGGL(stoi_spectra_kernel, dim3((unsigned)(sg * n_clips)), dim3(STFT_THREADS), 0, st, est, ref, L, p.nf_max, p.j_max,
                           (int)sg, idx, kept, env);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (p.wgs > 0) {
        hipLaunchKernelGGL(stoi_corr_kernel, dim3((unsigned)((long)p.wgs * n_clips)), dim3(256), 0, st, env, kept, p.j_max, p.wgs, rho);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(stoi_finish_kernel, dim3(n_clips), dim3(256), 0, st, rho, kept, p.wgs, out);
    return hipGetLastError();
}

}  // namespace adn
