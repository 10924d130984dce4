// Ingest half of the training path: rational-ratio polyphase resampler (what `librosa.load(path, sr=8000)` does in
// /root/reference/code/create_train_dataset.py:204,217) and the SNR noise mixer of add_noise (:147-157), batched.
//
// Resampler (definition in include/adn.h): y[m] = sum_i x[i] * h[m*down - i*up].  Output m = p + up*kk ("cycle" kk, residue p)
// reads inputs i = kk*down + a[p] + d, a[p] = floor(p*down/up), with the coefficient h[(p*down mod up) - d*up]: it depends on p
// and d only.  So the 64 lanes of a wave take 64 consecutive cycles of ONE residue: every coefficient is wave-uniform (scalar
// loads, an SGPR operand of v_pk_fma_f32) and the lanes read LDS samples one row of `down` words apart (an even `down` gets one
// unused word per row: 8 kHz -> 44.1 kHz, down = 80, is a 16-way bank conflict without it -- 33.6 ms against 10.1 ms for 10 000
// clips).  A wave carries R = 4 consecutive residues at once: their input windows start a[p] apart (a few samples), so one LDS
// read feeds 4 FMAs.  The host lays the table out for exactly that walk: tab[g][s][r] = coefficient of residue g*R + r at step s
// of group g's common window (zero where a residue's own window does not reach, or on an unused word), built in float64 and
// rounded once.  A workgroup stages the input of 64 cycles (44.1 -> 8 kHz: 28 224 samples + the filter's reach, 115 KB), its
// waves take one (64-cycle block, residue group) item each per round, and a round's outputs go through an LDS tile so that the
// stores are runs of consecutive residues instead of 64 words `up` apart.
// What limits it (profiles/bench_resample.md): the table (119 KB at 44.1 -> 8 kHz) does not fit the 16 KB scalar cache, so each
// pass of 8 steps waits for an L2 round trip of its 32 coefficients, and SMEM returns out of order: the wait cannot be counted
// down, and 32 more SGPRs of look-ahead do not exist.  At one workgroup (16 waves) per CU that is ~11 TFMA/s, 14 % of the
// packed-fp32 peak; where `down` is small enough for the LDS to hold several blocks, a lane takes J of them and each fetched
// coefficient feeds J FMAs per residue (8 -> 44.1 kHz, J = 4: 16 TFMA/s).
#include "adn_internal.h"

#include <cmath>
#include <map>
#include <mutex>
#include <vector>

namespace adn {
namespace {

constexpr int RS_ZEROS = 32;
constexpr double RS_BETA = 12.0;
constexpr double RS_ROLLOFF = 0.88;
constexpr int RS_THREADS = 1024;
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_MAX_LDS_FLOATS = 40 * 1024 - 64;  // the CU's 160 KiB: output tile + staged span

// steps of the window walk per pass of the kernel's inner loop; S is a multiple of it
constexpr int rs_steps_per_pass(int R) { return 32 / R < 16 ? 32 / R : 16; }

// what the kernel needs to know about a rate pair (passed by value)
struct ResampleShape {
    int G;                  // residue groups = ceil(up / R)
    int K;                  // floor(half / up): a residue's window is d = -K .. K + 1
    int S;                  // steps of a group's common window (multiple of rs_steps_per_pass)
    int ncb;                // 64-cycle blocks per workgroup
    int span;               // staged words per workgroup (rows of down + pad); 0 = the window does not fit the LDS, read global memory
    int pad;                // 1 = `down` is even: every staged row carries one unused word (the table has a zero step there)
    int tile;               // floats of the output tile in front of the staged span
    // a workgroup works in rounds of one (block, group) item per wave: rpc rounds cover the groups of ncbi blocks, Gr groups each
    int Gr, ncbi, rpc;
};
struct ResamplePlan {
    float *tab = nullptr;   // device [G][S][R]
    int R = 1;              // residues per wave
    int J = 1;              // blocks per lane (1, 2 or 4; more than 1 only with 16 or more groups and R = 4)
    ResampleShape s{};
};

// modified Bessel function I0 by its power series (all terms positive: no cancellation; x <= RS_BETA)
double bessel_i0(double x)
{
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}

// h[j] of adn.h, j in [-half, half]
double prototype_tap(long j, long half, int up, double fc, double i0_beta)
{
    const double pi = 3.14159265358979323846;
    const double t = fc * (double)j;
    const double sinc = j == 0 ? 1.0 : std::sin(pi * t) / (pi * t);
    const double r = (double)j / (double)half;
    const double arg = 1.0 - r * r;
    const double win = bessel_i0(RS_BETA * std::sqrt(arg > 0.0 ? arg : 0.0)) / i0_beta;
    return (double)up * fc * sinc * win;
}

template <int R, bool LDS, int J>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float *__restrict__ x, long L, float *__restrict__ y, long M,
                                                              int up, int down, ResampleShape p, int nblk, long ncyc,
                                                              const float *__restrict__ tab)
{
    extern __shared__ float lds[];
    float *tile = lds;                                     // [block of the round][wave's group][65 * R]: a round's outputs, transposed for the stores
    float *xs = lds + p.tile;                              // staged input
    const int S = p.S, G = p.G;
    const int clip = blockIdx.x / nblk, blk = blockIdx.x - clip * nblk;
    const float *__restrict__ xc = x + (long)clip * L;
    float *__restrict__ yc = y + (long)clip * M;
    const long kk0 = (long)blk * 64 * p.ncb;               // first cycle of this workgroup
    if (LDS) {
        // xs holds x[kk0*down - K + u] (zero outside the clip), one row of `down` samples per cycle; with an even `down` each row
        // is followed by one unused word, so that the lanes of a wave -- one row apart -- fall on different banks.  16 loads are
        // in flight per thread: the span is up to 140 KiB and the workgroup is alone on its CU while it is staged.
        const long base = kk0 * down - p.K;
        const int D = down + p.pad;
        for (int u0 = threadIdx.x; u0 < p.span; u0 += 16 * RS_THREADS) {
            float v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int ph = u0 + k * RS_THREADS;
                int u = ph;
                bool ok = ph < p.span;
                if (p.pad) {
                    const int c = ph / D, o = ph - c * D;
                    u = c * down + o;
                    ok = ok && o < down;
                }
                const long i = base + u;
                ok = ok && i >= 0 && i < L;
                v[k] = xc[ok ? i : 0];
                if (!ok) v[k] = 0.f;
            }
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int ph = u0 + k * RS_THREADS;
                if (ph < p.span) xs[ph] = v[k];
            }
        }
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int cbi = wave / p.Gr, gi = wave - cbi * p.Gr;   // this wave's 64-cycle block and residue group inside a round
    const int nround = J > 1 ? p.rpc : (p.ncb + p.ncbi - 1) / p.ncbi * p.rpc;
    constexpr int UNR = rs_steps_per_pass(R);
    for (int round = 0; round < nround; ++round) {
        const int cbr = round / p.rpc, g0 = (round - cbr * p.rpc) * p.Gr;
        const int cb = cbr * p.ncbi + cbi, g = g0 + gi;
        if (cbi < p.ncbi && g < G && cb < p.ncb && kk0 + (long)cb * 64 < ncyc) {       // (wave-uniform)
            const int a0 = (int)(((long)g * R * down) / up);           // a[g*R]: the group's window starts at d = -K of its first residue
            const float *__restrict__ t = tab + (size_t)g * S * R;
            const int rel = (cb * 64 + lane) * (down + (LDS ? p.pad : 0)) + a0;
            // J > 1 (small `down`, many groups): the lane also takes the same cycle of the next J - 1 blocks, so that a fetched
            // coefficient feeds J FMAs per residue -- the coefficient stream, not the FMA rate, is what bounds this kernel
            float acc[J][R];
#pragma unroll
            for (int j = 0; j < J; ++j)
#pragma unroll
                for (int r = 0; r < R; ++r) acc[j][r] = 0.f;
            if (LDS) {
                // Coefficients arrive by scalar loads from a table too large for the scalar cache: each wait costs an L2 round trip,
                // so a pass fetches as many coefficients as the compiler serves with one wait (32 SGPRs)
                const float *xp = xs + rel;
                const int blockw = 64 * (down + p.pad);            // words between the same cycle of two blocks
                for (int s = 0; s < S; s += UNR) {
#pragma unroll
                    for (int q = 0; q < UNR; ++q) {
#pragma unroll
                        for (int j = 0; j < J; ++j) {
                            const float v = xp[j * blockw + s + q];
#pragma unroll
                            for (int r = 0; r < R; ++r) acc[j][r] = fmaf(v, t[(s + q) * R + r], acc[j][r]);
                        }
                    }
                }
            } else {
                const long i0 = kk0 * down - p.K + rel;                  // (no padding on this path)
                for (int s = 0; s < S; ++s) {
                    const long i = i0 + s;
                    const float v = (i >= 0 && i < L) ? xc[i] : 0.f;
#pragma unroll
                    for (int r = 0; r < R; ++r) acc[0][r] = fmaf(v, t[s * R + r], acc[0][r]);
                }
            }
#pragma unroll
            for (int j = 0; j < J; ++j)
#pragma unroll
                for (int r = 0; r < R; ++r) tile[(j * p.Gr + wave) * (65 * R) + lane * R + r] = acc[j][r];
        }
        __syncthreads();
        // stores: row = (block, cycle) of the round, columns = its Gr * R consecutive residues, contiguous in y
        const int cols = p.Gr * R;
        for (int row = wave; row < p.ncbi * J * 64; row += RS_WAVES) {
            const int rcbi = row >> 6, rl = row & 63;          // (J > 1 comes with ncbi = 1, cbr = 0: rcbi is the lane's block j)
            const int rcb = J > 1 ? rcbi : cbr * p.ncbi + rcbi;
            const long kk = kk0 + (long)rcb * 64 + rl;
            for (int c = lane; c < cols; c += 64) {
                const int cg = c / R, r = c - cg * R;
                const int res = (g0 + cg) * R + r;
                const long m = res + (long)up * kk;
                if (g0 + cg < G && res < up && rcb < p.ncb && m < M) yc[m] = tile[(rcbi * p.Gr + cg) * (65 * R) + rl * R + r];
            }
        }
        __syncthreads();
    }
}

struct PlanKey {
    int device, up, down;
    bool operator<(const PlanKey &o) const
    {
        if (device != o.device) return device < o.device;
        return up != o.up ? up < o.up : down < o.down;
    }
};
std::mutex g_plan_mu;
std::map<PlanKey, ResamplePlan> g_plans;

hipError_t get_plan(int up, int down, ResamplePlan *out, hipStream_t st)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(g_plan_mu);
    auto it = g_plans.find(PlanKey{dev, up, down});
    if (it != g_plans.end()) { *out = it->second; return hipSuccess; }
    if (stream_is_capturing(st)) return ADN_COLD_IN_CAPTURE;      // the upload below blocks (adn_resample_prepare)
    ResamplePlan p;
    ResampleShape &sh = p.s;
    const int q = up > down ? up : down;
    const long half = (long)RS_ZEROS * q;
    const double fc = RS_ROLLOFF / (double)q;
    const double i0_beta = bessel_i0(RS_BETA);
    auto a_of = [&](int r) { return (long)r * down / up; };
    sh.K = (int)(half / up);
    // residues per wave: 4 where there are that many (one LDS read feeds 4 FMAs; a pass of 8 steps holds 32 coefficients)
    p.R = up >= 4 ? 4 : (up >= 2 ? 2 : 1);
    long spread = 0;                                       // widest distance between the window starts inside one group
    for (int g = 0; g * p.R < up; ++g) {
        const int last = g * p.R + p.R - 1 < up ? g * p.R + p.R - 1 : up - 1;
        const long d = a_of(last) - a_of(g * p.R);
        if (d > spread) spread = d;
    }
    // the window walk of a group: step s reads word a[g*R] + s of the lane's staged row(s); with padded rows (even `down`) the walk
    // crosses one unused word per row boundary -- a step with zero coefficients
    const int unr = rs_steps_per_pass(p.R);
    const long walk = 2L * sh.K + 2 + spread;              // samples a group's window covers
    auto steps_of = [&](int pad) {                         // at most one unused word per row the walk touches
        const long words = walk + (pad ? (down - 1 + walk) / down + 1 : 0);
        return (words + unr - 1) / unr * unr;
    };
    sh.pad = (down % 2 == 0) ? 1 : 0;
    if (sh.pad && 64L * (down + 1) + steps_of(1) + RS_WAVES * 65 * p.R > RS_MAX_LDS_FLOATS) sh.pad = 0;   // (global-memory path)
    const int D = down + sh.pad;
    auto logical = [&](long w) { return sh.pad ? (w % D == down ? -1L : w / D * down + w % D) : w; };   // staged word -> sample offset
    const long S = steps_of(sh.pad);
    const int R = p.R;
    sh.G = (up + R - 1) / R;
    sh.S = (int)S;
    std::vector<float> h((size_t)sh.G * S * R, 0.f);
    for (int g = 0; g < sh.G; ++g)
        for (int r = 0; r < R; ++r) {
            const int res = g * R + r;
            if (res >= up) continue;
            const long ph = (long)res * down % up;
            const long a0 = a_of(g * R);
            for (long s = 0; s < S; ++s) {
                const long lo = logical(a0 + s);
                if (lo < 0) continue;
                const long d = lo - sh.K - a_of(res);
                const long j = ph - d * up;
                if (j < -half || j > half) continue;
                h[((size_t)g * S + s) * R + r] = (float)prototype_tap(j, half, up, fc, i0_beta);
            }
        }
    // Rounds: with 16 or more groups, the groups of one 64-cycle block are dealt to Gr <= 16 waves in rpc equal rounds; with
    // fewer, a round takes all G groups of ncbi blocks (ncb blocks per workgroup give the waves their items, within the LDS).
    sh.ncb = 1;
    if (sh.G >= RS_WAVES) {
        sh.rpc = (sh.G + RS_WAVES - 1) / RS_WAVES;
        sh.Gr = (sh.G + sh.rpc - 1) / sh.rpc;
        sh.ncbi = 1;
        if (R == 4)                                        // blocks per lane: as many of 4, 2 as the LDS holds
            for (int j = 4; j > 1 && p.J == 1; j /= 2)
                if ((long)j * 64 * D + S + (long)sh.Gr * j * 65 * R <= RS_MAX_LDS_FLOATS) p.J = j;
        sh.ncb = p.J;
    } else {
        sh.rpc = 1;
        sh.Gr = sh.G;
        const int want = RS_WAVES / sh.G;                  // blocks per round
        while (sh.ncb < want && (long)(2 * sh.ncb) * 64 * D + S + RS_WAVES * 65 * R <= RS_MAX_LDS_FLOATS) sh.ncb *= 2;
        sh.ncbi = sh.ncb < want ? sh.ncb : want;
    }
    sh.tile = sh.ncbi * sh.Gr * p.J * 65 * R;
    const long span = (long)sh.ncb * 64 * D + S;
    sh.span = sh.tile + span <= RS_MAX_LDS_FLOATS ? (int)span : 0;
    e = hipMalloc(&p.tab, h.size() * sizeof(float));
    if (e != hipSuccess) return e;
    e = hipMemcpy(p.tab, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(p.tab); return e; }
    g_plans[PlanKey{dev, up, down}] = p;
    *out = p;
    return hipSuccess;
}

template <int R>
hipError_t launch_r(const float *x, int n_clips, long L, long M, int up, int down, const ResamplePlan &p, float *y, hipStream_t st)
{
    const long ncyc = (M + up - 1) / up;
    const long nblk = (ncyc + 64L * p.s.ncb - 1) / (64L * p.s.ncb);
    if (nblk * n_clips > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(nblk * n_clips)), block(RS_THREADS);
    const size_t lds = (size_t)(p.s.tile + p.s.span) * sizeof(float);
    auto kern = p.s.span ? resample_kernel<R, true, 1> : resample_kernel<R, false, 1>;
    if constexpr (R == 4) {
        if (p.s.span && p.J == 2) kern = resample_kernel<4, true, 2>;
        if (p.s.span && p.J == 4) kern = resample_kernel<4, true, 4>;
    }
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, grid, block, lds, st, x, L, y, M, up, down, p.s, (int)nblk, ncyc, p.tab);
    return hipGetLastError();
}

// ---- SNR mixer ------------------------------------------------------------------------------------------------------------
constexpr int MIX_BLK = 8192;       // samples per workgroup: a long clip spreads over L / 8192 workgroups

__device__ inline float wave_sum(float s)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    return s;
}

// ws[(clip * nblk + blk) * 2 + {0, 1}] = sum of clean^2 / noise^2 over the block: 32 strided terms per lane, then a fixed tree
__global__ __launch_bounds__(256) void mix_sumsq_kernel(const float *__restrict__ clean, const float *__restrict__ noise, long L,
                                                        int nblk, float *__restrict__ ws)
{
    __shared__ float part[2][4];
    const int clip = blockIdx.x / nblk, blk = blockIdx.x - clip * nblk;
    const long beg = (long)clip * L + (long)blk * MIX_BLK;
    const long end = (long)clip * L + (((long)blk + 1) * MIX_BLK < L ? ((long)blk + 1) * MIX_BLK : L);
    float sc = 0.f, sn = 0.f;
    for (long i = beg + threadIdx.x; i < end; i += 256) {
        const float c = clean[i], n = noise[i];
        sc = fmaf(c, c, sc);
        sn = fmaf(n, n, sn);
    }
    sc = wave_sum(sc);
    sn = wave_sum(sn);
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = sc; part[1][threadIdx.x >> 6] = sn; }
    __syncthreads();
    if (threadIdx.x < 2)
        ws[((long)clip * nblk + blk) * 2 + threadIdx.x] = (part[threadIdx.x][0] + part[threadIdx.x][1]) + (part[threadIdx.x][2] + part[threadIdx.x][3]);
}

// every workgroup adds its clip's nblk partial sums in the same fixed order, derives the scale and mixes its block
__global__ __launch_bounds__(256) void mix_apply_kernel(const float *__restrict__ clean, const float *noise, long L, int nblk,
                                                        const float *__restrict__ ws, float inv_snr_linear, float *out)
{
    __shared__ float part[2][4];
    const int clip = blockIdx.x / nblk, blk = blockIdx.x - clip * nblk;
    const float *w = ws + (long)clip * nblk * 2;
    float sc = 0.f, sn = 0.f;
    for (int b = threadIdx.x; b < nblk; b += 256) { sc += w[2 * b]; sn += w[2 * b + 1]; }
    sc = wave_sum(sc);
    sn = wave_sum(sn);
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = sc; part[1][threadIdx.x >> 6] = sn; }
    __syncthreads();
    const float msc = ((part[0][0] + part[0][1]) + (part[0][2] + part[0][3])) / (float)L;
    const float msn = ((part[1][0] + part[1][1]) + (part[1][2] + part[1][3])) / (float)L;
    const float scale = sqrtf(msc + 1e-12f) * inv_snr_linear / sqrtf(msn + 1e-12f);
    const long beg = (long)clip * L + (long)blk * MIX_BLK;
    const long end = (long)clip * L + (((long)blk + 1) * MIX_BLK < L ? ((long)blk + 1) * MIX_BLK : L);
    for (long i = beg + threadIdx.x; i < end; i += 256) {
        const float v = clean[i] + scale * noise[i];
        out[i] = fminf(fmaxf(v, -1.f), 1.f);
    }
}

long mix_blocks(long L) { return (L + MIX_BLK - 1) / MIX_BLK; }

}  // namespace

long resample_half(int up, int down) { return (long)RS_ZEROS * (up > down ? up : down); }

float resample_tap(long j, int up, int down)
{
    static const double i0_beta = bessel_i0(RS_BETA);
    const int q = up > down ? up : down;
    return (float)prototype_tap(j, resample_half(up, down), up, RS_ROLLOFF / (double)q, i0_beta);
}

bool resample_ratio(int src_rate, int dst_rate, int *up, int *down)
{
    if (src_rate < 1 || dst_rate < 1) return false;
    int a = src_rate, b = dst_rate;
    while (b) { const int t = a % b; a = b; b = t; }
    *up = dst_rate / a;
    *down = src_rate / a;
    return *up <= 4096 && *down <= 4096;
}

hipError_t resample_prepare(int up, int down, hipStream_t st)
{
    ResamplePlan p;
    return get_plan(up, down, &p, st);
}

hipError_t launch_resample(const float *audio, int n_clips, long L, long M, int up, int down, float *out, hipStream_t st)
{
    ResamplePlan p;
    hipError_t e = get_plan(up, down, &p, st);
    if (e != hipSuccess) return e;
    switch (p.R) {
        case 4: return launch_r<4>(audio, n_clips, L, M, up, down, p, out, st);
        case 2: return launch_r<2>(audio, n_clips, L, M, up, down, p, out, st);
        default: return launch_r<1>(audio, n_clips, L, M, up, down, p, out, st);
    }
}

size_t mix_snr_workspace_floats(int n_clips, long L) { return (size_t)n_clips * (size_t)mix_blocks(L) * 2; }

hipError_t launch_mix_snr(const float *clean, const float *noise, int n_clips, long L, float inv_snr_linear, float *workspace,
                          float *out, hipStream_t st)
{
    const long nblk = mix_blocks(L);
    if (nblk * n_clips > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(nblk * n_clips));
    hipLaunchKernelGGL(mix_sumsq_kernel, grid, dim3(256), 0, st, clean, noise, L, (int)nblk, workspace);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mix_apply_kernel, grid, dim3(256), 0, st, clean, noise, L, (int)nblk, workspace, inv_snr_linear, out);
    return hipGetLastError();
}

}  // namespace adn
