// The "reverb" noise type of the train-set builder (add_noise, /root/reference/code/create_train_dataset.py:87-102,116-121: a
// Pedalboard Reverb over each 2 s chunk): this project's own Freeverb, defined sample by sample in include/adn.h, batched.
//
// The effect is an IIR: eight parallel combs (delay line + one-pole low-pass in the feedback path) and four all-pass filters in
// series.  Only two things in it are sequential: a delay line returns what was written D samples earlier, and the low-pass
// `last` of a comb is a first-order recurrence over consecutive samples.  So a CHUNK of C = min(all twelve delays) consecutive
// samples never meets itself through a delay line (C = 40 at 8 kHz, 225 at 44.1 kHz), and inside a chunk
//   * the sum of the comb outputs and the whole all-pass chain read only what earlier chunks wrote: element-wise over the chunk;
//   * a comb is the scan v[i] = damp * v[i-1] + b[i], b[i] = o[i] * (1 - damp), with `last` of the previous chunk as carry-in.
// One workgroup owns one clip and walks its chunks in order; the twelve delay lines live in LDS for the whole clip (9 KB at 8 kHz,
// 50 KB at 44.1 kHz, 110 KB at 96 kHz) behind a 16 KB ring of staged input samples.  A wave scans 64 samples of one comb at a
// time with DPP moves (no LDS traffic): four row_shr steps give the prefix inside each row of 16 lanes, row_bcast:15 and
// row_bcast:31 carry the rows' last prefixes across, each weighted by the power of damp that the distance asks for; the carry-in
// is one more fma and the carry-out a v_readlane.  damp = damping * 0.4 <= 0.4, so the powers only shrink.
// A step of the walk does the comb update of chunk k and the element-wise half of chunk k + 1 (a comb delay is more than two
// chunks long: they touch different words), then ONE barrier.  Up to C = 64 (rates below 12.74 kHz) a single wave does all of it
// and the barrier is free; above, the eight combs go to eight waves.  The arithmetic of a sample does not depend on that choice,
// nor on the batch: no atomics, one fixed order, two calls are bit-identical.
#include "adn_internal.h"

namespace adn {
namespace {

constexpr int RV_COMBS = 8, RV_ALLPASS = 4, RV_LINES = RV_COMBS + RV_ALLPASS;
constexpr int RV_TUNING[RV_LINES] = {1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617, 556, 441, 341, 225};
constexpr int RV_XS = 4096;             // ring of staged input samples (a power of two) ...
constexpr int RV_XB = 2048;             // ... filled in blocks of this many; RV_XS - RV_XB >= 2 * C
constexpr int RV_MAX_LDS_FLOATS = 40 * 1024 - 64;

struct ReverbShape {
    int D[RV_LINES];                    // delay lengths: combs, then all-pass filters
    int off[RV_LINES];                  // first word of each line behind the ring
    int C;                              // chunk = shortest delay
    int words;                          // all lines together
};
struct ReverbCoef {
    float feedback, damp, omd, gain, wet1, dry;
    float dpow[7];                      // damp^(2^s)
    int clip;
};

// v_mov_dpp with bound_ctrl: lanes whose source does not exist, and rows outside ROW_MASK, read 0
template <int CTRL, int ROW_MASK>
__device__ inline float dpp0(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, true));
}

// lanes 0..63: b -> sum_{m <= lane} damp^(lane - m) b[m].  All 64 lanes must be active.
__device__ inline float wave_scan(float b, const ReverbCoef &c, float d16, float d32)
{
    b = fmaf(c.dpow[0], dpp0<0x111, 0xf>(b), b);          // row_shr:1
    b = fmaf(c.dpow[1], dpp0<0x112, 0xf>(b), b);          // row_shr:2
    b = fmaf(c.dpow[2], dpp0<0x114, 0xf>(b), b);          // row_shr:4
    b = fmaf(c.dpow[3], dpp0<0x118, 0xf>(b), b);          // row_shr:8
    b = fmaf(d16, dpp0<0x142, 0xa>(b), b);                // row_bcast:15 -> rows 1 and 3
    b = fmaf(d32, dpp0<0x143, 0xc>(b), b);                // row_bcast:31 -> rows 2 and 3
    return b;
}

__device__ inline float pow_bits(const ReverbCoef &c, int e)     // damp^e, e < 128, from the squarings in a fixed order
{
    float r = 1.f;
#pragma unroll
    for (int s = 0; s < 7; ++s)
        if ((e >> s) & 1) r *= c.dpow[s];
    return r;
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void reverb_kernel(const float *x, int L, float *y, ReverbShape p, ReverbCoef c)
{
    constexpr int T = 64 * NW, CPW = RV_COMBS / NW;        // threads; combs per wave
    extern __shared__ float lds[];
    float *xs = lds;                                       // xs[n & (RV_XS - 1)] = x[n]
    float *lines = lds + RV_XS;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float *xc = x + (long)blockIdx.x * L;
    float *yc = y + (long)blockIdx.x * L;
    const int C = p.C;
    const int nchunks = (int)(((long)L + C - 1) / C);

    for (int u = tid; u < p.words; u += T) lines[u] = 0.f;

    const float d16 = pow_bits(c, (lane & 15) + 1), d32 = pow_bits(c, (lane & 31) + 1), d64 = pow_bits(c, lane + 1);
    // this wave's combs: delay, line, position of the chunk's first sample in the line, low-pass state
    int cD[CPW], cpos[CPW];
    float *cline[CPW], carry[CPW];
#pragma unroll
    for (int q = 0; q < CPW; ++q) {
        const int j = wave + q * NW;
        cD[q] = p.D[j];
        cline[q] = lines + p.off[j];
        cpos[q] = 0;
        carry[q] = 0.f;
    }
    int epos[RV_LINES];                                    // the same positions for the element-wise half, one chunk ahead
#pragma unroll
    for (int j = 0; j < RV_LINES; ++j) epos[j] = 0;

    // (sample indices are 32-bit: L < 2^31 - RV_XB, so that `loaded` cannot overflow)
    int loaded = 0;                                        // samples [0, loaded) have been staged
    for (int k = -1; k < nchunks; ++k) {
        // this step reads samples up to the end of chunk k + 1.  A block lands on ring words whose samples lie before chunk k:
        // loaded < (k + 2) C and RV_XS - RV_XB >= 2 C.  (In place: a sample is staged before any output of its chunk is stored.)
        const int need = (long)(k + 2) * C < L ? (k + 2) * C : L;
        if (loaded < need) {
            while (loaded < need) {
#pragma unroll
                for (int u0 = 0; u0 < RV_XB; u0 += 8 * T) {
                    float v[8];
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        const int n = loaded + u0 + r * T + tid;
                        v[r] = u0 + r * T + tid < RV_XB && n < L ? xc[n] : 0.f;
                    }
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        const int n = loaded + u0 + r * T + tid;
                        if (u0 + r * T + tid < RV_XB) xs[n & (RV_XS - 1)] = v[r];
                    }
                }
                loaded += RV_XB;
            }
            __syncthreads();
        }
        if (k >= 0) {                                      // combs of chunk k
            const int n0 = k * C;
            const int cnt = L - n0 < C ? L - n0 : C;               // samples of the chunk inside the clip
            const int xb = n0 & (RV_XS - 1);
            // one wave: C <= 64, a single pass whose eight scans the compiler can interleave
            for (int i0 = 0; i0 < (NW == 1 ? 1 : C); i0 += 64) {
                const int i = i0 + lane;
                const bool ok = i < cnt;
                const float in = xs[(xb + (ok ? i : 0)) & (RV_XS - 1)] * c.gain;
                int idx[CPW];
                float v[CPW];
#pragma unroll
                for (int q = 0; q < CPW; ++q) {
                    // (one wave: comb q is line q, and its position is one chunk behind the element-wise half's)
                    const int back = epos[NW == 1 ? q : 0] - C;
                    idx[q] = (NW == 1 ? (back < 0 ? back + cD[q] : back) : cpos[q]) + i;
                    if (idx[q] >= cD[q]) idx[q] -= cD[q];
                    if (!ok) idx[q] = 0;                                  // (lanes past the chunk: any word of the line, value unused)
                    v[q] = cline[q][idx[q]];
                }
                const int lastl = C - 1 - i0 < 63 ? C - 1 - i0 : 63;
#pragma unroll
                for (int q = 0; q < CPW; ++q) {
                    const float s = wave_scan(ok ? v[q] * c.omd : 0.f, c, d16, d32);
                    v[q] = fmaf(d64, carry[q], s);                        // `last` at sample n0 + i
                    carry[q] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v[q]), lastl));
                }
                if (ok) {
#pragma unroll
                    for (int q = 0; q < CPW; ++q) cline[q][idx[q]] = fmaf(v[q], c.feedback, in);
                }
            }
            if (NW > 1) {
#pragma unroll
                for (int q = 0; q < CPW; ++q) {
                    cpos[q] += C;
                    if (cpos[q] >= cD[q]) cpos[q] -= cD[q];
                }
            }
        }
        if (k + 1 < nchunks) {                             // comb sum, all-pass chain and output of chunk k + 1
            const int n0 = (k + 1) * C;
            for (int i = tid; i < C; i += T) {
                const int n = n0 + i;
                if (n < L) {
                    const float xv = xs[n & (RV_XS - 1)];
                    float acc = 0.f;
#pragma unroll
                    for (int j = 0; j < RV_COMBS; ++j) {
                        int idx = epos[j] + i;
                        if (idx >= p.D[j]) idx -= p.D[j];
                        acc += lines[p.off[j] + idx];
                    }
#pragma unroll
                    for (int j = RV_COMBS; j < RV_LINES; ++j) {
                        int idx = epos[j] + i;
                        if (idx >= p.D[j]) idx -= p.D[j];
                        const float b = lines[p.off[j] + idx];
                        lines[p.off[j] + idx] = fmaf(b, 0.5f, acc);
                        acc = b - acc;
                    }
                    float r = fmaf(acc, c.wet1, xv * c.dry);
                    if (c.clip) r = fminf(fmaxf(r, -1.f), 1.f);
                    yc[n] = r;
                }
            }
#pragma unroll
            for (int j = 0; j < RV_LINES; ++j) {
                epos[j] += C;
                if (epos[j] >= p.D[j]) epos[j] -= p.D[j];
            }
        }
        __syncthreads();
    }
}

}  // namespace

bool reverb_rate_ok(int sample_rate) { return sample_rate >= ADN_REVERB_MIN_RATE && sample_rate <= ADN_REVERB_MAX_RATE; }

hipError_t launch_reverb(const float *audio, int n_clips, int L, int sample_rate, float feedback, float damp, float wet1, float dry,
                         int clip, float *out, hipStream_t st)
{
    ReverbShape p;
    p.words = 0;
    p.C = 0x7fffffff;
    for (int j = 0; j < RV_LINES; ++j) {
        p.D[j] = (int)(((long)sample_rate * RV_TUNING[j]) / 44100);
        p.off[j] = p.words;
        p.words += p.D[j];
        if (p.D[j] < p.C) p.C = p.D[j];
    }
    // what the kernel's walk rests on (reverb_rate_ok implies all of it)
    if (p.C < 1 || 2 * p.C > RV_XS - RV_XB || 2 * p.C > p.D[0] || RV_XS + p.words > RV_MAX_LDS_FLOATS) return hipErrorInvalidValue;
    ReverbCoef c;
    c.feedback = feedback;
    c.damp = damp;
    c.omd = 1.f - damp;
    c.gain = 0.015f;
    c.wet1 = wet1;
    c.dry = dry;
    c.clip = clip;
    c.dpow[0] = damp;
    for (int s = 1; s < 7; ++s) c.dpow[s] = c.dpow[s - 1] * c.dpow[s - 1];
    const size_t lds = (size_t)(RV_XS + p.words) * sizeof(float);
    auto kern = p.C <= 64 ? reverb_kernel<1> : reverb_kernel<8>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)n_clips), dim3(p.C <= 64 ? 64 : 512), lds, st, audio, L, out, p, c);
    return hipGetLastError();
}

}  // namespace adn
