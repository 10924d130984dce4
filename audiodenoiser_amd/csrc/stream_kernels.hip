// Streaming denoiser for gfx950: the stateful ends of the pipeline.  Definition: include/adn.h, "stream"; float64 restatement:
// tests/stream_ref.py.  Audio arrives in pieces; step k feeds the network the last W frames of |X| and takes B frames of its
// output back to audio.  Everything that has to survive between two calls lives in a caller-owned state buffer.
//
// State of one batch of n_streams streams (StreamGeom::*_off, floats; S = max_steps + 1 slots):
//   X     [stream][RX][F] float2   complex frames that are still to be emitted, ring over the FRAME index, RX = max_steps B + A
//   mag   [stream][RM][F]          |X| of the last frames, ring over the frame index, RM = W + (max_steps - 1) B
//   hist  [stream][S][n_fft - hop] the samples the first new frame of the next call shares with this one, slot = last step mod S
//   tail  [stream][S][n_fft - hop] overlap-add partial sums past the last emitted sample, slot = last step mod S
// Frames, and with them every ring position, follow from the step index the caller passes: nothing is ever shifted in place.
//
// Who writes what (no state word is written by one workgroup and read by another in the same launch):
//   stream_frames   (analysis, launch 1) reads hist slot (first_step - 1) mod S and the new samples; workgroup (x, stream) WRITES
//                   the X and mag ring rows of its own FB frames; the workgroups with x = 0 also WRITE hist slot last_step mod S.
//                   n_steps <= max_steps < S: the slot read and the slot written differ.  It reads neither ring.
//   stream_windows  (analysis, launch 2) READS the mag ring rows of frames [first B + B + A - W, last B + B + A) -- at most RM
//                   consecutive frames, so no two share a row -- and writes only the network input.  The frames of one call come
//                   from several workgroups of launch 1; the launch boundary is the only synchronisation.
//   stream_emit     READS X ring rows of frames [first B, last B + B) (at most RX consecutive frames together with the A frames
//                   beyond them that launch 1 has already written), READS tail slot (first_step - 1) mod S, WRITES tail slot
//                   last_step mod S (a different slot) and the audio.  A workgroup owns a span of samples; a sample of the
//                   output or of the new tail is written by exactly one thread.
// Order of the sums: a sample is the carried partial sum plus its frames in ascending frame order, all fp32 adds of one thread
// -- the same chain whether the frames arrive in one call or in many, so the same audio gives the same bits however it was
// split, and a stream never reads another stream's rows.  No atomics, no workspace.
//
// Stream pool (adn.h, "stream pool"): n_slots streams with independent timing in one state, the same kernel bodies.  A launch has
// ROWS of (slot, step, final_length), one step each, handed over by value in the kernel arguments; a workgroup derives its row's
// StreamCall with stream_call_of, the function the host uses for the lockstep call.  A slot has the geometry of max_steps = 1
// (S = 2, RX = B + A, RM = W), no hist section and
//   ring  [slot][R]                 its pending samples, sample s of the stream at s mod R (adn_stream_pool_write fills it)
// which serves the new samples and the n_fft - hop before them alike.  The rule above holds row for row: the frames workgroups of
// a row only READ the ring (no launch of these kernels writes it) and WRITE the X and mag rows of their own frames; windows only
// reads mag rows of its slot; emit reads tail slot (step - 1) mod 2 and writes tail slot step mod 2.  No two rows of a launch
// name the same slot (the host refuses such a call), so no state word of a slot has two writers, and no workgroup reads what
// another one writes in the same launch.  Still no atomics, no workspace.
#include "spectral.h"

#include <cfloat>

namespace adn {
namespace {

using namespace fftcore;

// Sample s of the stream: zero before the start and, once the length is known, from the end on; the call's new samples start at
// `base`, the n_fft - hop before them are the carried history.
struct Samples {
    const float *audio, *hist;
    int base, keep, L;               // L < 0 while the stream runs
    __device__ __forceinline__ float at(int s) const
    {
        if (s < 0 || (L >= 0 && s >= L)) return 0.f;
        return s >= base ? audio[s - base] : hist[s - (base - keep)];
    }
};

// The pool's form: the slot's ring of pending samples holds sample s at s mod R, the history included.
struct RingSamples {
    const float *ring;
    int R, L;
    __device__ __forceinline__ float at(int s) const
    {
        if (s < 0 || (L >= 0 && s >= L)) return 0.f;
        return ring[s % R];
    }
};

// Where a workgroup gets its StreamCall from: the kernels below are templates on the argument that says it.  A ROW of a launch is
// one stream's share of it: the row indexes the launch's input and output, the SLOT the state.  Lockstep (StreamCall): one call
// for all streams, made on the host, row = slot = stream.  Pooled (StreamPoolRows): a table of (slot, step, final_length) in the
// kernel arguments, one step per row, the call derived here by the function the host uses.
template <class Rows> constexpr bool POOLED = std::is_same_v<Rows, StreamPoolRows>;
__device__ __forceinline__ StreamCall call_of(const StreamCall &c, const StreamGeom &, long) { return c; }
__device__ __forceinline__ StreamCall call_of(const StreamPoolRows &t, const StreamGeom &g, long row)
{
    return stream_call_of(g, t.row[row].step, 1, t.row[row].final_length);
}
__device__ __forceinline__ long slot_of(const StreamCall &, long row) { return row; }
__device__ __forceinline__ long slot_of(const StreamPoolRows &t, long row) { return t.row[row].slot; }
__device__ __forceinline__ Samples samples_of(const StreamCall &, const StreamCall &c, const StreamGeom &g, int keep,
                                              const float *audio, long audio_stride, long strm, const float *state)
{
    Samples in;
    in.audio = audio + strm * audio_stride;
    in.hist = state + g.hist_off + (strm * g.S + c.slot_in) * (long)keep;
    in.base = c.base;
    in.keep = keep;
    in.L = c.L;
    return in;
}
__device__ __forceinline__ RingSamples samples_of(const StreamPoolRows &t, const StreamCall &c, const StreamGeom &, int,
                                                  const float *, long, long strm, const float *state)
{
    RingSamples in;
    in.ring = state + t.ring_off + strm * (long)t.R;
    in.R = t.R;
    in.L = c.L;
    return in;
}

// ---------------------------------------------------------------------------------------------- analysis 1: new frames
template <int M, class Rows>
__global__ __launch_bounds__(STFT_THREADS) void stream_frames_kernel(const float *__restrict__ audio, long audio_stride,
                                                                    StreamGeom g, Rows rows,
                                                                    const float *__restrict__ tables, float *__restrict__ state)
{
    using C = SpecCfg<M>;
    constexpr int N = C::N, TPF = C::TPF, FB = C::FB, F = C::F;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const SpecTables tb = C::view(smem);
    const int tid = threadIdx.x;
    C::load(smem, tables);
    __syncthreads();

    const long strm = slot_of(rows, blockIdx.y);
    const StreamCall &c = call_of(rows, g, blockIdx.y);
    const int keep = N - g.hop;
    const auto in = samples_of(rows, c, g, keep, audio, audio_stride, strm, state);

    if constexpr (POOLED<Rows>) {      // the grid is sized for the row with the most new frames (the first step brings A more)
        if (c.f_new0 + (int)blockIdx.x * FB >= c.f_new1) return;
    } else if (blockIdx.x == 0) {    // the samples the next call's first frame shares with this one (the pool's stay in the ring)
        float *h = state + g.hist_off + (strm * g.S + c.slot_out) * (long)keep;
        for (int i = tid; i < keep; i += STFT_THREADS) h[i] = in.at(c.end - keep + i);
    }

    const int fl = tid / TPF, t = tid - fl * TPF;
    const int f = c.f_new0 + blockIdx.x * FB + fl;
    const bool live = f < c.f_new1;
    const int s0 = (live ? f : c.f_new0) * g.hop - M;
    float2 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int n2 = 2 * (t + u * TPF);
        const float x0 = live ? in.at(s0 + n2) : 0.f;
        const float x1 = live ? in.at(s0 + n2 + 1) : 0.f;
        v[u] = make_float2(tb.win[n2] * x0, tb.win[n2 + 1] * x1);
    }
    float2 *sc = C::frames(smem) + fl * M;
    fft_frame<M>(sc, tb.tw, t, v);
    if (live) {
        // frames from T on (after the end of the stream) are zero in the windows and never emitted
        const bool past = c.T >= 0 && f >= c.T;
        float2 *o = reinterpret_cast<float2 *>(state + g.x_off) + (strm * g.RX + f % g.RX) * (long)F;
        float *m = state + g.mag_off + (strm * g.RM + f % g.RM) * (long)F;
        const auto put = [&](int k, float2 x) {
            o[k] = x;
            m[k] = past ? 0.f : mag_of(x);
        };
        forward_split<M>(sc, tb.tw2, t, [&](int k, float2 xa, float2 xb) { put(k, xa); put(M - k, xb); },
                         [&](float2 x0, float2 xM, float2 xh) { put(0, x0); put(M, xM); put(M / 2, xh); });
    }
}

// ---------------------------------------------------------------------------------------------- analysis 2: network input
// mag ring rows are frame-major [frame][F], the network's windows bin-major [window][F][W] with the frame index fastest: a
// 32 x 32 tile through LDS (pitch 33) keeps both sides contiguous along their fastest index.
template <class Rows>
__global__ __launch_bounds__(256) void stream_windows_kernel(const float *__restrict__ state, int F, StreamGeom g, Rows rows,
                                                             int tilesJ, int tilesF, float *__restrict__ out)
{
    __shared__ float tile[32][33];
    unsigned b = blockIdx.x;
    const int tj = (int)(b % (unsigned)tilesJ);
    b /= (unsigned)tilesJ;
    const int tf = (int)(b % (unsigned)tilesF);
    const long win = b / (unsigned)tilesF;                       // stream * n_steps + i; the pool's row
    const StreamCall &c = call_of(rows, g, win);
    const long strm = POOLED<Rows> ? slot_of(rows, win) : win / c.n_steps;
    const int i = POOLED<Rows> ? 0 : (int)(win - strm * c.n_steps);
    const int fw0 = (c.first + i) * g.B + g.B + g.A - g.W;       // first frame of the step's window
    const int j0 = tj * 32, f0 = tf * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float *mg = state + g.mag_off + strm * g.RM * (long)F;
    for (int r = ty; r < 32; r += 8) {
        const int j = j0 + r, fr = fw0 + j, bin = f0 + tx;
        float v = 0.f;
        if (j < g.W && fr >= 0 && (c.T < 0 || fr < c.T) && bin < F) v = mg[(long)(fr % g.RM) * F + bin];
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int bin = f0 + r, j = j0 + tx;
        if (bin < F && j < g.W) out[(win * F + bin) * (long)g.W + j] = tile[tx][r];
    }
}

// ---------------------------------------------------------------------------------------------- emit
// Positions are those of the untrimmed signal, p = n + n_fft/2: frame f covers [f hop, f hop + n_fft).  The calls before this one
// have emitted p < p_begin = first B hop and left the partial sums of [p_begin, p_begin + n_fft - hop) in the tail; this call adds
// frames [f_first, f_last], emits [p_begin, p_out) and leaves [p_tail, p_tail + n_fft - hop) in the new tail (p_tail = p_out
// while the stream runs; nothing once the stream's last sample is out).  A workgroup owns `span` positions of
// [p_begin, p_end); the frames that cover its span and belong to this call are rebuilt in LDS stage by stage (ResynthCfg<M>, spectral.h).
template <int M, class Rows>
__global__ __launch_bounds__(STFT_THREADS, (M == 256 ? 4 : 2)) void stream_emit_kernel(
    const float *__restrict__ y, StreamGeom g, Rows rows, int nblk, const float *__restrict__ tables,
    float *__restrict__ state, float *__restrict__ audio, long out_stride)
{
    using C = ResynthCfg<M>;
    using S = SpecCfg<M>;
    constexpr int N = S::N, TPF = S::TPF, FB = S::FB, SB = C::SB, F = S::F, P = C::PITCH, SPT = C::SPT, span = C::SPAN;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *s_win = smem;
    float2 *s_tw = reinterpret_cast<float2 *>(smem + N);
    float2 *s_tw2 = s_tw + M;                                   // exp(-2 pi i k / N), k = 0 .. M/2
    float2 *s_sc = reinterpret_cast<float2 *>(smem + S::TBL);
    float *s_fr = smem + S::TBL;                                // the same storage once a pass's frames are windowed: [FB][N]
    float *s_tile = smem + S::TBL + 2 * FB * M;                 // [SB][P] clamped magnitudes of the stage
    const int tid = threadIdx.x;
    for (int i = tid; i < S::TBL; i += STFT_THREADS) smem[i] = tables[i];
    __syncthreads();                                            // (a workgroup past the call's last frame runs no FFT pass)

    const long row = blockIdx.x / (unsigned)nblk, strm = slot_of(rows, row);
    const int bx = (int)(blockIdx.x - row * nblk);
    const StreamCall &c = call_of(rows, g, row);
    const int hop = g.hop, keep = N - hop;
    const int pa = c.p_begin + bx * span;
    if constexpr (POOLED<Rows>)                                 // nblk is sized for the longest row of the launch
        if (pa >= c.p_end) return;
    const int pb = pa + span < c.p_end ? pa + span : c.p_end;
    // frames of this call that cover [pa, pb): ceil((pa - n_fft + 1) / hop) .. floor((pb - 1) / hop), clipped to the call's frames
    int f_begin = pa < N ? 0 : (pa - N + hop) / hop;
    if (f_begin < c.f_first) f_begin = c.f_first;
    int f_end = (pb - 1) / hop;
    if (f_end > c.f_last) f_end = c.f_last;

    // the thread's positions pa + tid + u * 512 start from the carried partial sums (zero before the first step and past them)
    const int p0 = pa + tid;
    const float *tail_in = state + g.tail_off + (strm * g.S + c.slot_in) * (long)keep;
    float acc[SPT];
#pragma unroll
    for (int u = 0; u < SPT; ++u) {
        const int q = p0 + u * STFT_THREADS - c.p_begin;
        acc[u] = (c.first > 0 && q < keep && p0 + u * STFT_THREADS < pb) ? tail_in[q] : 0.f;
    }

    const float *ys = y + row * c.n_steps * (long)F * g.W;
    const float2 *Xs = reinterpret_cast<const float2 *>(state + g.x_off) + strm * g.RX * (long)F;
    const int fl = tid / TPF, t = tid - fl * TPF;               // FFT role: frame slot, lane inside the frame
    const int jf = tid & (SB - 1), kb = tid / SB;               // staging role: frame of the stage, first bin
    const float inv = 1.0f / (float)M;
    const int j_keep = g.W - g.B - g.A;                         // local frame of the first frame a step keeps

    for (int fs = f_begin; fs <= f_end; fs += SB) {
        {
            const int f = fs + jf;
            const bool lv = f <= f_end;
            const int fc = lv ? f : f_begin;
            const int step = fc / g.B;                          // frame f is local frame W - B - A + f mod B of step f / B
            constexpr int KS = STFT_THREADS / SB;               // bins between a thread's loads; 8 loads in flight per thread
            const float *yf = ys + (long)(step - c.first) * F * g.W + j_keep + (fc - step * g.B);
            for (int k0 = kb; k0 < F; k0 += 8 * KS) {
                float hi[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int k = k0 + e * KS < F ? k0 + e * KS : F - 1;
                    hi[e] = yf[(long)k * g.W];
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
            const float2 *Xf = Xs + (long)((live ? f : f_begin) % g.RX) * F;
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
            // gather: frame fr holds position p at j = p - fr * hop when 0 <= j < n_fft; frames ascend
            const int fr_last = fp + FB - 1 < f_end ? fp + FB - 1 : f_end;
            for (int fr = fp; fr <= fr_last; ++fr) {
                const float *frame = s_fr + (fr - fp) * N;
                const int j0 = p0 - fr * hop;
#pragma unroll
                for (int u = 0; u < SPT; ++u) {
                    const int j = j0 + u * STFT_THREADS;
                    const bool in = (unsigned)j < (unsigned)N;
                    const float s = frame[in ? j : 0];
                    if (in) acc[u] += s;
                }
            }
            // no barrier here: the next pass overwrites the frames behind fft_frame's first barrier, and a new stage only
            // touches the tile, which every thread has finished reading before that same barrier
        }
    }
    float *tail_out = state + g.tail_off + (strm * g.S + c.slot_out) * (long)keep;
#pragma unroll
    for (int u = 0; u < SPT; ++u) {
        const int p = p0 + u * STFT_THREADS;
        if (p >= pb) continue;
        if (p >= c.p_tail) tail_out[p - c.p_tail] = acc[u];     // partial sums the next call goes on from (p_tail >= p_out)
        if (p >= c.p_out || p < M) continue;                    // positions before n_fft/2 are the trimmed front
        // window sum-of-squares of the frames that cover the sample (no last frame while the stream runs)
        int f_hi = p / hop;
        if (c.T >= 0 && f_hi > c.T - 1) f_hi = c.T - 1;
        const int f_lo = p < N ? 0 : (p - N + hop) / hop;
        float wss = 0.f;
        for (int fr = f_lo; fr <= f_hi; ++fr) {
            const float w = s_win[p - fr * hop];
            wss += w * w;
        }
        audio[row * out_stride + (p - c.p_first)] = wss > FLT_MIN ? acc[u] / wss : acc[u];
    }
}

// Rows = StreamCall: the lockstep call of n_rows streams; Rows = StreamPoolRows: its rows.  max_new_frames / max_span: the row with
// the most new frames / positions to emit sizes the grid.
template <int M, class Rows>
hipError_t launch_frames_m(const float *audio, long audio_stride, int n_rows, const StreamGeom &g, const Rows &rows, int max_new_frames,
                           const float *tables, float *state, hipStream_t st)
{
    using C = SpecCfg<M>;
    constexpr auto kern = stream_frames_kernel<M, Rows>;
    const hipError_t e = lds_opt_in<kern>(C::LDS);
    if (e != hipSuccess) return e;
    dim3 grid((unsigned)((max_new_frames + C::FB - 1) / C::FB), (unsigned)n_rows);
    hipLaunchKernelGGL(kern, grid, dim3(STFT_THREADS), C::LDS, st, audio, audio_stride, g, rows, tables, state);
    return hipGetLastError();
}

template <int M, class Rows>
hipError_t launch_emit_m(const float *y, int n_rows, const StreamGeom &g, const Rows &rows, long max_span, const float *tables,
                         float *state, float *audio, long out_stride, hipStream_t st)
{
    using C = ResynthCfg<M>;
    constexpr auto kern = stream_emit_kernel<M, Rows>;
    const hipError_t e = lds_opt_in<kern>(C::LDS);
    if (e != hipSuccess) return e;
    if (max_span <= 0) return hipSuccess;
    const long nblk = (max_span + C::SPAN - 1) / C::SPAN;
    if (nblk * n_rows > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kern, dim3((unsigned)(nblk * n_rows)), dim3(STFT_THREADS), C::LDS, st, y, g, rows, (int)nblk, tables, state,
                       audio, out_stride);
    return hipGetLastError();
}

}  // namespace

bool stream_geom(int n_streams, int n_fft, int hop, int window, int block, int lookahead, int max_steps, StreamGeom *g)
{
    if (n_streams < 1 || n_fft < 64 || n_fft > 4096 || (n_fft & (n_fft - 1))) return false;
    if (hop < 1 || hop > n_fft / 4 || window < 16 || block < 1 || lookahead < 0) return false;
    if ((long)block + lookahead > window || max_steps < 1) return false;
    // ring lengths in frames stay far below 2^31 (the state of a larger plan could not be allocated anyway)
    if (window > (1 << 20) || max_steps > (1 << 16) || (long)max_steps * block > (1L << 24) || n_streams > (1 << 20)) return false;
    g->n_fft = n_fft;
    g->hop = hop;
    g->W = window;
    g->B = block;
    g->A = lookahead;
    g->S = max_steps + 1;
    g->RX = max_steps * block + lookahead;
    g->RM = window + (max_steps - 1) * block;
    const long F = n_fft / 2 + 1, keep = n_fft - hop, n = n_streams;
    g->x_off = 0;                                    // the float2 rows first: 8-byte aligned whatever follows
    g->mag_off = n * 2 * F * g->RX;
    g->hist_off = g->mag_off + n * F * g->RM;
    g->tail_off = g->hist_off + n * keep * g->S;
    g->total = g->tail_off + n * keep * g->S;
    return true;
}

bool stream_pool_geom(int n_slots, int n_fft, int hop, int window, int block, int lookahead, long ring, StreamGeom *g,
                      long *ring_off, long *total)
{
    if (!stream_geom(n_slots, n_fft, hop, window, block, lookahead, 1, g)) return false;
    // what a step reads at once (history, the first step's samples) and one block more that may arrive meanwhile
    const long keep = n_fft - hop, need = keep + ((long)block + lookahead - 1) * hop + n_fft / 2 + (long)block * hop;
    if (ring < need || ring > (1L << 28)) return false;
    g->hist_off = -1;                                // no hist section: the ring holds those samples
    g->tail_off = g->mag_off + (long)n_slots * (n_fft / 2 + 1) * g->RM;
    *ring_off = g->tail_off + (long)n_slots * keep * g->S;
    *total = g->total = *ring_off + (long)n_slots * ring;
    return true;
}

hipError_t launch_stream_pool_frames(const StreamGeom &g, const StreamPoolRows &t, int max_new_frames, float *state, hipStream_t st)
{
    const float *tables = nullptr;
    hipError_t e = stft_tables(g.n_fft, &tables, st);
    if (e != hipSuccess) return e;
    return dispatch_n_fft(g.n_fft, [&](auto m) {
        return launch_frames_m<m()>(nullptr, 0L, t.n, g, t, max_new_frames, tables, state, st);
    });
}

hipError_t launch_stream_pool_windows(const float *state, const StreamGeom &g, const StreamPoolRows &t, float *out, hipStream_t st)
{
    const int F = g.n_fft / 2 + 1;
    const long tilesJ = (g.W + 31) / 32, tilesF = (F + 31) / 32;
    const long grid = tilesJ * tilesF * t.n;         // W <= 2^20, F <= 2049, n <= 256: below 2^31
    hipLaunchKernelGGL(stream_windows_kernel<StreamPoolRows>, dim3((unsigned)grid), dim3(256), 0, st, state, F, g, t, (int)tilesJ, (int)tilesF,
                       out);
    return hipGetLastError();
}

hipError_t launch_stream_pool_emit(const float *y, const StreamGeom &g, const StreamPoolRows &t, int max_span, float *state,
                                   float *audio, long out_stride, hipStream_t st)
{
    const float *tables = nullptr;
    hipError_t e = stft_tables(g.n_fft, &tables, st);
    if (e != hipSuccess) return e;
    return dispatch_n_fft(g.n_fft, [&](auto m) {
        return launch_emit_m<m()>(y, t.n, g, t, (long)max_span, tables, state, audio, out_stride, st);
    });
}

hipError_t launch_stream_frames(const float *audio, long audio_stride, int n_streams, const StreamGeom &g, const StreamCall &c,
                                float *state, hipStream_t st)
{
    const float *tables = nullptr;
    hipError_t e = stft_tables(g.n_fft, &tables, st);
    if (e != hipSuccess) return e;
    return dispatch_n_fft(g.n_fft, [&](auto m) {
        return launch_frames_m<m()>(audio, audio_stride, n_streams, g, c, c.f_new1 - c.f_new0, tables, state, st);
    });
}

hipError_t launch_stream_windows(const float *state, int n_streams, const StreamGeom &g, const StreamCall &c, float *out,
                                 hipStream_t st)
{
    const int F = g.n_fft / 2 + 1;
    const long tilesJ = (g.W + 31) / 32, tilesF = (F + 31) / 32;
    const long grid = tilesJ * tilesF * c.n_steps * (long)n_streams;
    if (grid > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stream_windows_kernel<StreamCall>, dim3((unsigned)grid), dim3(256), 0, st, state, F, g, c, (int)tilesJ, (int)tilesF,
                       out);
    return hipGetLastError();
}

hipError_t launch_stream_emit(const float *y, int n_streams, const StreamGeom &g, const StreamCall &c, float *state, float *audio,
                              long out_stride, hipStream_t st)
{
    const float *tables = nullptr;
    hipError_t e = stft_tables(g.n_fft, &tables, st);
    if (e != hipSuccess) return e;
    return dispatch_n_fft(g.n_fft, [&](auto m) {
        return launch_emit_m<m()>(y, n_streams, g, c, (long)c.p_end - c.p_begin, tables, state, audio, out_stride, st);
    });
}

}  // namespace adn
