// Resampler inside a stream for gfx950: adn_resample's filter applied to audio that is still arriving, the filter's history carried
// on the device between calls.  Definition: include/adn.h, "resample stream"; float64 restatement: tests/stream_resample_ref.py.
//
// One launch per call.  Output m reads the inputs i = floor(m down / up) - K + s, s = 0 .. 2K + 1 (K = floor(half / up)), with the
// coefficient h[(m down mod up) - (s - K) up], zero where that index leaves [-half, half].  The offline kernel gives the 64 lanes
// of a wave 64 consecutive cycles of ONE residue; a 10 ms push at 44.1 kHz is 2.3 cycles, 3 busy lanes of 64.  Here a lane takes one
// output and consecutive lanes take consecutive m, so every lane of a wave is busy whatever up and down are:
//   grid       (spans of OW = 256 outputs) x streams.  A workgroup stages the inputs its span reads -- OW down / up + 2K + 2 samples:
//              1922 at 48 -> 8 kHz, 1765 at 44.1 -> 8 kHz, 109 at 8 -> 48 kHz -- into LDS through one accessor (StreamIn::at): zero
//              before the stream's start, the carried history below received_before, `audio` from there on, zero from the end of
//              what has arrived.  While the stream runs, an emitted output meets that last zero only with a zero coefficient
//              (adn.h, "Running"); once it has ended, those zeros are adn_resample's zero extension.  OW halves down to 64 where the
//              span would not fit the LDS (down / up > 140; the limit H <= 16384 keeps 64 outputs within 133 KB).
//   arithmetic acc = 0, then acc = fmaf(x[i], h32, acc) in ascending i, one thread per output: the chain of resample_kernel, whose
//              further steps carry zero coefficients or zero samples.  The fp32 taps are resample_tap()'s, rounded once from
//              float64 by the same function.  Hence a stream's samples are adn_resample's of the finished signal, bit for bit,
//              however it was cut into calls, and a stream never reads another stream's rows.  No atomics, no workspace.
//   table      tab[step s][residue p = m mod up], built per (device, up, down): the loads of a wave are consecutive words (the
//              residues wrap at up); up = 1 (48 -> 8 kHz) is a wave-uniform load.  119 KB at 44.1 -> 8 kHz: L2-resident.
//   LDS banks  ds_read_b32 banks are word mod 32 and conflicts count inside a 32-lane half.  The lanes of a half read words
//              floor((m0 + l) down / up) apart: 48 -> 8 kHz (stride 6, gcd(6, 32) = 2) and 16 -> 8 kHz (stride 2) put two lanes on
//              each of 16 banks, 2-way; 44.1 -> 8 kHz (stride 5.5125) 2-way at worst over every phase; 8 -> 48 and 8 -> 44.1 kHz
//              read runs of equal words (broadcast), conflict-free.  Strides that are multiples of 4 are worse: 32 -> 8 kHz 4-way,
//              64 -> 8 and 192 -> 8 kHz 8-way.  So staged word u lives at u + (u >> 5), one unused word per 32 -- the offline
//              kernel's row padding, with the bank row as the row: a stride of 4 k then moves k banks on every 32 / 4k lanes.  Worst
//              case over every starting phase with it: 1 for 16, 32 and 64 -> 8 kHz, 2 for 48, 44.1, 22.05, 96 and 192 -> 8 kHz.
//
// State: two slots of H samples per stream, [stream][2][H], slot j of a call holding samples [end - H, end) of the stream (zeros
// before its start).  Who writes what (no state word is written by one workgroup and read by another in the same launch):
//   every workgroup READS slot (call_index - 1) & 1 and the call's new samples; the x = 0 workgroup of each stream WRITES slot
//   call_index & 1 -- the other slot -- with the last H samples of (old history ++ new samples).  Call 0 has received_before = 0:
//   every position below it is before the stream's start and reads as zero, so no slot is read and a new stream needs no reset.
//   A ring indexed by absolute position would not do: a push longer than the ring makes one workgroup overwrite words another
//   is still reading.
//
// What bounds it: the work of a push is tiny (31 k FMAs for one stream and 10 ms at 48 kHz), one wave walks 2K + 2 dependent FMAs
// whose coefficients come from L2.  The kernel is latency-bound; what matters is that a call is a single launch with no host
// synchronisation.  FMA throughput is not tuned.
#include "adn_internal.h"

#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

namespace adn {
namespace {

constexpr int SR_THREADS = 256;
constexpr int SR_MAX_LDS_FLOATS = 40 * 1024 - 64;      // the CU's 160 KiB

// what one call covers (passed by value)
struct SrCall {
    long m0, n_out;            // first output and outputs per stream
    long rb, end;              // samples received before / after this call
    int up, down, K, H;
    int OW, nblk;              // outputs per workgroup, workgroups per stream
    int slot_in, slot_out, write_hist;
};

// Sample i of the stream: zero before its start and from the end of what has arrived; the call's new samples start at rb, the H
// before them are the carried history.
struct StreamIn {
    const float *audio, *hist;
    long rb, end;
    int H;
    __device__ __forceinline__ float at(long i) const
    {
        if (i < 0 || i >= end) return 0.f;
        if (i >= rb) return audio[i - rb];
        const long j = i - (rb - H);
        return j >= 0 ? hist[j] : 0.f;                 // (j < 0: below what any output of this call reads)
    }
};

// staged word u lives at u + u / 32 (header, "LDS banks")
__host__ __device__ __forceinline__ int skew(int u) { return u + (u >> 5); }

// Where a workgroup gets its call from: the kernel is a template on the argument that says it, as in stream_kernels.hip.
// Lockstep (SrCall): one call for all streams, made on the host; workgroup x belongs to stream x / nblk.  Pooled (SrPoolRows,
// adn.h "stream pool at a rate"): a table in the kernel arguments in which every ROW is a call of its own stream -- its own rate
// pair, table, position and span size OW; blk0 is the prefix of the rows' workgroup counts, and a workgroup finds its row by
// bisection.  A row's two history slots lie max_history floats apart in a caller-owned rate state, [2 slot + direction][2][max_history];
// the who-writes-what rule of the header holds row by row, for which a call names no (slot, direction) twice.
constexpr int SR_POOL_ROWS = STREAM_POOL_RATE_MAX_ROWS;
struct SrPoolRow {             // 48 bytes
    const float *tab;          // coefficient table of the row's rate pair; null for equal rates: a copy, no history
    long src_off;              // the row's new samples start at audio + src_off
    int hslot;                 // 2 slot + direction
    int rb, n_new;             // samples received before this call, and new ones
    int m0, n_out;             // first output and outputs
    int bits;                  // OW | slot_in << 16 | write_hist << 17
    unsigned short up, down, K, H;
};
struct SrPoolRows {
    long ring_off;             // ring destination: floats from the start of the pool state to slot 0's ring
    int R, max_history, n;
    int blk0[SR_POOL_ROWS + 1];
    SrPoolRow row[SR_POOL_ROWS];
};
static_assert(sizeof(SrPoolRow) == 48 && sizeof(SrPoolRows) + 6 * 8 <= 4096, "the row table must fit the kernel-argument segment");
template <class Rows> constexpr bool SR_POOLED = std::is_same_v<Rows, SrPoolRows>;

// RING (pooled only): output m of the row's stream goes to word m mod R of its slot's ring inside the pool state (`out`), the wrap
// handled per output; otherwise row i writes its outputs from out + i out_stride on.
template <class Rows, bool RING>
__global__ __launch_bounds__(SR_THREADS) void stream_resample_kernel(const float *__restrict__ audio, long audio_stride,
                                                                    float *__restrict__ state, Rows rows,
                                                                    const float *__restrict__ tab, float *__restrict__ out,
                                                                    long out_stride)
{
    static_assert(SR_POOLED<Rows> || !RING, "only a pool has rings");
    extern __shared__ float xs[];
    SrCall c;
    int stream, blk;                                      // the row of the launch and the workgroup inside it
    float *hist;
    long hist_stride;                                     // between the two history slots of a row
    if constexpr (SR_POOLED<Rows>) {
        int lo = 0, hi = rows.n;                          // blk0[lo] <= x < blk0[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (rows.blk0[mid] <= (int)blockIdx.x) lo = mid; else hi = mid;
        }
        const SrPoolRow &r = rows.row[lo];
        stream = lo, blk = (int)blockIdx.x - rows.blk0[lo];
        c.m0 = r.m0, c.n_out = r.n_out, c.rb = r.rb, c.end = (long)r.rb + r.n_new;
        c.up = r.up, c.down = r.down, c.K = r.K, c.H = r.H;
        c.OW = r.bits & 0xffff, c.slot_in = (r.bits >> 16) & 1, c.slot_out = c.slot_in ^ 1, c.write_hist = (r.bits >> 17) & 1;
        audio += r.src_off;
        tab = r.tab;
        hist_stride = rows.max_history;
        hist = state + (long)r.hslot * 2 * hist_stride;
        if constexpr (RING) out += rows.ring_off + (long)(r.hslot >> 1) * rows.R;
        else out += (long)stream * out_stride;
        if (tab == nullptr) {                             // equal rates: output m is input m
            const long rel = (long)blk * c.OW + threadIdx.x;
            if (rel < c.n_out) out[RING ? (c.m0 + rel) % rows.R : rel] = audio[rel];
            return;
        }
    } else {
        c = rows;
        stream = blockIdx.x / c.nblk, blk = blockIdx.x - stream * c.nblk;
        audio += (long)stream * audio_stride;
        hist_stride = c.H;
        hist = state + (long)stream * 2 * hist_stride;
        out += (long)stream * out_stride;
    }
    const StreamIn in{audio, hist + c.slot_in * hist_stride, c.rb, c.end, c.H};
    const long rel0 = (long)blk * c.OW;                   // first output of this workgroup, relative to m0
    const long mA = c.m0 + rel0;
    const long t0 = mA * c.down, A0 = t0 / c.up;
    const int ph0 = (int)(t0 - A0 * c.up);                // mA down = A0 up + ph0
    const long lo = A0 - c.K;                             // first staged sample
    const long left = c.n_out - rel0;
    const int nw = left < c.OW ? (int)left : c.OW;        // outputs of this workgroup (0: a call that only carries history)
    const int steps = 2 * c.K + 2;
    if (nw > 0) {
        const int cnt = (ph0 + (nw - 1) * c.down) / c.up + steps;
        for (int u = threadIdx.x; u < cnt; u += SR_THREADS) xs[skew(u)] = in.at(lo + u);
    }
    if (blk == 0 && c.write_hist) {
        float *ho = hist + c.slot_out * hist_stride;
        for (int j = threadIdx.x; j < c.H; j += SR_THREADS) ho[j] = in.at(c.end - c.H + j);
    }
    __syncthreads();
    if ((int)threadIdx.x < nw) {
        const int rel = (ph0 + (int)threadIdx.x * c.down) / c.up;          // floor(m down / up) - A0
        const int p = (int)((mA + threadIdx.x) % c.up);
        const float *__restrict__ t = tab + p;
        float acc = 0.f;
#pragma unroll 16
        for (int s = 0; s < steps; ++s) acc = fmaf(xs[skew(rel + s)], t[s * c.up], acc);
        if constexpr (RING) out[(mA + threadIdx.x) % rows.R] = acc;
        else out[rel0 + threadIdx.x] = acc;
    }
}

struct TabKey {
    int device, up, down;
    bool operator<(const TabKey &o) const
    {
        if (device != o.device) return device < o.device;
        return up != o.up ? up < o.up : down < o.down;
    }
};
std::mutex g_tab_mu;
std::map<TabKey, float *> g_tabs;

// tab[s][p]: coefficient of input floor(m down / up) - K + s for the outputs m = p mod up
hipError_t get_tab(const ResampleStreamGeom &g, const float **out, hipStream_t st)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(g_tab_mu);
    auto it = g_tabs.find(TabKey{dev, g.up, g.down});
    if (it != g_tabs.end()) { *out = it->second; return hipSuccess; }
    if (stream_is_capturing(st)) return ADN_COLD_IN_CAPTURE;      // the upload below blocks (adn_resample_prepare)
    const int steps = 2 * g.K + 2;
    std::vector<float> h((size_t)steps * g.up, 0.f);
    for (int p = 0; p < g.up; ++p) {
        const long ph = (long)p * g.down % g.up;
        for (int s = 0; s < steps; ++s) {
            const long j = ph - (long)(s - g.K) * g.up;
            if (j >= -g.half && j <= g.half) h[(size_t)s * g.up + p] = resample_tap(j, g.up, g.down);
        }
    }
    float *tab = nullptr;
    e = hipMalloc(&tab, h.size() * sizeof(float));
    if (e != hipSuccess) return e;
    e = hipMemcpy(tab, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(tab); return e; }
    g_tabs[TabKey{dev, g.up, g.down}] = tab;
    *out = tab;
    return hipSuccess;
}

// staged samples of a workgroup of `ow` outputs, at the worst phase
long staged(const ResampleStreamGeom &g, int ow) { return ((long)(g.up - 1) + (long)(ow - 1) * g.down) / g.up + 2L * g.K + 2; }

// outputs per workgroup for a rate pair: 256, halved down to 64 where the span would not fit the LDS; *words: its LDS floats
int span_outputs(const ResampleStreamGeom &g, long *words)
{
    int ow = SR_THREADS;
    while (ow > 64 && skew((int)staged(g, ow)) + 1 > SR_MAX_LDS_FLOATS) ow /= 2;
    *words = skew((int)staged(g, ow)) + 1;
    return ow;
}

hipError_t allow_lds(const void *kernel, long words)
{
    const size_t lds = (size_t)words * sizeof(float);
    return lds > 64 * 1024 ? hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) : hipSuccess;
}

}  // namespace

bool resample_stream_geom(int src_rate, int dst_rate, ResampleStreamGeom *g)
{
    if (!resample_ratio(src_rate, dst_rate, &g->up, &g->down)) return false;
    g->half = resample_half(g->up, g->down);
    g->K = (int)(g->half / g->up);
    g->H = 2L * g->K + (g->down + g->up - 1) / g->up + 1;
    g->latency = (g->half + g->up - 1) / g->up;
    if (g->up == g->down) g->H = g->latency = 0;          // equal rates: a copy
    return true;
}

long resample_stream_emitted(const ResampleStreamGeom &g, long n, bool final)
{
    if (g.up == g.down) return n;
    if (final) return (n * g.up + g.down - 1) / g.down;
    return n * g.up <= g.half ? 0 : (n * g.up - g.half - 1) / g.down + 1;
}

hipError_t resample_stream_prepare(const ResampleStreamGeom &g, hipStream_t st)
{
    const float *tab = nullptr;
    return get_tab(g, &tab, st);
}

hipError_t launch_resample_stream(float *state, const float *audio, long audio_stride, int n_streams, const ResampleStreamGeom &g,
                                  long call_index, long received_before, long n_new, bool final, float *out, long out_stride,
                                  hipStream_t st)
{
    SrCall c{};
    c.rb = received_before;
    c.end = received_before + n_new;
    c.m0 = resample_stream_emitted(g, c.rb, false);
    c.n_out = resample_stream_emitted(g, c.end, final) - c.m0;
    c.up = g.up, c.down = g.down, c.K = g.K, c.H = (int)g.H;
    c.slot_in = (int)((call_index - 1) & 1), c.slot_out = (int)(call_index & 1);
    c.write_hist = final ? 0 : 1;                         // nothing follows the last call
    if (c.n_out == 0 && !c.write_hist) return hipSuccess;
    long words = 0;
    c.OW = span_outputs(g, &words);
    if (words > SR_MAX_LDS_FLOATS) return hipErrorInvalidValue;
    const long nblk = c.n_out > 0 ? (c.n_out + c.OW - 1) / c.OW : 1;
    if (nblk * n_streams > 0x7fffffffL) return hipErrorInvalidValue;
    c.nblk = (int)nblk;
    const float *tab = nullptr;
    hipError_t e = get_tab(g, &tab, st);
    if (e != hipSuccess) return e;
    const auto kernel = stream_resample_kernel<SrCall, false>;
    e = allow_lds(reinterpret_cast<const void *>(kernel), words);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(nblk * n_streams)), dim3(SR_THREADS), (size_t)words * sizeof(float), st, audio,
                       audio_stride, state, c, tab, out, out_stride);
    return hipGetLastError();
}

hipError_t launch_resample_stream_rows(const ResampleStreamRow *rows, int n_rows, const float *audio, float *rate_state,
                                       long max_history, float *out, long out_stride, bool ring, long ring_off, long R, hipStream_t st)
{
    SrPoolRows t{};
    t.ring_off = ring_off, t.R = (int)R, t.max_history = (int)max_history, t.n = n_rows;
    long max_words = 1, total = 0;
    for (int i = 0; i < n_rows; ++i) {
        const ResampleStreamRow &r = rows[i];
        const ResampleStreamGeom &g = r.g;
        SrPoolRow &w = t.row[i];
        const long end = r.received_before + r.n_new;
        const long m0 = resample_stream_emitted(g, r.received_before, false);
        const long n_out = resample_stream_emitted(g, end, r.final) - m0;
        const bool copy = g.up == g.down, write_hist = !copy && !r.final;      // nothing follows the last call
        long words = 1;
        const int OW = copy ? SR_THREADS : span_outputs(g, &words);
        if (words > SR_MAX_LDS_FLOATS) return hipErrorInvalidValue;
        if (!copy) {                                      // one lookup per rate pair of the call, not per row
            int j = 0;
            while (j < i && (rows[j].g.up != g.up || rows[j].g.down != g.down)) ++j;
            if (j < i) w.tab = t.row[j].tab;
            else {
                const hipError_t e = get_tab(g, &w.tab, st);
                if (e != hipSuccess) return e;            // (cold in a capture: nothing has been enqueued)
            }
        }
        w.src_off = r.src_off;
        w.hslot = 2 * r.slot + r.direction;
        w.rb = (int)r.received_before, w.n_new = (int)r.n_new, w.m0 = (int)m0, w.n_out = (int)n_out;
        w.bits = OW | (int)((r.call_index - 1) & 1) << 16 | (write_hist ? 1 : 0) << 17;
        w.up = (unsigned short)g.up, w.down = (unsigned short)g.down, w.K = (unsigned short)g.K, w.H = (unsigned short)g.H;
        t.blk0[i] = (int)total;
        total += n_out > 0 ? (n_out + OW - 1) / OW : write_hist ? 1 : 0;
        if (total > 0x7fffffffL) return hipErrorInvalidValue;
        if (n_out > 0 && words > max_words) max_words = words;
    }
    for (int i = n_rows; i <= SR_POOL_ROWS; ++i) t.blk0[i] = (int)total;
    if (total == 0) return hipSuccess;
    const auto kernel = ring ? stream_resample_kernel<SrPoolRows, true> : stream_resample_kernel<SrPoolRows, false>;
    const hipError_t e = allow_lds(reinterpret_cast<const void *>(kernel), max_words);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3((unsigned)total), dim3(SR_THREADS), (size_t)max_words * sizeof(float), st, audio, 0L, rate_state,
                       t, static_cast<const float *>(nullptr), out, out_stride);
    return hipGetLastError();
}

}  // namespace adn
