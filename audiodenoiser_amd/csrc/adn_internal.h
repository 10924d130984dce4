// Internal declarations shared by the translation units of libadn.so (not part of the public ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace adn {

// Activation layout inside the library (never visible at the ABI: the network input and output have one channel):
// channel-blocked, one block = 32 bytes of channels per pixel -- [N][C/8][H][W][8] for fp32 ("C8"), [N][C/16][H][W][16]
// for fp16 ("C16").  The 3x3 kernels walk K in chunks of one block and copy a halo of neighbouring pixels per chunk: blocked,
// a halo row of one chunk is one contiguous run (34 pixels x 32 bytes), so the LDS-DMA gather fetches whole cache lines; in
// NHWC every 16-byte piece sat in a different 128-byte line of which a chunk used a quarter (measured on the F(4x4,3x3)
// kernel: the gather pattern alone cost 8 % of the batch-64 forward).  Every C is a multiple of 16 (64 ... 1024).
// act_off: element offset of (pixel, channel) inside one image of C channels and HW pixels; ACT_BLOCK<T>: channels per block.
template <typename T> constexpr int ACT_BLOCK = 32 / (int)sizeof(T);
template <typename T>
__host__ __device__ __forceinline__ long act_off(int C, long HW, long pix, int c)
{
    constexpr int B = ACT_BLOCK<T>;
    (void)C;
    return ((long)(c / B) * HW + pix) * B + (c % B);
}

#ifdef __HIPCC__
// Vector types of the kernels: the register images of 4 / 8 / 16-byte memory operations and the operands of the MFMAs.
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// volatile LDS views: keep each patch / B-fragment read of the Winograd kernels a single ds_read_b64 / ds_read_b128
typedef const volatile f32x2 __attribute__((address_space(3))) lds_cv_f32x2;
typedef const volatile f32x4 __attribute__((address_space(3))) lds_cv_f32x4;

// Bijective remap of the workgroup id so that the workgroups sharing an XCD (ids congruent mod 8, observed round-robin placement)
// work on neighbouring tiles: what they fetch meets in ONE L2.  Affects speed only, never results.
__device__ __forceinline__ int xcd_remap(int b, int nwg)
{
    const int xcd = b & 7, q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
}

// lane id without the work-item-id register: values derived from threadIdx.x would otherwise have to survive a K loop
// (in registers the loop needs, i.e. as scratch spills: measured 0.3 GB of spill traffic per full-resolution wino4_conv_f32 launch)
__device__ __forceinline__ int lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// GEMM column of the transposed convolution -> sub-pixel ij = 2*di + dj and output channel:
//   column = ((di*(Cout/64) + cg)*2 + dj)*64 + c64, co = 64*cg + c64: the 128 columns of a workgroup are both dj of one di and
//   64 channels, so that its stores cover whole runs of output pixels (2*gx + dj) per channel block.  The kernels, the weight
//   packers (pack_convt*, unet.hip) and the bias vector all take the order from here.
__host__ __device__ __forceinline__ void convt_column(int col, int Cout, int &ij, int &co)
{
    const int c64 = col & 63, dj = (col >> 6) & 1, g = col >> 7, ncg = Cout >> 6;
    const int di = g / ncg, cg = g - di * ncg;
    ij = 2 * di + dj;
    co = 64 * cg + c64;
}
#endif

// LDS-DMA through a buffer descriptor (buffer_load_dwordx4 ... offen lds): lane l of the wave copies the 16 bytes at
// descriptor base + voff + soff to lds_wave_base + 16 l.  The range check compares voff with the descriptor's size MINUS soff
// (measured in round 5: a scalar offset that leaves the range drops the access although voff alone is inside), and a
// lane that fails it writes ZEROS into its LDS slot (tools/ubench/buffer_lds_oob.hip): the convolutions' zero padding and the
// pad slots of the LDS layouts cost no select against a zero block and no 64-bit address arithmetic -- a copy piece is one
// scalar add and the instruction.  ADN_DMA_OOB: voff of a padding lane (every image is smaller than that: F*T < 2^24).
#ifdef __HIPCC__
constexpr unsigned ADN_DMA_OOB = 0xfffffff0u;
__device__ __forceinline__ void dma16_buf(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff, float *lds_wave_base)
{
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void *)lds_wave_base, 16, voff, soff, 0, 0);
}
// descriptor over `bytes` bytes at `base` (both wave-uniform)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t dma_rsrc(const void *base, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, bytes, 0x00020000);
}
#endif

#ifdef __HIPCC__
// ReLU and max-pool as the reference computes them (torch.relu / nn.MaxPool2d, /root/reference/code/model.py:13,16,26): a NaN
// operand gives NaN, -inf gives 0, +inf stays +inf -- IEEE-754-2019 `maximum`, ONE instruction on gfx950 (v_maximum3_f32;
// v_pk_maximum3_f16 for packed halfs).  fmaxf / v_max_f32 is maxNum: it returns the other operand, i.e. it would turn the NaN
// that an inf pixel of the reference's own loader (data_loader.py:41-42: fp16 overflow) becomes into a plausible-looking zero.
// Every ReLU and pooling maximum of the library goes through these.
__device__ __forceinline__ float relu_nan(float v) { return __builtin_elementwise_maximum(v, 0.f); }
__device__ __forceinline__ float max_nan(float a, float b) { return __builtin_elementwise_maximum(a, b); }
__device__ __forceinline__ float max4_nan(float a, float b, float c, float d) { return max_nan(max_nan(a, b), max_nan(c, d)); }
#endif

#ifdef __HIPCC__
// Three-term bf16 split of eight fp32 values (the fp32 transposed convolutions on the bf16 matrix cores: conv_dma<..., SPLIT> in
// conv_kernels.hip): x = hi + mid + lo with round-to-nearest terms, 24 mantissa bits in all.  hi is clamped to
// the largest finite bf16 so that every FINITE x splits exactly (round-to-nearest would make a bf16 infinity of |x| >= 3.3961e38);
// x = +-inf gives hi = 3.39e38, mid = +-inf, lo = NaN: non-finite stays non-finite.
constexpr float ADN_BF16_MAX_F = 0x1.fep127f;                  // largest finite bf16
__device__ __forceinline__ void split3_bf16(const f32x4 &x0, const f32x4 &x1, bf16x8 &hi, bf16x8 &mid, bf16x8 &lo)
{
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = e < 4 ? x0[e] : x1[e - 4];
        const float hf = __builtin_amdgcn_fmed3f((float)(__bf16)x, -ADN_BF16_MAX_F, ADN_BF16_MAX_F);
        const float r1 = x - hf;
        const __bf16 m = (__bf16)r1;
        const float r2 = r1 - (float)m;
        hi[e] = (__bf16)hf;
        mid[e] = m;
        lo[e] = (__bf16)r2;
    }
}
#endif

#ifdef __HIPCC__
// The transforms of Winograd F(4x4,3x3) for the points (0, 1, -1, 2, -2, inf), on one value per lane (float) or on packed values
// (f32x2, f32x4: the same operations element by element).  One definition: wino4_conv_f32 forms V = B^T d B and A^T M A in
// registers with them, the three-stage form (wino3s_kernels.hip) in kernels of their own, and both give the same bits.
template <typename V>
__device__ __forceinline__ V wino_fma(float c, V a, V b)
{
    if constexpr (std::is_same_v<V, float>) return __builtin_fmaf(c, a, b);
    else return __builtin_elementwise_fma((V)c, a, b);
}
// B^T x, in place:
//   [ 4  0 -5  0  1  0 ]      twelve operations
//   [ 0 -4 -4  1  1  0 ]
//   [ 0  4 -4 -1  1  0 ]
//   [ 0 -2 -1  2  1  0 ]
//   [ 0  2 -1 -2  1  0 ]
//   [ 0  4  0 -5  0  1 ]
template <typename V>
__device__ __forceinline__ void bt6(V &d0, V &d1, V &d2, V &d3, V &d4, V &d5)
{
    const V pe = wino_fma(-4.f, d2, d4);
    const V po = wino_fma(-4.f, d1, d3);
    const V se = d4 - d2;
    const V so = d3 - d1;
    const V r0 = wino_fma(4.f, d0, pe) - d2;
    const V r5 = wino_fma(4.f, d1, wino_fma(-5.f, d3, d5));
    d0 = r0;
    d1 = pe + po;
    d2 = pe - po;
    d3 = wino_fma(2.f, so, se);
    d4 = wino_fma(-2.f, so, se);
    d5 = r5;
}
// A^T m (6 -> 4), ten operations:
//   [ 1 1  1 1  1 0 ]
//   [ 0 1 -1 2 -2 0 ]
//   [ 0 1  1 4  4 0 ]
//   [ 0 1 -1 8 -8 1 ]
template <typename V>
__device__ __forceinline__ void at6(V m0, V m1, V m2, V m3, V m4, V m5, V &y0, V &y1, V &y2, V &y3)
{
    const V a = m1 + m2, b = m1 - m2, c = m3 + m4, d = m3 - m4;
    y0 = m0 + a + c;
    y1 = wino_fma(2.f, d, b);
    y2 = wino_fma(4.f, c, a);
    y3 = wino_fma(8.f, d, b) + m5;
}
#endif

// One activation source of a convolution (fp32 or fp16 storage, decided by the launcher).  (offY, offX) is
// the zero-pad placed above / left of the tensor when it is aligned to the output domain (UpSampleLayer's F.pad,
// reference model.py:44-47).
struct ConvSrc {
    const void *ptr;
    int H, W, C;
    int offY, offX;
};

// Division of a wave-uniform index by a launch constant without the ~25-instruction software divide: q = mulhi(n, ceil(2^32 / d)),
// exact while n * d < 2^32 (the launcher checks its grid against that); d == 1 passes n through.
struct FastDiv {
    unsigned d, m;
};
inline FastDiv make_fastdiv(unsigned d) { return FastDiv{d, d > 1 ? (unsigned)((0x100000000ull + d - 1) / d) : 0u}; }
#ifdef __HIPCC__
__device__ __forceinline__ int fastdiv(int n, unsigned d, unsigned m) { return d == 1 ? n : (int)__umulhi((unsigned)n, m); }
#endif

// Arguments of the matrix-core convolution kernels (3x3 convolution or 2x2-stride-2 transposed convolution).
struct ConvArgs {
    ConvSrc s0, s1;        // channels [0, s0.C) come from s0, [s0.C, s0.C + s1.C) from s1 (virtual concat)
    int nchunk0, nchunk;   // K-chunks served by s0 / in total
    const void *wpk;       // packed weights, see pack_* in unet.hip
    const void *wpk4;      // fp32 3x3 layers: the same weights packed for the F(4x4,3x3) kernel (pack_wino4_3x3), or nullptr
    const float *bias;     // per GEMM column (BatchNorm folded), always fp32
    void *out;             // output in the blocked layout (above)
    void *pool;            // optional 2x2 max-pooled output, same layout (CONV3X3_RELU_POOL)
    int N, H, W;           // tile domain: output H,W for 3x3; INPUT h,w for the transposed convolution
    int Cout;              // output channels of the layer (GEMM columns = Cout, or 4*Cout for convT)
    int tilesY, tilesX, nct;
    int pair;              // wino4_conv_f32 only: 1 = a workgroup tile holds two clips side by side (images <= 16 px wide)
    FastDiv fdGc, fdNcg, fdTx, fdTy;   // wino4_conv_f32 only: the divisors of its tile decode (fdGc.d == 0: plain division)
    int nwg_total;         // wino4_conv_f32 only: logical workgroup ids (= tiles incl. supertile padding) of the launch
    int split;             // fp32 transposed convolution only: 1 = weights are three bf16 planes (pack_convt_split), the contraction
                           // runs as six bf16 MFMA products per term pair with fp32 accumulation (conv_dma<..., SPLIT>);
                           // 1 + SplitTile (below): planes packed for that workgroup tile, nct = 4 Cout / its columns (no K split)
    // split-K (small batches; F(2x2,3x3) kernel, and the fp32 transposed convolutions with `out` = the partial buffer -- see
    // conv_dma's KSPLIT): `ksplit` workgroups share one output tile, each sums a slice
    // of nchunk/ksplit chunks and writes raw partial sums to `partial` [split][N][H][W][Cout]; a second launch adds
    // them in a fixed order and applies bias / ReLU / pooling.  ksplit = 1: everything in one launch.
    int ksplit;
    int nwg_base;          // workgroups per split (grid = nwg_base * ksplit)
    float *partial;
    // CONV3X3_RELU_DOT: weights of the fused 1x1 convolution (Cout floats) and its partial planes [nct][N][H][W]
    const float *dotw;
    float *dot_out;
    float dot_bias;        // fp16 kernel only (one workgroup holds all 64 channels: dot_out IS the network output)
    // Fused first layer (Winograd kernel, down1's second conv): s0.ptr is the network INPUT (N,1,H,W) and the halo of the
    // 64-channel tensor Conv2d(1->64)+BN+ReLU (model.py:11-13 via :56) is computed on the fly from firstw [9 taps][64] and
    // firstb [64] (BatchNorm folded) instead of being copied; nullptr = ordinary activation source
    const float *firstw, *firstb;
    // WINO_GEMM only (the matrix stage of the three-stage F(4x4,3x3) form, below): the GEMM's rows = 4x4 output tiles of the
    // whole batch; 0 for every other kind
    long rows;
};

// wino4_conv_f32's pair mode: a workgroup tile holds the same 32 rows of TWO neighbouring clips side by side (images at most 16
// pixels wide, e.g. the 32x16 bottleneck of a 513x256 input).  Its copies reach both clips through one buffer descriptor, so the
// image of a clip plus one channel block must stay inside the 4 GB a descriptor spans (always, except for absurdly tall 16-wide
// images, which then run unpaired or on the F(2x2,3x3) kernel).
inline bool wino4_pair_mode(const ConvArgs &a)
{
    if (a.W > 16) return false;
    const size_t i0 = (size_t)a.s0.C * a.s0.H * a.s0.W * 4, i1 = (size_t)a.s1.C * a.s1.H * a.s1.W * 4;
    return (i0 > i1 ? i0 : i1) + (size_t)a.H * a.W * 32 < (size_t)0xfffffff0u;
}

// Largest number of K splits any launcher asks for (wino_ksplit, convt_ksplit, conv16_ksplit); the reduce kernels read all the
// copies of an element before adding them (one memory latency per element instead of one per copy)
constexpr int ADN_MAX_KSPLIT = 8;

// Workgroups of one K split of a launch whose tile grid is written into its arguments (conv_mfma_tiles / wino_tiles below): what the
// launchers size their grid by, and what the *_ksplit rules are asked about.
inline long conv_workgroups(const ConvArgs &a) { return (long)a.N * a.tilesY * a.tilesX * a.nct; }

// Number of K splits for a 3x3 layer launched as `nwg` Winograd workgroups of `nchunk` chunks: only when the grid
// cannot fill the 512 workgroup slots of the chip (2 per CU) and the K loop is long enough to be worth cutting.
inline int wino_ksplit(long nwg, int nchunk)
{
    int ks = 1;
    while (ks < 8 && nwg * ks * 2 <= 512 && nchunk % (ks * 2) == 0 && nchunk / (ks * 2) >= 4) ks *= 2;
    return ks;
}

// Number of K splits for a 3x3 layer launched as `grid` F(4x4,3x3) workgroups (one per CU) of `nchunk` chunks: while the cut grid
// stays within a workgroup per CU and a slice keeps >= 8 chunks (the kernel's 20 000 clocks around the K loop want amortising).
inline int wino4_ksplit(long grid, int nchunk)
{
    int ks = 1;
    while (ks < ADN_MAX_KSPLIT && grid * ks * 2 <= 256 && nchunk % (ks * 2) == 0 && nchunk / (ks * 2) >= 8) ks *= 2;
    return ks;
}

// Number of K splits for a transposed convolution (fp32 split-bf16 form) launched as `nwg` workgroups of `nchunk` 16-channel chunks
// whose output is `out_floats` floats.  A chunk is 12 KB of weights and 32 MFMAs per wave: latency-bound at ~1.3 us whatever the
// occupancy, so one clip at the two deepest levels (64 / 128 workgroups, 64 / 32 chunks) is cut over several workgroups.  Chosen by
// the measured times (profiles/r05_b1_timelines.txt), in microseconds: 8 + 1.28 per chunk and round of 768 workgroups (three per
// CU); a reduce launch 4 + (copies + 1) x output bytes at 8 TB/s; a slice keeps >= 8 chunks.
inline int convt_ksplit(long nwg, int nchunk, size_t out_floats)
{
    const double out_mb = (double)out_floats * 4.0 * 1e-6;
    int best = 1;
    double tbest = 0.0;
    for (int ks = 1; ks <= ADN_MAX_KSPLIT; ks *= 2) {
        if (nchunk % ks || (ks > 1 && nchunk / ks < 8)) break;
        const double t = 8.0 + 1.28 * (nchunk / ks) * (double)((nwg * ks + 767) / 768) + (ks > 1 ? 4.0 + (ks + 1) * out_mb / 8.0 : 0.0);
        if (ks == 1 || t < tbest - 0.5) {
            best = ks;
            tbest = t;
        }
    }
    return best;
}

// Number of K splits for an fp16 3x3 layer launched as `nwg` workgroups (32x16 pixels x 64 couts) of `nchunk` 16-channel chunks:
// one clip at the deep levels is 16-64 workgroups running 16-64 chunks of ~1.3 us each on a chip of 256 CUs.  Cut while the grid stays
// within a workgroup per CU, a slice keeps >= 4 chunks and the partial sums (ksplit * out_floats fp32) stay small (32 MB).
inline int conv16_ksplit(long nwg, int nchunk, size_t out_floats)
{
    if (nwg > 64) return 1;
    int ks = 1;
    while (ks < 8 && nwg * ks * 2 <= 256 && nchunk % (ks * 2) == 0 && nchunk / (ks * 2) >= 4 &&
           (size_t)(ks * 2) * out_floats * 4 <= ((size_t)32 << 20))
        ks *= 2;
    return ks;
}

// CONV3X3_RELU_DOT (Winograd kernel only): conv3x3 + BN + ReLU whose 64-channel result is never written; instead every
// workgroup contracts its 32 output channels with the weights of the following 1x1 convolution (reference model.py:68,93,
// the network's last layer) and stores one float per pixel into plane `ct` of ConvArgs::dot_out; launch_dot_finish adds
// the planes and the bias.  Saves the 64-channel tensor's HBM round trip (write + read of N*H*W*64 floats).
// fp16 kernel (conv_dma, 64 couts per workgroup): the dot is complete inside the workgroup, dot_out is the final output.
// WINO_GEMM (conv_dma, fp32 split-bf16 form only): one of the 36 transform-domain GEMMs of the three-stage F(4x4,3x3) form --
// "clip" = position, the "image" = the rows of V 16 to a line, raw sums stored in the same layout (launch_wino_gemm).
enum ConvKind { CONV3X3_RELU = 0, CONV3X3_RELU_POOL = 1, CONVT2X2 = 2, CONV3X3_RELU_DOT = 3, WINO_GEMM = 4 };

// Tile geometry chosen per layer (must match the weight packing).
struct ConvGeom {
    int TH;      // tile rows (tile is TH x 16 pixels)
    int BN;      // GEMM columns per block
    int KC;      // channels per K-chunk
};
ConvGeom conv_geom(ConvKind kind, int Cout, bool f16);
// The direct kernels' tile grid of a layer (conv_geom's tiles over a.N / H / W / Cout) written into a.tilesY / tilesX / nct; returns
// conv_workgroups(a).  The one place the workspace plan, the kernel choice and the launch arguments get that grid from.
long conv_mfma_tiles(ConvKind kind, bool f16, ConvArgs &a);

// Opts KERNELS in to `bytes` of dynamic LDS (more than the 64 KB a launch may ask for by default) on the current device, once per
// device: the attribute is per device, and a handle may be created on any.  A device's bit is marked only after every kernel of the
// group took the attribute; the first error is returned.
template <auto... KERNELS>
hipError_t lds_opt_in(size_t bytes)
{
    static std::atomic<unsigned long long> done{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return hipErrorInvalidDevice;
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
    for (const void *k : {reinterpret_cast<const void *>(KERNELS)...}) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
    }
    done.fetch_or(bit, std::memory_order_release);
    return hipSuccess;
}
// CUs of the device the persistent kernels size their grids by, in whole slots on each of the 8 XCDs; looked up once (one device
// model per process: gfx950 only, checked at handle creation).  0: the lookup failed.
inline int device_cus()
{
    static std::atomic<int> cus{0};
    int c = cus.load(std::memory_order_relaxed);
    if (c == 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c < 8)
            return 0;
        c &= ~7;
        cus.store(c, std::memory_order_relaxed);
    }
    return c;
}

// Direct implicit-GEMM kernels (conv_kernels.hip), fp32 or fp16 storage.
hipError_t launch_conv_mfma(ConvKind kind, const ConvArgs &a, bool f16, hipStream_t st);
// second launch of a K-split 3x3 layer (conv_kernels.hip): the slices of wino_conv_dma_f32, wino4_conv_f32 (fp32) or conv_dma (fp16)
// wrote fp32 sums [split][N][H][W][Cout] into a.partial; a.ksplit copies + a.bias, ReLU -> a.out (+ a.pool) in the blocked layout
hipError_t launch_conv_reduce(ConvKind kind, const ConvArgs &a, bool f16, hipStream_t st);
// second launch of a K-split transposed convolution (ConvArgs::ksplit > 1, fp32 split-bf16 form): out = sum of the copies + bias
hipError_t launch_convt_reduce(const float *partial, const float *bias, float *out, int ksplit, int N, int Ho, int Wo, int Cout,
                               hipStream_t st);
// Winograd F(2x2,3x3) variant of the 3x3 kinds, fp32 only (wino_kernels.hip): tile 16x16 px x WINO_BN couts, 8-ch chunks.
constexpr int WINO_BN = 32;
hipError_t launch_wino_conv(ConvKind kind, const ConvArgs &a, hipStream_t st);
// its tile grid of a layer written into a.tilesY / tilesX / nct (the launcher does the same); returns conv_workgroups(a): the
// workgroups of one K split that have a tile to compute (what wino_ksplit() is asked about)
long wino_tiles(ConvArgs &a);
// Winograd F(4x4,3x3) variant (wino4_kernels.hip): tile 32x32 px x 32 couts, 8-ch chunks, weights from ConvArgs::wpk
// in pack_wino4_3x3 layout.  wino4_applicable: plain / pooled 3x3 layers whose image the 32x32 tiles cover with little
// waste; everything else (fused first / last layer, split-K, small images) stays on F(2x2,3x3).
bool wino4_applicable(ConvKind kind, const ConvArgs &a, bool force);
// workgroups of one K split of its launch of a layer, without the supertile padding (what wino4_ksplit() is asked about): 32x32-pixel
// tiles x 32 couts over a.N / H / W / Cout, two clips per tile in pair mode
long wino4_workgroups(const ConvArgs &a);
hipError_t launch_wino4_conv(ConvKind kind, const ConvArgs &a, hipStream_t st);

// Three-stage F(4x4,3x3) for the deep fp32 3x3 layers (wino3s_kernels.hip + conv_dma<..., WINO_GEMM> in conv_kernels.hip): the
// products of wino4_conv_f32 on the bf16 matrix cores.  Stage 1 writes V = B^T d B of every 4x4 output tile (tiles numbered over the
// whole batch = GEMM rows) as V[pos 0..35][Cin/8][row][8]; stage 2 is 36 GEMMs M_pos = V_pos U_pos in the three-term bf16 split of
// the transposed convolutions (128 x 128 tiles, six products per term pair, fp32 sums) -> M[pos][Cout/8][row][8]; stage 3 applies
// A^T M A + bias + ReLU (+ 2x2 max-pool) and writes the C8 output.  V and M are 2.25x the layer's input / output: the form pays only
// where images are small and channels many (levels 3 and 4).  U: pack_wino4_split (unet.hip).
struct Wino3sGeom {
    int tilesY, tilesX;        // 4x4 output tiles of one image
    long rows;                 // N * tilesY * tilesX
    size_t v_bytes, m_bytes;   // of V and M
    long gemm_grid;            // workgroups of stage 2 on 128-column tiles: the measure choose_conv3 (unet.hip) compares with its
                               // threshold whatever tile the layer's launch has (a 256-column launch has half as many)
};
// Workgroup tile of stage 2: 128 rows x 128 columns (4 waves, three workgroups per CU), or 128 rows x 256 columns (two workgroups per
// CU; Cout % 256 == 0) with 4 waves of 64 x 128 each or 8 waves of 64 x 64 each.  A wider tile stages 0.8x the bytes per MFMA and has
// half the barriers; an output element sees the same chunks and products in the same order in all three, so the results are
// bit-identical.  U is packed per column tile (pack_wino4_split), so a layer's planes fix its tile width.
enum SplitTile { SPLIT_BN128 = 0, SPLIT_BN256 = 1, SPLIT_BN256W8 = 2 };
inline int split_tile_bn(SplitTile t) { return t == SPLIT_BN128 ? 128 : 256; }
bool wino3s_applicable(ConvKind kind, const ConvArgs &a);
Wino3sGeom wino3s_geom(const ConvArgs &a);
// a.wpk = the U planes packed for `tile`; V, M: wino3s_geom's bytes, 16-byte aligned, disjoint from the layer's tensors
hipError_t launch_wino3s_conv(ConvKind kind, const ConvArgs &a, float *V, float *M, SplitTile tile, hipStream_t st);
// stage 2 alone (conv_kernels.hip)
hipError_t launch_wino_gemm(const float *V, const void *U, float *M, long rows, int Cin, int Cout, SplitTile tile, hipStream_t st);

// fp16 3x3 layers on v_mfma_f32_16x16x32_f16 (conv16_kernels.hip): 32 x 16-pixel tiles x 64 couts, 32-channel chunks (ConvArgs::
// nchunk0 / nchunk count those), persistent workgroups, weights from ConvArgs::wpk in pack_conv16 layout; `resident`: the whole
// weight tensor of a 64 -> 64 layer stays in LDS
bool conv16_applicable(ConvKind kind, const ConvArgs &a);
hipError_t launch_conv16(ConvKind kind, const ConvArgs &a, bool resident, hipStream_t st);

// fp16 transposed convolutions on v_mfma_f32_16x16x32_f16 (convt16_kernels.hip): items of 256 pixels x 256 columns, persistent
// workgroups, 16-byte stores from the accumulators; weights from ConvArgs::wpk in pack_convt16 layout, ConvArgs::bias = the
// layer's Cout biases (plain), N / H / W = the INPUT's
bool convt16_applicable(const ConvArgs &a);
hipError_t launch_convt16(const ConvArgs &a, hipStream_t st);

// First layer: Conv2d(1 -> 64, 3x3, pad 1) + folded BN + ReLU, fp32 input, blocked-layout output.  w9x64: [tap][cout].
hipError_t launch_conv_first(const float *x, const float *w9x64, const float *bias, void *out, bool f16,
                             int N, int H, int W, int Cin, hipStream_t st);
// y[i] = bias + sum over `planes` partial planes of CONV3X3_RELU_DOT (fixed order): the tail of the fused last layer.
hipError_t launch_dot_finish(const float *planes, int nplanes, float bias, float *y, long npix, hipStream_t st);
// Last layer: Conv2d(64 -> 1, 1x1), fp32 output.
hipError_t launch_conv_out(const void *in, bool f16, const float *w64, float bias, float *out, long npix, long HW,
                           long out_stride, hipStream_t st);
// internal blocked layout -> NCHW fp32 (parity-test export only).
hipError_t launch_nhwc_to_nchw(const void *in, bool f16, float *out, int N, int H, int W, int C, hipStream_t st);

hipError_t launch_stft_mag(const float *audio, int n_clips, long L, int n_fft, int hop, int center, long n_frames,
                           float *out, int rows, long row_stride, long clip_stride, int quantize, hipStream_t st);
// Constant tables are built on first use per (device, n_fft) / per device: a blocking hipMalloc + hipMemcpy.  On a stream
// that is being captured nothing may block or allocate: a cold lookup there returns ADN_COLD_IN_CAPTURE (the ABI turns it into
// ADN_ERR_INVALID with a message that names adn_prepare); adn_prepare builds the tables ahead of time.
constexpr hipError_t ADN_COLD_IN_CAPTURE = hipErrorStreamCaptureUnsupported;
bool stream_is_capturing(hipStream_t st);
hipError_t stft_tables(int n_fft, const float **out, hipStream_t st);
hipError_t loss_tables(hipStream_t st);      // mel filterbank of adn_perceptual_loss on the current device
// Griffin-Lim building blocks (gl_kernels.hip); complex spectrograms are frame-major [clip][frame][F] float2
hipError_t launch_gl_polar(const float *mag, const float *rnd, int n_clips, int F, int T, void *spec, hipStream_t st);
hipError_t launch_istft_frames(const void *spec, int n_clips, int T, int n_fft, float *buf, hipStream_t st);
hipError_t launch_istft_ola(const float *buf, int n_clips, int T, int n_fft, int hop, float *audio, hipStream_t st);
hipError_t launch_stft_complex(const float *audio, int n_clips, long L, int n_fft, int hop, int T, void *spec,
                               hipStream_t st);
// Long-form denoising (denoise_kernels.hip).  DenoiseGeom: the window plan of adn.h ("denoise", rule 2) for T frames --
// K windows of Wd frames, S = window - overlap frames apart, V = overlap shared frames; denoise_geom is false outside
// n_frames >= 1, window >= 16, 0 <= overlap <= window / 2.  Windows are bin-major [clip * K + k][F][Wd], X frame-major float2.
struct DenoiseGeom {
    int T, K, Wd, S, V;
};
bool denoise_geom(int n_frames, int window, int overlap, DenoiseGeom *g);
hipError_t launch_denoise_windows(const void *spec, int n_clips, int F, const DenoiseGeom &g, float *out, hipStream_t st);
hipError_t launch_denoise_stitch(const float *y, int n_clips, int F, const DenoiseGeom &g, int clamp, float *out,
                                 hipStream_t st);
hipError_t launch_denoise_resynth(const float *y, const void *spec, int n_clips, long L, int n_fft, int hop,
                                  const DenoiseGeom &g, float *audio, hipStream_t st);
// Spectral baseline (baseline_kernels.hip; adn.h, "baseline").  SpectralConsts: the six parameters and the three constants derived
// from them once per call on the host, in fp32: 1 - smooth, (1 - gamma) / (1 - beta), 1 - alpha.  spec frame-major float2, out
// bin-major [clip][F][width] written at columns [col0, col0 + T), state [clip][3][F] (P, Pmin, S; NULL in = fresh, NULL out = dropped).
struct SpectralConsts {
    float smooth, one_minus_smooth, beta, gamma, growth, alpha, one_minus_alpha, gain_floor, bias;
};
hipError_t launch_spectral_gain(const void *spec, int n_clips, int T, int F, const SpectralConsts &k, const float *state_in,
                                float *state_out, float *out, int width, int col0, hipStream_t st);
// The magnitude form on stream windows (adn.h, "baseline", "The magnitude form"): windows / y bin-major [row * n_steps + s][F][W],
// columns [col0, col0 + n_cols) of every step read and written, state [slot][3][F] in place.  SpectralRows travels by value in the
// kernel arguments as the pool's table does (2 KB of the 4 KB segment): n = 0 means row i is slot i and continues, otherwise
// row i uses row[i].slot and starts fresh when row[i].fresh != 0.
constexpr int SPECTRAL_MAX_ROWS = 256;          // adn.h: ADN_SPECTRAL_MAX_ROWS
struct SpectralRow {
    int slot, fresh;
};
struct SpectralRows {
    int n;
    SpectralRow row[SPECTRAL_MAX_ROWS];
};
hipError_t launch_spectral_gain_windows(const float *windows, float *y, int n_rows, int n_steps, int F, int W, int col0, int n_cols,
                                        const SpectralConsts &k, float *state, const SpectralRows &rows, hipStream_t st);
// Dereverberation (dereverb_mc_kernels.hip, dereverb_kernels.hip; adn.h, "dereverb" and "dereverb multichannel"): I iterations of
// WPE at K taps per channel and delay D on the N = C K stacked past frames of the C consecutive clips of a group, 1 <= C <= 8 and
// C K <= 32, for every (group, bin) of a frame-major float2 spectrogram [group * C + channel][frame][F], in one launch without a
// workspace.  mag_out (may be null) is bin-major [group * C + channel][F][width], columns [0, T) written.  C = 1 is the
// single-channel operator and runs its own kernel; the launcher chooses, callers pass C and never ask.  wpe_grid: the workgroups of
// the launch, n_groups x ceil(F / (256 / lanes per bin)).
struct WpeConsts {
    int K, D, I;
    float loading, rho;
};
long wpe_grid(int n_groups, int C, int F, int K);
hipError_t launch_wpe(const void *spec, int n_groups, int C, int T, int F, const WpeConsts &k, void *spec_out, float *mag_out,
                      int width, hipStream_t st);
// Beamformer (beamform_kernels.hip; adn.h, "beamform"): mask-driven MVDR of the C consecutive clips of a group, 1 <= C <= 8, for every
// (group, bin) of a frame-major float2 spectrogram [group * C + channel][frame][F] and bin-major mask magnitudes
// [group * C + channel][F][mag_width], in one launch without a workspace.  spec_out is [group][frame][F] float2; mag_out (may be
// null) is [group][F][width], columns [0, T) written.  MvdrConsts: the parameters and 1 - mask_floor, derived once per call on the
// host in fp32.  mvdr_grid: the workgroups of the launch, n_groups x ceil(F / (64 / lanes per bin)), 4 lanes up to C = 4, 8 beyond.
struct MvdrConsts {
    int ref;
    float loading, rho, one_minus_rho;
};
long mvdr_grid(int n_groups, int C, int F);
hipError_t launch_mvdr(const void *spec, const float *mag, int mag_width, int n_groups, int C, int T, int F, const MvdrConsts &k,
                       void *spec_out, float *mag_out, int width, hipStream_t st);
// Streaming denoiser (stream_kernels.hip; adn.h, "stream").  StreamGeom: the plan and the layout of the state buffer of one batch
// of streams, in floats (sections X, mag, hist, tail; `total` floats in all); stream_geom is false outside the limits of adn.h.
// StreamCall: what one call of n_steps steps from step `first` covers, derived from the step index alone (stream_call):
// samples [base, end) arrive, frames [f_new0, f_new1) are transformed, frames [f_first, f_last] go back to audio over the
// untrimmed positions [p_begin, p_end), of which [p_first, p_out) are written out and [p_tail, p_tail + n_fft - hop) carried.
struct StreamGeom {
    int n_fft, hop, W, B, A;
    int S, RX, RM;                       // history / tail slots, ring lengths in frames
    long x_off, mag_off, hist_off, tail_off, total;
};
struct StreamCall {
    int first, n_steps, T, L;            // T, L: frames and samples of the finished stream, -1 while it runs
    int base, end, f_new0, f_new1;
    int slot_in, slot_out;
    int f_first, f_last, p_begin, p_first, p_out, p_tail, p_end;
};
// The arithmetic of a StreamCall, for steps first .. first + n_steps - 1 inside the limits the ABI has checked (final_length -1 or
// the stream's length, no step past the last one of a finished stream).  The lockstep entry points evaluate it on the host, the
// pool's kernels per row on the device: one function, so the two cannot drift apart.
__host__ __device__ inline StreamCall stream_call_of(const StreamGeom &g, long first, int n_steps, long final_length)
{
    StreamCall c;
    const long B = g.B, D = g.B + g.A, hop = g.hop, M = g.n_fft / 2, keep = g.n_fft - g.hop;
    const long last = first + n_steps - 1;
    c.first = (int)first;
    c.n_steps = n_steps;
    c.T = -1;
    c.L = -1;
    bool closes = false;
    if (final_length > 0) {
        const long T = 1 + final_length / hop, K = (T + B - 1) / B;
        c.T = (int)T;
        c.L = (int)final_length;
        closes = last == K - 1;
    }
    c.base = first == 0 ? 0 : (int)((first * B + g.A - 1) * hop + M);
    c.end = (int)((last * B + D - 1) * hop + M);
    c.f_new0 = first == 0 ? 0 : (int)(first * B + g.A);
    c.f_new1 = (int)(last * B + D);
    c.slot_in = first == 0 ? 0 : (int)((first - 1) % g.S);
    c.slot_out = (int)(last % g.S);
    c.f_first = (int)(first * B);
    c.f_last = (int)((last + 1) * B - 1);
    c.p_begin = (int)(first * B * hop);
    c.p_first = c.p_begin > M ? c.p_begin : (int)M;
    if (closes) {
        if (c.f_last > c.T - 1) c.f_last = c.T - 1;
        c.p_out = (int)(final_length + M);
        c.p_tail = 0x7fffffff;
        c.p_end = c.p_out;
    } else {
        c.p_out = (int)((last + 1) * B * hop);
        c.p_tail = c.p_out;
        c.p_end = (int)(c.p_out + keep);
    }
    return c;
}
bool stream_geom(int n_streams, int n_fft, int hop, int window, int block, int lookahead, int max_steps, StreamGeom *g);
// Stream pool (adn.h, "stream pool"): n_slots independent streams in one state, each with the geometry of max_steps = 1 (S = 2,
// RX = B + A, RM = W), no hist section and one more section, `ring` [slot][R]: the slot's pending samples, sample s at s mod R.
// A launch covers n rows of (slot, step, final_length); the table travels by value in the kernel arguments (3 KB of the 4 KB
// segment) and a workgroup derives its row's StreamCall with stream_call_of.
constexpr int STREAM_POOL_MAX_ROWS = 256;       // adn.h: ADN_STREAM_POOL_MAX_ROWS
struct StreamPoolRow {
    int slot, step, final_length;
};
struct StreamPoolRows {
    long ring_off;                       // floats from the start of the state
    int R, n;
    StreamPoolRow row[STREAM_POOL_MAX_ROWS];
};
bool stream_pool_geom(int n_slots, int n_fft, int hop, int window, int block, int lookahead, long ring, StreamGeom *g,
                      long *ring_off, long *total);
hipError_t launch_stream_pool_frames(const StreamGeom &g, const StreamPoolRows &rows, int max_new_frames, float *state, hipStream_t st);
hipError_t launch_stream_pool_windows(const float *state, const StreamGeom &g, const StreamPoolRows &rows, float *out, hipStream_t st);
hipError_t launch_stream_pool_emit(const float *y, const StreamGeom &g, const StreamPoolRows &rows, int max_span, float *state,
                                   float *audio, long out_stride, hipStream_t st);
hipError_t launch_stream_frames(const float *audio, long audio_stride, int n_streams, const StreamGeom &g, const StreamCall &c,
                                float *state, hipStream_t st);
hipError_t launch_stream_windows(const float *state, int n_streams, const StreamGeom &g, const StreamCall &c, float *out,
                                 hipStream_t st);
hipError_t launch_stream_emit(const float *y, int n_streams, const StreamGeom &g, const StreamCall &c, float *state, float *audio,
                              long out_stride, hipStream_t st);
// Streaming dereverberation (dereverb_mc_stream_kernels.hip, dereverb_stream_kernels.hip; adn.h, "dereverb stream" and "dereverb
// stream multichannel"): one RLS update per frame on the N = C K stacked past frames of the C consecutive rows of a group,
// 1 <= C <= 8 and C K <= 32, c.K the taps per channel.  C = 1 is the single-channel operator and runs its own kernel; the launcher
// chooses.  WpeStreamConsts: the parameters and the two constants derived from them once per call on the host, in fp32:
// p0 = 1 / loading, 1 - smooth.  wstate: wpe_stream_record_floats(C, K, D) = 2 N^2 + 2 N C + 2 C (D + K) + 2 floats per (slot,
// bin), [slot][bin] consecutive, group i = slot i; a group that starts at frame 0 reads none of it.  The launches differ in where a
// row's frames are: frame-major spectrograms (n_groups * C rows, frames first_frame .. first_frame + T - 1); the X rings of a
// lockstep stream state whose streams g C .. g C + C - 1 are group g (frames f_first .. f_last of `call`, in place, M_t into
// columns [W - B, W) of y); the same for the rows of a pool.  wpe_stream_grid: the workgroups of a launch over n_rows groups.
struct WpeStreamConsts {
    int K, D;
    float alpha, p0, rho, beta, one_minus_beta;
};
long wpe_stream_record_floats(int C, int K, int D);
long wpe_stream_grid(long n_rows, int F);
hipError_t launch_wpe_online(const void *spec, int n_groups, int C, int T, int F, int first_frame, const WpeStreamConsts &c,
                             float *wstate, void *spec_out, float *mag_out, int width, int col0, hipStream_t st);
hipError_t launch_wpe_stream(float *state, float *y, int n_streams, int C, const StreamGeom &g, const StreamCall &call,
                             const WpeStreamConsts &c, float *wstate, hipStream_t st);
// a pool's rows are single-channel streams: C is fixed at 1
hipError_t launch_wpe_stream_pool(float *state, float *y, const StreamGeom &g, const StreamPoolRows &rows, const WpeStreamConsts &c,
                                  float *wstate, hipStream_t st);
// a pool's RECORDINGS: C consecutive rows are the channels of one, their slots r C ... r C + C - 1 in channel order and their steps
// equal (the caller has checked it); wstate slot r.  C = 1 is launch_wpe_stream_pool.
hipError_t launch_wpe_mc_stream_pool(float *state, float *y, int C, const StreamGeom &g, const StreamPoolRows &rows,
                                     const WpeStreamConsts &c, float *wstate, hipStream_t st);
// Streaming beamformer (beamform_stream_kernels.hip; adn.h, "beamform stream"): the recursion of the two covariances of "beamform",
// one update per frame, a filter every R frames, for the C consecutive rows of a group, 1 <= C <= 8.  MvdrStreamConsts: MvdrConsts,
// the refresh period R and the forgetting factor.  state: mvdr_stream_record_floats(C) = 2 (C (C + 1) + C) floats per (slot, bin) --
// both packed triangles and the filter -- entry-major over the bins of a slot, group i = slot i; a group that starts at frame 0
// reads none of it.  The launches differ in where the frames are, as launch_wpe_online / launch_wpe_stream: frame-major spectrograms
// with bin-major mask magnitudes [group * C + channel][F][mag_width] from column mag_col0, the result [group][frame][F] and
// [group][F][width] from col0; or the X rings of a lockstep stream state whose streams g C .. g C + C - 1 are group g, M_t read from
// columns [W - B, W) of every channel's windows of y, Y_t and |Y_t| written in place over stream g C's.
struct MvdrStreamConsts {
    MvdrConsts m;
    int R;
    float alpha;
};
long mvdr_stream_record_floats(int C);
long mvdr_stream_grid(long n_groups, int C, int F);
hipError_t launch_mvdr_online(const void *spec, const float *mag, int mag_width, int mag_col0, int n_groups, int C, int T, int F,
                              int first_frame, const MvdrStreamConsts &k, float *state, void *spec_out, float *mag_out, int width,
                              int col0, hipStream_t st);
hipError_t launch_mvdr_stream(float *sstate, float *y, int n_streams, int C, const StreamGeom &g, const StreamCall &call,
                              const MvdrStreamConsts &k, float *state, hipStream_t st);
// the same for a pool's recordings, as launch_wpe_mc_stream_pool: Y_t and |Y_t| over the first row of each group
hipError_t launch_mvdr_stream_pool(float *sstate, float *y, int C, const StreamGeom &g, const StreamPoolRows &rows,
                                   const MvdrStreamConsts &k, float *state, hipStream_t st);
// Acoustic echo cancellation (echo_stream_kernels.hip; adn_echo.h, "echo stream"): one RLS update per frame from the K delayed far-end
// frames to the microphone, per (pair, bin).  AecConsts: the parameters and p0 = 1 / loading, derived once per call on the host in
// fp32.  astate: aec_record_floats(K, D) = 2 K^2 + 4 K + 2 D floats per (slot, bin) -- P, h and the last D + K far-end frames --
// [slot][bin] consecutive, pair i = slot i; a pair that starts at frame 0 reads none of it.  The launches differ in where the frames
// are: frame-major spectrograms mic / far / spec_out [row][frame][F] (frames first_frame .. first_frame + T - 1); or the X rings of a
// lockstep stream state whose streams 2 g and 2 g + 1 are the microphone and the far end of pair g (frames f_first .. f_last of
// `call`; e_t over stream 2 g's ring cells, M_t into columns [W - B, W) of its windows of y, nothing of stream 2 g + 1 written).
// aec_stream_grid: the workgroups of a launch over n_pairs pairs.
struct AecConsts {
    int K, D;
    float alpha, p0, quiet;
};
long aec_record_floats(int K, int D);
long aec_stream_grid(long n_pairs, int F, int K);
hipError_t launch_aec_online(const void *mic, const void *far, int n_rows, int T, int F, int first_frame, const AecConsts &c, float *astate,
                             void *spec_out, float *mag_out, int width, int col0, hipStream_t st);
hipError_t launch_aec_stream(float *state, float *y, int n_streams, const StreamGeom &g, const StreamCall &call, const AecConsts &c,
                             float *astate, hipStream_t st);
// the same for a pool's CALLS of `mics` microphones that share one far end (adn_call.h): rows = mics + 1 per call, the microphones
// first; pair (call, m) uses operator-state slot (first slot of the call / (mics + 1)) mics + m
hipError_t launch_aec_stream_pool(float *state, float *y, int mics, const StreamGeom &g, const StreamPoolRows &rows, const AecConsts &c,
                                  float *astate, hipStream_t st);
hipError_t launch_quantize_pad(const float *in, int n, int h, int w, float *out, int H, int W, hipStream_t st);
hipError_t launch_per_clip_l1(const float *a, const float *b, int n_clips, long elems, float *out, hipStream_t st);
// Polyphase resampler and SNR mixer (resample_kernels.hip).  resample_ratio: up / down of a rate pair, false outside the limits
// of adn.h.  The coefficient table is built on first use per (device, up, down) like stft_tables (ADN_COLD_IN_CAPTURE applies).
bool resample_ratio(int src_rate, int dst_rate, int *up, int *down);
hipError_t resample_prepare(int up, int down, hipStream_t st);
hipError_t launch_resample(const float *audio, int n_clips, long L, long M, int up, int down, float *out, hipStream_t st);
// The prototype low-pass of adn.h for a reduced rate pair: half = ZEROS max(up, down), and tap h[j], |j| <= half, computed in
// float64 and rounded once to fp32 -- the one function both resampler tables take their coefficients from.
long resample_half(int up, int down);
float resample_tap(long j, int up, int down);
// Resampler inside a stream (stream_resample_kernels.hip; adn.h, "resample stream").  ResampleStreamGeom: the plan of a rate pair
// -- K = floor(half / up), H carried samples per slot, latency in input samples (H = latency = 0 for equal rates, a copy);
// resample_stream_geom is false outside the rate limits of adn_resample.  The state is [stream][2][H] floats.  The coefficient table
// is built on first use per (device, up, down) or by resample_stream_prepare (ADN_COLD_IN_CAPTURE applies).
constexpr long ADN_RESAMPLE_STREAM_MAX_H = 16384;
struct ResampleStreamGeom {
    int up, down, K;
    long half, H, latency;
};
bool resample_stream_geom(int src_rate, int dst_rate, ResampleStreamGeom *g);
long resample_stream_emitted(const ResampleStreamGeom &g, long received, bool final);
hipError_t resample_stream_prepare(const ResampleStreamGeom &g, hipStream_t st);
hipError_t launch_resample_stream(float *state, const float *audio, long audio_stride, int n_streams, const ResampleStreamGeom &g,
                                  long call_index, long received_before, long n_new, bool final, float *out, long out_stride,
                                  hipStream_t st);
// The same kernel over a table of rows that each carry their own stream (adn.h, "stream pool at a rate"): row i is call
// `call_index` of the stream in (slot, direction), its history slots in rate_state, [2 slot + direction][2][max_history] floats,
// its new samples at audio + src_off.  Linear: row i writes at out + i out_stride.  Ring: `out` is the pool state and output m
// goes to word m mod R of the ring of `slot`, out + ring_off + slot R.  One launch; the caller has checked every row.
constexpr int STREAM_POOL_RATE_MAX_ROWS = 64;   // adn.h: ADN_STREAM_POOL_RATE_MAX_ROWS
struct ResampleStreamRow {
    ResampleStreamGeom g;
    int slot, direction;
    long call_index, received_before, n_new, src_off;
    bool final;
};
hipError_t launch_resample_stream_rows(const ResampleStreamRow *rows, int n_rows, const float *audio, float *rate_state,
                                       long max_history, float *out, long out_stride, bool ring, long ring_off, long R, hipStream_t st);
size_t mix_snr_workspace_floats(int n_clips, long L);
hipError_t launch_mix_snr(const float *clean, const float *noise, int n_clips, long L, float inv_snr_linear, float *workspace,
                          float *out, hipStream_t st);
// Freeverb over a batch of clips (reverb_kernels.hip; definition in adn.h).  The scalars arrive as adn.h derives them; the
// delay lines of a clip live in the LDS of its workgroup, which bounds the rate from above, the shortest delay from below.
constexpr int ADN_REVERB_MIN_RATE = 2000, ADN_REVERB_MAX_RATE = 128000;
bool reverb_rate_ok(int sample_rate);
hipError_t launch_reverb(const float *audio, int n_clips, int L, int sample_rate, float feedback, float damp, float wet1, float dry,
                         int clip, float *out, hipStream_t st);
// Quality metrics (quality_kernels.hip; definitions in adn.h, "quality").  `lengths` (device, may be null) is read by the kernels.
// adn_quality: fp64 partial sums per 8192-sample block, six per block.  adn_stoi: StoiPlan lays out the workspace for the row pitch
// L -- nf_max frames and j_max compacted frames per clip at most, wgs workgroups of segments per clip -- in byte offsets.
constexpr int ADN_SEG_FRAME_MIN = 16, ADN_SEG_FRAME_MAX = 8192;
constexpr long ADN_QUALITY_MAX_LENGTH = 1L << 30;
size_t quality_workspace_bytes(int n_clips, long L);
hipError_t launch_quality(const float *est, const float *ref, const long *lengths, int n_clips, long L, int seg_frame,
                          void *workspace, float *out, hipStream_t st);
struct StoiPlan {
    long nf_max, j_max;
    int wgs;
    size_t norm_off, idx_off, kept_off, env_off, rho_off, total;
};
StoiPlan stoi_plan(int n_clips, long L);
hipError_t launch_stoi(const float *est, const float *ref, const long *lengths, int n_clips, long L, void *workspace, float *out,
                       hipStream_t st);
size_t perceptual_loss_workspace_floats(int n_clips, int F, int T);
// LDS the finishing kernel needs for T frames (ADN_LOSS_MAX_LDS: 160 KiB per CU minus the kernel's static reduction scratch):
// up to ADN_LOSS_LDS_T frames a clip's series and mel spectra are held on chip, longer clips keep the series in the workspace
size_t perceptual_loss_lds_bytes(int T);
constexpr size_t ADN_LOSS_MAX_LDS = 160 * 1024 - 64;
constexpr int ADN_LOSS_LDS_T = 6784;
constexpr int ADN_LOSS_MAX_T = 1 << 24;     // (partial sums and frame indices are 32-bit)
constexpr int ADN_LOSS_MIN_T = 32;          // loss.py:39-41: the mel transform's reflect padding (31 samples) needs T > 31
hipError_t launch_perceptual_loss(const float *pred, const float *tgt, int n_clips, int F, int T, float *workspace,
                                  float *out, hipStream_t st);
// Backward of launch_perceptual_loss: grad_out (n_clips, 4) -> grad_pred / grad_tgt (either may be null), written.
size_t perceptual_loss_backward_workspace_floats(int n_clips, int F, int T);
hipError_t launch_perceptual_loss_backward(const float *pred, const float *tgt, int n_clips, int F, int T, const float *grad_out,
                                           float *workspace, float *grad_pred, float *grad_tgt, hipStream_t st);

}  // namespace adn
