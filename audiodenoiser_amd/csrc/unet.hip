// The U-Net behind the adn_unet_* entry points of include/adn.h: the layer table, BatchNorm folding + weight packing, workspace
// planning, the choice of kernel per layer and the launch sequence of the forward (reference /root/reference/code/model.py:70-94).
#include "adn_host.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

using adn::aligned_to;
using adn::DeviceGuard;
using adn::fail;
using adn::fail_hip;

namespace {

constexpr float BN_EPS = 1e-5f;   // nn.BatchNorm2d default (reference model.py:12,15)
constexpr int CH[5] = {64, 128, 256, 512, 1024};   // channels of the DoubleConv at level 0 .. 4 (level l: F >> l x T >> l pixels)

// The 21 matrix-core layers of the network in execution order (= state_dict order): the 17 3x3 convolutions and the 4 transposed
// convolutions.  Conv2d(in_channels -> 64), the first half of down1, and the 1x1 output convolution have kernels of their own.
// Weight packing, the workspace plan and the forward all walk this table.
enum LayerKind { CONV3, CONVT };
struct LayerDesc {
    LayerKind kind;
    int level;     // level of the tile domain: the OUTPUT of a 3x3 layer, the INPUT of a transposed convolution (ConvArgs::N/H/W)
    int C0, C1;    // input channels from source 0 / source 1 (up path: the virtual cat([skip, upsampled]), model.py:44-49)
    int Cout;
};
constexpr int N_CONV3 = 17, N_CONVT = 4, N_LAYERS = N_CONV3 + N_CONVT;
struct LayerTable {
    LayerDesc v[N_LAYERS];
    int n;
};
constexpr LayerTable make_layers()
{
    LayerTable t{};
    for (int l = 0; l <= 4; ++l) {                       // down1 .. down4 and the bottleneck (model.py:72-81): DoubleConv at level l
        if (l > 0) t.v[t.n++] = LayerDesc{CONV3, l, CH[l - 1], 0, CH[l]};
        t.v[t.n++] = LayerDesc{CONV3, l, CH[l], 0, CH[l]};
    }
    for (int l = 3; l >= 0; --l) {                       // up1 .. up4 (model.py:84-91): convT from level l + 1, DoubleConv at level l
        t.v[t.n++] = LayerDesc{CONVT, l + 1, CH[l + 1], 0, CH[l]};
        t.v[t.n++] = LayerDesc{CONV3, l, CH[l], CH[l], CH[l]};
        t.v[t.n++] = LayerDesc{CONV3, l, CH[l], 0, CH[l]};
    }
    return t;
}
constexpr LayerTable NET = make_layers();
static_assert(NET.n == N_LAYERS && NET.v[0].Cout == 64 && NET.v[8].C0 == 1024 && NET.v[9].kind == CONVT && NET.v[N_LAYERS - 1].Cout == 64,
              "layer table: 9 layers down to the bottleneck, then 4 x (convT, conv, conv)");
// state_dict walk (adn.h): 6 tensors per conv + BatchNorm (the first convolution included), 2 per transposed / output convolution
static_assert(6 * (1 + N_CONV3) + 2 * N_CONVT + 2 == ADN_N_WEIGHT_TENSORS, "layer table does not match the weight tensor list");
static_assert(1 + N_LAYERS + 1 == ADN_N_LAUNCHES, "layer table does not match the timing slots");

// Where the packed forms of a layer's weights sit: float offsets into the device buffer, 0 = form not packed.
struct LayerWeights {
    size_t w_off, b_off;   // the form the path's own kernel reads, and the bias per GEMM column
    size_t w4_off;         // 3x3, fp32 Winograd path: F(4x4,3x3) pack of the same weights
    size_t w3_off;         // 3x3 at levels 3 and 4 from 512 input channels on, fp32 Winograd path: U as three bf16 planes (pack_wino4_split)
    adn::SplitTile w3_tile;  // ... packed once, for this workgroup tile of the GEMM stage (split_tile); transposed convolutions: of wt_off
    size_t w16_off;        // fp16 path: pack_conv16 / pack_convt16 form (16x16x32 MFMA kernels)
    size_t braw_off;       // transposed convolution: the Cout biases as they are (convt16_f16; the K-split reduce launch)
    size_t wt_off;         // fp32 split-bf16 transposed convolution on a 256-column tile (w3_tile): the planes packed for it, beside
                           // the 128-column planes at w_off that its K-split launches at small batches keep reading (17 MB in all)
};

}  // namespace

struct adn_unet {
    int device = 0;
    float *dev = nullptr;          // all packed weights
    size_t dev_floats = 0;
    size_t first_w = 0, first_b = 0;       // Conv2d(1->64): [9][64] + bias[64]
    LayerWeights lw[N_LAYERS] = {};        // one per entry of NET
    size_t out_w = 0;               // Conv2d(64 -> num_classes, 1x1): [class][64]
    size_t zero_off = 0;            // 2048 zero floats
    float out_b = 0.f;              // bias of class 0 (the fused 1x1 tails handle one class)
    std::vector<float> out_bias;    // all classes
    int in_ch = 1, n_classes = 1;   // UNet(in_channels, num_classes) (model.py:54); the reference's callers use (1, 1)
    // optional per-launch timing (adn_unet_set_timing)
    std::vector<hipEvent_t> events;
    int timing_max = 0, timing_count = 0;
    bool f16 = false;              // fp16 storage + fp16 MFMA (fp32 accumulate); x and y stay fp32 at the ABI
    bool use_wino = true;          // fp32 3x3 layers: Winograd F(2x2,3x3) kernel (false: direct implicit GEMM)
    // F(4x4,3x3) kernel where its 32x32 tiles fit the layer (ADN_WINO_TILE when the handle is created: 2 = F(2x2,3x3) for
    // every layer, 4 = F(4x4,3x3) for every plain / pooled 3x3 layer whatever its size)
    bool use_wino4 = true, force_wino4 = false;
    // split-K for layers that cannot fill the chip at small batch (ADN_WINO_SPLITK=1 when the handle is created).
    // Off by default: it changes the summation order, and the default path keeps a clip's result bit-identical
    // whatever batch it is computed in.
    bool allow_split = false;
    // fp32 transposed convolutions on the bf16 matrix cores through a three-term split of both operands (six products, fp32
    // accumulation; conv_dma<..., SPLIT>): the accuracy of an fp32 accumulation chain -- twelve roundings per 16 channels against the
    // exact-fp32 MFMA's sixteen, a block with them within 1.1 x of its fp32 floor (profiles/f32_blocks.md) -- at 3/8 of the exact-fp32
    // matrix time.  ADN_CONVT_SPLIT=0 when the handle is created keeps the exact-fp32 MFMA form.
    bool convt_split = true;
    // Small grids (one or a few clips): a 3x3 layer whose F(4x4,3x3) launch would be fewer than `auto_grid` workgroups (2 per CU)
    // runs on the finer-grained F(2x2,3x3) kernel instead, cut along K where even that grid cannot fill the chip
    // (choose_conv3 below).  The choice then depends on the batch size, so the same clip computed alone or inside a large batch
    // differs in the last bits (both within 1e-4 of the reference).  ADN_BATCH_INVARIANT=1 when the handle is created pins one
    // kernel per layer by geometry alone: a clip's result is bit-identical whatever batch it is computed in.
    // fp16 path, 3x3 layers: 0 = conv_dma<_Float16> (32x32x16 MFMA, rounds 1-3) everywhere, 1 = conv16_f16 (16x16x32 MFMA,
    // persistent, LDS-resident weights for the 64 -> 64 layers) wherever it applies = the default (ADN_F16_CONV=32 / 16)
    int f16_conv = 1;
    int f16_convt = 1;             // fp16 transposed convolutions: 1 = convt16_f16 (16x16x32 MFMA, persistent; default), 0 = conv_dma<_Float16>
                                   // (ADN_F16_CONVT=dma when the handle is created)
    bool f16_fuse_first = true;    // ADN_F16_FIRST=0: Conv2d(1 -> 64) as its own launch (conv_first_kernel) on the fp16 path (A/B runs)
    bool batch_invariant = false;
    // thresholds of the rule, in F(4x4,3x3) workgroups of the launch, calibrated on per-launch timings at batch 1-16
    // (tools/small_grid_probe.py, profiles/r04_small_grid_probe.txt): F(2x2,3x3) + split-K wins by 20-70 % up to 128
    // workgroups, is level at 160 and loses by 25-50 % from 240 on; the 64-channel full-resolution layers (8-chunk K loops,
    // where the prologue and epilogue of the 32x32-tile kernel weigh most, and down1 can take the first convolution in) switch at 512
    long auto_grid = 192, auto_grid64 = 512;
    // Deep fp32 3x3 layers (levels 3 and 4) as three launches -- input transform, 36 split-bf16 GEMMs, output transform
    // (wino3s_kernels.hip): 0 = never, 1 = where its V and M fit the workspace and the GEMM launch is at least `gemm_grid`
    // workgroups, or the handle is pinned (choose_conv3), 2 = wherever they fit (tests).  ADN_WINO_GEMM when the handle is created.
    // gemm_grid: two rounds of three workgroups per CU (batch 11 of 513x256 at level 3, 21 at level 4).  Measured per layer at batch
    // 4 ... 32 (profiles/wino_gemm_ab.md) the form also wins from 576 workgroups on; the whole suite has only been run with 1536.
    // The threshold counts 128-column workgroups whatever tile a layer runs (Wino3sGeom::gemm_grid): a 256-column launch of the
    // same layer has half as many at two per CU, i.e. 768 of its own = one and a half of its rounds.  Two of its rounds (1 024)
    // would move the first batch of 513x256 that takes the form from 11 to 15 at level 3 and from 21 to 29 at level 4; the set of
    // batches that take the form does not depend on the tile.
    int wino_gemm = 1;
    long gemm_grid = 1536;
    // Workgroup tile of the GEMM stage (ADN_SPLIT_BN when the handle is created): -1 = per layer by measurement (split_tile below),
    // else an adn::SplitTile for every layer whose Cout % 256 == 0.
    int split_bn = -1;
    // A transposed convolution keeps both packings (LayerWeights::wt_off), so its tile is chosen per launch: 256 columns from two
    // rounds of two workgroups per CU on (1 024 of them = 2 048 of the 128-column launch), below that 128 columns -- a small grid
    // of tiles twice as large leaves CUs idle (pinned handle, one clip of 513x256: 1.46 -> 1.55 ms per forward with wide tiles
    // everywhere).
    long convt_wide_grid = 2048;
};

namespace {

// Fold eval-mode BatchNorm into the convolution in front of it:
//   BN(conv(x)) = scale * (W*x + b - mean) + beta,  scale = gamma / sqrt(var + eps)
void bn_fold(const float *b, const float *gamma, const float *beta, const float *mean, const float *var, int C,
             std::vector<float> &scale, std::vector<float> &bias)
{
    scale.resize(C);
    bias.resize(C);
    for (int c = 0; c < C; ++c) {
        const float s = gamma[c] / std::sqrt(var[c] + BN_EPS);
        scale[c] = s;
        bias[c] = (b[c] - mean[c]) * s + beta[c];
    }
}

// Packed layout consumed by conv_mfma<T> (conv_kernels.hip): [column tile][chunk][tap][kgroup][half][n][EPV]
// where EPV = elements per 16 bytes (4 floats / 8 halfs) and element kk of (kgroup s, half h) is input channel
// chunk*KC + 2*EPV*s + EPV*h + kk.
template <typename T>
void pack_conv3x3(const float *w /*(Cout,Cin,3,3)*/, const std::vector<float> &scale, int Cin, int Cout, T *dst)
{
    constexpr int EPV = 16 / sizeof(T);
    const adn::ConvGeom g = adn::conv_geom(adn::CONV3X3_RELU, Cout, sizeof(T) == 2);
    const int BN = g.BN, KC = g.KC, KG = KC / (2 * EPV);
    const int nct = Cout / BN, nchunk = Cin / KC;
    size_t o = 0;
    for (int ct = 0; ct < nct; ++ct)
        for (int ch = 0; ch < nchunk; ++ch)
            for (int tap = 0; tap < 9; ++tap)
                for (int s = 0; s < KG; ++s)
                    for (int h = 0; h < 2; ++h)
                        for (int n = 0; n < BN; ++n) {
                            const int co = ct * BN + n;
                            for (int kk = 0; kk < EPV; ++kk) {
                                const int ci = ch * KC + 2 * EPV * s + EPV * h + kk;
                                dst[o++] = (T)(w[((size_t)co * Cin + ci) * 9 + tap] * scale[co]);
                            }
                        }
}

// fp16 weights for conv16_f16 (conv16_kernels.hip): [cout tile of 64][chunk of 32 channels][tap][cout block j of 16][k group g]
// [cout % 16][8 halfs], input channel = chunk*32 + 8g + e: the W fragment of (tap, j) is 64 lanes x 16 bytes = 1 KB contiguous,
// lane = 16 g + cout % 16.  BatchNorm scale folded.
void pack_conv16(const float *w /*(Cout,Cin,3,3)*/, const std::vector<float> &scale, int Cin, int Cout, _Float16 *dst)
{
    const int nchunk = Cin / 32;
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci) {
            const int ct = co / 64, j = (co % 64) / 16, c16 = co % 16, ch = ci / 32, g = (ci % 32) / 8, e = ci % 8;
            for (int tap = 0; tap < 9; ++tap)
                dst[(((((size_t)ct * nchunk + ch) * 9 + tap) * 4 + j) * 64 + g * 16 + c16) * 8 + e] =
                    (_Float16)(w[((size_t)co * Cin + ci) * 9 + tap] * scale[co]);
        }
}

// Winograd F(2x2,3x3) weights U = G g G^T (double precision, BatchNorm scale folded), packed for wino_conv_f32:
// [column tile of 64][chunk of 8 channels][pos = 4*xi+nu][q][n][e] with input channel = chunk*8 + 2q + e.
void pack_wino3x3(const float *w /*(Cout,Cin,3,3)*/, const std::vector<float> &scale, int Cin, int Cout, int BN,
                  float *dst)
{
    static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    const int nct = Cout / BN, nchunk = Cin / 8;
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci) {
            const float *g = w + ((size_t)co * Cin + ci) * 9;
            double tmp[4][3], U[4][4];
            for (int x = 0; x < 4; ++x)
                for (int b = 0; b < 3; ++b)
                    tmp[x][b] = G[x][0] * g[0 * 3 + b] + G[x][1] * g[1 * 3 + b] + G[x][2] * g[2 * 3 + b];
            for (int x = 0; x < 4; ++x)
                for (int v = 0; v < 4; ++v)
                    U[x][v] = (tmp[x][0] * G[v][0] + tmp[x][1] * G[v][1] + tmp[x][2] * G[v][2]) * (double)scale[co];
            const int ct = co / BN, n = co % BN, ch = ci / 8, q = (ci % 8) / 2, e = ci & 1;
            float *blk = dst + ((size_t)ct * nchunk + ch) * (16 * 4 * BN * 2);
            // slab layout [pos/2][j = n/16][q][n%16][pos%2][e]: a wave's B-fragment read of one (position pair, cout
            // block) is 64 lanes x 16 bytes = 1 KB contiguous -> one conflict-free ds_read_b128 (BN = 32)
            for (int pos = 0; pos < 16; ++pos)
                blk[(((((pos >> 1) * (BN / 16) + n / 16) * 4 + q) * 16) + (n % 16)) * 4 + (pos & 1) * 2 + e] =
                    (float)U[pos >> 2][pos & 3];
        }
    (void)nct;
}

// Winograd F(4x4,3x3): U = G g G^T (6x6, points 0, +-1, +-2, inf) of one 3x3 filter with the BatchNorm scale of its output channel
// folded in, U[6 x + v]; double arithmetic, rounded once to fp32.  Both packers below take the layer's weights from here.
void wino4_u(const float *g /*3x3*/, float scale, float (&U)[36])
{
    static const double G[6][3] = {{1.0 / 4, 0, 0},           {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                   {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
    double tmp[6][3];
    for (int x = 0; x < 6; ++x)
        for (int b = 0; b < 3; ++b)
            tmp[x][b] = G[x][0] * g[0 * 3 + b] + G[x][1] * g[1 * 3 + b] + G[x][2] * g[2 * 3 + b];
    for (int x = 0; x < 6; ++x)
        for (int v = 0; v < 6; ++v)
            U[6 * x + v] = (float)((tmp[x][0] * G[v][0] + tmp[x][1] * G[v][1] + tmp[x][2] * G[v][2]) * (double)scale);
}

// U packed for wino4_conv_f32: [column tile of 32][chunk of 8 channels][jh][group g][pass h][q][cout%16][k] with input channel
// = chunk*8 + 2q + h.  A wave owns the positions (row i, column j) of U with j / 3 = jh, numbered p = 3i + j%3; float k of
// group g is position p = 2g + k/2 for cout block (k & 1) ^ jh (block 0 of a wave is the one it finishes, = jh): a wave's
// B-fragment read of one group and pass is 64 lanes x 16 bytes = 1 KB contiguous.
void pack_wino4_3x3(const float *w /*(Cout,Cin,3,3)*/, const std::vector<float> &scale, int Cin, int Cout, float *dst)
{
    const int nchunk = Cin / 8;
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci) {
            float U[36];
            wino4_u(w + ((size_t)co * Cin + ci) * 9, scale[co], U);
            const int ct = co / 32, cb = (co % 32) / 16, n16 = co % 16, ch = ci / 8, q = (ci % 8) / 2, h = ci & 1;
            float *blk = dst + ((size_t)ct * nchunk + ch) * (36 * 8 * 32);
            for (int x = 0; x < 6; ++x)
                for (int v = 0; v < 6; ++v) {
                    const int jh = v / 3, pp = 3 * x + v % 3, grp = pp >> 1, k = ((pp & 1) << 1) | (cb ^ jh);
                    blk[(((((jh * 9 + grp) * 2 + h) * 4 + q) * 16) + n16) * 4 + k] = U[6 * x + v];
                }
        }
}

// ConvTranspose2d(k2,s2) as a GEMM with columns (sub-pixel, output channel) in convt_column order (adn_internal.h), K = Cin.
template <typename T>
void pack_convt(const float *w /*(Cin,Cout,2,2)*/, int Cin, int Cout, T *dst)
{
    constexpr int EPV = 16 / sizeof(T);
    const adn::ConvGeom g = adn::conv_geom(adn::CONVT2X2, Cout, sizeof(T) == 2);
    const int BN = g.BN, KC = g.KC, KG = KC / (2 * EPV);
    const int ncol = 4 * Cout, nct = ncol / BN, nchunk = Cin / KC;
    size_t o = 0;
    for (int ct = 0; ct < nct; ++ct)
        for (int ch = 0; ch < nchunk; ++ch)
            for (int s = 0; s < KG; ++s)
                for (int h = 0; h < 2; ++h)
                    for (int n = 0; n < BN; ++n) {
                        const int col = ct * BN + n;
                        int ij, co;
                        adn::convt_column(col, Cout, ij, co);
                        for (int kk = 0; kk < EPV; ++kk) {
                            const int ci = ch * KC + 2 * EPV * s + EPV * h + kk;
                            dst[o++] = (T)w[((size_t)ci * Cout + co) * 4 + ij];
                        }
                    }
}

// fp16 weights for convt16_f16 (convt16_kernels.hip): GEMM columns come in PAIRS of 16-column blocks -- the same 16 output channels
// at dj = 0 and dj = 1 --, pair P = di * (Cout / 16) + (16-channel group), eight pairs (256 columns) per column tile:
// [column tile][chunk of 32 channels][column block cb = 2 * (pair % 8) + dj][k group g][column % 16][8 halfs], input channel =
// chunk*32 + 8g + e: the W fragment of a column block is 64 lanes x 16 bytes = 1 KB contiguous, lane = 16 g + column % 16.
void pack_convt16(const float *w /*(Cin,Cout,2,2)*/, int Cin, int Cout, _Float16 *dst)
{
    const int nchunk = Cin / 32, npair = Cout / 16, nct = Cout / 64;
    for (int ct = 0; ct < nct; ++ct)
        for (int ch = 0; ch < nchunk; ++ch)
            for (int cb = 0; cb < 16; ++cb) {
                const int P = ct * 8 + (cb >> 1), dj = cb & 1, di = P / npair, cg = P % npair;
                for (int g = 0; g < 4; ++g)
                    for (int c16 = 0; c16 < 16; ++c16)
                        for (int e = 0; e < 8; ++e) {
                            const int ci = ch * 32 + 8 * g + e, co = cg * 16 + c16;
                            dst[(((((size_t)ct * nchunk + ch) * 16 + cb) * 4 + g) * 16 + c16) * 8 + e] =
                                (_Float16)w[(((size_t)ci * Cout + co) * 2 + di) * 2 + dj];
                        }
            }
}

// The same GEMM for the split-bf16 form of conv_dma (fp32 path; conv_kernels.hip, SPLIT): every weight is written as three bf16
// terms w = hi + mid + lo (round-to-nearest-even each, 24 mantissa bits in all), one plane per term:
// [column tile][chunk of 16 channels][plane][half h][column n][8 bf16], element kk of half h = input channel chunk*16 + 8h + kk.
inline uint16_t bf16_rne(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline float bf16_to_float(uint16_t b)
{
    const uint32_t u = (uint32_t)b << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
// x = hi + mid + lo in bf16, round-to-nearest each; a finite x in the top 0.2 % of fp32's range rounds to a bf16 infinity: largest
// finite bf16 instead (split3_bf16 in adn_internal.h clamps the activations the same way); the residuals stay finite
inline void split3_host(float v, uint16_t (&t)[3])
{
    uint16_t hi = bf16_rne(v);
    if ((hi & 0x7fffu) == 0x7f80u && std::isfinite(v)) hi = (uint16_t)((hi & 0x8000u) | 0x7f7fu);
    const float r1 = v - bf16_to_float(hi);
    const uint16_t mid = bf16_rne(r1);
    const float r2 = r1 - bf16_to_float(mid);
    t[0] = hi;
    t[1] = mid;
    t[2] = bf16_rne(r2);
}

// U for the three-stage form (wino3s_kernels.hip): the fp32 values of wino4_u split into three bf16 planes and packed per
// transform-domain position as the GEMM slabs of conv_dma<..., SPLIT, WINO_GEMM>: [pos = 6x + v][column tile of BN couts][chunk of
// 16 channels][plane][half h][cout n][8 bf16], element kk of half h = input channel chunk*16 + 8h + kk.  BN = 128 or 256: the
// columns of the workgroup tile the layer's GEMM launches run (adn::SplitTile).
void pack_wino4_split(const float *w /*(Cout,Cin,3,3)*/, const std::vector<float> &scale, int Cin, int Cout, int BN, uint16_t *dst)
{
    const int nct = Cout / BN, nchunk = Cin / 16;
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci) {
            float U[36];
            wino4_u(w + ((size_t)co * Cin + ci) * 9, scale[co], U);
            const int ct = co / BN, n = co % BN, ch = ci / 16, hh = (ci % 16) / 8, kk = ci % 8;
            for (int pos = 0; pos < 36; ++pos) {
                uint16_t t[3];
                split3_host(U[pos], t);
                uint16_t *slab = dst + (((size_t)pos * nct + ct) * nchunk + ch) * ((size_t)3 * 2 * BN * 8);
                for (int plane = 0; plane < 3; ++plane) slab[((plane * 2 + hh) * BN + n) * 8 + kk] = t[plane];
            }
        }
}

void pack_convt_split(const float *w /*(Cin,Cout,2,2)*/, int Cin, int Cout, int BN /*columns of the workgroup tile: 128 | 256*/, uint16_t *dst)
{
    const int KC = 16;
    const int ncol = 4 * Cout, nct = ncol / BN, nchunk = Cin / KC;
    size_t o = 0;
    for (int ct = 0; ct < nct; ++ct)
        for (int ch = 0; ch < nchunk; ++ch)
            for (int plane = 0; plane < 3; ++plane)
                for (int h = 0; h < 2; ++h)
                    for (int n = 0; n < BN; ++n) {
                        int ij, co;
                        adn::convt_column(ct * BN + n, Cout, ij, co);
                        for (int kk = 0; kk < 8; ++kk) {
                            const int ci = ch * KC + 8 * h + kk;
                            uint16_t t[3];
                            split3_host(w[((size_t)ci * Cout + co) * 4 + ij], t);
                            dst[o++] = t[plane];
                        }
                    }
}

// ---- geometry, workspace plan --------------------------------------------------------------------------------------------------

// A layer on an N x H x W tile domain without its buffers: sizes, channel split, K chunks and the tile grid of the path's own
// kernel (F(2x2,3x3) for the 3x3 layers of the fp32 Winograd path, the direct kernels' otherwise).  Everything the workspace plan
// and the kernel choice ask about; conv_args / convt_args add the pointers.
adn::ConvArgs geom_args(const LayerDesc &d, bool f16, bool wino, int N, int H, int W)
{
    const adn::ConvKind kind = d.kind == CONVT ? adn::CONVT2X2 : adn::CONV3X3_RELU;   // (a 3x3 epilogue changes neither tiles nor chunks)
    adn::ConvArgs a{};
    a.s0.C = d.C0;
    a.s1.C = d.C1;
    a.N = N;
    a.H = H;
    a.W = W;
    a.Cout = d.Cout;
    a.ksplit = 1;
    const int kc = adn::conv_geom(kind, d.Cout, f16).KC;       // (8 channels for every fp32 3x3 kernel, the Winograd ones included)
    a.nchunk0 = d.C0 / kc;
    a.nchunk = (d.C0 + d.C1) / kc;
    if (wino && d.kind == CONV3) adn::wino_tiles(a);
    else adn::conv_mfma_tiles(kind, f16, a);
    return a;
}

struct Plan {
    int N, H[5], W[5];
    size_t tA, tB, skip[4], pool[4], part, total;   // BYTE offsets into the workspace (part: split-K partial sums)
    size_t part_bytes;                              // capacity of `part`, the last region: what a K-split launch may write
};

bool make_plan(int N, int F, int T, bool f16, Plan &p)
{
    // F*T < 2^27: ONE 8-channel block of a full-resolution fp32 image (F*T*32 bytes) stays below 4 GB, the range of a buffer
    // descriptor -- the copy kernels walk an image block by block with a rebased descriptor, so the image itself (32 GB of fp32 at
    // that size) may exceed it.  No other limit: the reference's network is fully convolutional (model.py:70-94), any F, T >= 16.
    if (N < 1 || F < 16 || T < 16 || (long)F * T >= (1L << 27)) return false;
    p.N = N;
    p.H[0] = F;
    p.W[0] = T;
    for (int l = 1; l < 5; ++l) {
        p.H[l] = p.H[l - 1] / 2;
        p.W[l] = p.W[l - 1] / 2;
    }
    const size_t es = f16 ? 2 : 4;
    size_t o = 0;
    auto take = [&](size_t n) {
        const size_t at = o;
        o += (n * es + 255) & ~size_t(255);   // 256-byte granules
        return at;
    };
    const size_t full = (size_t)N * p.H[0] * p.W[0] * 64;
    p.tA = take(full);
    p.tB = take(full);
    for (int l = 0; l < 4; ++l) {
        p.skip[l] = take((size_t)N * p.H[l] * p.W[l] * CH[l]);
        p.pool[l] = take((size_t)N * p.H[l + 1] * p.W[l + 1] * CH[l]);
    }
    // K-split partial sums (small batches only): the largest ksplit * output floats over the layers, whatever kernel a handle of
    // this dtype may choose -- the same rules on the same grids as choose_conv3 / choose_convt, without a handle's switches
    p.part = o;
    size_t need = 0;
    for (const LayerDesc &d : NET.v) {
        const int H = p.H[d.level], W = p.W[d.level];
        const adn::ConvArgs a = geom_args(d, f16, !f16, N, H, W);
        size_t outf = (size_t)N * H * W * d.Cout;
        int ks = 1;
        if (d.kind == CONVT) {
            outf *= 4;
            if (!f16) ks = adn::convt_ksplit(adn::conv_workgroups(a), a.nchunk, outf);
        } else if (f16) {
            ks = adn::conv16_ksplit(adn::conv_workgroups(a), a.nchunk, outf);
        } else {
            // (no sources in `a`: pair mode is granted to every image at most 16 pixels wide -- the smallest F(4x4,3x3) grid, the
            // largest split, a forward may see)
            ks = std::max(adn::wino_ksplit(adn::conv_workgroups(a), a.nchunk), adn::wino4_ksplit(adn::wino4_workgroups(a), a.nchunk));
        }
        if (ks > 1) need = std::max(need, (size_t)ks * outf);
    }
    p.part_bytes = (need * 4 + 255) & ~size_t(255);
    o += p.part_bytes;
    p.total = o;
    return true;
}

// Layer i of NET with its buffers: in0 (+ in1 of H1 x W1 pixels, zero-padded to the output domain) -> out (+ pool).
adn::ConvArgs conv_args(const adn_unet *h, const Plan &p, int i, const void *in0, const void *in1, int H1, int W1, void *out, void *pool)
{
    const LayerDesc &d = NET.v[i];
    const LayerWeights &L = h->lw[i];
    const int H = p.H[d.level], W = p.W[d.level];
    adn::ConvArgs a = geom_args(d, h->f16, h->use_wino, p.N, H, W);
    a.s0 = adn::ConvSrc{in0, H, W, d.C0, 0, 0};
    if (in1) {
        const int dy = H - H1, dx = W - W1;   // F.pad(x1, [dx//2, dx-dx//2, dy//2, dy-dy//2]) (model.py:44-47)
        a.s1 = adn::ConvSrc{in1, H1, W1, d.C1, dy / 2, dx / 2};
    } else {
        a.s1 = adn::ConvSrc{in0, 0, 0, 0, 0, 0};
    }
    a.wpk = h->dev + L.w_off;
    a.wpk4 = (h->use_wino && h->use_wino4 && L.w4_off) ? h->dev + L.w4_off : (h->f16 && L.w16_off) ? h->dev + L.w16_off : nullptr;
    a.bias = h->dev + L.b_off;
    a.out = out;
    a.pool = pool;
    return a;
}

// Transposed convolution i of NET: in (level d.level) -> out (twice the size)
adn::ConvArgs convt_args(const adn_unet *h, const Plan &p, int i, const void *in, void *out)
{
    const LayerDesc &d = NET.v[i];
    const int H = p.H[d.level], W = p.W[d.level];
    adn::ConvArgs a = geom_args(d, h->f16, false, p.N, H, W);
    a.s0 = adn::ConvSrc{in, H, W, d.C0, 0, 0};
    a.s1 = adn::ConvSrc{in, 0, 0, 0, 0, 0};
    a.wpk = h->dev + h->lw[i].w_off;
    a.bias = h->dev + h->lw[i].b_off;
    a.out = out;
    a.split = h->convt_split ? 1 : 0;
    return a;
}

// ---- which kernel runs a layer -------------------------------------------------------------------------------------------------

enum Conv3Kernel {
    DIRECT,    // conv_mfma<float> / conv_dma<_Float16> (conv_kernels.hip)
    CONV16,    // fp16: conv16_f16
    WINO2,     // fp32: F(2x2,3x3), wino_conv_dma_f32
    WINO4,     // fp32: F(4x4,3x3), wino4_conv_f32
    WINO3S     // fp32, levels 3 and 4: F(4x4,3x3) in three launches with the products on the bf16 matrix cores (wino3s_kernels.hip)
};
// What the three-stage form needs beside the layer's arguments: its U planes and room for V and M.  The ping-pong buffers are
// sized for the 64-channel full-resolution tensors; at levels 3 and 4 a tensor fills at most an eighth of one, so V lives behind
// the layer's tensors in the first buffer and M in the second (forward_impl).  U == nullptr: the layer has no such form.
struct WinoScratch {
    const void *U = nullptr;
    adn::SplitTile tile = adn::SPLIT_BN128;      // the workgroup tile U is packed for
    float *V = nullptr, *M = nullptr;
    size_t v_bytes = 0, m_bytes = 0;
};
struct Conv3Choice {
    Conv3Kernel kernel;
    int ksplit;         // > 1: K-split slices of that kernel (fp16: conv_dma<_Float16>) into the partial buffer + a reduce launch
    bool fuse_first;    // Conv2d(1 -> 64) is computed inside this launch (down1's second conv): no launch of its own
    bool fuse_out;      // the 1x1 output convolution is contracted in this launch's epilogue (CONV3X3_RELU_DOT)
};

// The kernel of a 3x3 layer from the handle's switches and the layer's arguments (conv_args: `a` is the plain layer, no fused form
// entered yet -- the fused forms add pointers, never geometry, so applicability is asked about the plain layer).
// first: down1's second conv of a one-plane network, which may take Conv2d(1 -> 64) in;  tail: the network's last 3x3 layer where
// the 1x1 output convolution may be fused behind it (one class, no block outputs exported: the up4 tap IS the tensor between them).
Conv3Choice choose_conv3(const adn_unet *h, adn::ConvKind kind, const adn::ConvArgs &a, bool first = false, bool tail = false,
                         const WinoScratch &sc = WinoScratch())
{
    Conv3Choice c{DIRECT, 1, false, false};
    if (h->f16) {
        // fp16 path: conv16_f16 on every layer it applies to (all but the two with a single input or output plane).  Measured per
        // launch at batch 256 and as whole forwards at batch 1 / 4 / 16 (profiles/r04_f16_kernels.txt, r04_f16_small_batch.txt):
        // ahead of conv_dma<_Float16> on every layer since the bookkeeping of a step moved out of its tail.
        // (a.wpk4 carries the pack_conv16 form: there unless ADN_F16_CONV=32; conv16_applicable refuses images beyond its 32-bit offsets)
        const bool c16 = a.wpk4 && adn::conv16_applicable(kind, a);
        // a workgroup of either fp16 kernel holds all 64 channels of the last layer: the dot is finished in its epilogue (writes y)
        c.fuse_out = tail && a.nct == 1;
        // the first layer is computed inside conv16_f16's halo stage of down1's second conv (conv16_kernels.hip, FIRST)
        if (first && h->f16_fuse_first && c16) {
            c.kernel = CONV16;
            c.fuse_first = true;
            return c;
        }
        // one clip at the deep levels: 16-64 workgroups of a long K loop on 256 CUs -- the loop is cut over up to 8 workgroups
        // (conv_dma<_Float16> slices, fp32 sums) and a reduce launch finishes the layer.  Automatic kernel choice only: like the
        // fp32 path's split it makes the summation order depend on the batch size (adn_unet_set_batch_invariant pins one form)
        if (a.wpk4 && !h->batch_invariant && !c.fuse_out)
            c.ksplit = adn::conv16_ksplit(adn::conv_workgroups(a), a.nchunk, (size_t)a.N * a.H * a.W * a.Cout);
        if (c.ksplit == 1 && c16) c.kernel = CONV16;
        return c;
    }
    if (!h->use_wino) return c;
    // fp32 Winograd path: F(4x4,3x3) or F(2x2,3x3), and how many K splits.  The last two layers (up4's second conv3x3 and the 1x1
    // output convolution, model.py:91,93) run fused: the 64-channel tensor between them is never written (the layer's output buffer
    // holds the two partial planes of its two cout tiles instead).
    c.kernel = WINO2;
    c.fuse_out = tail && a.nct == 2;
    // Conv2d(1 -> 64) is fused into down1's second conv -- its 64-channel result is computed tile by tile inside that kernel and
    // never written -- where that layer stays on unsplit F(2x2,3x3): where the F(4x4,3x3) kernel takes it the first layer runs as its
    // own launch (the fused form is time-neutral on F(2x2,3x3); unfused + F(4x4,3x3) is 1.1 ms faster at batch 64); split-K has no
    // fused variant either
    auto done = [&]() {
        c.fuse_first = first && c.kernel == WINO2 && c.ksplit == 1;
        return c;
    };
    const bool can_split = !c.fuse_out;
    const bool f4_ok = a.wpk4 && adn::wino4_applicable(kind, a, h->force_wino4);
    const long g2 = adn::conv_workgroups(a);             // `a` carries the F(2x2,3x3) grid (wino_tiles)
    if (h->allow_split && can_split) {                   // ADN_WINO_SPLITK=1: split wherever the F(2x2,3x3) grid cannot fill the chip
        c.ksplit = adn::wino_ksplit(g2, a.nchunk);
        if (c.ksplit == 1 && f4_ok) c.kernel = WINO4;
        return done();
    }
    const bool automatic = !h->batch_invariant && !h->force_wino4;
    const long thr = a.Cout <= 64 ? h->auto_grid64 : h->auto_grid;
    const long g4 = f4_ok ? adn::wino4_workgroups(a) : 0;
    // Three-stage form (levels 3 and 4; sc.U is there for those layers only).  Whether V and M fit is a matter of geometry alone
    // (every term is linear in N).  A pinned handle takes it wherever it fits -- one kernel per layer whatever the batch, and the
    // kernel a large batch runs by default --, the automatic choice where the GEMM launch fills the chip; ADN_WINO_TILE=4 keeps
    // F(4x4,3x3) in one launch.
    if (h->wino_gemm && sc.U && !c.fuse_out && !first && adn::wino3s_applicable(kind, a)) {
        const adn::Wino3sGeom g3 = adn::wino3s_geom(a);
        const bool fits = g3.v_bytes <= sc.v_bytes && g3.m_bytes <= sc.m_bytes;
        const bool pinned = h->batch_invariant && !h->force_wino4;
        if (fits && (h->wino_gemm == 2 || pinned || (automatic && g3.gemm_grid >= h->gemm_grid))) {
            c.kernel = WINO3S;
            return c;
        }
    }
    if (f4_ok && (!automatic || g4 >= thr)) {
        c.kernel = WINO4;
        return done();
    }
    // F(2x2,3x3); small grids are cut along K where even its finer grid cannot fill the chip
    if (automatic && can_split) c.ksplit = adn::wino_ksplit(g2, a.nchunk);
    // ... or F(4x4,3x3) cut along K (4.5 instead of 8 matrix FLOP per pixel, but 32x32-pixel tiles: a quarter of the workgroups).
    // Decided by the per-launch times measured on one-clip and mid-size forwards (profiles/r05_b1_timelines.txt,
    // r04_small_grid_probe.txt), in microseconds: F(4x4) 12 + 2.79 per chunk and round of 256 workgroups, F(2x2) 8 + 2.06 per chunk
    // and round of 512; a reduce launch 4 + (copies + 1) x output bytes at 8 TB/s.
    if (automatic && can_split && f4_ok) {
        const int ks4 = adn::wino4_ksplit(g4, a.nchunk);
        if (ks4 > 1) {
            const double out_mb = (double)a.N * a.H * a.W * a.Cout * 4.0 * 1e-6;
            auto reduce_us = [&](int ks) { return ks > 1 ? 4.0 + (ks + 1) * out_mb / 8.0 : 0.0; };
            const double t4 = 12.0 + 2.79 * (a.nchunk / ks4) * (double)((g4 * ks4 + 255) / 256) + reduce_us(ks4);
            const double t2 = 8.0 + 2.06 * (a.nchunk / c.ksplit) * (double)((g2 * c.ksplit + 511) / 512) + reduce_us(c.ksplit);
            if (t4 < t2) {
                c.kernel = WINO4;
                c.ksplit = ks4;
            }
        }
    }
    return done();
}

// Executes a choice.  `a`: the layer with the pointers of the chosen fused forms filled in (ConvArgs::firstw / dotw).
hipError_t launch_conv3_kernels(const adn_unet *h, adn::ConvKind kind, const Conv3Choice &c, adn::ConvArgs a, float *partial, hipStream_t st,
                                const WinoScratch &sc)
{
    if (c.fuse_out) kind = adn::CONV3X3_RELU_DOT;
    switch (c.kernel) {
    case WINO3S:
        a.wpk = sc.U;
        return adn::launch_wino3s_conv(kind, a, sc.V, sc.M, sc.tile, st);
    case CONV16:
        a.wpk = a.wpk4;
        a.nchunk0 = a.s0.C / 32;                         // conv16_f16 walks K in chunks of 32 channels
        a.nchunk = (a.s0.C + a.s1.C) / 32;
        if (c.fuse_first) a.nchunk0 = a.nchunk = 2;      // the 64 input channels are computed inside the kernel
        return adn::launch_conv16(kind, a, c.fuse_first || (a.s0.C + a.s1.C == 64 && a.Cout == 64), st);
    case DIRECT:
        if (c.ksplit > 1) {
            adn::ConvArgs sl = a;
            sl.ksplit = c.ksplit;
            sl.out = partial;
            sl.pool = nullptr;
            hipError_t e = adn::launch_conv_mfma(adn::CONV3X3_RELU, sl, true, st);
            if (e != hipSuccess) return e;
            a.ksplit = c.ksplit;
            a.partial = partial;
            return adn::launch_conv_reduce(kind, a, true, st);
        }
        return adn::launch_conv_mfma(kind, a, h->f16, st);
    case WINO4:
        a.wpk = a.wpk4;
        [[fallthrough]];
    case WINO2:
        a.ksplit = c.ksplit;
        a.partial = partial;
        return c.kernel == WINO4 ? adn::launch_wino4_conv(kind, a, st) : adn::launch_wino_conv(kind, a, st);
    }
    return hipErrorInvalidValue;
}

// A launch's status as the entry points return it.
inline int hip_status(hipError_t e, const char *what)
{
    return e == hipSuccess ? ADN_OK : fail_hip(e, what);
}

// make_plan sizes the partial buffer, choose_conv3 / choose_convt decide the split again at launch from the real arguments: a
// choice of `ks` copies of `out_floats` floats that the buffer does not hold is refused before anything is launched.
int check_part(int layer, int ks, size_t out_floats, size_t part_bytes)
{
    if (ks <= 1 || (size_t)ks * out_floats * sizeof(float) <= part_bytes) return ADN_OK;
    const LayerDesc &d = NET.v[layer];
    return fail(ADN_ERR_WORKSPACE, "adn_unet_forward: layer " + std::to_string(layer) + " (" + (d.kind == CONVT ? "transposed convolution" : "3x3 convolution") +
                " at level " + std::to_string(d.level) + ", " + std::to_string(d.C0 + d.C1) + " -> " + std::to_string(d.Cout) + " channels): " +
                std::to_string(ks) + " K-split copies of " + std::to_string(out_floats * sizeof(float)) + " bytes do not fit the " +
                std::to_string(part_bytes) + " bytes the workspace plan reserves for them");
}

// Executes a choice for layer `layer` of NET.  `a`: the layer with the pointers of the chosen fused forms filled in
// (ConvArgs::firstw / dotw).  part_bytes: capacity of `partial`.  Returns an ADN status.
int launch_conv3(const adn_unet *h, int layer, adn::ConvKind kind, const Conv3Choice &c, adn::ConvArgs a, float *partial, size_t part_bytes,
                 hipStream_t st, const WinoScratch &sc = WinoScratch())
{
    if (int rc = check_part(layer, c.ksplit, (size_t)a.N * a.H * a.W * a.Cout, part_bytes)) return rc;
    return hip_status(launch_conv3_kernels(h, kind, c, a, partial, st, sc), "launch_conv3");
}

struct ConvTChoice {
    bool t16;      // fp16: convt16_f16 (convt16_kernels.hip) instead of conv_dma
    int ksplit;    // > 1: K-split slices into the partial buffer + a reduce launch (fp32 split-bf16 form)
};

ConvTChoice choose_convt(const adn_unet *h, const LayerWeights &L, const adn::ConvArgs &a)
{
    ConvTChoice c{false, 1};
    if (h->f16) {                                        // convt16_f16 wherever it applies (packed unless ADN_F16_CONVT=dma)
        c.t16 = L.w16_off && adn::convt16_applicable(a);
        return c;
    }
    // one clip at the deep levels: the K loop cut over several workgroups + a reduce launch (fp32 split-bf16 form, automatic
    // kernel choice only: like the 3x3 layers' split, it makes the summation order depend on the batch size)
    if (h->convt_split && !h->batch_invariant)
        c.ksplit = adn::convt_ksplit(adn::conv_workgroups(a), a.nchunk, (size_t)a.N * (2 * a.H) * (2 * a.W) * a.Cout);
    return c;
}

hipError_t launch_convt_kernels(const adn_unet *h, const LayerWeights &L, const ConvTChoice &c, adn::ConvArgs a, float *partial, hipStream_t st)
{
    if (c.t16) {
        a.wpk = h->dev + L.w16_off;
        a.bias = h->dev + L.braw_off;
        return adn::launch_convt16(a, st);
    }
    if (c.ksplit > 1) {
        float *out = static_cast<float *>(a.out);
        a.ksplit = c.ksplit;
        a.out = partial;
        a.bias = h->dev + h->zero_off;
        hipError_t e = adn::launch_conv_mfma(adn::CONVT2X2, a, h->f16, st);
        if (e != hipSuccess) return e;
        return adn::launch_convt_reduce(partial, h->dev + L.braw_off, out, c.ksplit, a.N, 2 * a.H, 2 * a.W, a.Cout, st);
    }
    // The layer's wide tile (its own planes, half the column tiles) where the launch fills the chip with it, or the switch names it;
    // the bits are those of the 128-column tile, so a pinned handle may choose by the batch as well.
    if (a.split && L.wt_off && (h->split_bn >= 0 || adn::conv_workgroups(a) >= h->convt_wide_grid)) {
        a.split = 1 + L.w3_tile;
        a.wpk = h->dev + L.wt_off;
        a.nct /= 2;
    }
    return adn::launch_conv_mfma(adn::CONVT2X2, a, h->f16, st);
}

int launch_convt(const adn_unet *h, int layer, const ConvTChoice &c, const adn::ConvArgs &a, float *partial, size_t part_bytes, hipStream_t st)
{
    if (int rc = check_part(layer, c.ksplit, (size_t)a.N * (2 * a.H) * (2 * a.W) * a.Cout, part_bytes)) return rc;
    return hip_status(launch_convt_kernels(h, h->lw[layer], c, a, partial, st), "launch_convt");
}

// ---- forward -------------------------------------------------------------------------------------------------------------------

int forward_impl(adn_unet *h, const float *x, float *y, int N, int F, int T, void *workspace, size_t ws_bytes,
                 float *const *taps, hipStream_t st)
{
    if (!h || !x || !y) return fail(ADN_ERR_INVALID, "adn_unet_forward: null handle/x/y");
    Plan p;
    if (!make_plan(N, F, T, h->f16, p)) return fail(ADN_ERR_INVALID, "adn_unet_forward: need N>=1, F,T>=16 and F*T<2^27");
    if (!workspace || ws_bytes < p.total)
        return fail(ADN_ERR_WORKSPACE, "adn_unet_forward: workspace too small (see adn_unet_workspace_bytes)");
    // the activation buffers are carved out of the workspace in 256-byte granules and read with 16-byte LDS-DMA /
    // b128 accesses; x and y are accessed as single floats
    if (!aligned_to(workspace, 16)) return fail(ADN_ERR_INVALID, "adn_unet_forward: workspace must be 16-byte aligned");
    if (!aligned_to(x, 4) || !aligned_to(y, 4)) return fail(ADN_ERR_INVALID, "adn_unet_forward: x and y must be 4-byte aligned");
    DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return fail_hip(guard.err, "hipSetDevice");

    char *ws = static_cast<char *>(workspace);      // activations are fp32 or fp16 (h->f16); offsets are bytes
    void *tA = ws + p.tA, *tB = ws + p.tB;
    float *part = reinterpret_cast<float *>(ws + p.part);      // split-K partial sums (small batches)
    const bool f16 = h->f16;
    // timing hook: events[slot*(L+1) + k] is recorded before launch k (k = L: after the last one)
    const bool timed = h->timing_max > 0 && h->timing_count < h->timing_max && !taps;
    hipEvent_t *ev = timed ? h->events.data() + (size_t)h->timing_count * (ADN_N_LAUNCHES + 1) : nullptr;
    int evi = 0;
#define ADN_MARK()                                          \
    do {                                                    \
        if (timed) ADN_HIP(hipEventRecord(ev[evi++], st));  \
    } while (0)

    // block output `idx` = what layer `layer` of NET wrote to `buf`
    auto export_tap = [&](int idx, const void *buf, int layer) -> hipError_t {
        if (!taps || !taps[idx]) return hipSuccess;
        const LayerDesc &d = NET.v[layer];
        return adn::launch_nhwc_to_nchw(buf, f16, taps[idx], N, p.H[d.level], p.W[d.level], d.Cout, st);
    };
    int i = 0;                                           // next layer of NET
    // Room for V and M of the three-stage Winograd form of layer `li`: the two ping-pong buffers behind `front` bytes, the largest
    // tensor the layer reads or writes (whichever of them live in tA / tB start at the buffers' first byte; everything in the
    // ratio is linear in N, so the answer is the same for every batch size)
    auto wino_scratch = [&](int li) {
        WinoScratch sc;
        const LayerDesc &d = NET.v[li];
        if (f16 || !h->lw[li].w3_off) return sc;
        const size_t full = (size_t)N * p.H[0] * p.W[0] * 64 * sizeof(float);
        const size_t front = (size_t)N * p.H[d.level] * p.W[d.level] * std::max(std::max(d.C0, d.C1), d.Cout) * sizeof(float);
        if (front >= full) return sc;
        sc.U = h->dev + h->lw[li].w3_off;
        sc.tile = h->lw[li].w3_tile;
        sc.V = reinterpret_cast<float *>(static_cast<char *>(tA) + front);
        sc.M = reinterpret_cast<float *>(static_cast<char *>(tB) + front);
        sc.v_bytes = sc.m_bytes = full - front;
        return sc;
    };

    // ---- down path (model.py:72-79) ----
    const void *cur = tA;
    for (int l = 0; l < 4; ++l) {
        void *skip = ws + p.skip[l], *pool = ws + p.pool[l];
        if (l > 0) {
            const WinoScratch sc = wino_scratch(i);
            const adn::ConvArgs a = conv_args(h, p, i++, ws + p.pool[l - 1], nullptr, 0, 0, tA, nullptr);
            ADN_MARK();
            ADN_TRY(launch_conv3(h, i - 1, adn::CONV3X3_RELU, choose_conv3(h, adn::CONV3X3_RELU, a, false, false, sc), a, part, p.part_bytes, st, sc));
        }
        const WinoScratch sc = wino_scratch(i);
        adn::ConvArgs a = conv_args(h, p, i++, cur, nullptr, 0, 0, skip, pool);
        const Conv3Choice c = choose_conv3(h, adn::CONV3X3_RELU_POOL, a, l == 0 && h->in_ch == 1, false, sc);
        if (l == 0) {                                    // Conv2d(in_channels -> 64): its own launch, or inside the next one (its timing slot stays empty)
            ADN_MARK();
            if (c.fuse_first) {
                a.s0 = adn::ConvSrc{x, p.H[0], p.W[0], 1, 0, 0};    // the network input; the 64 channels are computed on the fly
                a.firstw = h->dev + h->first_w;
                a.firstb = h->dev + h->first_b;
            } else {
                ADN_HIP(adn::launch_conv_first(x, h->dev + h->first_w, h->dev + h->first_b, tA, f16, N, p.H[0], p.W[0], h->in_ch, st));
            }
        }
        ADN_MARK();
        ADN_TRY(launch_conv3(h, i - 1, adn::CONV3X3_RELU_POOL, c, a, part, p.part_bytes, st, sc));
        ADN_HIP(export_tap(l, skip, i - 1));
    }
    // ---- bottleneck (model.py:81) ----
    {
        const WinoScratch sa = wino_scratch(i);
        const adn::ConvArgs a = conv_args(h, p, i++, ws + p.pool[3], nullptr, 0, 0, tA, nullptr);
        ADN_MARK();
        ADN_TRY(launch_conv3(h, i - 1, adn::CONV3X3_RELU, choose_conv3(h, adn::CONV3X3_RELU, a, false, false, sa), a, part, p.part_bytes, st, sa));
        const WinoScratch sb = wino_scratch(i);
        const adn::ConvArgs b = conv_args(h, p, i++, tA, nullptr, 0, 0, tB, nullptr);
        ADN_MARK();
        ADN_TRY(launch_conv3(h, i - 1, adn::CONV3X3_RELU, choose_conv3(h, adn::CONV3X3_RELU, b, false, false, sb), b, part, p.part_bytes, st, sb));
        ADN_HIP(export_tap(4, tB, i - 1));
    }
    // ---- up path (model.py:84-91): convT -> (virtual) pad + cat([skip, up]) -> DoubleConv ----
    void *X = tB, *Y = tA;   // X holds the current tensor
    Conv3Choice last{};                                  // of the network's last 3x3 layer
    for (int l = 3; l >= 0; --l) {
        const adn::ConvArgs t = convt_args(h, p, i++, X, Y);
        ADN_MARK();
        ADN_TRY(launch_convt(h, i - 1, choose_convt(h, h->lw[i - 1], t), t, part, p.part_bytes, st));
        // first conv of the DoubleConv reads cat([skip, x1]) virtually
        const WinoScratch sa = wino_scratch(i);
        const adn::ConvArgs a = conv_args(h, p, i++, ws + p.skip[l], Y, 2 * t.H, 2 * t.W, X, nullptr);
        ADN_MARK();
        ADN_TRY(launch_conv3(h, i - 1, adn::CONV3X3_RELU, choose_conv3(h, adn::CONV3X3_RELU, a, false, false, sa), a, part, p.part_bytes, st, sa));
        const WinoScratch sb = wino_scratch(i);
        adn::ConvArgs b = conv_args(h, p, i++, X, nullptr, 0, 0, Y, nullptr);
        // (the fused tails finish ONE class; UNet(..., num_classes > 1) runs the 1x1 convolution class by class below)
        last = choose_conv3(h, adn::CONV3X3_RELU, b, false, l == 0 && !taps && h->n_classes == 1, sb);
        if (last.fuse_out) {
            b.dotw = h->dev + h->out_w;
            b.dot_out = f16 ? y : static_cast<float *>(Y);          // fp16: the network output; Winograd: the two partial planes
            if (f16) b.dot_bias = h->out_b;
        }
        ADN_MARK();
        ADN_TRY(launch_conv3(h, i - 1, adn::CONV3X3_RELU, last, b, part, p.part_bytes, st, sb));
        ADN_HIP(export_tap(5 + (3 - l), Y, i - 1));
        std::swap(X, Y);
    }
    // ---- 1x1 output convolution (model.py:93) ----
    ADN_MARK();
    if (last.fuse_out && f16) {
        // y was written by the previous launch; this timing slot stays empty
    } else if (last.fuse_out)   // X = the buffer the fused layer wrote its partial planes to (the loop swapped X and Y)
        ADN_HIP(adn::launch_dot_finish(static_cast<const float *>(X), 2, h->out_b, y, (long)N * F * T, st));
    else
        for (int k = 0; k < h->n_classes; ++k)          // y is (N, K, F, T): class k is plane k of every clip
            ADN_HIP(adn::launch_conv_out(X, f16, h->dev + h->out_w + (size_t)64 * k, h->out_bias[k], y + (size_t)k * F * T,
                                         (long)N * F * T, (long)F * T, (long)h->n_classes * F * T, st));
    ADN_MARK();
    if (timed) {
        if (evi != ADN_N_LAUNCHES + 1) return fail(ADN_ERR_INVALID, "internal: launch count mismatch");
        ++h->timing_count;
    }
#undef ADN_MARK
    if (taps && taps[9])
        ADN_HIP(hipMemcpyAsync(taps[9], y, (size_t)N * h->n_classes * F * T * sizeof(float), hipMemcpyDeviceToDevice, st));
    return ADN_OK;
}

// ---- handle creation -----------------------------------------------------------------------------------------------------------

int check_create_args(adn_unet **handle, int device, const float *const *t, int n_tensors, int dtype, int in_channels, int num_classes)
{
    if (!handle || !t) return fail(ADN_ERR_INVALID, "adn_unet_create: null argument");
    if (in_channels < 1 || in_channels > 64 || num_classes < 1 || num_classes > 64)
        return fail(ADN_ERR_INVALID, "adn_unet_create_general: need 1 <= in_channels <= 64 and 1 <= num_classes <= 64");
    if (dtype != ADN_DTYPE_F32 && dtype != ADN_DTYPE_F16) return fail(ADN_ERR_INVALID, "adn_unet_create: dtype must be ADN_DTYPE_F32 or ADN_DTYPE_F16");
    if (n_tensors != ADN_N_WEIGHT_TENSORS) return fail(ADN_ERR_INVALID, "adn_unet_create: expected 118 tensors");
    for (int i = 0; i < n_tensors; ++i)
        if (!t[i]) return fail(ADN_ERR_INVALID, "adn_unet_create: null tensor pointer");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(ADN_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(ADN_ERR_INVALID, "adn_unet_create: bad device index");
    return ADN_OK;
}

int check_device_arch(int device)
{
    hipDeviceProp_t prop;
    ADN_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(ADN_ERR_NO_DEVICE, std::string("libadn is built for gfx950 only, device is ") + prop.gcnArchName);
    return ADN_OK;
}

// The environment switches of include/adn.h, read once per handle (h.f16 is set).
void read_switches(adn_unet &h)
{
    if (const char *algo = std::getenv("ADN_CONV_ALGO"))       // "direct": implicit-GEMM kernel instead of Winograd
        h.use_wino = std::strcmp(algo, "direct") != 0;
    if (h.f16) h.use_wino = false;                             // the fp16 path runs the direct fp16-MFMA kernels
    if (const char *sk = std::getenv("ADN_WINO_SPLITK")) h.allow_split = std::atoi(sk) != 0;
    if (const char *cs = std::getenv("ADN_CONVT_SPLIT")) h.convt_split = std::atoi(cs) != 0;
    if (const char *bi = std::getenv("ADN_BATCH_INVARIANT")) h.batch_invariant = std::atoi(bi) != 0;
    if (const char *ff = std::getenv("ADN_F16_FIRST")) h.f16_fuse_first = std::atoi(ff) != 0;
    if (const char *fc = std::getenv("ADN_F16_CONV")) h.f16_conv = std::atoi(fc) == 32 ? 0 : 1;
    if (const char *ft = std::getenv("ADN_F16_CONVT")) h.f16_convt = std::strcmp(ft, "dma") == 0 ? 0 : 1;
    if (const char *ag = std::getenv("ADN_AUTO_GRID")) h.auto_grid = std::atol(ag);      // tuning knobs of the small-grid rule
    if (const char *ag = std::getenv("ADN_AUTO_GRID64")) h.auto_grid64 = std::atol(ag);
    if (h.f16) h.convt_split = false;
    if (const char *wg = std::getenv("ADN_WINO_GEMM")) h.wino_gemm = std::atoi(wg) == 2 ? 2 : std::atoi(wg) != 0;
    if (const char *sb = std::getenv("ADN_SPLIT_BN"))
        h.split_bn = !std::strcmp(sb, "128") ? adn::SPLIT_BN128 : !std::strcmp(sb, "256") ? adn::SPLIT_BN256 : !std::strcmp(sb, "256w8") ? adn::SPLIT_BN256W8 : -2;
    if (const char *wt = std::getenv("ADN_WINO_TILE")) {
        h.use_wino4 = std::atoi(wt) != 2;
        h.force_wino4 = std::atoi(wt) == 4;
    }
}

// Workgroup tile of a split-bf16 GEMM -- the GEMM stage of the three-stage form, a transposed convolution (4 Cout columns) -- for
// layer `d`: the handle's switch where the layer has whole 256-column tiles, else the measured default
// (profiles/split_gemm_tile_ab.md).
adn::SplitTile split_tile(const adn_unet &h, const LayerDesc &d)
{
    if ((d.kind == CONVT ? 4 * d.Cout : d.Cout) % 256) return adn::SPLIT_BN128;
    if (h.split_bn >= 0) return static_cast<adn::SplitTile>(h.split_bn);
    // Measured at batch 64 x 513x256, interleaved with the 128-column library: 256 columns on 4 waves is faster in every pair, by
    // more than the 128-column spread, for the five GEMM stages (6 - 9 %) and for up1 ... up3 (13, 11, 3 %); up4's transposed
    // convolution (8 chunks, 256 columns in all) is inside the spread and stays; the 8-wave form gains 1 - 3 % and is nowhere ahead.
    return d.kind == CONVT && d.Cout < 128 ? adn::SPLIT_BN128 : adn::SPLIT_BN256;
}

// Folds BatchNorm and packs every tensor of the state_dict walk (adn.h) into `host` in the forms the handle's kernels read; the
// offsets go into h.
void pack_weights(adn_unet &h, const float *const *t, std::vector<float> &host)
{
    auto reserve = [&](size_t n) {
        const size_t at = host.size();
        host.resize(at + ((n + 63) & ~size_t(63)), 0.f);
        return at;
    };
    auto halfs = [&](size_t off) { return reinterpret_cast<_Float16 *>(host.data() + off); };
    std::vector<float> scale, bias;
    // downconv1: first conv has Cin = in_channels -> direct kernel, weights [input plane][tap][64]
    bn_fold(t[1], t[2], t[3], t[4], t[5], 64, scale, bias);
    h.first_w = reserve((size_t)h.in_ch * 9 * 64);
    for (int ci = 0; ci < h.in_ch; ++ci)
        for (int tap = 0; tap < 9; ++tap)
            for (int co = 0; co < 64; ++co)
                host[h.first_w + ((size_t)ci * 9 + tap) * 64 + co] = t[0][((size_t)co * h.in_ch + ci) * 9 + tap] * scale[co];
    h.first_b = reserve(64);
    std::memcpy(host.data() + h.first_b, bias.data(), sizeof(float) * 64);
    int ti = 6;
    for (int i = 0; i < N_LAYERS; ++i) {
        const LayerDesc &d = NET.v[i];
        LayerWeights &L = h.lw[i];
        const int Cin = d.C0 + d.C1, Cout = d.Cout;
        const size_t n16 = ((size_t)(d.kind == CONVT ? 4 : 9) * Cin * Cout + 1) / 2;      // floats that hold the layer's weights as fp16
        if (d.kind == CONVT) {
            if (h.f16) {
                L.w_off = reserve(n16);
                pack_convt<_Float16>(t[ti], Cin, Cout, halfs(L.w_off));
                if (h.f16_convt != 0 && Cin % 128 == 0 && Cout % 64 == 0) {
                    L.w16_off = reserve(n16);
                    pack_convt16(t[ti], Cin, Cout, halfs(L.w16_off));
                    L.braw_off = reserve(Cout);
                    std::memcpy(host.data() + L.braw_off, t[ti + 1], sizeof(float) * Cout);
                }
            } else if (h.convt_split) {
                L.w_off = reserve(3 * n16);                                      // three bf16 planes
                pack_convt_split(t[ti], Cin, Cout, 128, reinterpret_cast<uint16_t *>(host.data() + L.w_off));
                L.w3_tile = split_tile(h, d);
                if (L.w3_tile != adn::SPLIT_BN128) {
                    L.wt_off = reserve(3 * n16);
                    pack_convt_split(t[ti], Cin, Cout, adn::split_tile_bn(L.w3_tile), reinterpret_cast<uint16_t *>(host.data() + L.wt_off));
                }
                L.braw_off = reserve(Cout);
                std::memcpy(host.data() + L.braw_off, t[ti + 1], sizeof(float) * Cout);
            } else {
                L.w_off = reserve((size_t)4 * Cin * Cout);
                pack_convt<float>(t[ti], Cin, Cout, host.data() + L.w_off);
            }
            L.b_off = reserve((size_t)4 * Cout);
            for (int col = 0; col < 4 * Cout; ++col) {          // bias per GEMM column
                int ij, c;
                adn::convt_column(col, Cout, ij, c);
                host[L.b_off + col] = t[ti + 1][c];
            }
            ti += 2;
            continue;
        }
        bn_fold(t[ti + 1], t[ti + 2], t[ti + 3], t[ti + 4], t[ti + 5], Cout, scale, bias);
        if (h.f16 && h.f16_conv != 0 && Cin % 32 == 0 && Cout % 64 == 0) {
            L.w16_off = reserve(n16);
            pack_conv16(t[ti], scale, Cin, Cout, halfs(L.w16_off));
        }
        if (h.use_wino) {
            L.w_off = reserve((size_t)16 * Cin * Cout);
            pack_wino3x3(t[ti], scale, Cin, Cout, adn::WINO_BN, host.data() + L.w_off);
            if (h.use_wino4) {
                L.w4_off = reserve((size_t)36 * Cin * Cout);
                pack_wino4_3x3(t[ti], scale, Cin, Cout, host.data() + L.w4_off);
                // levels 3 and 4 from 512 input channels on: the three-stage form's planes (five layers, 0.57 GB).  down4's first conv
                // (256 -> 512) stays on F(4x4,3x3): V and M cost it what the faster products save (0.742 -> 0.718 ms at batch 64,
                // inside the run-to-run spread; profiles/wino_gemm_ab.md)
                if (h.wino_gemm && d.level >= 3 && Cin >= 512 && Cin % 16 == 0 && Cout % 128 == 0) {
                    L.w3_off = reserve((size_t)36 * Cin * Cout * 3 / 2);
                    L.w3_tile = split_tile(h, d);
                    pack_wino4_split(t[ti], scale, Cin, Cout, adn::split_tile_bn(L.w3_tile), reinterpret_cast<uint16_t *>(host.data() + L.w3_off));
                }
            }
        } else if (h.f16) {
            L.w_off = reserve(n16);
            pack_conv3x3<_Float16>(t[ti], scale, Cin, Cout, halfs(L.w_off));
        } else {
            L.w_off = reserve((size_t)9 * Cin * Cout);
            pack_conv3x3<float>(t[ti], scale, Cin, Cout, host.data() + L.w_off);
        }
        L.b_off = reserve(Cout);
        std::memcpy(host.data() + L.b_off, bias.data(), sizeof(float) * Cout);
        ti += 6;
    }
    h.zero_off = reserve(4 * 512);                                   // zeros: the bias of K-split transposed convolutions' slices
    h.out_w = reserve((size_t)64 * h.n_classes);                     // out.weight (K, 64, 1, 1) is already [class][64]
    std::memcpy(host.data() + h.out_w, t[ti], sizeof(float) * 64 * h.n_classes);
    h.out_bias.assign(t[ti + 1], t[ti + 1] + h.n_classes);
    h.out_b = t[ti + 1][0];
}

// Frees what a handle owns on its device, then the handle.
struct UnetDeleter {
    void operator()(adn_unet *h) const
    {
        {
            DeviceGuard guard(h->device);
            for (hipEvent_t e : h->events) (void)hipEventDestroy(e);
            if (h->dev) (void)hipFree(h->dev);
        }
        delete h;
    }
};

}  // namespace

extern "C" {

int adn_unet_create(adn_unet **handle, int device, const float *const *t, int n_tensors)
{
    return adn_unet_create_ex(handle, device, t, n_tensors, ADN_DTYPE_F32);
}

int adn_unet_create_ex(adn_unet **handle, int device, const float *const *t, int n_tensors, int dtype)
{
    return adn_unet_create_general(handle, device, t, n_tensors, dtype, 1, 1);
}

int adn_unet_channels(const adn_unet *h, int *in_channels, int *num_classes)
{
    if (!h || !in_channels || !num_classes) return fail(ADN_ERR_INVALID, "adn_unet_channels: null argument");
    *in_channels = h->in_ch;
    *num_classes = h->n_classes;
    return ADN_OK;
}

int adn_unet_set_batch_invariant(adn_unet *h, int on)
{
    if (!h) return fail(ADN_ERR_INVALID, "adn_unet_set_batch_invariant: null handle");
    h->batch_invariant = on != 0;
    return ADN_OK;
}

int adn_unet_create_general(adn_unet **handle, int device, const float *const *t, int n_tensors, int dtype, int in_channels,
                            int num_classes)
{
    if (int rc = check_create_args(handle, device, t, n_tensors, dtype, in_channels, num_classes)) return rc;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return fail_hip(guard.err, "hipSetDevice");
    if (int rc = check_device_arch(device)) return rc;

    std::unique_ptr<adn_unet, UnetDeleter> h(new adn_unet());
    h->device = device;
    h->in_ch = in_channels;
    h->n_classes = num_classes;
    h->f16 = dtype == ADN_DTYPE_F16;
    read_switches(*h);
    // (a tile the library does not have is refused: the planes are packed for it, so a misspelt width must not pass for the default)
    if (h->split_bn < -1) return fail(ADN_ERR_INVALID, "adn_unet_create: ADN_SPLIT_BN must be 128, 256 or 256w8");
    std::vector<float> host;
    pack_weights(*h, t, host);
    h->dev_floats = host.size();
    hipError_t e = hipMalloc(&h->dev, host.size() * sizeof(float));
    if (e != hipSuccess) return fail_hip(e, "hipMalloc(weights)");
    e = hipMemcpy(h->dev, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail_hip(e, "hipMemcpy(weights)");
    *handle = h.release();
    return ADN_OK;
}

int adn_unet_set_timing(adn_unet *h, int max_forwards)
{
    if (!h || max_forwards < 0 || max_forwards > 4096) return fail(ADN_ERR_INVALID, "adn_unet_set_timing: bad argument");
    DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return fail_hip(guard.err, "hipSetDevice");
    for (hipEvent_t e : h->events) (void)hipEventDestroy(e);
    h->events.clear();
    h->timing_max = 0;
    h->timing_count = 0;
    h->events.resize((size_t)max_forwards * (ADN_N_LAUNCHES + 1));
    for (size_t i = 0; i < h->events.size(); ++i) ADN_HIP(hipEventCreate(&h->events[i]));
    h->timing_max = max_forwards;
    return ADN_OK;
}

int adn_unet_get_timing(adn_unet *h, int index, float *ms)
{
    if (!h || !ms || index < 0 || index >= h->timing_count) return fail(ADN_ERR_INVALID, "adn_unet_get_timing: no such forward");
    DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) return fail_hip(guard.err, "hipSetDevice");
    hipEvent_t *ev = h->events.data() + (size_t)index * (ADN_N_LAUNCHES + 1);
    ADN_HIP(hipEventSynchronize(ev[ADN_N_LAUNCHES]));
    for (int k = 0; k < ADN_N_LAUNCHES; ++k) ADN_HIP(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
    return ADN_OK;
}

int adn_unet_destroy(adn_unet *h)
{
    if (h) UnetDeleter()(h);
    return ADN_OK;
}

int adn_unet_workspace_bytes(const adn_unet *h, int N, int F, int T, size_t *bytes)
{
    if (!bytes) return fail(ADN_ERR_INVALID, "adn_unet_workspace_bytes: null");
    Plan p;
    if (!make_plan(N, F, T, h ? h->f16 : false, p)) return fail(ADN_ERR_INVALID, "adn_unet_workspace_bytes: need N>=1, F,T>=16 and F*T<2^27");
    *bytes = p.total;
    return ADN_OK;
}

int adn_unet_forward(adn_unet *h, const float *x, float *y, int N, int F, int T, void *workspace,
                     size_t workspace_bytes, void *stream)
{
    return forward_impl(h, x, y, N, F, T, workspace, workspace_bytes, nullptr, static_cast<hipStream_t>(stream));
}

int adn_unet_forward_taps(adn_unet *h, const float *x, float *y, int N, int F, int T, void *workspace,
                          size_t workspace_bytes, float *const *taps, void *stream)
{
    return forward_impl(h, x, y, N, F, T, workspace, workspace_bytes, taps, static_cast<hipStream_t>(stream));
}

}  // extern "C"
