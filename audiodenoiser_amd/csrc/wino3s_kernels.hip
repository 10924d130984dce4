// Three-stage Winograd F(4x4,3x3) for the deep fp32 3x3 layers (levels 3 and 4: small images, 256-1024 channels).
//
// wino4_conv_f32 (wino4_kernels.hip) keeps V = B^T d B and M = sum V .* U on chip, which binds its matrix stage to a 32-cout
// tile and to the exact-fp32 MFMA.  Here the same products run on the bf16 matrix cores through the three-term split of the
// transposed convolutions (conv_dma<..., SPLIT, WINO_GEMM>, conv_kernels.hip), whose 128 x 128 tile pays for the split of an
// activation 128 columns wide (or 256: SplitTile, adn_internal.h) -- at the price of V and M in memory, 2.25x the layer's input and output:
//   stage 1  wino3s_input_kernel    C8 activations (virtual pad + cat of two sources) -> V[pos][Cin/8][row][8]
//   stage 2  launch_wino_gemm       M_pos = V_pos U_pos, 36 GEMMs in one launch      -> M[pos][Cout/8][row][8]
//   stage 3  wino3s_output_kernel   A^T M A + bias, ReLU (+ 2x2 max-pool)             -> C8 output (+ pooled tensor)
// row = 4x4 output tile, numbered over the whole batch: (clip * tilesY + tile row) * tilesX + tile column; pos = 6 i + j of
// the 6x6 transform domain (i: vertical).  Stages 1 and 3 are memory-bound: one thread per (row, half channel block) holds the
// 36 values of four channels as 16-byte vectors, so a wave reads / writes V and M in 1 KB runs.
// A row of the GEMM is one tile: a non-finite input pixel reaches the tiles whose 6x6 patch holds it and no other.
//
// Numerics (tests/test_gpu_f32_blocks.py, profiles/f32_blocks.md): the split is exact, so what the form adds to F(4x4,3x3) in fp32
// is the roundings of its accumulator alone -- twelve per 16 channels (six products, and the bf16 instruction rounds after each 8
// of its 16 terms) where the exact-fp32 MFMA rounds sixteen times.  A block that runs the form sits ON the floor of that
// arithmetic restated in another order (E rms 7 - 35 fp32 ulps of the block's rms against floors of 8 - 38, 0.73 - 1.09 of the
// floor; the one-launch F(4x4) kernel: 7 - 48), and every product is needed: with one of the three second-order products missing a
// block lands 1.4 - 4 x outside the bound of twice the floor.
#include "adn_internal.h"

namespace adn {

namespace {

constexpr int NT = 256;

// grid: (ceil(2 rows / NT), Cin / 8); thread = (row, half of the channel block)
__global__ __launch_bounds__(NT) void wino3s_input_kernel(const ConvArgs p, float *__restrict__ V, int tilesY, int tilesX, long rows)
{
    const long id = (long)blockIdx.x * NT + threadIdx.x;
    const long row = id >> 1;
    const int half = (int)(id & 1), cb = blockIdx.y;
    if (row >= rows) return;
    const int tx = (int)(row % tilesX);
    const long r2 = row / tilesX;
    const int ty = (int)(r2 % tilesY), n = (int)(r2 / tilesY);
    // channel block cb of the virtual cat([s0, s1]); s1 sits (offY, offX) inside the output domain, zeros around it
    const bool second = cb >= p.s0.C / 8;
    const ConvSrc &s = second ? p.s1 : p.s0;
    const int cbl = second ? cb - p.s0.C / 8 : cb;
    const float *src = static_cast<const float *>(s.ptr) + ((size_t)n * (s.C / 8) + cbl) * ((size_t)s.H * s.W * 8) + half * 4;
    const int y0 = 4 * ty - 1 - s.offY, x0 = 4 * tx - 1 - s.offX;
    f32x4 d[6][6];
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const int y = y0 + a, x = x0 + b;
            d[a][b] = (y >= 0 && y < s.H && x >= 0 && x < s.W) ? *reinterpret_cast<const f32x4 *>(src + ((size_t)y * s.W + x) * 8)
                                                                : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    // row stage (along the pixel columns of every patch row), then column stage: the order of wino4_conv_f32, whose transform
    // functions these are (bt6 / at6, adn_internal.h), so V has the bits that kernel forms in registers
#pragma unroll
    for (int a = 0; a < 6; ++a) bt6(d[a][0], d[a][1], d[a][2], d[a][3], d[a][4], d[a][5]);
#pragma unroll
    for (int b = 0; b < 6; ++b) bt6(d[0][b], d[1][b], d[2][b], d[3][b], d[4][b], d[5][b]);
    const int ncb = (p.s0.C + p.s1.C) / 8;
    float *vp = V + ((size_t)cb * rows + row) * 8 + half * 4;
    const size_t pstr = (size_t)ncb * rows * 8;                       // floats between positions
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) *reinterpret_cast<f32x4 *>(vp + (size_t)(6 * i + j) * pstr) = d[i][j];
}

// grid: (ceil(2 rows / NT), Cout / 8); thread = (row, half of the channel block)
template <bool POOL>
__global__ __launch_bounds__(NT) void wino3s_output_kernel(const ConvArgs p, const float *__restrict__ M, int tilesY, int tilesX,
                                                           long rows)
{
    const long id = (long)blockIdx.x * NT + threadIdx.x;
    const long row = id >> 1;
    const int half = (int)(id & 1), cb = blockIdx.y;
    if (row >= rows) return;
    const int tx = (int)(row % tilesX);
    const long r2 = row / tilesX;
    const int ty = (int)(r2 % tilesY), n = (int)(r2 / tilesY);
    const float *mp = M + ((size_t)cb * rows + row) * 8 + half * 4;
    const size_t pstr = (size_t)(p.Cout / 8) * rows * 8;
    f32x4 w[4][6];                                                    // A^T M: output row a, transform-domain column j
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        f32x4 m[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) m[i] = *reinterpret_cast<const f32x4 *>(mp + (size_t)(6 * i + j) * pstr);
        at6(m[0], m[1], m[2], m[3], m[4], m[5], w[0][j], w[1][j], w[2][j], w[3][j]);
    }
    const f32x4 bias = *reinterpret_cast<const f32x4 *>(p.bias + cb * 8 + half * 4);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 y[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        at6(w[a][0], w[a][1], w[a][2], w[a][3], w[a][4], w[a][5], y[a][0], y[a][1], y[a][2], y[a][3]);
#pragma unroll
        for (int b = 0; b < 4; ++b) y[a][b] = __builtin_elementwise_maximum(y[a][b] + bias, zero);     // relu_nan: NaN stays NaN
    }
    float *ob = static_cast<float *>(p.out) + ((size_t)n * (p.Cout / 8) + cb) * ((size_t)p.H * p.W * 8) + half * 4;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int gy = 4 * ty + a, gx = 4 * tx + b;
            if (gy < p.H && gx < p.W) *reinterpret_cast<f32x4 *>(ob + ((size_t)gy * p.W + gx) * 8) = y[a][b];
        }
    if constexpr (POOL) {
        // MaxPool2d(2), floor mode: a 4x4 tile holds four whole windows; NaN-propagating maximum as nn.MaxPool2d (max4_nan)
        const int Hp = p.H >> 1, Wp = p.W >> 1;
        float *pb = static_cast<float *>(p.pool) + ((size_t)n * (p.Cout / 8) + cb) * ((size_t)Hp * Wp * 8) + half * 4;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int py = 2 * ty + a, px = 2 * tx + b;
                const f32x4 mx = __builtin_elementwise_maximum(__builtin_elementwise_maximum(y[2 * a][2 * b], y[2 * a][2 * b + 1]),
                                                               __builtin_elementwise_maximum(y[2 * a + 1][2 * b], y[2 * a + 1][2 * b + 1]));
                if (py < Hp && px < Wp) *reinterpret_cast<f32x4 *>(pb + ((size_t)py * Wp + px) * 8) = mx;
            }
    }
}

}  // namespace

bool wino3s_applicable(ConvKind kind, const ConvArgs &a)
{
    if (kind != CONV3X3_RELU && kind != CONV3X3_RELU_POOL) return false;
    if (kind == CONV3X3_RELU_POOL && !a.pool) return false;
    const int Cin = a.s0.C + a.s1.C;
    if (a.firstw || a.ksplit > 1 || Cin < 16 || (Cin & 15) || (a.s0.C & 7) || a.Cout < 128 || (a.Cout & 127)) return false;
    return a.N >= 1 && a.H >= 1 && a.W >= 1 && wino3s_geom(a).rows < (1L << 25);
}

Wino3sGeom wino3s_geom(const ConvArgs &a)
{
    Wino3sGeom g{};
    g.tilesY = (a.H + 3) / 4;
    g.tilesX = (a.W + 3) / 4;
    g.rows = (long)a.N * g.tilesY * g.tilesX;
    g.v_bytes = (size_t)36 * g.rows * (a.s0.C + a.s1.C) * sizeof(float);
    g.m_bytes = (size_t)36 * g.rows * a.Cout * sizeof(float);
    g.gemm_grid = 36 * ((g.rows + 127) / 128) * (a.Cout / 128);
    return g;
}

hipError_t launch_wino3s_conv(ConvKind kind, const ConvArgs &a, float *V, float *M, SplitTile tile, hipStream_t st)
{
    if (!wino3s_applicable(kind, a) || !V || !M || !a.wpk || !a.bias || !a.out) return hipErrorInvalidValue;
    const Wino3sGeom g = wino3s_geom(a);
    const long bx = (2 * g.rows + NT - 1) / NT;
    const int Cin = a.s0.C + a.s1.C;
    hipLaunchKernelGGL(wino3s_input_kernel, dim3((unsigned)bx, (unsigned)(Cin / 8)), dim3(NT), 0, st, a, V, g.tilesY, g.tilesX, g.rows);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_wino_gemm(V, a.wpk, M, g.rows, Cin, a.Cout, tile, st);
    if (e != hipSuccess) return e;
    if (kind == CONV3X3_RELU_POOL)
        hipLaunchKernelGGL(wino3s_output_kernel<true>, dim3((unsigned)bx, (unsigned)(a.Cout / 8)), dim3(NT), 0, st, a, M, g.tilesY,
                           g.tilesX, g.rows);
    else
        hipLaunchKernelGGL(wino3s_output_kernel<false>, dim3((unsigned)bx, (unsigned)(a.Cout / 8)), dim3(NT), 0, st, a, M, g.tilesY,
                           g.tilesX, g.rows);
    return hipGetLastError();
}

}  // namespace adn
