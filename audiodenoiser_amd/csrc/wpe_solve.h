// What the two offline WPE kernels share (dereverb_kernels.hip, dereverb_mc_kernels.hip): the grid of a launch, the block a lane
// owns, and the Cholesky solve: one definition, so that the multichannel operator at one channel and the single-channel one
// cannot drift apart.  include/adn.h, "dereverb": A = L L^H column by column, L y = P, L^H g = y, inner sums sequential in k.
#pragma once
#include "wpe_common.h"                              // max_keep_nan, the complex multiply-adds

namespace adn {

// The workgroups of an offline launch: n rows (clips or groups) x ceil(F / bins of a 256-lane tile at `lanes` lanes per bin)
inline long wpe_tile_grid(int n, int F, int lanes)
{
    const long bins = 256 / lanes;
    return (((long)F + bins - 1) / bins) * n;
}

// Lane gl's block (rb, cb) of a lower triangle cut into blocks, row after row: block rb (rb + 1) / 2 + cb, cb <= rb
__device__ __forceinline__ void wpe_tri_block(int gl, int &rb, int &cb)
{
    rb = 0;
    while ((rb + 1) * (rb + 2) / 2 <= gl) ++rb;
    cb = gl - rb * (rb + 1) / 2;
}

// The solve of one row by its group of LPB lanes (lane gl): A (packed lower triangle, row r at r (r + 1) / 2) holds R; g holds
// n_rhs right-hand sides P, column c at g + c * pitch, n_rhs <= LPB.  On return the columns hold the taps.  One factorisation; lane
// c < n_rhs then substitutes column c, every column in the same order.  The loops are uniform over the workgroup, the barriers are
// the workgroup's.
template <int LPB>
__device__ __forceinline__ void wpe_solve(float2 *A, float2 *g, int K, float loading, int gl, int n_rhs = 1, int pitch = 0)
{
#pragma clang fp contract(off)
    if (gl == 0) {                                   // A = R + (loading tr(R) / K + 1e-30) I; the diagonal is real
        float tr = 0.f;
        for (int j = 0; j < K; ++j) tr += A[j * (j + 1) / 2 + j].x;
        const float eps = (loading * tr) / (float)K + 1e-30f;
        for (int j = 0; j < K; ++j) {
            float2 &a = A[j * (j + 1) / 2 + j];
            a.x = a.x + eps;
            a.y = 0.f;
        }
    }
    __syncthreads();
    for (int c = 0; c < K; ++c) {                    // A = L L^H, column after column, L in A's place
        const float2 *rc = A + c * (c + 1) / 2;
        if (gl == 0) {
            float s = rc[c].x;
            for (int k = 0; k < c; ++k) {
                s = fmaf(-rc[k].x, rc[k].x, s);
                s = fmaf(-rc[k].y, rc[k].y, s);
            }
            A[c * (c + 1) / 2 + c].x = sqrtf(s);
        }
        __syncthreads();
        const float lcc = rc[c].x;
        for (int r = c + 1 + gl; r < K; r += LPB) {
            float2 *rr = A + r * (r + 1) / 2;
            float2 v = rr[c];
            for (int k = 0; k < c; ++k) {            // v -= L_rk conj(L_ck)
                const float2 a = rr[k];
                v = cfma_conj_yx(make_float2(-a.x, -a.y), rc[k], v);
            }
            rr[c] = make_float2(v.x / lcc, v.y / lcc);
        }
        __syncthreads();
    }
    if (gl < n_rhs) {
        g += gl * pitch;
        for (int r = 0; r < K; ++r) {                // L y = P
            const float2 *rr = A + r * (r + 1) / 2;
            float2 v = g[r];
            for (int k = 0; k < r; ++k) {            // v -= L_rk y_k
                const float2 a = rr[k];
                v = cfma(make_float2(-a.x, -a.y), g[k], v);
            }
            g[r] = make_float2(v.x / rr[r].x, v.y / rr[r].x);
        }
        for (int r = K - 1; r >= 0; --r) {           // L^H g = y
            float2 v = g[r];
            for (int k = K - 1; k > r; --k) {        // v -= conj(L_kr) g_k
                v = cfms_conj(A[k * (k + 1) / 2 + r], g[k], v);
            }
            const float lrr = A[r * (r + 1) / 2 + r].x;
            g[r] = make_float2(v.x / lrr, v.y / lrr);
        }
    }
    __syncthreads();
}

}  // namespace adn
