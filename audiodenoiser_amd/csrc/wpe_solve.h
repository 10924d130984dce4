// The Cholesky solve of the offline WPE kernels (dereverb_kernels.hip, dereverb_mc_kernels.hip): one definition, so that the
// multichannel operator at one channel and the single-channel one cannot drift apart.  include/adn.h, "dereverb": A = L L^H column
// by column, L y = P, L^H g = y, inner sums sequential in k.
#pragma once
#include <hip/hip_runtime.h>

namespace adn {

// max(x, c) of adn.h: a NaN x stays NaN
__device__ __forceinline__ float max_keep_nan(float x, float c) { return x < c ? c : x; }

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
                const float2 a = rr[k], b = rc[k];
                v.x = fmaf(-a.y, b.y, fmaf(-a.x, b.x, v.x));
                v.y = fmaf(a.x, b.y, fmaf(-a.y, b.x, v.y));
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
                const float2 a = rr[k], y = g[k];
                v.x = fmaf(a.y, y.y, fmaf(-a.x, y.x, v.x));
                v.y = fmaf(-a.y, y.x, fmaf(-a.x, y.y, v.y));
            }
            g[r] = make_float2(v.x / rr[r].x, v.y / rr[r].x);
        }
        for (int r = K - 1; r >= 0; --r) {           // L^H g = y
            float2 v = g[r];
            for (int k = K - 1; k > r; --k) {        // v -= conj(L_kr) g_k
                const float2 a = A[k * (k + 1) / 2 + r], y = g[k];
                v.x = fmaf(-a.y, y.y, fmaf(-a.x, y.x, v.x));
                v.y = fmaf(a.y, y.x, fmaf(-a.x, y.y, v.y));
            }
            const float lrr = A[r * (r + 1) / 2 + r].x;
            g[r] = make_float2(v.x / lrr, v.y / lrr);
        }
    }
    __syncthreads();
}

}  // namespace adn
