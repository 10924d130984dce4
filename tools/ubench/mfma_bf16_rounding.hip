// What one v_mfma_f32_32x32x16_bf16 rounds (the instruction of the split-bf16 forms, conv_dma<..., SPLIT>): sums chosen so that an
// intermediate rounding shows.  Every row of A and every column of B is the same, so every element of D is the same sum.
// Build: hipcc --offload-arch=gfx950 -O2 -o mfma_bf16_rounding mfma_bf16_rounding.hip.  Result (MI355X): profiles/f32_blocks.md.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <cstdint>
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
__global__ void k(const float *a16, float c, float *out)
{
    const int hh = threadIdx.x >> 5;
    bf16x8 a, b;
    for (int e = 0; e < 8; ++e) {
        a[e] = (__bf16)a16[8 * hh + e];
        b[e] = (__bf16)1.0f;
    }
    f32x16 acc;
    for (int i = 0; i < 16; ++i) acc[i] = c;
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    if (threadIdx.x == 0) out[0] = acc[0];
    if (threadIdx.x == 37) out[1] = acc[5];
}
int main()
{
    float *da, *dout;
    if (hipMalloc(&da, 64) != hipSuccess || hipMalloc(&dout, 8) != hipSuccess) return 2;
    struct T { const char *name; float c; int idx[4]; float val[4]; double exact; };
    const float P24 = 16777216.f;
    T tests[] = {
        {"C=2^24 + a0=1 + a1=1        ", P24, {0, 1, -1, -1}, {1, 1, 0, 0}, 16777218.0},
        {"C=2^24 + a0=1 + a2=1        ", P24, {0, 2, -1, -1}, {1, 1, 0, 0}, 16777218.0},
        {"C=2^24 + a0=1 + a4=1        ", P24, {0, 4, -1, -1}, {1, 1, 0, 0}, 16777218.0},
        {"C=2^24 + a0=1 + a8=1        ", P24, {0, 8, -1, -1}, {1, 1, 0, 0}, 16777218.0},
        {"C=2^24 + a3=1 + a12=1       ", P24, {3, 12, -1, -1}, {1, 1, 0, 0}, 16777218.0},
        {"C=2^24 + a0=3               ", P24, {0, -1, -1, -1}, {3, 0, 0, 0}, 16777219.0},
        {"C=2^24 + a0=1 + a1=0.5      ", P24, {0, 1, -1, -1}, {1, 0.5f, 0, 0}, 16777217.5},
        {"C=2^24 + a0=1 + a8=0.5      ", P24, {0, 8, -1, -1}, {1, 0.5f, 0, 0}, 16777217.5},
        {"C=2^24 + 4 x 0.5 (a0..a3)   ", P24, {0, 1, 2, 3}, {0.5f, 0.5f, 0.5f, 0.5f}, 16777218.0},
        {"C=2^24 + 4 x 0.5 (a0,4,8,12)", P24, {0, 4, 8, 12}, {0.5f, 0.5f, 0.5f, 0.5f}, 16777218.0},
        {"C=0 + a0=2^12 + a1=a2=2^-12 ", 0.f, {0, 1, 2, -1}, {4096.f, 1.f / 4096, 1.f / 4096, 0}, 4096.0 + 2.0 / 4096},
        {"C=0 + a0=2^12 + a8=a9=2^-12 ", 0.f, {0, 8, 9, -1}, {4096.f, 1.f / 4096, 1.f / 4096, 0}, 4096.0 + 2.0 / 4096},
        {"C=1 + a0=2^-24 + a1=2^-24   ", 1.f, {0, 1, -1, -1}, {1.f / 16777216, 1.f / 16777216, 0, 0}, 1.0 + 2.0 / 16777216},
        {"C=-2^24 + a0=2^24 + a1=2^-8 ", -P24, {0, 1, -1, -1}, {P24, 1.f / 256, 0, 0}, 1.0 / 256},
    };
    for (const T &t : tests) {
        float a[16] = {0};
        for (int i = 0; i < 4; ++i)
            if (t.idx[i] >= 0) a[t.idx[i]] = t.val[i];
        if (hipMemcpy(da, a, 64, hipMemcpyHostToDevice) != hipSuccess) return 3;
        hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, da, t.c, dout);
        float o[2];
        if (hipMemcpy(o, dout, 8, hipMemcpyDeviceToHost) != hipSuccess) return 4;
        printf("%s -> %.10g (other lane %.10g)   exact %.10g, rounded once %.10g\n", t.name, (double)o[0], (double)o[1], t.exact, (double)(float)t.exact);
    }
    return 0;
}
