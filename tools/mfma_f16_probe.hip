// Fragment-layout probe for v_mfma_f32_32x32x16_f16 on gfx950, and for the
// chaining that k_attn_chunk (dllama_amd/ops/csrc/attn.hip) relies on.
// Hypothesis (the f16 sibling of the i8 layout in mfma_probe.hip):
//   A[m][k]: lane = (m & 31) | ((k >> 3) << 5), half = k & 7
//   B[k][n]: lane = (n & 31) | ((k >> 3) << 5), half = k & 7
//   C[m][n]: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
// Chaining: with C = S^T = K Q^T (m = timestep, n = query row), accumulator
// registers 8c..8c+7 of a lane, rounded to f16, ARE a B operand of the next
// MFMA for query row n, over the 8 timesteps
//   t(c, hi, j) = 16c + 8 * (j >> 2) + 4 * hi + (j & 3)
// k is only a summation index, so O^T = V^T P^T is right as long as the A
// operand (V^T) is gathered over the same 8 timesteps: no shuffle of P.
// Operands are asymmetric random (K, Q and V unrelated), so a transposed or
// permuted fragment cannot pass.
// Build: hipcc --offload-arch=gfx950 -O2 tools/mfma_f16_probe.hip -o /tmp/mfma_f16_probe
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>

typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int D = 32;  // head_dim of the probe: two k-blocks of S, one m-block of O

// K [32 t][D], Q [32 rows][D], V [32 t][32 d]  ->  St [32 t][32 rows] f32,
// Ot [32 d][32 rows] f32 with P = f16(St) (no softmax: the layouts are the point)
__global__ void k_probe(const _Float16 *K, const _Float16 *Q, const _Float16 *V,
                        float *St, float *Ot) {
    const int lane = threadIdx.x;
    const int mn = lane & 31, hi = lane >> 5;
    v16f s = {};
    for (int kb = 0; kb < D / 16; kb++) {
        v8h a, b;
        for (int j = 0; j < 8; j++) {
            a[j] = K[mn * D + kb * 16 + hi * 8 + j];
            b[j] = Q[mn * D + kb * 16 + hi * 8 + j];
        }
        s = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, s, 0, 0, 0);
    }
    for (int r = 0; r < 16; r++)
        St[((r & 3) + 8 * (r >> 2) + 4 * hi) * 32 + mn] = s[r];
    v16f o = {};
    for (int c = 0; c < 2; c++) {
        v8h p, v;
        for (int j = 0; j < 8; j++) {
            p[j] = (_Float16)s[8 * c + j];
            const int t = 16 * c + 8 * (j >> 2) + 4 * hi + (j & 3);
            v[j] = V[t * 32 + mn];  // V^T[d = mn][t]
        }
        o = __builtin_amdgcn_mfma_f32_32x32x16_f16(v, p, o, 0, 0, 0);
    }
    for (int r = 0; r < 16; r++)
        Ot[((r & 3) + 8 * (r >> 2) + 4 * hi) * 32 + mn] = o[r];
}

int main() {
    static _Float16 hK[32 * D], hQ[32 * D], hV[32 * 32];
    static float hS[1024], hO[1024];
    srand(42);
    auto rnd = [] { return (_Float16)((rand() % 2001 - 1000) / 1000.0f); };
    for (int i = 0; i < 32 * D; i++) { hK[i] = rnd(); hQ[i] = rnd(); }
    for (int i = 0; i < 1024; i++) hV[i] = rnd();
    _Float16 *dK, *dQ, *dV;
    float *dS, *dO;
    hipMalloc(&dK, sizeof hK); hipMalloc(&dQ, sizeof hQ); hipMalloc(&dV, sizeof hV);
    hipMalloc(&dS, sizeof hS); hipMalloc(&dO, sizeof hO);
    hipMemcpy(dK, hK, sizeof hK, hipMemcpyHostToDevice);
    hipMemcpy(dQ, hQ, sizeof hQ, hipMemcpyHostToDevice);
    hipMemcpy(dV, hV, sizeof hV, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_probe, dim3(1), dim3(64), 0, 0, dK, dQ, dV, dS, dO);
    if (hipMemcpy(hS, dS, sizeof hS, hipMemcpyDeviceToHost) != hipSuccess
        || hipMemcpy(hO, dO, sizeof hO, hipMemcpyDeviceToHost) != hipSuccess) {
        printf("FAIL: HIP error\n");
        return 2;
    }
    int bad = 0;
    static float refS[1024];
    for (int t = 0; t < 32; t++)
        for (int r = 0; r < 32; r++) {
            float acc = 0.0f;
            for (int d = 0; d < D; d++) acc += (float)hK[t * D + d] * (float)hQ[r * D + d];
            refS[t * 32 + r] = acc;
            if (fabsf(hS[t * 32 + r] - acc) > 1e-4f && bad++ < 8)
                printf("S MISMATCH t=%d row=%d got %g want %g\n", t, r,
                       hS[t * 32 + r], acc);
        }
    for (int d = 0; d < 32; d++)
        for (int r = 0; r < 32; r++) {
            float acc = 0.0f;
            for (int t = 0; t < 32; t++)  // P from the device S: only the layout differs
                acc += (float)hV[t * 32 + d] * (float)(_Float16)hS[t * 32 + r];
            if (fabsf(hO[d * 32 + r] - acc) > 1e-3f && bad++ < 8)
                printf("O MISMATCH d=%d row=%d got %g want %g\n", d, r,
                       hO[d * 32 + r], acc);
        }
    printf(bad ? "FAIL (%d)\n" : "PASS: f16 32x32x16 layouts and S^T -> P^T chaining confirmed\n", bad);
    return bad ? 1 : 0;
}
