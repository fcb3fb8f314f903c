// The register-tile NT GEMM on exact-fp32 MFMA (v_mfma_f32_16x16x4_f32) shared by the token linear (linear_kernel,
// gp_fusion.hip) and the image encoder's batched products (bgemm_nt_kernel, gp_imgenc.hip). The kernels keep their
// own signatures and epilogues; the body is inlined.
#pragma once
#include "gp_common.h"

// C[i][j] = sum_k a[i][k] b[j][k] for a (M, K) with row stride lda and b (N, K) with row stride ldb; K a multiple
// of 16, rows 16-byte aligned. 4 waves as 2 (i) x 2 (j), a wave owns TM i-tiles x TN j-tiles of 16; block x walks
// i, block y walks j. b rows are the MFMA A input and a rows the B input: lane (q, r) feeds float4 k-slices
// 16g + 4q .. +3 of row r of both, so one 16-deep k-group is 4 MFMAs per tile pair and the accumulator holds columns
// j .. j + 3 of one row i (a float4 store). The next k-group's operands are loaded while this one multiplies. Rows
// past M / N are clamped for the loads and never stored.
// column(j) is called once per live 16-column tile with the lane's first column and returns put(i, v), called once
// per live row with the lane's four sums: what is per column (a bias) is fetched once.
template <int TM, int TN, class Column>
__device__ __forceinline__ void gemm_nt_body(const float* __restrict__ a, int lda, int M, const float* __restrict__ b,
                                             int ldb, int N, int K, Column column) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int q = lane >> 4, r = lane & 15;
    const int i0 = blockIdx.x * (32 * TM) + (wid & 1) * (16 * TM);
    const int j0 = blockIdx.y * (32 * TN) + (wid >> 1) * (16 * TN);
    const float* ap[TM];
    const float* bp[TN];
#pragma unroll
    for (int t = 0; t < TM; ++t) ap[t] = a + (size_t)min(i0 + 16 * t + r, M - 1) * lda + 4 * q;
#pragma unroll
    for (int u = 0; u < TN; ++u) bp[u] = b + (size_t)min(j0 + 16 * u + r, N - 1) * ldb + 4 * q;
    f32x4 acc[TN][TM];
#pragma unroll
    for (int u = 0; u < TN; ++u)
#pragma unroll
        for (int t = 0; t < TM; ++t) acc[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int KG = K >> 4;
    f32x4 aa[TM], ba[TN];
#pragma unroll
    for (int t = 0; t < TM; ++t) aa[t] = ld4(ap[t]);
#pragma unroll
    for (int u = 0; u < TN; ++u) ba[u] = ld4(bp[u]);
    for (int g = 0; g < KG; ++g) {
        f32x4 an[TM], bn[TN];
        const int kn = (g + 1 < KG ? g + 1 : g) * 16;
#pragma unroll
        for (int t = 0; t < TM; ++t) an[t] = ld4(ap[t] + kn);
#pragma unroll
        for (int u = 0; u < TN; ++u) bn[u] = ld4(bp[u] + kn);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
            for (int u = 0; u < TN; ++u)
#pragma unroll
                for (int t = 0; t < TM; ++t) acc[u][t] = mfma4(ba[u][jj], aa[t][jj], acc[u][t]);
#pragma unroll
        for (int t = 0; t < TM; ++t) aa[t] = an[t];
#pragma unroll
        for (int u = 0; u < TN; ++u) ba[u] = bn[u];
    }
#pragma unroll
    for (int u = 0; u < TN; ++u) {
        const int jt = j0 + 16 * u;
        if (jt >= N) continue;
        const auto put = column(jt + 4 * q);
#pragma unroll
        for (int t = 0; t < TM; ++t) {
            const int i = i0 + 16 * t + r;
            if (i < M) put(i, acc[u][t]);
        }
    }
}
