// vs_fuse_score.h -- one pass over a stored row for several sub-queries at once, shared by the fused search
// (vs_fuse.hip) and the multi-vector search (vs_maxsim.hip).
#pragma once
#include "vs_device.h"

namespace vs {

// The canonical fp64 scores of R stored rows with m sub-queries at once (row[i] < 0: absent): the loop of
// exact_score_rows (vs_device.h) with one accumulator per (sub-query, row).  Each accumulator takes the
// same additions in the same order as there -- lane l's 8-element groups ascending, then the xor
// butterfly 32..1 -- so out[j][i] is the canonical score.  qs: the sub-queries as fp64 [m][8][ng] in LDS
// (QLDS), qg: [m][d] fp32 in global memory.
template <int DT, int METRIC, bool QLDS, int R>
__device__ __forceinline__ void fuse_score_rows(const uint8_t* __restrict__ corpus, const int64_t (&row)[R],
                                                const double* __restrict__ qs, const float* __restrict__ qg, int m,
                                                int d, int dpad, int lane, double (&out)[FUSE_MAX_Q][R]) {
#pragma clang fp contract(off)
    constexpr int ES = DT == DT_F32 ? 4 : 2;
    constexpr int NV = DT == DT_F32 ? 2 : 1;
    constexpr int RU = 3;
    constexpr int CE = CHB / ES;
    const uint8_t* rb[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int64_t r = row[i] >= 0 ? row[i] : row[0];
        rb[i] = corpus + (r / TR) * (int64_t)TR * dpad * ES + (r % TR) * CHB;
    }
    const int ng = (d + 7) >> 3;
    double acc[FUSE_MAX_Q][R];
#pragma unroll
    for (int j = 0; j < FUSE_MAX_Q; ++j)
#pragma unroll
        for (int i = 0; i < R; ++i) acc[j][i] = 0.0;
    for (int g0 = lane; g0 < ng; g0 += 64 * RU) {
        uint4 raw[RU][R][NV];
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const int g = g0 + 64 * u;
            if (g < ng) {
                const int e0 = 8 * g;
                const int64_t off = (int64_t)(e0 / CE) * TR * CHB + (e0 % CE) * ES;
#pragma unroll
                for (int i = 0; i < R; ++i)
                    if (i == 0 || row[i] >= 0)
#pragma unroll
                        for (int v = 0; v < NV; ++v) raw[u][i][v] = *(const uint4*)(rb[i] + off + 16 * v);
            }
        }
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const int g = g0 + 64 * u;
            if (g < ng) {
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    if (i > 0 && row[i] < 0) continue;
                    float x[8];
#pragma unroll
                    for (int v = 0; v < NV; ++v) unpack16<DT>(raw[u][i][v], x + 4 * v);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int ie = 8 * g + e;
                        if (ie < d) {
                            const double xa = (double)x[e];
#pragma unroll
                            for (int j = 0; j < FUSE_MAX_Q; ++j) {
                                if (j < m) {  // (uniform)
                                    const double qq = QLDS ? qs[((size_t)j * 8 + e) * ng + g] : (double)qg[(int64_t)j * d + ie];
                                    if constexpr (METRIC == METRIC_IP) {
                                        const double pa = xa * qq;
                                        acc[j][i] = acc[j][i] + pa;
                                    } else {
                                        const double da = xa - qq;
                                        const double pa = da * da;
                                        acc[j][i] = acc[j][i] + pa;
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1)
#pragma unroll
        for (int j = 0; j < FUSE_MAX_Q; ++j)
            if (j < m)
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    const double o = __shfl_xor(acc[j][i], sft, 64);
                    acc[j][i] = acc[j][i] + o;
                }
#pragma unroll
    for (int j = 0; j < FUSE_MAX_Q; ++j)
#pragma unroll
        for (int i = 0; i < R; ++i) out[j][i] = acc[j][i];
}

}  // namespace vs
