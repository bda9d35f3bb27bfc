// The wide 1x1 layers of the U-Nets' heads as a streaming GEMM (gemm1x1.hip): the stage of conv_dispatch (conv.hip) for
// unmasked forward and backward-data calls with many reduced channels.  Host only, not part of the ABI.
#pragma once
#include "common.h"

namespace sprk {

// y[n][c][p] = act(scale[c] * sum_k x[n][k][p] * w[k][c] + shift[c]) over the weight slabs transform_weights (conv.hip)
// prepared for conv_mfma_kernel<4, 6>: nblkN slabs [rows][ldw] of 96 output channels, the K rows in chunks of 16 that
// occupy 16 rows each (slab row = reduced channel, zero rows up to the next multiple of 16).
struct Gemm1x1Call {
    const float *x, *wT, *zeros;   // zeros: >= 1 readable zero float (the head of the call's workspace)
    const float *bias, *scale, *shift;
    float *y;
    int N, K, Cn, HW;              // images, reduced channels, output channels, pixels per plane
    int rows, ldw, nblkN;
    int act;
};

constexpr int kGemm1x1MinK = 192;
constexpr int kGemm1x1Ldw = 112;   // row stride of a slab of 6 channel tiles (plan_fwd: NT * 16 + 16)

// may the kernel take a call of these sizes (the geometry part of conv.hip's gemm1x1_takes)
bool gemm1x1_fits(int N, int K, int HW);
// workgroups of the launch (persistent: each walks its items)
int gemm1x1_grid(int N, int HW, int nblkN);
int gemm1x1_run(const Gemm1x1Call &c, hipStream_t s);

extern std::atomic<long> g_gemm1x1_launches;
extern std::atomic<int> g_gemm1x1_on;

}  // namespace sprk
