// Backward-data of a 1x1 layer with the producing layer's activation backward in its store (mask1x1.hip): the stage of
// conv_dispatch (conv.hip) for the few-channel GEMMs of the U-Nets' heads.  Host only, not part of the ABI.
#pragma once
#include "common.h"

namespace sprk {

// gin[n][c][p] = act'(mask[n][c][p]) * sum_k gy[n][k][p] * w[k][c] over the weight slabs transform_weights (conv.hip)
// prepared for conv_mfma_kernel: nblkN slabs [rows][ldw] of NT * 16 output channels, the K rows in chunks of CK that
// occupy R4 rows each.
struct Mask1x1Call {
    const float *gy, *wT, *mask;
    float *gin;
    int N, K, Cn, HW;              // images, reduced channels, output channels, pixels per plane
    int CK, R4, rows, ldw, NT, nblkN;
    int act;                       // SPRK_ACT_LEAKY / SPRK_ACT_RELU
};

constexpr int kMask1x1MaxK = 96;

// k-steps (v_mfma_f32_16x16x4_f32) a call walks, chunk by chunk as conv_mfma_kernel does; 0: outside the kernel's limits
int mask1x1_steps(int K, int CK);
int mask1x1_run(const Mask1x1Call &c, hipStream_t s);

}  // namespace sprk
