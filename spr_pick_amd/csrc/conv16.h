// 16-bit-operand (bf16 / fp16) MFMA convolution path (conv16.hip); called from conv.hip when the geometry asks
// for it (sprk_conv_geom.dtype) and the layer is eligible.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "corr.h"

namespace sprk {

bool conv16_eligible(const Corr &c);
// 0 = no 16-bit kernel, 1 = conv16_mfma_kernel (fp32 storage only), 2 = conv16_tile_kernel, 3 = conv16_head_kernel
int conv16_kind(const Corr &c);
size_t conv16_ws_bytes(const Corr &c);
// x, x2, y: fp32 tensors, or 16-bit tensors of the operand type where c.x16() / c.y16() say so
int conv16_run(const Corr &c, const void *x, const void *x2, const float *w, void *y, void *ws,
               size_t ws_bytes, hipStream_t s);
long conv16_launches();
// rec[1 .. SPRK_VARIANT_INTS - 1] of sprk_conv2d_variant's record for stage SPRK_STAGE_16BIT (sprk.h): the kernel that
// conv16_run launches for c and the loops it runs there, from the same plans; rec[0] is the caller's
void conv16_variant(const Corr &c, int32_t *rec);

}  // namespace sprk
