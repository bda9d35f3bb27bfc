// 16-bit-operand backward-weight of the 3x3 stride-1 layers (wgrad16.hip); called from conv.hip when the geometry
// asks for 16-bit operands (sprk_conv_geom.dtype) and the layer is eligible.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace sprk {

// c: the layer; with SPRK_DT_X16 in c.dtype x, x2 and gy are 16-bit tensors of the operand type.
// The workspace of a call, 0 for a layer that is not eligible: one plan answers both questions of wgrad_dispatch
size_t wgrad16_ws_bytes(const sprk_conv_geom &c);
inline bool wgrad16_eligible(const sprk_conv_geom &c) { return wgrad16_ws_bytes(c) != 0; }
// ws: at least wgrad16_ws_bytes(c); item: see sprk_conv2d_bwd_weight_partial (nullptr = add the workgroups' partial dW now)
int wgrad16_run(const sprk_conv_geom &c, const void *x, const void *x2, const void *gy, float *gw, void *ws,
                sprk_reduce_item *item, hipStream_t s);
long wgrad16_launches();
// rec[1 .. SPRK_VARIANT_INTS - 1] of sprk_conv2d_variant's record for stage SPRK_STAGE_16BIT, which 2 (sprk.h): the
// kernel that wgrad16_run launches for c and the loops it runs there, from the same plans; rec[0] is the caller's
void wgrad16_variant(const sprk_conv_geom &c, int32_t *rec);

}  // namespace sprk
