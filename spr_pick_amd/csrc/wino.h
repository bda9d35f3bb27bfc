// Winograd F(2x2, 3x3) path of the 3x3 stride-1 convolutions (wino.hip); called from conv.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "corr.h"

namespace sprk {

bool wino_eligible(const Corr &c);
size_t wino_ws_bytes(const Corr &c);
// x, x2: sources [N,C1,H,W], [N,C2,H,W] (x2 may be null); w: the forward layer's taps (c.taps); y: [N,Cout,H,W], or
// [N,Cout,2H,2W] with c.ep.up2 (every output written to its 2x2 block); U: workspace of wino_ws_bytes().
// mask: [N,Cout,H,W] or null: y *= d act / d (mask), act = mask_act (backward-data: the saved conv input)
// unrotB > 0 (wino_unrot_eligible; N = 4 * unrotB images of a 4-rotation stack): y is the un-rotated tensor
// f [unrotB, 4 * Cout, H, W] of sprk_unrot4_shift_concat_fwd, written by the output transform itself
int wino_conv(const Corr &c, const float *x, const float *x2, const float *w, float *y, float *U, const float *mask,
              int mask_act, hipStream_t s, int unrotB = 0);
bool wino_unrot_eligible(const Corr &c);
bool wino_wgrad_eligible(const sprk_conv_geom &g);
size_t wino_wgrad_ws_bytes(const sprk_conv_geom &g);
// x, x2: sources [N,C1,H,W], [N,C2,H,W] (x2 may be null); gy: [N,Cout,H,W]; gw: [Cout][C1+C2][3][3]; ws: workspace of
// wino_wgrad_ws_bytes().  The kernel's own pass sums its partial results: nothing is left pending in the reduce item.
int wino_wgrad(const sprk_conv_geom &g, const float *x, const float *x2, const float *gy, float *gw, void *ws,
               sprk_reduce_item *, hipStream_t s);

}  // namespace sprk
