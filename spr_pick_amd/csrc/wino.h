// Winograd F(2x2, 3x3) path of the 3x3 stride-1 convolutions (wino.hip); called from conv.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "corr.h"

namespace sprk {

bool wino_eligible(const Corr &c);
size_t wino_ws_bytes(const Corr &c);
// Everything a forward / backward-data call on the Winograd stage is launched with, and the shape of the loops its
// workgroups then run.  wino_variant fills it; wino_conv launches from it and sprk_conv2d_variant returns it (sprk.h
// lists the fields in this order): neither decides anything itself.
struct WinoVariant {
    int NT, SQ, UNROT;      // wino_conv_kernel<NT, SQ, UNROT>
    int groups, lastCh;     // channel groups of NT * 16 (grid.y), output channels in the last one
    int nc1, nch, r1, r2;   // 4-channel chunks of source 1 / of both sources, C1 % 4, C2 % 4
    int pairs;              // pairs of steady-state (unchecked) K iterations per tile
    int sw;                 // where the cursor moves to source 2: 0 no second source, 1 in first_loads (nc1 == 1), 2 in
                            // iteration 0 (nc1 == 2), 3 in a checked iteration, 4 in a steady-state one
    int gridX, ntiles, tpwMin, tpwMax;   // grid.x, tiles, tiles per workgroup (fewest, most)
    int xcd;                // XCD order in effect: the knob is on and grid.x is a multiple of 8
    int tilesX, tilesY, padT, padL;
    int mode;               // reader of the output transform: 0 plain, 1 mask, 2 up2, 3 un-rotated store
    int unrotB;             // images per rotation of an un-rotated store (not part of the record)
};
// masked: the call carries the mask of a fused activation backward; unrotB > 0: the un-rotated store
WinoVariant wino_variant(const Corr &c, bool masked, int unrotB);
// x, x2: sources [N,C1,H,W], [N,C2,H,W] (x2 may be null); w: the forward layer's taps (c.taps); y: [N,Cout,H,W], or
// [N,Cout,2H,2W] with c.ep.up2 (every output written to its 2x2 block); U: workspace of wino_ws_bytes().
// mask: [N,Cout,H,W] or null: y *= d act / d (mask), act = mask_act (backward-data: the saved conv input)
// v.unrotB > 0 (wino_unrot_eligible; N = 4 * unrotB images of a 4-rotation stack): y is the un-rotated tensor
// f [unrotB, 4 * Cout, H, W] of sprk_unrot4_shift_concat_fwd, written by the output transform itself
int wino_conv(const Corr &c, const WinoVariant &v, const float *x, const float *x2, const float *w, float *y, float *U,
              const float *mask, int mask_act, hipStream_t s);
bool wino_unrot_eligible(const Corr &c);
bool wino_wgrad_eligible(const sprk_conv_geom &g);
size_t wino_wgrad_ws_bytes(const sprk_conv_geom &g);
// The launches of a backward-weight call on the Winograd stage: per source the 48-channel groups (MT = 3, grid.y = g48,
// K split over parts = CUs / g48 workgroups), then its tail of <= 16 channels (MT = 1, one group, parts = CUs).  Each
// launch leaves one column range of wino_wgrad_reduce_kernel.  wino_wgrad_variant fills it, wino_wgrad launches from it.
struct WinoWgVariant {
    int launches;           // 1..4 = reduce ranges
    struct Launch {
        int MT, ch, parts;  // ch: groups of 48 channels (MT 3) or channels of the tail (MT 1)
        int src, xcd;       // source 0 | 1; XCD order in effect (not part of the record's launch triple)
    } l[4];
    int regionsX, regionsY;
    int cx, cy;             // bit i: some workgroup of launch i carries its region cursor over a row / over an image
    int padT, padL, Cout;
    int xcdMask;            // bit i: launch i walks its regions in XCD order
};
WinoWgVariant wino_wgrad_variant(const sprk_conv_geom &g);
// x, x2: sources [N,C1,H,W], [N,C2,H,W] (x2 may be null); gy: [N,Cout,H,W]; gw: [Cout][C1+C2][3][3]; ws: workspace of
// wino_wgrad_ws_bytes().  The kernel's own pass sums its partial results: nothing is left pending in the reduce item.
int wino_wgrad(const sprk_conv_geom &g, const WinoWgVariant &v, const float *x, const float *x2, const float *gy, float *gw,
               void *ws, sprk_reduce_item *, hipStream_t s);

}  // namespace sprk
