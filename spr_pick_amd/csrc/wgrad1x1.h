// The backward-weight of the wide 1x1 layers of the U-Nets' heads as a streaming kernel (wgrad1x1.hip): the stage of
// wgrad_dispatch (conv.hip) for fp32 1x1 calls whose plan is the row form with 3 k-tiles per wave and 6 output tiles
// per block, over planes whose 64-pixel tiles are 64 consecutive floats.  Host only, not part of the ABI.
#pragma once
#include "common.h"

namespace sprk {

// partial[group][k][CoutP] = sum over the group's tiles of x[k][pixel] * gy[pixel][co], on plan_wgrad's split: `groups`
// groups of tilesPerGroup consecutive 64-pixel tiles (the last one may be shorter), nChunks chunks of CKW reduced-
// channel rows, nblkN blocks of 96 output channels.  Tile t is pixels 64 (t % tilesPerImg) .. + 63 of image
// t / tilesPerImg.
struct Wgrad1x1Call {
    const float *x, *gy;
    float *partial;
    int N, Cin, Cout, CoutP;
    int plane;                         // pixels per image plane (a multiple of 64)
    int nTiles, tilesPerGroup, groups;
    int CKW, nChunks, nblkN;
};

constexpr int kWgrad1x1Rows = 192;     // most reduced-channel rows of a chunk (12 k-tiles: 3 per wave)

int wgrad1x1_run(const Wgrad1x1Call &c, hipStream_t s);

extern std::atomic<long> g_wgrad1x1_launches;
extern std::atomic<int> g_wgrad1x1_on;

}  // namespace sprk
