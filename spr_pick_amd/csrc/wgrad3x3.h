// The backward-weight of the U-Nets' 3x3 layers that the Winograd kernel does not take, as a streaming kernel
// (wgrad3x3.hip): the stage of wgrad_dispatch (conv.hip) for fp32 3x3 stride-1 same-size calls whose plan is MODE 2 with
// chunks of 48 input channels (27 k-tiles, 7 per wave of the general kernel) and blocks of 3 or 6 output tiles, over
// planes of 16, 32 or 64 columns, so that a 64-pixel tile is 4, 2 or 1 whole rows of one image.  Host only, not part of
// the ABI.
#pragma once
#include "common.h"

namespace sprk {

// partial[group][(c * 9 + tap)][CoutP] = sum over the group's tiles of x[c][pixel + tap] * gy[pixel][co], on plan_wgrad's
// split: `groups` groups of tilesPerGroup consecutive 64-pixel tiles (the last one may be shorter), nChunks chunks of 48
// input channels (the first C1 / 48 of them from x, the others from x2), nblkN blocks of 16 NT output channels.  Tile t is
// rows (64 / W) (t % tilesPerImg) ... of image t / tilesPerImg.
struct Wgrad3x3Call {
    const float *x, *x2, *gy;
    float *partial;
    int N, C1, C2, Cout, CoutP;
    int H, W, padT, padL;
    int NT;                            // output tiles per block: 3 or 6
    int nTiles, tilesPerGroup, groups;
    int nChunks, nblkN;
};

constexpr int kWgrad3x3Chunk = 48;     // input channels of a chunk: a 16-row k-tile is one tap x 16 channels

// planes the kernel walks: W = 16, 32 or 64 and whole tiles of 64 / W rows
inline bool wgrad3x3_plane(int H, int W) { return (W == 16 || W == 32 || W == 64) && H >= 64 / W && H % (64 / W) == 0; }

int wgrad3x3_run(const Wgrad3x3Call &c, hipStream_t s);

extern std::atomic<long> g_wgrad3x3_launches;
extern std::atomic<int> g_wgrad3x3_on;

}  // namespace sprk
