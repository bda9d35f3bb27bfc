// The backward-weight of the 3x3 stride-1 layers on chunks of 48 input channels (48 -> 48, 96 -> 96, 144 -> 96 at 16 to
// 64 columns) as a streaming kernel.
//
//   partial[group][c * 9 + tap][co] = sum over the group's 64-pixel tiles, in order, of  x[c][pixel + tap] * gy[pixel][co]
//
// The sums are conv_wgrad_mfma_kernel<7, NT, ., 2>'s (conv.hip: wgrad_tile), operation for operation, on plan_wgrad's
// split: every element has ONE accumulator that starts at 0 and takes, per tile, 16 v_mfma_f32_16x16x4_f32 in the order
// of the k-steps 4j + s, x in the A operand (row k = tap * 48 + channel: a k-tile is one tap x 16 channels) and gy in
// the B operand, lane group lq holding pixel 16j + 4lq + s of the tile, operands outside the image +0.  The slab layout
// [group][c * 9 + tap][CoutP] and the reduction that follows are unchanged.
//
// What differs is everything around the MFMAs.  The predicate (conv.hip: wgrad3x3_takes) admits only planes of W = 16,
// 32 or 64 columns, so a tile is TR = 64 / W whole rows of one image: 64 consecutive floats of every gy plane, and the
// TR + 2 rows iy0 .. iy0 + TR + 1 (iy0 = first output row - pad_top) of every x plane.  The DMA runs from a scalar cursor
// (two 64-bit offsets, the tile's row block and the tiles left) that advances with carries: no division after the
// prologue, no table.  A lane's x offset is loop invariant (its halo row r and 4-column chunk q against the tile's
// origin; chunks left and right of the image carry the zero-filling offset for good) and is made zero-filling per tile by
// one unsigned compare of iy0 + r with H.
//
// Eight waves, two per SIMD, for both block widths.  NT = 3: wave w owns k-tiles w, w + 8, w + 16, w + 24 (4 4 4 3 3 3 3
// 3: the waves w and w + 4 share a SIMD, so 7 7 7 6 per SIMD) x the 3 output tiles.  NT = 6: wave (wi, wj) owns k-tiles
// wi, wi + 4, .. (7 7 7 6) x output tiles 3 wj .. 3 wj + 2, as in the general kernel.
//
// LDS image of x (this kernel's own): channel c at float offset 288 c + z(c), z(c) = (c & 3) + 8 ((c >> 2) & 3); inside,
// halo row r at (W + 8) r and input column ix at ix + 4.  One wave DMA fills one channel: lane u <-> (r, q) = (u / Q,
// u % Q), Q = W / 4 + 2, 16 bytes each, lane linear from a base that is only 4-byte aligned.  The A operand is read by
// ds_read_b32 at  base(lane, k-tile) + immediate(j, s): the lanes of one 32-lane half (16 channels l15 x lq in {0, 1} or
// {2, 3}) sit at float offsets 288 l15 + z(l15) + 4 lq + const, and 288 = 0 (mod 32), so their banks are const + {0 1 2
// 3, 8 .. 11, 16 .. 19, 24 .. 27} (z) + {0, 4} (lq): all 32 banks once, no conflict.  (With channel planes that start on
// 16-byte boundaries every lane of a half reads the same offset mod 4: 8 banks for 32 lanes, the general kernel's 4-way
// conflict.)  gy is staged and read as the general kernel does it: rows of 64 floats whose 16-byte chunks are
// XOR-swizzled by row & 15, one ds_read_b128 per output tile and 4 k-steps, no conflict.
//
// Two LDS stages.  One barrier per tile, LDS-only, behind the LAST operand fetch of tile i (the A values of step 15,
// fetched in front of the MFMAs of step 14): behind it every wave is done reading stage i & 1, so the DMA of tile i + 2
// goes out into it under the MFMAs of steps 14 and 15, and tile i + 1 (issued a whole tile earlier, waited for by one vmcnt in
// front of the barrier) is published: its first operands are fetched under the MFMAs of step 15.  After the last tile the
// cursor stays where it is: the surplus DMAs re-read the last tile into a stage nobody reads (no branch in the loop).
#include "wgrad3x3.h"

#include <type_traits>

#include "conv_dev.h"

namespace {

constexpr int kCK = sprk::kWgrad3x3Chunk;
constexpr int kCS = 288;                        // channel stride of the x image, floats: = 0 (mod 32), >= 256 + 27
constexpr int kXFloats = kCK * kCS + 32;        // (the last channel's wave DMA ends at 47 * 288 + 27 + 256)
constexpr int NW = 8;                           // waves
constexpr int kXDma = kCK / NW;                 // wave DMAs (one channel each) per wave and tile: x
static_assert(kCS % 32 == 0 && kCS >= 256 + 27 + 1 && kXFloats % 4 == 0, "x image");

struct W3Args {
    const float *x, *x2, *gy;
    float *partial;
    int C1, C2, Cout, CoutP, H, padT, padL;
    int tilesPerImg, nTiles, tilesPerGroup;
};

typedef const __attribute__((address_space(3))) f32x4 *lds_c4p;

__device__ __forceinline__ int zoff(int c) { return (c & 3) + 8 * ((c >> 2) & 3); }

// KT: most k-tiles of a wave (4: blocks of 3 output tiles, 7: blocks of 6); W = 1 << LGW columns
template <int KT, int LGW>
__global__ __launch_bounds__(64 * NW) void wgrad3x3_kernel(const W3Args a) {
    constexpr int NT = KT == 4 ? 3 : 6;         // output tiles of a block
    constexpr int NTW = 3;                      // ... of a wave
    constexpr int KS = KT == 4 ? 8 : 4;         // k-tile stride of a wave
    constexpr int kCols = NT * 16;
    constexpr int W = 1 << LGW, TR = 64 / W, Q = W / 4 + 2, P = 4 * Q, U = (TR + 2) * Q;
    constexpr int kGDma = (NT * 4 + NW - 1) / NW;   // wave DMAs (4 rows each) per wave and tile: gy
    constexpr int kStageFloats = kXFloats + kCols * 64;
    constexpr int kStageBytes = kStageFloats * 4;
    static_assert(U <= 64 && KT * KS + 3 >= 27, "one wave DMA per channel; every k-tile has an owner");
    // LDS: stage 0, 1: x [48 channels] | gy [kCols][64]
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    const int k0 = KT == 4 ? wave : (wave & 3);             // first k-tile of this wave
    const int g0 = KT == 4 ? 0 : (wave >> 2) * NTW;         // first output tile of this wave
    const int nk = (27 - k0 + KS - 1) / KS;                 // its k-tiles: KT or KT - 1
    const int c0 = blockIdx.y * kCK;
    const int second = c0 >= a.C1 ? 1 : 0;                  // the chunk's source: chunks do not straddle (C1 % 48 == 0)
    const float *src = second ? a.x2 : a.x;
    const int Cs = second ? a.C2 : a.C1, cs0 = c0 - (second ? a.C1 : 0);
    const int co0 = blockIdx.z * kCols;
    const int plane = a.H * W;
    const int t_begin = blockIdx.x * a.tilesPerGroup;
    const int nt = min(a.nTiles, t_begin + a.tilesPerGroup) - t_begin;   // tiles of this group

    // x DMA: lane u -> halo row rl, chunk q: input columns 4q - 4 .. 4q - 1 of input row iy0 + rl
    const int rl = lane / Q, ql = lane - rl * Q;
    const int xcol = (lane < U && ql >= 1 && ql <= W / 4) ? (rl * W + 4 * ql - 4) * 4 : kXZero;
    // gy DMA: one wave instruction fills 4 rows; lane -> (row 4 gi + lq, swizzled chunk l15) <- pixels 4q .. 4q + 3 of
    // the tile, q = l15 ^ (row & 15).  Wave w stages row groups w + NW i; past the block's last group (NT = 3: 12 groups
    // for 16 slots) it stages one of the first groups again (the same bytes into the same place)
    int gv[kGDma], ggi[kGDma];
#pragma unroll
    for (int i = 0; i < kGDma; ++i) {
        int gi = wave + NW * i;
        if (gi >= NT * 4) gi -= NT * 4;
        const int r = 4 * gi + lq;
        ggi[i] = gi;
        gv[i] = (co0 + r < a.Cout) ? (r * plane + ((l15 ^ (r & 15)) << 2)) * 4 : kXZero;
    }

    // the cursor: the tile the next issue() stages.  All scalar, moved by arithmetic on 0 / 1 flags
    const int n0 = __builtin_amdgcn_readfirstlane(t_begin / a.tilesPerImg);
    int ty = __builtin_amdgcn_readfirstlane(t_begin - n0 * a.tilesPerImg);
    long xo = ((long)n0 * Cs + cs0) * plane + (long)(ty * TR - a.padT) * W;   // first halo row of the first channel
    long go = ((long)n0 * a.Cout + co0) * plane + ty * 64;
    int left = __builtin_amdgcn_readfirstlane(nt - 1);   // tiles of the group behind the cursor's
    const int xwrap = (Cs - 1) * plane, gwrap = (a.Cout - 1) * plane;   // (< 2^28: the host checks)
    auto advance = [&]() {
        const int more = left > 0 ? 1 : 0;
        const int wrap = (ty + 1 == a.tilesPerImg ? 1 : 0) & more;
        left -= more;
        ty = (ty + more) & (wrap - 1);
        xo += more * 64 + wrap * xwrap;
        go += more * 64 + wrap * gwrap;
    };
    const int chanStep = NW * plane * 4;        // bytes between the channels of consecutive DMAs of a wave
    auto issue = [&](int b) {
        const rsrc_t xr = make_rsrc(src + xo), gr = make_rsrc(a.gy + go);
        const int iy = ty * TR - a.padT + rl;
        const int xv = (unsigned)iy < (unsigned)a.H ? xcol : kXZero;
        float *xs = smem + b * kStageFloats;
        float *gs = xs + kXFloats;
#pragma unroll
        for (int i = 0; i < kXDma; ++i) {
            const int c = wave + NW * i;
            bdma16(xr, xv, wave * (plane * 4) + i * chanStep, xs + c * kCS + zoff(c));
        }
#pragma unroll
        for (int i = 0; i < kGDma; ++i) bdma16(gr, gv[i], 0, gs + ggi[i] * 256);
    };

    // operands.  A: k-tile t of this wave is tap (ky, kx) x channels 16 cb ..; the value of step (j, s) is the float at
    // ab[t] + stage + 4 ((16 j >> LGW) P + (16 j & (W - 1)) + s).  B: chunk (4j + lq) ^ l15 of this lane's row of output
    // tile g0 + n
    int ab[KT], boff[4];
    {
        const int lbase = lds_addr(smem) + (l15 * kCS + zoff(l15)) * 4 + 16 * lq;
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            const int kt = min(k0 + KS * t, 26);
            const int tap = kt / 3, cb = kt - 3 * tap, ky = tap / 3, kx = tap - 3 * ky;
            ab[t] = lbase + (cb * 16 * kCS + ky * P + kx - a.padL + 4) * 4;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            boff[j] = lds_addr(smem) + (kXFloats + (g0 * 16 + l15) * 64) * 4 + (((4 * j) ^ lq ^ l15) << 4);
    }
    f32x4 acc[KT][NTW];
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
        for (int n = 0; n < NTW; ++n) acc[t][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    // the tile loop, written once per k-tile count of a wave (a wave-uniform choice made once, as in the general kernel)
    auto tiles = [&](auto nkc) {
        constexpr int NK = decltype(nkc)::value;
        float a0[NK], a1[NK];
        f32x4 b0[NTW], b1[NTW];
        auto ldA = [&](float (&av)[NK], int so, int ks) {
            const int j = ks >> 2, s = ks & 3;
#pragma unroll
            for (int t = 0; t < NK; ++t) av[t] = lds_f(ab[t] + so)[((16 * j) >> LGW) * P + ((16 * j) & (W - 1)) + s];
        };
        auto ldB = [&](f32x4 (&bv)[NTW], int so, int j) {
#pragma unroll
            for (int n = 0; n < NTW; ++n) bv[n] = *(lds_c4p)(__SIZE_TYPE__)(unsigned)(boff[j] + so + n * (16 * 256));
        };
        auto mm = [&](const float (&av)[NK], const f32x4 (&bv)[NTW], int s) {
#pragma unroll
            for (int t = 0; t < NK; ++t)
#pragma unroll
                for (int n = 0; n < NTW; ++n)
                    acc[t][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], bv[n][s], acc[t][n], 0, 0, 0);
        };
        issue(0);
        advance();
        issue(1);
        advance();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        lds_only_barrier();
        ldA(a0, 0, 0);
        ldB(b0, 0, 0);
        for (int i = 0; i < nt; ++i) {
            const int so = (i & 1) * kStageBytes, son = kStageBytes - so;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j + 1 < 4) {
                    if (j & 1) ldB(b0, so, j + 1); else ldB(b1, so, j + 1);
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int ks = 4 * j + s;
                    if (ks + 1 < 16) {
                        if (ks & 1) ldA(a0, so, ks + 1); else ldA(a1, so, ks + 1);
                    }
                    if (ks == 15) {
                        ldA(a0, son, 0);
                        ldB(b0, son, 0);
                    }
                    if (ks & 1) {
                        if (j & 1) mm(a1, b1, s); else mm(a1, b0, s);
                    } else {
                        if (j & 1) mm(a0, b1, s); else mm(a0, b0, s);
                    }
                    if (ks == 14) {
                        // (behind the MFMAs of step 14 in program order: the wait for the operands of step 15 runs under
                        // them.)  This wave's part of tile i + 1 has landed (issued a tile ago); behind the barrier every
                        // wave's has, and every wave has fetched its last operands of tile i
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        lds_only_barrier();
                        issue(i & 1);
                        advance();
                    }
                }
            }
        }
        // the surplus DMAs: LDS is not released under them
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    if (nt > 0) {
        if (nk == KT)
            tiles(std::integral_constant<int, KT>{});
        else
            tiles(std::integral_constant<int, KT - 1>{});
    }

    // partial slab of this group: rows = c * 9 + tap, cols = output channel (64-byte runs per store).  D layout:
    // col = lane & 15, row = 4 lq + register
    float *dst = a.partial + (long)blockIdx.x * (a.C1 + a.C2) * 9 * a.CoutP;
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        const int kt = k0 + KS * t;
        if (kt >= 27) continue;
        const int tap = kt / 3, cb = kt - 3 * tap;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + cb * 16 + lq * 4 + j;
#pragma unroll
            for (int n = 0; n < NTW; ++n) dst[((long)c * 9 + tap) * a.CoutP + co0 + (g0 + n) * 16 + l15] = acc[t][n][j];
        }
    }
}

template <int KT, int LGW>
int launch3x3(const W3Args &a, dim3 grid, hipStream_t s) {
    constexpr size_t lds = 2 * (size_t)(kXFloats + (KT == 4 ? 3 : 6) * 16 * 64) * 4;
    if (int rc = sprk::lds_optin(wgrad3x3_kernel<KT, LGW>, lds, "wgrad3x3")) return rc;
    hipLaunchKernelGGL((wgrad3x3_kernel<KT, LGW>), grid, dim3(64 * NW), lds, s, a);
    return SPRK_OK;
}

template <int KT>
int launch3x3_w(const W3Args &a, int W, dim3 grid, hipStream_t s) {
    return W == 16 ? launch3x3<KT, 4>(a, grid, s) : W == 32 ? launch3x3<KT, 5>(a, grid, s) : launch3x3<KT, 6>(a, grid, s);
}

}  // namespace

namespace sprk {

std::atomic<long> g_wgrad3x3_launches{0};
std::atomic<int> g_wgrad3x3_on{1};

int wgrad3x3_run(const Wgrad3x3Call &c, hipStream_t s) {
    const int Cin = c.C1 + c.C2;
    const long plane = (long)c.H * c.W;
    SPRK_REQUIRE(wgrad3x3_plane(c.H, c.W) && (c.NT == 3 || c.NT == 6) && c.C1 > 0 && c.C1 % kCK == 0 && c.C2 % kCK == 0 &&
                     (c.C2 == 0 || c.x2) && c.nChunks == Cin / kCK && c.nblkN == cdiv(c.Cout, c.NT * 16) &&
                     c.CoutP == c.nblkN * c.NT * 16 && c.padT >= 0 && c.padT <= 2 && c.padL >= 0 && c.padL <= 2 &&
                     (long)std::max(c.C1, c.C2) * plane < (1L << 28) && (long)c.Cout * plane < (1L << 28) &&
                     c.nTiles == (long)c.N * (plane / 64) && c.tilesPerGroup >= 1 &&
                     c.groups == cdiv(c.nTiles, c.tilesPerGroup),
                 "wgrad3x3: call outside the kernel's limits");
    W3Args a{};
    a.x = c.x; a.x2 = c.x2; a.gy = c.gy; a.partial = c.partial;
    a.C1 = c.C1; a.C2 = c.C2; a.Cout = c.Cout; a.CoutP = c.CoutP; a.H = c.H; a.padT = c.padT; a.padL = c.padL;
    a.tilesPerImg = (int)(plane / 64); a.nTiles = c.nTiles; a.tilesPerGroup = c.tilesPerGroup;
    const dim3 grid(c.groups, c.nChunks, c.nblkN);
    if (int rc = c.NT == 3 ? launch3x3_w<4>(a, c.W, grid, s) : launch3x3_w<7>(a, c.W, grid, s)) return rc;
    g_wgrad3x3_launches.fetch_add(1, std::memory_order_relaxed);
    return SPRK_OK;
}

}  // namespace sprk
