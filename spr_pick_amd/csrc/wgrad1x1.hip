// The backward-weight of the wide 1x1 layers of the U-Nets' heads (384 -> 384, 384 -> 96 at 64 x 64) as a streaming kernel.
//
//   partial[group][k][co] = sum over the group's 64-pixel tiles, in order, of  x[k][pixel] * gy[pixel][co]
//
// The sums are conv_wgrad_mfma_kernel<3, 6, 2, 1>'s (conv.hip: wgrad_tile), operation for operation, on plan_wgrad's
// split: every element has ONE accumulator that starts at 0 and takes, per tile, 16 v_mfma_f32_16x16x4_f32 in the order
// of the k-steps 4j + s, x in the A operand (row = reduced channel k) and gy in the B operand, lane group lq holding
// pixel 16j + 4lq + s of the tile.  The slab layout [group][k][CoutP] and the reduction that follows are unchanged.
//
// What differs is everything around the MFMAs.  The predicate (conv.hip: wgrad1x1_takes) admits only planes whose
// 64-pixel tiles are 64 consecutive floats, so a tile is "the next 64 floats of every row": the DMA runs from a scalar
// cursor (two 64-bit offsets and a tile-in-image counter) with loop-invariant per-lane offsets, no divisions, no range
// tests and no tables.  Eight waves, two per SIMD; wave (wi, wj) owns k-tiles wi, wi + 4, wi + 8 x output tiles 3 wj ..
// 3 wj + 2 (36 accumulator registers), as in the general kernel.  Both operands are staged as the general kernel stages
// them (rows of 64 floats whose 16-byte chunks are XOR-swizzled by row & 15), so the four values a lane needs for steps
// 4j .. 4j + 3 are ONE 16-byte chunk of its row, for x as for gy: 6 ds_read_b128 per 36 MFMAs and no bank conflict (the
// general kernel reads x by ds_read_b32, 48 per tile and wave, and those conflict).  Two operand register sets: the chunks
// of j + 1 are fetched under the MFMAs of j.  Two LDS stages of 72 KB (192 x rows + 96 gy rows).  One barrier per tile,
// LDS-only, placed after the LAST operand fetch of tile i (in front of the MFMAs of j = 3): behind it every wave is done
// reading stage i & 1, so the DMA of tile i + 2 goes out into it between those MFMAs, and tile i + 1 (whose DMA was
// issued a whole tile earlier and is waited for by one vmcnt in front of the barrier) is published, so its first chunks
// are fetched under the same MFMAs: no wave waits for LDS latency at the head of a tile.  After the last tile the cursor
// stays where it is: the surplus DMAs re-read the last tile into a stage nobody reads (no branch in the loop).
#include "wgrad1x1.h"

#include "conv_dev.h"

namespace {

constexpr int kRows = sprk::kWgrad1x1Rows;          // x rows of a stage
constexpr int kCols = 96;                           // gy rows of a stage (6 output tiles)
constexpr int kStageFloats = (kRows + kCols) * 64;
constexpr int kStageBytes = kStageFloats * 4;
static_assert(kRows % 64 == 0 && kCols == 96, "three k-tiles per wave, six output tiles");
// Two waves per SIMD.  The same loop on four waves, each owning 3 k-tiles x all 6 output tiles (72 accumulators, 9
// operand reads per 72 MFMAs), was built first and measured slower: with nothing else on its SIMD a wave's waits at the
// barrier and for its operands are exposed
constexpr int WJ = 2;
constexpr int NW = 4 * WJ;                      // waves
constexpr int NTW = 6 / WJ;                     // output tiles per wave
constexpr int kXDma = kRows / (4 * NW);         // 16-byte wave DMAs (4 rows each) per wave and tile: x
constexpr int kGDma = kCols / (4 * NW);         // ... gy

struct W1Args {
    const float *x, *gy;
    float *partial;
    int Cin, Cout, CoutP, plane;
    int tilesPerImg, nTiles, tilesPerGroup, CKW;
};

typedef const __attribute__((address_space(3))) f32x4 *lds_c4p;

__global__ __launch_bounds__(256 * WJ) void wgrad1x1_kernel(const W1Args a) {
    // LDS: stage 0, 1: x [kRows][64] | gy [kCols][64]
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    const int wi = wave & 3, wj = wave >> 2;
    const int c0 = blockIdx.y * a.CKW;
    const int cke = min(a.CKW, a.Cin - c0);
    const int co0 = blockIdx.z * kCols;
    const int t_begin = blockIdx.x * a.tilesPerGroup;
    const int nt = min(a.nTiles, t_begin + a.tilesPerGroup) - t_begin;   // tiles of this group

    // DMA: one wave instruction fills 4 rows; lane -> (row 4 gi + lq, swizzled chunk l15) <- pixels 4q .. 4q + 3 of the
    // tile, q = l15 ^ (row & 15).  Wave w stages row groups gi = w + NW i: row & 15 = (4w + lq) & 15 for every i, so the
    // lane's offset against (first row of the chunk, first pixel of the tile) is the same for every i but for the 4 NW i
    // rows that go into the scalar offset.  Rows past the chunk's or the layer's end are zero-filled (offset out of range)
    int xv[kXDma], gv[kGDma];
    {
        const int r = 4 * wave + lq;
        const int vo = (r * a.plane + ((l15 ^ (r & 15)) << 2)) * 4;
#pragma unroll
        for (int i = 0; i < kXDma; ++i) xv[i] = (r + 4 * NW * i < cke) ? vo : kXZero;
#pragma unroll
        for (int i = 0; i < kGDma; ++i) gv[i] = (co0 + r + 4 * NW * i < a.Cout) ? vo : kXZero;
    }
    const int rowStep = 4 * NW * a.plane * 4;   // bytes between the rows of consecutive DMAs of a wave

    // the cursor: the tile the next issue() stages.  All scalar, and moved by arithmetic on 0 / 1 flags (a select of
    // 64-bit values is compiled into a branch, which would cut the tile loop's scheduling region in two)
    const int n0 = __builtin_amdgcn_readfirstlane(t_begin / a.tilesPerImg);
    int tt = __builtin_amdgcn_readfirstlane(t_begin - n0 * a.tilesPerImg);
    long xo = ((long)n0 * a.Cin + c0) * a.plane + tt * 64;
    long go = ((long)n0 * a.Cout + co0) * a.plane + tt * 64;
    int left = __builtin_amdgcn_readfirstlane(nt - 1);   // tiles of the group behind the cursor's
    const int xwrap = (a.Cin - 1) * a.plane, gwrap = (a.Cout - 1) * a.plane;   // (< 2^28: the host checks)
    auto advance = [&]() {
        const int more = left > 0 ? 1 : 0;
        const int wrap = (tt + 1 == a.tilesPerImg ? 1 : 0) & more;
        left -= more;
        tt = (tt + more) & (wrap - 1);
        xo += more * 64 + wrap * xwrap;
        go += more * 64 + wrap * gwrap;
    };
    auto issue = [&](int b) {
        const rsrc_t xr = make_rsrc(a.x + xo), gr = make_rsrc(a.gy + go);
        float *xs = smem + b * kStageFloats + wave * 256;
        float *gs = xs + kRows * 64;
#pragma unroll
        for (int i = 0; i < kXDma; ++i) bdma16(xr, xv[i], i * rowStep, xs + i * (NW * 256));
#pragma unroll
        for (int i = 0; i < kGDma; ++i) bdma16(gr, gv[i], i * rowStep, gs + i * (NW * 256));
    };

    // operands: chunk (4j + lq) ^ l15 of this lane's row, l15 of k-tile wi + 4t (x) / of output tile NTW wj + n (gy)
    int aoff[4], boff[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = ((4 * j) ^ lq ^ l15) << 4;
        aoff[j] = lds_addr(smem) + (wi * 16 + l15) * 256 + q;
        boff[j] = lds_addr(smem) + (kRows + wj * (NTW * 16) + l15) * 256 + q;
    }
    auto ld = [&](f32x4 (&av)[3], f32x4 (&bv)[NTW], int so, int j) {
#pragma unroll
        for (int t = 0; t < 3; ++t) av[t] = *(lds_c4p)(__SIZE_TYPE__)(unsigned)(aoff[j] + so + t * (64 * 256));
#pragma unroll
        for (int n = 0; n < NTW; ++n) bv[n] = *(lds_c4p)(__SIZE_TYPE__)(unsigned)(boff[j] + so + n * (16 * 256));
    };
    f32x4 acc[3][NTW];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int n = 0; n < NTW; ++n) acc[t][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto mm = [&](const f32x4 (&av)[3], const f32x4 (&bv)[NTW]) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int n = 0; n < NTW; ++n)
                    acc[t][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][s], bv[n][s], acc[t][n], 0, 0, 0);
    };

    if (nt > 0) {
        f32x4 a0[3], b0[NTW], a1[3], b1[NTW];
        issue(0);
        advance();
        issue(1);
        advance();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        lds_only_barrier();
        ld(a0, b0, 0, 0);
        for (int i = 0; i < nt; ++i) {
            const int so = (i & 1) * kStageBytes, son = kStageBytes - so;
            ld(a1, b1, so, 1);
            mm(a0, b0);
            ld(a0, b0, so, 2);
            mm(a1, b1);
            ld(a1, b1, so, 3);
            mm(a0, b0);
            // this wave's part of tile i + 1 has landed (issued a tile ago); behind the barrier every wave's has, and
            // every wave has fetched its last operands of tile i
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            lds_only_barrier();
            ld(a0, b0, son, 0);
            issue(i & 1);
            advance();
            mm(a1, b1);
            // the operand reads first, then the DMAs spread over the MFMAs: issued as a block in front of the MFMAs they
            // would leave the pipe idle for their whole length, once per tile
#pragma unroll
            for (int k = 0; k < 3 + NTW; ++k) {
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);   // MFMA
            }
#pragma unroll
            for (int k = 0; k < kXDma + kGDma; ++k) {
                __builtin_amdgcn_sched_group_barrier(0x008, (12 * NTW - 2 * (3 + NTW)) / (kXDma + kGDma), 0);   // MFMA
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                                               // VMEM
            }
        }
        // the surplus DMAs: LDS is not released under them
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }

    // partial slab of this group: rows = reduced channel, cols = output channel (64-byte runs per store).  D layout:
    // col = lane & 15, row = 4 lq + register
    float *dst = a.partial + (long)blockIdx.x * a.Cin * a.CoutP;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = (wi + 4 * t) * 16 + lq * 4 + j;
            if (k >= cke) continue;
#pragma unroll
            for (int n = 0; n < NTW; ++n) dst[(long)(c0 + k) * a.CoutP + co0 + (wj * NTW + n) * 16 + l15] = acc[t][n][j];
        }
    }
}

}  // namespace

namespace sprk {

std::atomic<long> g_wgrad1x1_launches{0};
std::atomic<int> g_wgrad1x1_on{1};

int wgrad1x1_run(const Wgrad1x1Call &c, hipStream_t s) {
    SPRK_REQUIRE(c.plane >= 64 && c.plane % 64 == 0 && c.CKW >= 1 && c.CKW <= kRows && c.nChunks == cdiv(c.Cin, c.CKW) &&
                     c.nblkN == cdiv(c.Cout, kCols) && c.CoutP == c.nblkN * kCols && (long)kRows * c.plane * 4 < (1L << 31) &&
                     (long)c.Cin * c.plane < (1L << 28) && (long)c.Cout * c.plane < (1L << 28) &&
                     c.nTiles == (long)c.N * (c.plane / 64) && c.tilesPerGroup >= 1 &&
                     c.groups == cdiv(c.nTiles, c.tilesPerGroup),
                 "wgrad1x1: call outside the kernel's limits");
    W1Args a{};
    a.x = c.x; a.gy = c.gy; a.partial = c.partial;
    a.Cin = c.Cin; a.Cout = c.Cout; a.CoutP = c.CoutP; a.plane = c.plane;
    a.tilesPerImg = c.plane / 64; a.nTiles = c.nTiles; a.tilesPerGroup = c.tilesPerGroup; a.CKW = c.CKW;
    const size_t lds = 2 * (size_t)kStageBytes;
    if (int rc = lds_optin(wgrad1x1_kernel, lds, "wgrad1x1")) return rc;
    hipLaunchKernelGGL(wgrad1x1_kernel, dim3(c.groups, c.nChunks, c.nblkN), dim3(256 * WJ), lds, s, a);
    g_wgrad1x1_launches.fetch_add(1, std::memory_order_relaxed);
    return SPRK_OK;
}

}  // namespace sprk
