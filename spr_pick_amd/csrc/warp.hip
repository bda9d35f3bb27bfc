// Local motion correction: sprk_align_warp (`joint align --patch`).
//
// One frame resampled through a smooth displacement field and written to, or added to, a running sum:
//   out(i, j) = src(i + sy(i, j), j + sx(i, j)) with periodic edges,   y = out when `first`, else y + out.
// The field is a quadratic per axis in the normalised coordinates of the pixel, its 6 + 6 coefficients kernel arguments:
//   u = fmaf((float)j, inv_nx, -0.5f),  v = fmaf((float)i, inv_ny, -0.5f),  uu = u * u,  uv = u * v,  vv = v * v;
//   s = c0;  s = fmaf(c1, u, s);  s = fmaf(c2, v, s);  s = fmaf(c3, uu, s);  s = fmaf(c4, uv, s);  s = fmaf(c5, vv, s);
//   s = fminf(fmaxf(s, -16.0f), 16.0f)   (a NaN, which only an overflow can make, becomes -16);
//   fl = floorf(s),  t = s - fl (exact, in [0, 1)),  tt = t * t;  the first tap is row i + (int)fl - 1;
//   w0 = fmaf(fmaf(-0.5f, t, 1.0f), t, -0.5f) * t,    w1 = fmaf(fmaf(1.5f, t, -2.5f), tt, 1.0f),
//   w2 = fmaf(fmaf(-1.5f, t, 2.0f), t, 0.5f) * t,     w3 = fmaf(0.5f, t, -0.5f) * tt               (Catmull-Rom);
//   r_a = fmaf chain from 0.0f over b = 0 .. 3 of wx_b * src((i0 - 1 + a) mod ny, (j0 - 1 + b) mod nx),  a = 0 .. 3;
//   out = fmaf chain from 0.0f over a = 0 .. 3 of wy_a * r_a.
// The fraction comes from the shift, not from the coordinate: the weights have all their bits at column 16000.  The clamp
// is what bounds the source region of a workgroup, whatever the coefficients hold.
//
// One workgroup of four waves per 64 x 64 output pixels.  Its source region, the tile and 18 pixels a side (the clamp's 16
// and the taps' 2), is staged once in LDS from wrapped addresses, a row of 100 consecutive floats per half workgroup and
// step, ten rows of a thread in flight at a time; a thread then has one column and 16 rows of the tile, reads its 16 taps from LDS (neighbouring lanes read
// neighbouring words: the field varies by a fraction of a pixel per pixel) and stores rows of 64 consecutive floats.
// No atomics, no host synchronisation, no workspace.
//
// Compiled with -ffp-contract=off (Makefile): the fmaf above are the only fused operations.
#include <cmath>
#include <cstdint>

#include "common.h"

namespace {

constexpr int kMaxSide = 16384;                  // ny * nx stays below 2^31
constexpr int kThreads = 256;
constexpr int kTile = 64;                        // output pixels a side per workgroup
constexpr int kHalo = 18;                        // |shift| <= 16, taps from -1 to +2 around its floor
constexpr int kRegion = kTile + 2 * kHalo;       // 100: staged source pixels a side
constexpr int kStageBatch = 10;                  // region rows a thread loads before it stores them: 50 = 5 batches
static_assert(kRegion % (2 * kStageBatch) == 0, "a thread stages whole batches");
constexpr float kClamp = 16.0f;

struct Field {
    float y[6], x[6];
};

__device__ __forceinline__ float shift_at(const float *c, float u, float v, float uu, float uv, float vv) {
    float s = c[0];
    s = __fmaf_rn(c[1], u, s);
    s = __fmaf_rn(c[2], v, s);
    s = __fmaf_rn(c[3], uu, s);
    s = __fmaf_rn(c[4], uv, s);
    s = __fmaf_rn(c[5], vv, s);
    return fminf(fmaxf(s, -kClamp), kClamp);
}

__device__ __forceinline__ void catmull_rom(float t, float w[4]) {
    const float tt = t * t;
    w[0] = __fmaf_rn(__fmaf_rn(-0.5f, t, 1.0f), t, -0.5f) * t;
    w[1] = __fmaf_rn(__fmaf_rn(1.5f, t, -2.5f), tt, 1.0f);
    w[2] = __fmaf_rn(__fmaf_rn(-1.5f, t, 2.0f), t, 0.5f) * t;
    w[3] = __fmaf_rn(0.5f, t, -0.5f) * tt;
}

// grid (ceil(nx / 64), ceil(ny / 64))
__global__ __launch_bounds__(kThreads) void align_warp_kernel(const float *__restrict__ src, int ny, int nx, float inv_ny,
                                                              float inv_nx, Field f, float *y, int first) {
    __shared__ float region[kRegion * kRegion];                // rows i0-18 .. i0+81, columns j0-18 .. j0+81, wrapped
    const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
    const int tid = threadIdx.x;

    // staging: a half workgroup per row, a thread keeps its column; both indices stay in 0 .. n-1 for every n >= 1
    const int k = tid & 127;
    if (k < kRegion) {
        int col = (j0 - kHalo + k) % nx;
        if (col < 0) col += nx;
        int row = (i0 - kHalo + (tid >> 7)) % ny;
        if (row < 0) row += ny;
        const int step = 2 % ny;
        // kStageBatch loads in flight per thread before the first is written to LDS: one round trip per batch, not per row
        for (int g = tid >> 7; g < kRegion; g += 2 * kStageBatch) {
            float v[kStageBatch];
#pragma unroll
            for (int b = 0; b < kStageBatch; ++b) {
                v[b] = src[(long)row * nx + col];
                row += step;
                if (row >= ny) row -= ny;
            }
#pragma unroll
            for (int b = 0; b < kStageBatch; ++b) region[(g + 2 * b) * kRegion + k] = v[b];
        }
    }
    __syncthreads();

    const int lj = tid & 63, j = j0 + lj;
    if (j >= nx) return;
    const float u = __fmaf_rn((float)j, inv_nx, -0.5f), uu = u * u;
    for (int li = tid >> 6; li < kTile; li += kThreads / 64) {
        const int i = i0 + li;
        if (i >= ny) break;
        const long at = (long)i * nx + j;
        float sum = 0.0f;
        if (!first) sum = y[at];                                 // asked for early, used last
        const float v = __fmaf_rn((float)i, inv_ny, -0.5f), uv = u * v, vv = v * v;
        const float sy = shift_at(f.y, u, v, uu, uv, vv), sx = shift_at(f.x, u, v, uu, uv, vv);
        const float fy = floorf(sy), fx = floorf(sx);
        float wy[4], wx[4];
        catmull_rom(sy - fy, wy);
        catmull_rom(sx - fx, wx);
        // rows li + 1 .. li + 36 and columns lj + 1 .. lj + 36 of the region at most: inside it for every field
        const float *p = region + (li + kHalo - 1 + (int)fy) * kRegion + (lj + kHalo - 1 + (int)fx);
        float val = 0.0f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            float r = 0.0f;
#pragma unroll
            for (int b = 0; b < 4; ++b) r = __fmaf_rn(wx[b], p[a * kRegion + b], r);
            val = __fmaf_rn(wy[a], r, val);
        }
        y[at] = first ? val : sum + val;
    }
}

}  // namespace

extern "C" int sprk_align_warp(const float *src, int ny, int nx, const float *cy, const float *cx, float *y, int first,
                               void *stream) {
    SPRK_REQUIRE(src && cy && cx && y, "align_warp: null pointer");
    SPRK_REQUIRE(1 <= ny && ny <= kMaxSide && 1 <= nx && nx <= kMaxSide, "align_warp: a %dx%d frame (both sides in 1..%d)", ny,
                 nx, kMaxSide);
    SPRK_REQUIRE(((uintptr_t)src & 3) == 0 && ((uintptr_t)y & 3) == 0, "align_warp: src and y must be 4-byte aligned");
    SPRK_REQUIRE(src != y, "align_warp: y must not be src (other workgroups read what one writes)");
    Field f;
    for (int k = 0; k < 6; ++k) {
        SPRK_REQUIRE(std::isfinite(cy[k]) && std::isfinite(cx[k]), "align_warp: coefficient %d is not finite (%g, %g)", k,
                     (double)cy[k], (double)cx[k]);
        f.y[k] = cy[k];
        f.x[k] = cx[k];
    }
    const dim3 grid(sprk::cdiv(nx, kTile), sprk::cdiv(ny, kTile));
    hipLaunchKernelGGL(align_warp_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, src, ny, nx, 1.0f / (float)ny,
                       1.0f / (float)nx, f, y, first);
    return sprk::check_launch("align_warp");
}
