// Raw detector movies in: sprk_movie_correct (`joint align --gain / --dark / --defects / --hot_sigma`).
//
// One frame per launch: the samples decoded to fp32, minus the dark reference, times the gain reference, and every pixel the
// fix map marks replaced by the mean of the good pixels around it.  Per pixel p = (y, x), d the sample as fp32:
//   c(p) = d;  with dark: c = d - dark[p] (one fp32 subtraction);  with gain: c = c * gain[p] (one fp32 multiplication);
//   fix[p] == 0 (or no fix map):  out[p] = c(p);
//   fix[p] == r > 0:              r = min(r, SPRK_FIX_MAX_RADIUS); over the window of rows max(0, y-r) .. min(ny-1, y+r) and the
//                                 same for the columns, in row-major order, over the pixels q with fix[q] == 0:
//                                 S = S + c(q) from 0.0f, n their count; out[p] = S / (float)n, or 0.0f when n == 0;
//   with sum:                     sum[p] = out[p] when `first`, else sum[p] + out[p].
// Nothing is fused (the file is built with -ffp-contract=off) and the division is the correctly rounded one.  The window
// recomputes c(q) from raw, gain and dark, so a frame is finished in one launch and a bad pixel's own sample, gain or dark
// reaches no output, whatever it holds.
//
// The fast path takes the frame as ny*nx pixels in a row: a thread has four consecutive ones, with one load of 4 / 8 / 16
// bytes for the samples, one of 4 bytes for the fix map and 16-byte loads and stores for gain, dark, out and sum; the
// threads after the last whole group take the ny*nx % 4 pixels of the tail one by one.  The window is per pixel and
// divergent: bad pixels are 1e-4 .. 1e-2 of a frame.  No atomics, no host synchronisation.
#include <cstdint>

#include "common.h"
#include "mrc_host.h"

namespace {

constexpr int kMaxSide = 16384;                  // ny * nx stays below 2^31
constexpr int kThreads = 256;

__device__ __forceinline__ float corrected(float d, const float *__restrict__ gain, const float *__restrict__ dark, long p) {
    float c = d;
    if (dark) c = c - dark[p];
    if (gain) c = c * gain[p];
    return c;
}

// the replacement of pixel p, whose fix value is r > 0
template <typename T>
__device__ float window_mean(const T *__restrict__ raw, const float *__restrict__ gain, const float *__restrict__ dark,
                             const uint8_t *__restrict__ fix, int ny, int nx, long p, int r) {
    r = min(r, SPRK_FIX_MAX_RADIUS);
    const int y = (int)(p / nx), x = (int)(p - (long)y * nx);
    const int y0 = max(0, y - r), y1 = min(ny - 1, y + r), x0 = max(0, x - r), x1 = min(nx - 1, x + r);
    float S = 0.0f;
    int n = 0;
    for (int yy = y0; yy <= y1; ++yy)
        for (int xx = x0; xx <= x1; ++xx) {
            const long q = (long)yy * nx + xx;
            if (fix[q] == 0) {
                S = S + corrected((float)raw[q], gain, dark, q);
                ++n;
            }
        }
    return n ? S / (float)n : 0.0f;
}

// grid ceil((ny*nx / 4 + ny*nx % 4) / kThreads)
template <typename T>
__global__ __launch_bounds__(kThreads) void movie_correct_kernel(const T *__restrict__ raw, int ny, int nx,
                                                                 const float *__restrict__ gain,
                                                                 const float *__restrict__ dark,
                                                                 const uint8_t *__restrict__ fix, float *out, float *sum,
                                                                 int first) {
    typedef T T4 __attribute__((ext_vector_type(4)));
    const long n = (long)ny * nx, n4 = n >> 2;
    const long t = (long)blockIdx.x * kThreads + threadIdx.x;
    if (t < n4) {
        const long p = t * 4;
        const T4 v = *reinterpret_cast<const T4 *>(raw + p);
        float c[4] = {(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
        if (dark) {
            const float4 k = *reinterpret_cast<const float4 *>(dark + p);
            c[0] = c[0] - k.x; c[1] = c[1] - k.y; c[2] = c[2] - k.z; c[3] = c[3] - k.w;
        }
        if (gain) {
            const float4 g = *reinterpret_cast<const float4 *>(gain + p);
            c[0] = c[0] * g.x; c[1] = c[1] * g.y; c[2] = c[2] * g.z; c[3] = c[3] * g.w;
        }
        if (fix) {
            const uint32_t f = *reinterpret_cast<const uint32_t *>(fix + p);
            if (f) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = (f >> (8 * e)) & 255;
                    if (r) c[e] = window_mean(raw, gain, dark, fix, ny, nx, p + e, r);
                }
            }
        }
        if (sum) {
            if (!first) {
                const float4 s = *reinterpret_cast<const float4 *>(sum + p);
                *reinterpret_cast<float4 *>(sum + p) = make_float4(s.x + c[0], s.y + c[1], s.z + c[2], s.w + c[3]);
            } else {
                *reinterpret_cast<float4 *>(sum + p) = make_float4(c[0], c[1], c[2], c[3]);
            }
        }
        *reinterpret_cast<float4 *>(out + p) = make_float4(c[0], c[1], c[2], c[3]);
    } else if (t < n4 + (n & 3)) {
        const long p = n4 * 4 + (t - n4);
        const int r = fix ? fix[p] : 0;
        const float c = r ? window_mean(raw, gain, dark, fix, ny, nx, p, r) : corrected((float)raw[p], gain, dark, p);
        if (sum) sum[p] = first ? c : sum[p] + c;
        out[p] = c;
    }
}

template <typename T>
int launch(const void *raw, int ny, int nx, const float *gain, const float *dark, const uint8_t *fix, float *out, float *sum,
           int first, hipStream_t s) {
    const long n = (long)ny * nx;
    hipLaunchKernelGGL(movie_correct_kernel<T>, dim3(sprk::cdiv((n >> 2) + (n & 3), kThreads)), dim3(kThreads), 0, s,
                       (const T *)raw, ny, nx, gain, dark, fix, out, sum, first);
    return sprk::check_launch("movie_correct");
}

}  // namespace

extern "C" int sprk_movie_correct(const void *raw, int mode, int ny, int nx, const float *gain, const float *dark,
                                  const uint8_t *fix, float *out, float *sum, int first, void *stream) {
    SPRK_REQUIRE(raw && out, "movie_correct: null pointer (raw and out are needed)");
    SPRK_REQUIRE_MRC_MODE("movie_correct", mode);
    SPRK_REQUIRE(1 <= ny && ny <= kMaxSide && 1 <= nx && nx <= kMaxSide, "movie_correct: a %dx%d frame (both sides in 1..%d)", ny,
                 nx, kMaxSide);
    SPRK_REQUIRE(sprk::aligned16(raw, gain, dark, fix, out, sum),
                 "movie_correct: the samples, the references, the fix map, the output and the sum must start 16-byte aligned");
    SPRK_REQUIRE(out != raw && out != gain && out != dark && out != sum,
                 "movie_correct: out must not be raw, gain, dark or sum (the windows read them while out is written)");
    hipStream_t s = (hipStream_t)stream;
    return dispatch_mrc(mode, [&](auto t) { return launch<decltype(t)>(raw, ny, nx, gain, dark, fix, out, sum, first, s); });
}
