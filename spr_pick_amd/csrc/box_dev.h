// What the per-particle workgroups of extract.hip and extractfilter.hip share: the workgroup sum in a fixed order, the
// zeros of a box that is not written, and the background normalisation of a box of Y that lies in memory.  Not part of
// the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace {

constexpr int kBoxThreads = 256;                 // threads of a workgroup that owns one particle
constexpr int kBoxWaves = kBoxThreads / 64;
constexpr int kBoxUnroll = 8;                    // pixels of Y a lane of normalize_box has in flight

// the workgroup's sum in a fixed order, returned to every thread (all threads must call); red: kBoxWaves slots
template <typename S>
__device__ __forceinline__ S block_sum(S v, S *red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    S t = red[0];
    for (int w = 1; w < kBoxWaves; ++w) t += red[w];
    __syncthreads();                            // red is used again
    return t;
}

__device__ __forceinline__ void zero_box(float *__restrict__ o, int npix, int *__restrict__ status, int code) {
    for (int e = threadIdx.x; e < npix; e += kBoxThreads) o[e] = 0.0f;
    if (threadIdx.x == 0) *status = code;
}

// The normalised output of one particle from its Y [S, S] at o, in place, by the whole workgroup (all threads must call,
// after a barrier that makes Y visible): background = {(i - S/2)^2 + (j - S/2)^2 > R2}, n pixels; mean = sum_bg Y / n and
// var = sum_bg (Y - mean)^2 / n in double, block_sum's fixed order; out = float((double(Y) - mean) / sqrt(var)), negated
// with invert, status 0; n == 0 or !(var > 0): zeros and status 2.  inv_s = 1.0f / S; red: kBoxWaves slots of 8 bytes.
__device__ __forceinline__ void normalize_box(float *__restrict__ o, int S, float inv_s, long R2, bool invert,
                                              int *__restrict__ status, void *red) {
    const int npix = S * S, c = S / 2, tid = threadIdx.x;
    auto is_bg = [&](int e) {
        const int i = fast_div(e, inv_s), j = e - i * S;       // exact: e < 2^20 (common.h)
        return (long)((i - c) * (i - c) + (j - c) * (j - c)) > R2;
    };
    int n = 0;
    double s = 0.0;
    // f(e, Y[e]) for this thread's pixels e = tid, tid + kBoxThreads, ... in ascending order, kBoxUnroll loads in flight
    // (one at a time, a pass is S*S / kBoxThreads dependent round trips to L2: 48 of them at S = 64 cost more than a GEMM)
    auto for_each_y = [&](auto f) {
        for (int e0 = tid; e0 < npix; e0 += kBoxUnroll * kBoxThreads) {
            float v[kBoxUnroll];
#pragma unroll
            for (int u = 0; u < kBoxUnroll; ++u) v[u] = e0 + u * kBoxThreads < npix ? o[e0 + u * kBoxThreads] : 0.0f;
#pragma unroll
            for (int u = 0; u < kBoxUnroll; ++u)
                if (e0 + u * kBoxThreads < npix) f(e0 + u * kBoxThreads, v[u]);
        }
    };
    for_each_y([&](int e, float y) {
        if (is_bg(e)) {
            s += (double)y;
            ++n;
        }
    });
    n = block_sum(n, reinterpret_cast<int *>(red));
    if (n == 0) {
        zero_box(o, npix, status, 2);
        return;
    }
    const double mean = block_sum(s, reinterpret_cast<double *>(red)) / (double)n;
    double q = 0.0;
    for_each_y([&](int e, float y) {
        if (is_bg(e)) {
            const double t = (double)y - mean;
            q += t * t;
        }
    });
    const double var = block_sum(q, reinterpret_cast<double *>(red)) / (double)n;
    if (!(var > 0.0)) {                                        // the same bits in every lane: a uniform branch
        zero_box(o, npix, status, 2);
        return;
    }
    const double sd = sqrt(var);
    for_each_y([&](int e, float y) {
        const float r = (float)(((double)y - mean) / sd);
        o[e] = invert ? -r : r;
    });
    if (tid == 0) *status = 0;
}

}  // namespace
