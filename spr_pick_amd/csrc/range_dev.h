// The range of an image as order-preserving encodings of its min / max: every workgroup of a producing kernel leaves one
// Part, ingest_range_kernel reduces them (ingest.hip, resample.hip; contam.hip takes the encodings and the wave steps).
// No atomics, nothing to initialise.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int kRangeThreads = 256;

struct Part {
    unsigned int min_enc, max_enc;               // order-preserving encodings of one workgroup's min / max
};

__device__ __forceinline__ unsigned int enc(float f) {
    const unsigned int b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float dec(unsigned int e) {
    return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}
__device__ __forceinline__ unsigned int wave_min(unsigned int v) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned int)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ __forceinline__ unsigned int wave_max(unsigned int v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned int)__shfl_xor((int)v, o, 64));
    return v;
}

// the workgroup's min / max (all THREADS threads must call); thread 0 returns true and holds the pair in lo / hi
template <int THREADS>
__device__ __forceinline__ bool block_reduce(unsigned int &lo, unsigned int &hi) {
    __shared__ unsigned int red[2][THREADS / 64];
    lo = wave_min(lo);
    hi = wave_max(hi);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][wave] = lo;
        red[1][wave] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < THREADS / 64; ++w) {
            lo = min(lo, red[0][w]);
            hi = max(hi, red[1][w]);
        }
        return true;
    }
    return false;
}

// grid: one workgroup of THREADS (a template, so that a file that only takes the helpers above carries no kernel)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void ingest_range_kernel(const Part *__restrict__ parts, int nparts,
                                                               float *__restrict__ range) {
    unsigned int lo = 0xffffffffu, hi = 0u;
    for (int k = threadIdx.x; k < nparts; k += THREADS) {
        lo = min(lo, parts[k].min_enc);
        hi = max(hi, parts[k].max_enc);
    }
    if (block_reduce<THREADS>(lo, hi)) {
        range[0] = dec(lo);
        range[1] = dec(hi);
    }
}

}  // namespace
