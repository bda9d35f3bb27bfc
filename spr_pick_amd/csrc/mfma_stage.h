// Fetching and staging one chunk of K for the tiled fp32 GEMMs on v_mfma_f32_16x16x4_f32 whose K loop over one accumulator is
// a contract's fmaf chain (resample.hip, psd.hip).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int kKC = 64;                          // columns of K staged per chunk
constexpr int kLd = kKC + 2;                     // floats per staged row of an A operand (and of a row-major B^T operand)

// Fetching and zeroing are apart.  A fetch is an unconditional load from an address clamped into the part of its array
// that may be read, and nothing touches the value until the chunk is staged, two chunks later: only so are a chunk's loads
// in flight together and behind the MFMAs of the chunks before.  (With the load under a branch, or a select on its value
// next to it, the compiler waited for every load right behind its issue: one round trip to memory after the other.)
// Staging then turns every element outside the operand into a zero formed in registers.
// fetch4: the float4 at row min(row, rows-1), columns min(q, cols4-4) .. +3 (cols4 a multiple of 4, at least 4)
__device__ __forceinline__ float4 fetch4(const float *__restrict__ m, int ld, int rows, int cols4, int row, int q) {
    return *reinterpret_cast<const float4 *>(m + (long)min(row, rows - 1) * ld + min(q, cols4 - 4));
}
// zero4: the elements at K positions q .. q+3 that lie at or past `end`, or all four unless `in`, become zeros
__device__ __forceinline__ float4 zero4(float4 v, bool in, int q, int end) {
    return make_float4(in && q < end ? v.x : 0.0f, in && q + 1 < end ? v.y : 0.0f, in && q + 2 < end ? v.z : 0.0f,
                       in && q + 3 < end ? v.w : 0.0f);
}

// a float4 into a staged row of kLd floats (8-byte aligned: kLd is even)
__device__ __forceinline__ void stage4(float *d, float4 v) {
    *reinterpret_cast<float2 *>(d) = make_float2(v.x, v.y);
    *reinterpret_cast<float2 *>(d + 2) = make_float2(v.z, v.w);
}

}  // namespace
