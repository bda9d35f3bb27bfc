// Dynamic loss scaling on the device (graph_step.LossScaler): the unscale + non-finite check of the flat gradient and
// the GradScaler schedule.  Every value lives in device memory and nothing synchronises with the host, so the
// scaler's tail (unscale, skip-aware Adam in elem.hip, schedule) costs three launches and no host round trip.
#include "common.h"

#include <algorithm>

namespace {

// exponent bits all set: +-inf or NaN.  A bit test, not isfinite(): no fast-math flag can fold it away.
__device__ __forceinline__ int nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// x[0 .. n) *= inv_scale[0] in place; *flag |= 1 when a result is +-inf or NaN.
// x + head is 16-byte aligned (head < 4); n4 float4s follow it; the head and the tail (< 4 elements each) are
// handled by the first threads of the grid.  The flag is raised by at most ONE atomic per workgroup, after a
// workgroup-wide OR of the threads' findings.
__global__ __launch_bounds__(256) void unscale_check_kernel(float *__restrict__ x, long n, long head, long n4,
                                                            const float *__restrict__ inv_scale,
                                                            int *__restrict__ flag) {
    const float s = inv_scale[0];
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
    int bad = 0;
    float4 *x4 = reinterpret_cast<float4 *>(x + head);
    for (long i = tid; i < n4; i += stride) {
        float4 v = x4[i];
        v.x *= s; v.y *= s; v.z *= s; v.w *= s;
        bad |= nonfinite(v.x) | nonfinite(v.y) | nonfinite(v.z) | nonfinite(v.w);
        x4[i] = v;
    }
    const long tail0 = head + 4 * n4, edge = head + (n - tail0);
    if (tid < edge) {
        const long e = tid < head ? tid : tail0 + (tid - head);
        const float v = x[e] * s;
        bad |= nonfinite(v);
        x[e] = v;
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(flag, 1);
}

// torch.amp.GradScaler's rule (_amp_update_scale_): a non-finite step backs the scale off and restarts the count of
// clean steps; `interval` clean steps in a row grow it (unless the grown scale would be infinite).  The step's flag
// is only read here; the flag of the NEXT step (the other half of the double buffer) is cleared.
__global__ void scale_update_kernel(float *__restrict__ scale, float *__restrict__ inv_scale, int *__restrict__ tracker,
                                    int *__restrict__ skipped, const int *__restrict__ found, int *__restrict__ next_found,
                                    float growth, float backoff, int interval) {
    if (threadIdx.x != 0) return;
    float sc = scale[0];
    int t = tracker[0];
    if (found[0] != 0) {
        sc *= backoff;
        t = 0;
        skipped[0] += 1;
    } else if (++t >= interval) {
        const float grown = sc * growth;
        if (!nonfinite(grown)) sc = grown;
        t = 0;
    }
    scale[0] = sc;
    inv_scale[0] = 1.f / sc;
    tracker[0] = t;
    next_found[0] = 0;
}

}  // namespace

extern "C" {

int sprk_unscale_check(float *x, long n, const float *inv_scale, int *found_nonfinite, void *stream) {
    SPRK_REQUIRE(x && n > 0 && inv_scale && found_nonfinite && ((uintptr_t)x & 3) == 0, "unscale_check: bad arguments");
    const long head = std::min<long>(n, (long)((16 - ((uintptr_t)x & 15)) & 15) / 4);
    const long n4 = (n - head) / 4, edge = n - 4 * n4;
    hipLaunchKernelGGL(unscale_check_kernel, dim3(sprk::ew_blocks(std::max(n4, edge))), dim3(256), 0,
                       (hipStream_t)stream, x, n, head, n4, inv_scale, found_nonfinite);
    return sprk::check_launch("unscale_check");
}

int sprk_loss_scale_update(float *scale, float *inv_scale, int *growth_tracker, int *skipped,
                           const int *found_nonfinite, int *next_found, float growth, float backoff, int interval,
                           void *stream) {
    SPRK_REQUIRE(scale && inv_scale && growth_tracker && skipped && found_nonfinite && next_found &&
                 (const int *)next_found != found_nonfinite && interval > 0 && growth > 0.f && backoff > 0.f,
                 "loss_scale_update: bad arguments");
    hipLaunchKernelGGL(scale_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, scale, inv_scale, growth_tracker,
                       skipped, found_nonfinite, next_found, growth, backoff, interval);
    return sprk::check_launch("loss_scale_update");
}

}  // extern "C"
