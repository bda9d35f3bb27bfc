// Internal helpers shared by the libsprk.so translation units (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/sprk.h"

namespace sprk {

void set_error(const char *fmt, ...);
extern std::atomic<long> g_launches, g_wino_launches, g_mask1x1_launches;
// wino_wgrad_stream_kernel (wino.hip): calls it ran, and its host switch (sprk_wino_wgrad_stream_*)
extern std::atomic<long> g_wino_wgrad_stream_launches;
extern std::atomic<int> g_wino_wgrad_stream_on;

// event bracketing of the MFMA convolution launches (sprk_prof_*)
void prof_begin(int kclass, double flops, hipStream_t s);
void prof_end(int kclass, hipStream_t s);
void prof_bytes(double bytes);   // algorithmic HBM bytes of the launch opened by prof_begin (HBM-bound kernel classes)

// Per-DEVICE facts and one-time set-up (a process may drive any device; nothing here is per process):
// compute units of the calling thread's current device (persistent kernels launch one workgroup per CU)
int num_cus();
// allow a kernel `bytes` of dynamic LDS on the current device, before every launch that asks for them (core.hip);
// what: the kernel family the error text names
int lds_optin(const void *kernel, size_t bytes, const char *what);
template <typename K>
int lds_optin(K *kernel, size_t bytes, const char *what) {
    return lds_optin(reinterpret_cast<const void *>(kernel), bytes, what);
}

inline int check_launch(const char *what) {
    g_launches.fetch_add(1, std::memory_order_relaxed);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return SPRK_ELAUNCH;
    }
    return SPRK_OK;
}

// SPRK_EWORKSPACE (and the error text) when the caller's workspace is missing or shorter than `need`
inline int check_ws(const char *who, const void *ws, size_t ws_bytes, size_t need) {
    if (ws && ws_bytes >= need) return SPRK_OK;
    set_error("%s: workspace %zu < %zu", who, ws_bytes, need);
    return SPRK_EWORKSPACE;
}

// second-stage sums (sprk_reduce_items); item == nullptr in the callers below means "finish now"
int reduce_items(const sprk_reduce_item *items, int n, hipStream_t s);
inline int finish_or_defer(const sprk_reduce_item &it, sprk_reduce_item *out, hipStream_t s) {
    if (out) {
        *out = it;
        return SPRK_OK;
    }
    return it.kind == SPRK_RED_NONE ? (int)SPRK_OK : reduce_items(&it, 1, s);
}

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
inline int roundup(int a, int b) { return (a + b - 1) / b * b; }
__host__ __device__ constexpr int roundup4(int n) { return (n + 3) & ~3; }   // K and row strides of the fp32 MFMA stages
inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }   // workspace parts start 16-byte aligned
// every one of the pointers starts 16-byte aligned (a null pointer does)
template <typename... P>
bool aligned16(const P *...p) {
    return ((... | (uintptr_t)p) & 15) == 0;
}
inline int pow2_ceil(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}
inline int ilog2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

#define SPRK_REQUIRE(cond, ...)                \
    do {                                       \
        if (!(cond)) {                         \
            sprk::set_error(__VA_ARGS__);      \
            return SPRK_EINVAL;                \
        }                                      \
    } while (0)

// grid-stride launch size for HBM-bound elementwise kernels (guide: cap ~2048 blocks)
inline int ew_blocks(long n, int threads = 256) {
    long b = (n + threads - 1) / threads;
    if (b > 4096) b = 4096;
    if (b < 1) b = 1;
    return (int)b;
}

// algorithmic (direct-convolution) FLOPs of a layer: the same for its forward, backward-data and backward-weight call
inline double conv_flops(const sprk_conv_geom &g) {
    return 2.0 * g.N * g.Hout * g.Wout * (double)g.Cout * (g.C1 + g.C2) * g.KH * g.KW;
}

}  // namespace sprk

// XCD-aware start slot of a persistent workgroup.  Workgroups are dispatched round-robin over the 8 XCDs (id % 8), each
// with its own L2; work items that share input rows (spatially adjacent tiles / regions) should therefore go to
// workgroups of the SAME XCD.  With the workgroups walking items  slot + t * nwg  (t = 0, 1, ...), slot = xcd_slot(id)
// gives XCD k the contiguous items [k * nwg / 8, (k + 1) * nwg / 8) of every round instead of every 8th item.
__device__ __forceinline__ int xcd_slot(int id, int nwg, int on) {
    if (!on || (nwg & 7)) return id;
    return (id & 7) * (nwg >> 3) + (id >> 3);
}
namespace sprk {
// Every environment variable the library reads goes through these two, and both are alive only in a library built with
// -DSPRK_DIAG (make DIAG=1); the shipped libsprk.so ignores the variables, so an inherited environment cannot corrupt a
// run.
// Selection and sweep knobs (SPRK_WINO, SPRK_CONV16, SPRK_FWD_NTBLK, SPRK_XCD, ...): which kernel takes a call and how
// it is tiled, hence the summation order of the result.
inline int knob_env(const char *name, int dflt) {
#ifdef SPRK_DIAG
    const char *v = getenv(name);
    return v ? atoi(v) : dflt;
#else
    (void)name;
    return dflt;
#endif
}
// Timing experiments that switch phases of a kernel OFF (the results are then wrong on purpose: SPRK_WG_DIAG,
// SPRK_C16_DIAG, SPRK_NMS_DIAG, SPRK_WINO_DIAG).
inline int diag_env(const char *name) { return knob_env(name, 0); }
inline int xcd_on() {
    static const int on = knob_env("SPRK_XCD", 1);   // 0 = plain round-robin order
    return on;
}
}  // namespace sprk

// exact floor(a / d) for 0 <= a < 2^21 via a float reciprocal (inv = 1.0f / d)
__device__ __forceinline__ int fast_div(int a, float inv) { return (int)(((float)a + 0.5f) * inv); }
