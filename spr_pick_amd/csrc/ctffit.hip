// Scores of the 2-D Thon-ring fit: sprk_ctf_score (`joint ctf --astigmatism`).
//
// bins fp32 [5, ldb]: rows b, p, q, r, Y of n bins of the spectrum (spr_pick_amd.ctf.fit_bins); cand fp32 [ncand, 3]: the
// candidates (d0, e1, e2).  Per bin i and candidate c, in fp32:
//   t = fmaf(r[i], e2, fmaf(q[i], e1, fmaf(p[i], d0, b[i])))     the phase of cos 2 chi in turns;
//   x = cospif(2 t)                                              within 2^-22 of cos(2 pi t);
// and in fp64 S1 += x, S2 += x * x, S3 += Y[i] * x (the products of two converted floats are exact).
//
// ctf_score_kernel: a thread owns one candidate, a workgroup of four waves 256 consecutive candidates and one slice of
//   consecutive bins (grid.x = candidates / 256, grid.y = slices).  The slice goes through LDS in chunks of 256 bins, (b, p,
//   q, r) of a bin as one float4 and Y beside it: every lane reads the same address, so a bin costs one ds_read_b128 and
//   one ds_read_b32 against the ~40 VALU instructions of its phase, cosine and three fp64 updates.  The loop runs over the
//   bins that exist: no padded bin is ever evaluated (cos of a zero-filled bin would be 1, not 0), and nothing past column
//   n of `bins` is read.  Lanes past ncand work on the last candidate and store nothing.
// The number of slices is a function of (n, ncand) alone (slices_of), chosen so that the fit's fine grid of 9261
// candidates still starts about 2000 workgroups.  One slice: the sums go straight to `out`.  More: they go to the
// workspace [slices, ncand, 3] and ctf_reduce_kernel adds them in ascending slice order from 0.0.  No atomics.
#include <cstdint>

#include "common.h"

namespace {

constexpr int kThreads = 256;                    // four waves: 256 candidates per workgroup
constexpr int kChunk = 256;                      // bins staged at a time (5 KiB of LDS)
constexpr int kMaxBins = 1 << 20, kMaxCand = 1 << 24;
constexpr int kTargetBlocks = 2048;              // 256 CUs x 8 workgroups

// bins per slice: a multiple of kChunk; with c = ceil(ncand / 256) workgroups per slice, as many slices as bring the grid
// to about kTargetBlocks, never shorter than one chunk
inline int slice_of(int n, int ncand) {
    const int cblocks = sprk::cdiv(ncand, kThreads);
    int want = sprk::cdiv(kTargetBlocks, cblocks);
    const int most = sprk::cdiv(n, kChunk);
    if (want > most) want = most;
    if (want < 1) want = 1;
    return sprk::roundup(sprk::cdiv(n, want), kChunk);
}
inline int slices_of(int n, int ncand) { return sprk::cdiv(n, slice_of(n, ncand)); }
inline bool sizes_ok(int n, int ncand) { return n >= 1 && n <= kMaxBins && ncand >= 1 && ncand <= kMaxCand; }

// grid (ceil(ncand / 256), slices); part: [slices, ncand, 3]
__global__ __launch_bounds__(kThreads) void ctf_score_kernel(const float *__restrict__ bins, int ldb, int n,
                                                             const float *__restrict__ cand, int ncand, int slice,
                                                             double *__restrict__ part) {
    __shared__ __align__(16) float4 Bs[kChunk];                // (b, p, q, r) of a staged bin
    __shared__ float Ys[kChunk];
    const int tid = threadIdx.x;
    const int c = blockIdx.x * kThreads + tid, cc = min(c, ncand - 1);
    const float d0 = cand[(long)cc * 3], e1 = cand[(long)cc * 3 + 1], e2 = cand[(long)cc * 3 + 2];
    const int i0 = blockIdx.y * slice, i1 = min(n, i0 + slice);
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int base = i0; base < i1; base += kChunk) {
        const int m = min(kChunk, i1 - base);
        __syncthreads();                                       // the chunk before this one has been summed
        if (tid < m) {                                         // kChunk == kThreads: a thread stages one bin
            const long i = base + tid;
            Bs[tid] = make_float4(bins[i], bins[(long)ldb + i], bins[2L * ldb + i], bins[3L * ldb + i]);
            Ys[tid] = bins[4L * ldb + i];
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < m; ++j) {
            const float4 v = Bs[j];
            const float t = __fmaf_rn(v.w, e2, __fmaf_rn(v.z, e1, __fmaf_rn(v.y, d0, v.x)));
            const double x = (double)cospif(__fmul_rn(2.0f, t));
            s1 += x;
            s2 = fma(x, x, s2);                                // x * x is exact in fp64: fused or not, the same bits
            s3 = fma((double)Ys[j], x, s3);
        }
    }
    if (c < ncand) {
        double *__restrict__ o = part + ((long)blockIdx.y * ncand + c) * 3;
        o[0] = s1;
        o[1] = s2;
        o[2] = s3;
    }
}

// out[e] = ((0 + part[0][e]) + part[1][e]) + ..., e over the ncand * 3 sums
__global__ __launch_bounds__(256) void ctf_reduce_kernel(const double *__restrict__ part, long total, int slices,
                                                         double *__restrict__ out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    double acc = 0.0;
    for (int s = 0; s < slices; ++s) acc += part[(long)s * total + e];
    out[e] = acc;
}

}  // namespace

extern "C" {

size_t sprk_ctf_score_ws_bytes(int n, int ncand) {
    if (!sizes_ok(n, ncand)) return 0;
    const int slices = slices_of(n, ncand);
    return slices == 1 ? 0 : (size_t)slices * ncand * 3 * sizeof(double);
}

int sprk_ctf_score(const float *bins, int ldb, int n, const float *cand, int ncand, double *out, void *ws, size_t ws_bytes,
                   void *stream) {
    SPRK_REQUIRE(sizes_ok(n, ncand), "ctf_score: %d bins and %d candidates (1 <= bins <= %d, 1 <= candidates <= %d)", n, ncand,
                 kMaxBins, kMaxCand);
    SPRK_REQUIRE(ldb >= n && ldb % 4 == 0, "ctf_score: row stride ldb %d of the bins (a multiple of 4, at least the %d bins)",
                 ldb, n);
    SPRK_REQUIRE(bins && cand && out, "ctf_score: null pointer");
    SPRK_REQUIRE(sprk::aligned16(bins, cand, out, ws),
                 "ctf_score: the bins, the candidates, the output and the workspace must start 16-byte aligned");
    const size_t need = sprk_ctf_score_ws_bytes(n, ncand);
    if (need)
        if (int rc = sprk::check_ws("ctf_score", ws, ws_bytes, need)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int slice = slice_of(n, ncand), slices = slices_of(n, ncand);
    double *part = slices == 1 ? out : (double *)ws;
    hipLaunchKernelGGL(ctf_score_kernel, dim3(sprk::cdiv(ncand, kThreads), slices), dim3(kThreads), 0, s, bins, ldb, n, cand,
                       ncand, slice, part);
    if (int rc = sprk::check_launch("ctf_score")) return rc;
    if (slices > 1) {
        const long total = (long)ncand * 3;
        hipLaunchKernelGGL(ctf_reduce_kernel, dim3(sprk::cdiv(total, 256)), dim3(256), 0, s, (const double *)ws, total, slices,
                           out);
        if (int rc = sprk::check_launch("ctf_score (reduce)")) return rc;
    }
    return SPRK_OK;
}

}  // extern "C"
