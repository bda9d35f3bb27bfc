// Wiener-weighted class averages: sprk_class_spectrum, sprk_class_wiener and sprk_class_synthesize (`joint class2d
// --ctf_weight`).  The contracts are stated in include/sprk.h and modelled in tests/classctf_model.py.
//
// Per class A = IDFT2(sum_i wn_i . DFT2(y_i) / (sum_i wd_i + tau)) over the half plane that sprk_extract_filter keeps: rows
// k = -h .. h (index kk = k + h), columns v = 0 .. h, h = S/2, Hs = h + 1, Ku = S + 1, ldv = roundup4(Hs), ldz =
// roundup4(2Hs).  The four real fp32 GEMMs of extractfilter.hip with B = S and the caller's matrices of
// spr_pick_amd.extract.filter_matrices(S, S), split where the class sums go in between:
//   class_spectrum,   stage 1, K = S:    U[r, q] = chain over c of img[r, c] * W1[q, c];  V = [U[:, :Hs] ; U[:, Hs:]]   [2S, ldv]
//                     stage 2, K = 2S:   Re[kk, v] = chain over t of W2[kk, t] * V[t, v], Im with row Ku + kk     spec [2Ku, ldv]
//   class_wiener:     per class and bin  nr = fmaf(wn[g_m], Re_m, nr), ni likewise, d = d + wd[g_m] over the members m in list
//                     order, from 0.0f;  out = nr / (d + tau), ni / (d + tau)                                       [2Ku, ldv]
//   class_synthesize, stage 3, K = 2Ku:  Zr[i, v] = chain over t of W3[i, t] * F[t, v], Zi with row S + i;  Z = [Zr, Zi] [S, ldz]
//                     stage 4, K = 2Hs:  A[i, j] = chain over t of Z[i, t] * W4[j, t]                                   [S, S]
// every chain an fmaf chain over its K ascending from 0.0f, one accumulator per element and stage, K never split.  Nothing
// here knows any trigonometry.  Each GEMM kernel is its index set-up, one stage body of mfma_stage.h and its store; grid.z is
// the image of the batch.  Columns Hs .. ldv-1 of a spectrum are written by nobody and read by nobody (the K-major loader
// stages them as zeros); the workspaces may hold anything.
//
// class_wiener_kernel: one workgroup per (class, 256 bins), a thread per bin, the members read straight from memory with
// kAhead of them in flight and the chain in list order (class_average_kernel's scheme).  Every index that comes from device
// memory (a member, its group, a class offset) is clamped into its array.  An empty class is not written.
// No atomics, no host synchronisation; class_wiener has no workspace.
//
// Compiled with -ffp-contract=off (Makefile): the fmaf, the adds and the divisions above are the operations the contract
// names and nothing else.
#include <cmath>
#include <cstdint>

#include "common.h"
#include "mfma_stage.h"

namespace {

constexpr int kMinSide = 16, kMaxSide = 128;
constexpr int kThreads = 256;                    // four waves, every kernel
constexpr int kTile = 64;                        // 64 x 64 outputs per workgroup, every stage
constexpr int kMaxBatch = 65535;                 // grid.z
constexpr size_t kBudget = (size_t)256 << 20;    // the library's own choice of a batch keeps the workspace near this

struct Geo {
    int S, Hs, Ku;                               // side, S/2 + 1, S + 1
    int ldv, ldz;                                // floats per row of V and a spectrum: roundup(Hs, 4); of Z and W4: roundup(2Hs, 4)
    int ld1, ld3;                                // floats per row of W1: roundup(S, 4); of W3: roundup(2Ku, 4); W2 has 2S
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ---- stage 1: U of image p0 + blockIdx.z, rows r0 .., columns q0 .., stored as V -----------------------------------------
// grid (ceil(2Hs / 64), ceil(S / 64), nb)
__global__ __launch_bounds__(kThreads) void spectrum_rows_kernel(const float *__restrict__ img, Geo g, int p0,
                                                                 const float *__restrict__ w1, float *__restrict__ v_out) {
    const int S = g.S;
    const float *__restrict__ origin = img + (long)(p0 + blockIdx.z) * S * S;
    float *__restrict__ vp = v_out + (long)blockIdx.z * 2 * S * g.ldv;
    // a row of an image is only 8-byte aligned (S is even): element loads.  Rows and columns past the image are fetched from
    // its last row / column; rows of W1 past 2Hs are staged as zeros
    sample_rows_body<false>(origin, S, S, S, 0.0f, w1, g.ld1, 2 * g.Hs, blockIdx.y * kTile, blockIdx.x * kTile,
                            [=](int r, int q, float u) { store_v_split(vp, g.ldv, S, g.Hs, r, q, u); });
}

// ---- stages 2 and 3: rows u0 .. and M + u0 .. of W times a K-major operand ------------------------------------------------
// kStage 2: W = W2 [2Ku, 2S], the operand V [2S, ldv] of the workspace, out spec [2Ku, ldv] = [Re ; Im];     M = Ku, K = 2S
// kStage 3: W = W3 [2S, ld3], the operand F [2Ku, ldv],                 out Z [S, ldz] = [Zr, Zi];           M = S,  K = 2Ku
// grid (ceil(Hs / 64), ceil(M / 64), nb); b_in and c_out are those of the launch's first image
template <int kStage>
__global__ __launch_bounds__(kThreads) void spectrum_cols_kernel(Geo g, const float *__restrict__ w,
                                                                 const float *__restrict__ b_in, float *__restrict__ c_out) {
    const int Hs = g.Hs, ldv = g.ldv;
    const int M = kStage == 2 ? g.Ku : g.S, K = kStage == 2 ? 2 * g.S : 2 * g.Ku, ldw = kStage == 2 ? 2 * g.S : g.ld3;
    const float *__restrict__ bt = b_in + (long)blockIdx.z * K * ldv;
    float *__restrict__ ct = c_out + (long)blockIdx.z * (kStage == 2 ? 2 * g.Ku * ldv : g.S * g.ldz);
    // A: rows u and M + u of W, the K positions at or past K staged as zeros.  B: columns Hs .. ldv-1 of the operand were
    // never written: staged as zeros, like every row at or past K
    paired_rows_body(w, ldw, M, K, bt, ldv, Hs, blockIdx.y * kTile, blockIdx.x * kTile, [=](int u, int v, float x, float y) {
        if constexpr (kStage == 2) {
            if (u < M && v < Hs) {
                ct[(long)u * ldv + v] = x;
                ct[(long)(M + u) * ldv + v] = y;
            }
        } else {
            store_zr_zi(ct, g.ldz, M, Hs, u, v, x, y);
        }
    });
}

// ---- stage 4: the average of class blockIdx.z, rows i0 .., columns j0 .. ----------------------------------------------------
// grid (ceil(S / 64), ceil(S / 64), K)
__global__ __launch_bounds__(kThreads) void synthesize_out_kernel(Geo g, const float *__restrict__ z_in,
                                                                  const float *__restrict__ w4, float *__restrict__ out) {
    const int S = g.S;
    const float *__restrict__ zt = z_in + (long)blockIdx.z * S * g.ldz;
    float *__restrict__ o = out + (long)blockIdx.z * S * S;
    // rows of Z and of W4 at or past S and the K positions at or past 2Hs are staged as zeros
    matrix_rows_body<false>(zt, g.ldz, S, w4, g.ldz, S, 2 * g.Hs, blockIdx.y * kTile, blockIdx.x * kTile,
                            [=](int i, int j, float y) {
                                if (i < S && j < S) o[i * S + j] = y;
                            });
}

// ---- the class sums ------------------------------------------------------------------------------------------------------
struct Wiener {
    const float *spec;                           // [n, 2Ku, ldv]
    const float *wn, *wd;                        // [G, Ku, ldv]
    const int *group;                            // [n]: by image
    const int *members, *offsets;                // [N], [K + 1]
    int n, G, N, Ku, Hs, ldv;
    float tau;
    float *out;                                  // [K, 2Ku, ldv]
};

// grid (ceil(Ku * Hs / 256), K)
__global__ __launch_bounds__(kThreads) void class_wiener_kernel(Wiener t) {
    const int k = blockIdx.y;
    const int beg = clampi(t.offsets[k], 0, t.N), end = clampi(t.offsets[k + 1], 0, t.N);
    if (end <= beg) return;                                    // an empty class keeps what it has
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= t.Ku * t.Hs) return;
    const int kk = e / t.Hs, v = e - kk * t.Hs;
    const long plane = (long)t.Ku * t.ldv;                     // floats of a table and of either half of a spectrum
    const long bin = (long)kk * t.ldv + v;
    // kAhead members' loads are in flight together (one at a time, a member is three dependent round trips to memory); the
    // chain stays in list order
    constexpr int kAhead = 4;
    float nr = 0.0f, ni = 0.0f, d = 0.0f;
    auto load = [&](int n, float &a, float &b, float &re, float &im) {
        const int m = clampi(t.members[n], 0, t.n - 1), g = clampi(t.group[m], 0, t.G - 1);
        const float *__restrict__ s = t.spec + (long)m * 2 * plane + bin;
        a = t.wn[(long)g * plane + bin];
        b = t.wd[(long)g * plane + bin];
        re = s[0];
        im = s[plane];
    };
    int n = beg;
    for (; n + kAhead <= end; n += kAhead) {
        float a[kAhead], b[kAhead], re[kAhead], im[kAhead];
#pragma unroll
        for (int q = 0; q < kAhead; ++q) load(n + q, a[q], b[q], re[q], im[q]);
#pragma unroll
        for (int q = 0; q < kAhead; ++q) {
            nr = __fmaf_rn(a[q], re[q], nr);
            ni = __fmaf_rn(a[q], im[q], ni);
            d = d + b[q];
        }
    }
    for (; n < end; ++n) {
        float a, b, re, im;
        load(n, a, b, re, im);
        nr = __fmaf_rn(a, re, nr);
        ni = __fmaf_rn(a, im, ni);
        d = d + b;
    }
    const float den = d + t.tau;
    float *__restrict__ o = t.out + (long)k * 2 * plane + bin;
    o[0] = __fdiv_rn(nr, den);
    o[plane] = __fdiv_rn(ni, den);
}

inline bool side_ok(int S) { return kMinSide <= S && S <= kMaxSide && S % 2 == 0; }
inline bool aligned4(const void *p) { return ((uintptr_t)p & 3) == 0; }
inline Geo geo_of(int S) {
    const int Hs = S / 2 + 1, Ku = S + 1;
    using sprk::roundup4;
    return Geo{S, Hs, Ku, roundup4(Hs), roundup4(2 * Hs), roundup4(S), roundup4(2 * Ku)};
}
inline size_t v_bytes(const Geo &g) { return sprk::align16((size_t)2 * g.S * g.ldv * sizeof(float)); }
inline size_t z_bytes(const Geo &g) { return sprk::align16((size_t)g.S * g.ldz * sizeof(float)); }
// images per batch: the caller's, or as many as keep the workspace within kBudget (one at least)
inline int batch_of(long n, const Geo &g, int max_batch) {
    long nb = max_batch > 0 ? max_batch : (long)(kBudget / v_bytes(g));
    if (nb < 1) nb = 1;
    if (nb > kMaxBatch) nb = kMaxBatch;
    return (int)(nb < n ? nb : n);
}

}  // namespace

extern "C" {

size_t sprk_class_spectrum_ws_bytes(int n, int side, int max_batch) {
    if (!side_ok(side) || n < 1 || max_batch < 0) return 0;
    const Geo g = geo_of(side);
    return (size_t)batch_of(n, g, max_batch) * v_bytes(g);
}

int sprk_class_spectrum(const float *img, int n, int side, const float *w1, const float *w2, int max_batch, float *spec,
                        void *ws, size_t ws_bytes, void *stream) {
    SPRK_REQUIRE(side_ok(side), "class_spectrum: images of side %d (even, %d..%d; `joint extract --scale 64` writes such)",
                 side, kMinSide, kMaxSide);
    SPRK_REQUIRE(max_batch >= 0, "class_spectrum: max_batch %d (0 = the library's choice, or a positive number of images)",
                 max_batch);
    SPRK_REQUIRE(n >= 0, "class_spectrum: %d images (at least 0)", n);
    if (n == 0) return SPRK_OK;
    SPRK_REQUIRE(img && w1 && w2 && spec, "class_spectrum: null pointer (img, w1, w2 and spec are all needed)");
    SPRK_REQUIRE(sprk::aligned16(img, w1, w2, spec, ws),
                 "class_spectrum: the images, the matrices, the spectra and the workspace must start 16-byte aligned");
    if (int rc = sprk::check_ws("class_spectrum", ws, ws_bytes, sprk_class_spectrum_ws_bytes(n, side, max_batch))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const Geo g = geo_of(side);
    const int batch = batch_of(n, g, max_batch);
    float *v = (float *)ws;                                    // V of a batch's image k starts k * 2S * ldv floats in
    const dim3 block(kThreads);
    for (int p0 = 0; p0 < n; p0 += batch) {
        const int nb = n - p0 < batch ? n - p0 : batch;
        hipLaunchKernelGGL(spectrum_rows_kernel, dim3(sprk::cdiv(2 * g.Hs, kTile), sprk::cdiv(g.S, kTile), nb), block, 0, s, img,
                           g, p0, w1, v);
        if (int rc = sprk::check_launch("class_spectrum (stage 1)")) return rc;
        hipLaunchKernelGGL(spectrum_cols_kernel<2>, dim3(sprk::cdiv(g.Hs, kTile), sprk::cdiv(g.Ku, kTile), nb), block, 0, s, g,
                           w2, (const float *)v, spec + (size_t)p0 * 2 * g.Ku * g.ldv);
        if (int rc = sprk::check_launch("class_spectrum (stage 2)")) return rc;
    }
    return SPRK_OK;
}

int sprk_class_wiener(const float *spec, int n, int side, const float *wn, const float *wd, int G, const int *group,
                      const int *members, int N, const int *offsets, int K, float tau, float *out, void *stream) {
    SPRK_REQUIRE(side_ok(side), "class_wiener: spectra of side %d (even, %d..%d)", side, kMinSide, kMaxSide);
    SPRK_REQUIRE(n >= 0 && N >= 0, "class_wiener: %d spectra and %d members (at least 0 each)", n, N);
    SPRK_REQUIRE(1 <= K && K <= 65535, "class_wiener: %d classes (1..65535)", K);
    SPRK_REQUIRE(G >= 1, "class_wiener: %d weight tables (at least 1: ctf.weight_tables builds them)", G);
    SPRK_REQUIRE(std::isfinite(tau) && tau > 0.0f, "class_wiener: tau %g (finite and > 0; 1.0 is the default of --wiener)",
                 (double)tau);
    if (n == 0 || N == 0) return SPRK_OK;                      // every class is empty
    SPRK_REQUIRE(spec && wn && wd && group && members && offsets && out, "class_wiener: null pointer");
    SPRK_REQUIRE(sprk::aligned16(spec, wn, wd, out) && aligned4(group) && aligned4(members) && aligned4(offsets),
                 "class_wiener: the spectra, the tables and the output must start 16-byte aligned, the index arrays 4-byte "
                 "aligned");
    SPRK_REQUIRE(spec != out, "class_wiener: out must not be spec");
    const Geo g = geo_of(side);
    const Wiener t{spec, wn, wd, group, members, offsets, n, G, N, g.Ku, g.Hs, g.ldv, tau, out};
    hipLaunchKernelGGL(class_wiener_kernel, dim3(sprk::cdiv(g.Ku * g.Hs, kThreads), K), dim3(kThreads), 0, (hipStream_t)stream,
                       t);
    return sprk::check_launch("class_wiener");
}

size_t sprk_class_synthesize_ws_bytes(int K, int side) {
    if (!side_ok(side) || K < 1 || K > kMaxBatch) return 0;
    return (size_t)K * z_bytes(geo_of(side));
}

int sprk_class_synthesize(const float *f, int K, int side, const float *w3, const float *w4, float *out, void *ws,
                          size_t ws_bytes, void *stream) {
    SPRK_REQUIRE(side_ok(side), "class_synthesize: spectra of side %d (even, %d..%d)", side, kMinSide, kMaxSide);
    SPRK_REQUIRE(1 <= K && K <= kMaxBatch, "class_synthesize: %d spectra (1..%d; split a larger stack into several calls)", K,
                 kMaxBatch);
    SPRK_REQUIRE(f && w3 && w4 && out, "class_synthesize: null pointer (f, w3, w4 and out are all needed)");
    SPRK_REQUIRE(sprk::aligned16(f, w3, w4, out, ws),
                 "class_synthesize: the spectra, the matrices, the output and the workspace must start 16-byte aligned");
    if (int rc = sprk::check_ws("class_synthesize", ws, ws_bytes, sprk_class_synthesize_ws_bytes(K, side))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const Geo g = geo_of(side);
    float *z = (float *)ws;                                    // Z of spectrum k starts k * S * ldz floats in
    const dim3 block(kThreads);
    hipLaunchKernelGGL(spectrum_cols_kernel<3>, dim3(sprk::cdiv(g.Hs, kTile), sprk::cdiv(g.S, kTile), K), block, 0, s, g, w3, f,
                       z);
    if (int rc = sprk::check_launch("class_synthesize (stage 3)")) return rc;
    hipLaunchKernelGGL(synthesize_out_kernel, dim3(sprk::cdiv(g.S, kTile), sprk::cdiv(g.S, kTile), K), block, 0, s, g,
                       (const float *)z, w4, out);
    return sprk::check_launch("class_synthesize (stage 4)");
}

}  // extern "C"
