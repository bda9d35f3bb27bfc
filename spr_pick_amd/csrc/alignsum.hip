// Dose-weighted movie sums in Fourier space: sprk_align_spectrum and sprk_align_synthesize (`joint align --dose`).
//
// Y = IDFT2[by, bx]( sum over the frames f of G_f . crop(DFT2[ny, nx](D_f)) ): D_f the [ny, nx] samples of frame f (integer
// modes: minus the anchor the caller passes, exact in fp32), G_f [Ku, Hs] the caller's complex filter of that frame over the
// kept frequencies (the dose weight times the phase ramp of the frame's shift; spr_pick_amd/dose.py).  The four real fp32
// GEMMs of extractfilter.hip on v_mfma_f32_16x16x4_f32 over a whole rectangular frame, the first two once per frame and
// the last two once per movie:
//   stage 1, K = nx:   U[r, q] = chain over c of D[r, c] * W1[q, c], q < 2Hs;   V = [U[:, :Hs] ; U[:, Hs:]]     [2ny, ldv]
//   stage 2, K = 2ny:  A[kk, v] = chain over t of W2[kk, t] * V[t, v], B with row Ku + kk;
//                      Fr = fmaf(A, Gr, fmaf(-B, Gi, Fr_old)), Fi = fmaf(A, Gi, fmaf(B, Gr, Fi_old)), F_old = 0.0f and F
//                      not read when `first`;   F = [Fr ; Fi]                                                   [2Ku, ldv]
//   stage 3, K = 2Ku:  Zr[i, v] = chain over t of W3[i, t] * F[t, v], Zi with row by + i;   Z = [Zr, Zi]        [by, ldz]
//   stage 4, K = 2Hs:  Y[i, j]  = chain over t of Z[i, t] * W4[j, t]                                            [by, bx]
// ldv = roundup(Hs, 4), ldz = roundup(2Hs, 4); every chain an fmaf chain over its K ascending from 0.0f, one accumulator
// per element and stage, K never split.  The matrices come from the caller (dose.spectrum_matrices; the weights of the
// shared rows and columns and 1 / (ny nx) sit inside W3 and W4): nothing here knows any trigonometry, or which frequency a
// row or a column stands for.  K positions past K (padded to a multiple of 4), rows and columns past an operand are zeros
// formed in registers at staging, or values that only reach outputs nobody stores: the workspace and, with `first`, F may
// hold anything.
//
// Two launches per entry point on the caller's stream; no host synchronisation, no atomics.
//   spectrum_rows_kernel<T> (stage 1) and synthesize_out_kernel (stage 4): sample_rows_body and matrix_rows_body of
//     mfma_stage.h (a kernel is its index set-up, one call of a body and its store), one workgroup of four waves per
//     64 x 64 outputs, a wave on 16 rows with four accumulators; both operands in chunks of 64 K positions through LDS, two
//     chunks fetched ahead from clamped addresses.
//   paired_cols_kernel<kStage> (stages 2 and 3): the paired form of that pipeline (paired_rows_body), a wave holds the
//     accumulators of rows u and M + u of its 16 rows (A and B, Zr and Zi), so that the complex multiply-add of stage 2 is
//     its epilogue.
//
// Compiled with -ffp-contract=off (Makefile): the four fmaf of the epilogue are the operations the contract names and
// nothing else.
#include <cstdint>
#include <type_traits>

#include "common.h"
#include "mfma_stage.h"
#include "mrc_host.h"

namespace {

constexpr int kMaxSide = 16384;                  // a side of a frame at most: V's 2 ny * roundup(Hs, 4) stays below 2^31
constexpr int kThreads = 256;                    // four waves, every kernel
constexpr int kTile = 64;                        // 64 x 64 outputs per workgroup, every stage

struct Geo {
    int ny, nx, by, bx, Hs, Ku;
    int ldv, ldz;                                // floats per row of V, F and G: roundup(Hs, 4); of Z and W4: roundup(2Hs, 4)
    int ld1, ld2, ld3;                           // floats per row of W1: roundup(nx, 4); W2: roundup(2ny, 4); W3: roundup(2Ku, 4)
};

// ---- stage 1: U rows r0 .., columns q0 .., stored as V --------------------------------------------------------------------
// grid (ceil(2Hs / 64), ceil(ny / 64))
template <typename T>
__global__ __launch_bounds__(kThreads) void spectrum_rows_kernel(const T *__restrict__ raw, Geo g, T first,
                                                                 const float *__restrict__ w1, float *__restrict__ v_out) {
    // rows and columns past the frame are fetched from its last row / column; rows of W1 past 2Hs are staged as zeros
    sample_rows_body<true>(raw, g.nx, g.ny, g.nx, first, w1, g.ld1, 2 * g.Hs, blockIdx.y * kTile, blockIdx.x * kTile,
                           [=](int r, int q, float u) { store_v_split(v_out, g.ldv, g.ny, g.Hs, r, q, u); });
}

// ---- stages 2 and 3: rows u0 .. and M + u0 .. of W times the K-major operand ---------------------------------------------
// kStage 2: W = W2 [2Ku, ld2], the operand V [2ny, ldv], out F [2Ku, ldv] (+)= G (A + iB);  M = Ku, K = 2ny
// kStage 3: W = W3 [2by, ld3], the operand F [2Ku, ldv], out Z [by, ldz] = [Zr, Zi];        M = by, K = 2Ku
// grid (ceil(Hs / 64), ceil(M / 64))
template <int kStage>
__global__ __launch_bounds__(kThreads) void paired_cols_kernel(Geo g, const float *__restrict__ w,
                                                               const float *__restrict__ b_in, const float *__restrict__ gf,
                                                               int first, float *__restrict__ c_out) {
    const int Hs = g.Hs, ldv = g.ldv;
    const int M = kStage == 2 ? g.Ku : g.by, K = kStage == 2 ? 2 * g.ny : 2 * g.Ku, ldw = kStage == 2 ? g.ld2 : g.ld3;
    // A: rows u and M + u of W, the K positions at or past K staged as zeros.  B: columns Hs .. ldv-1 of the operand were
    // never written: staged as zeros, like every row at or past K
    paired_rows_body(w, ldw, M, K, b_in, ldv, Hs, blockIdx.y * kTile, blockIdx.x * kTile, [=](int u, int v, float x, float y) {
        if constexpr (kStage == 2) {
            if (u < M && v < Hs) {
                const long at_re = (long)u * ldv + v, at_im = (long)(M + u) * ldv + v;
                const float gr = gf[at_re], gi = gf[at_im];
                float fr = 0.0f, fi = 0.0f;
                if (!first) {
                    fr = c_out[at_re];
                    fi = c_out[at_im];
                }
                c_out[at_re] = __fmaf_rn(x, gr, __fmaf_rn(-y, gi, fr));
                c_out[at_im] = __fmaf_rn(x, gi, __fmaf_rn(y, gr, fi));
            }
        } else {
            store_zr_zi(c_out, g.ldz, M, Hs, u, v, x, y);
        }
    });
}

// ---- stage 4: Y rows i0 .., columns j0 .. ---------------------------------------------------------------------------------
// grid (ceil(bx / 64), ceil(by / 64))
__global__ __launch_bounds__(kThreads) void synthesize_out_kernel(Geo g, const float *__restrict__ z_in,
                                                                  const float *__restrict__ w4, float *__restrict__ out) {
    const int by = g.by, bx = g.bx;
    // rows of Z at or past by, rows of W4 at or past bx and the K positions at or past 2Hs are staged as zeros
    matrix_rows_body<true>(z_in, g.ldz, by, w4, g.ldz, bx, 2 * g.Hs, blockIdx.y * kTile, blockIdx.x * kTile,
                           [=](int i, int j, float y) {
                               if (i < by && j < bx) out[(long)i * bx + j] = y;
                           });
}

using sprk::roundup4;
// a [rows, cols] image (the frame, or the sum) with Ku kept rows and Hs kept columns of its spectrum
inline bool sizes_ok(int rows, int cols, int Ku, int Hs) {
    return 2 <= rows && rows <= kMaxSide && 2 <= cols && cols <= kMaxSide && 1 <= Hs && Hs <= cols / 2 + 1 && 1 <= Ku &&
           Ku <= rows + 1;
}
inline Geo geo_of(int ny, int nx, int by, int bx, int Ku, int Hs) {
    return Geo{ny, nx, by, bx, Hs, Ku, roundup4(Hs), roundup4(2 * Hs), roundup4(nx), roundup4(2 * ny), roundup4(2 * Ku)};
}

template <typename T>
int launch_rows(const void *raw, const Geo &g, float anchor, const float *w1, float *v, hipStream_t s) {
    const dim3 grid(sprk::cdiv(2 * g.Hs, kTile), sprk::cdiv(g.ny, kTile));
    hipLaunchKernelGGL(spectrum_rows_kernel<T>, grid, dim3(kThreads), 0, s, (const T *)raw, g, (T)anchor, w1, v);
    return sprk::check_launch("align_spectrum (stage 1)");
}

}  // namespace

extern "C" {

size_t sprk_align_spectrum_ws_bytes(int ny, int nx, int Hs) {
    if (!sizes_ok(ny, nx, 1, Hs)) return 0;
    return (size_t)2 * ny * roundup4(Hs) * sizeof(float);
}

int sprk_align_spectrum(const void *raw, int mode, int ny, int nx, int Ku, int Hs, const float *w1, const float *w2,
                        const float *g, float anchor, float *F, int first, void *ws, size_t ws_bytes, void *stream) {
    SPRK_REQUIRE_MRC_MODE("align_spectrum", mode);
    SPRK_REQUIRE(sizes_ok(ny, nx, Ku, Hs),
                 "align_spectrum: a %dx%d frame with %d kept rows and %d kept columns (2 <= ny, nx <= %d, 1 <= Ku <= ny + 1, "
                 "1 <= Hs <= nx / 2 + 1)", ny, nx, Ku, Hs, kMaxSide);
    SPRK_REQUIRE(anchor_ok(mode, anchor),
                 "align_spectrum: anchor %g (a sample value of mode %d; 0 for float32)", (double)anchor, mode);
    SPRK_REQUIRE(raw && w1 && w2 && g && F, "align_spectrum: null pointer");
    SPRK_REQUIRE(sprk::aligned16(raw, w1, w2, g, F, ws),
                 "align_spectrum: the sample buffer, the matrices, the filter, the spectrum and the workspace must start "
                 "16-byte aligned");
    if (int rc = sprk::check_ws("align_spectrum", ws, ws_bytes, sprk_align_spectrum_ws_bytes(ny, nx, Hs))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const Geo geo = geo_of(ny, nx, 0, 0, Ku, Hs);
    float *v = (float *)ws;
    if (int rc = dispatch_mrc(mode, [&](auto t) { return launch_rows<decltype(t)>(raw, geo, anchor, w1, v, s); })) return rc;
    hipLaunchKernelGGL(paired_cols_kernel<2>, dim3(sprk::cdiv(Hs, kTile), sprk::cdiv(Ku, kTile)), dim3(kThreads), 0, s, geo, w2,
                       (const float *)v, g, first, F);
    return sprk::check_launch("align_spectrum (stage 2)");
}

size_t sprk_align_synthesize_ws_bytes(int by, int Hs) {
    if (by < 2 || by > kMaxSide || Hs < 1 || Hs > kMaxSide / 2 + 1) return 0;
    return (size_t)by * roundup4(2 * Hs) * sizeof(float);
}

int sprk_align_synthesize(const float *F, int Ku, int Hs, int by, int bx, const float *w3, const float *w4, float *y, void *ws,
                          size_t ws_bytes, void *stream) {
    SPRK_REQUIRE(sizes_ok(by, bx, Ku, Hs),
                 "align_synthesize: a %dx%d sum from %d kept rows and %d kept columns (2 <= by, bx <= %d, 1 <= Ku <= by + 1, "
                 "1 <= Hs <= bx / 2 + 1)", by, bx, Ku, Hs, kMaxSide);
    SPRK_REQUIRE(F && w3 && w4 && y, "align_synthesize: null pointer");
    SPRK_REQUIRE(sprk::aligned16(F, w3, w4, y, ws),
                 "align_synthesize: the spectrum, the matrices, the sum and the workspace must start 16-byte aligned");
    if (int rc = sprk::check_ws("align_synthesize", ws, ws_bytes, sprk_align_synthesize_ws_bytes(by, Hs))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const Geo geo = geo_of(0, 0, by, bx, Ku, Hs);
    float *z = (float *)ws;
    hipLaunchKernelGGL(paired_cols_kernel<3>, dim3(sprk::cdiv(Hs, kTile), sprk::cdiv(by, kTile)), dim3(kThreads), 0, s, geo, w3,
                       F, (const float *)nullptr, 0, z);
    if (int rc = sprk::check_launch("align_synthesize (stage 3)")) return rc;
    hipLaunchKernelGGL(synthesize_out_kernel, dim3(sprk::cdiv(bx, kTile), sprk::cdiv(by, kTile)), dim3(kThreads), 0, s, geo,
                       (const float *)z, w4, y);
    return sprk::check_launch("align_synthesize (stage 4)");
}

}  // extern "C"
