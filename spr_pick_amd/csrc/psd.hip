// Tiled power spectra of ONE raw micrograph: sprk_psd_tiles (`joint ctf`).
//
// The image is cut into T x T tiles at a step of T/2 (ty = (ny - T) / (T/2) + 1 rows of tx tiles; tile t = i*tx + j starts
// at (i*T/2, j*T/2); the trailing margin of fewer than T/2 samples is not covered).  Each tile's half-plane DFT is two
// real fp32 GEMMs on v_mfma_f32_16x16x4_f32 with the operand layout of resample.hip, H = T/2 + 1:
//   U[r, q]  = fmaf chain over c = 0 .. T-1 ascending of D_t[r, c] * W1[q, c], from 0.0f, q < 2H      (stage 1);
//   V        = [U[:, :H] ; U[:, H:]], [2T, H], in the workspace;
//   Re[u, v] = fmaf chain over k = 0 .. 2T-1 ascending of W2[u, k] * V[k, v], from 0.0f; Im with row T+u   (stage 2);
//   Q_t      = fmaf(Im, Im, Re * Re)  (the product rounded first), in the workspace;
//   P[u, v]  = ((0 + Q_0) + Q_1) + ... in ascending tile order, plain fp32 adds                          (reduction).
// W1 [2H, T] (cosine rows, then sine rows) and W2 [2T, 2T] = [[C, -S], [S, C]] come from the caller
// (spr_pick_amd.ctf.dft_matrices): nothing here knows any trigonometry.  One accumulator per element and stage, K never
// split; K is T (a multiple of 16) and 2T, so no K position is padded, and what is padded in M and N is a zero formed in
// registers at staging or a value that only reaches outputs nobody stores: the workspace may hold anything.
//
// Tiles run in batches of nb (the workspace holds V and Q of one batch); batch b adds its tiles to P in index order on
// top of what the batches before left there, so the bits do not depend on nb.  Three launches per batch on the caller's
// stream, no host synchronisation, no atomics:
//   psd_rows_kernel<T>: one workgroup of four waves per 64 rows x 64 columns of one tile's U (grid.z = the tile), a wave
//     on 16 rows with four accumulators; sample_rows_body of mfma_stage.h (fetch two chunks of K ahead from clamped
//     addresses, zeros formed at staging, staged rows of 66 floats) with plain fragment reads and the V-split store.
//     2H = T + 2 is never a multiple of 16: the ragged last column tile is the normal case, its rows of W1 past 2H staged
//     as zeros and its columns not stored.
//   psd_cols_kernel: one workgroup of four waves per 64 rows u x 64 columns v of one tile's spectrum; the paired form of
//     the same pipeline (paired_rows_body): a wave holds the Re and the Im accumulators of its 16 rows (eight of them),
//     so that Q needs no second pass: A is rows u and T+u of W2, B the chunk of V.
//   psd_sum_kernel: one thread per element of P over the batch's tiles.
#include <cstdint>
#include <type_traits>

#include "common.h"
#include "mfma_stage.h"
#include "mrc_host.h"

namespace {

constexpr int kMaxSide = 16384, kMinTile = 16, kMaxTile = 1024;
constexpr int kThreads = 256;                    // four waves, both stages
constexpr int kTile = 64;                        // 64 x 64 outputs per workgroup, both stages
constexpr int kMaxBatch = 65535;                 // grid.z
constexpr size_t kBudget = (size_t)256 << 20;    // the library's own choice of a batch keeps the workspace near this

struct Tiling {
    int T, H, tx, nx;                            // tile side, T/2 + 1, tiles per row of tiles, samples per image row
    int ldv;                                     // floats per row of V: roundup(H, 4)
};

// ---- stage 1: U of tile t0 + blockIdx.z, rows r0 .., columns q0 .., stored as V ----------------------------------------
// grid (ceil(2H / 64), ceil(T / 64), nb)
template <typename S>
__global__ __launch_bounds__(kThreads) void psd_rows_kernel(const S *__restrict__ raw, Tiling g, int t0,
                                                            const float *__restrict__ w1, int ldw1,
                                                            float *__restrict__ v_out) {
    const int T = g.T, H = g.H, ldv = g.ldv, half = T >> 1;
    const int tile = t0 + blockIdx.z, ti = tile / g.tx, tj = tile - ti * g.tx;
    const S *__restrict__ base = raw + (long)ti * half * g.nx + (long)tj * half;   // the tile's first sample
    const S first = raw[0];                                    // of the micrograph; every lane the same address
    float *__restrict__ vt = v_out + (long)blockIdx.z * 2 * T * ldv;
    // rows and columns past the tile are fetched from its last row / column (inside the image); rows of W1 past 2H are
    // staged as zeros.  T is a multiple of 16: no K position is padded
    sample_rows_body<false>(base, g.nx, T, T, first, w1, ldw1, 2 * H, blockIdx.y * kTile, blockIdx.x * kTile,
                            [=](int r, int q, float u) { store_v_split(vt, ldv, T, H, r, q, u); });
}

// ---- stage 2: Q of the batch's tile blockIdx.z, rows u0 .., columns v0 .. ----------------------------------------------
// grid (ceil(H / 64), ceil(T / 64), nb)
__global__ __launch_bounds__(kThreads) void psd_cols_kernel(const float *__restrict__ w2, int ldw2,
                                                            const float *__restrict__ v_in, Tiling g,
                                                            float *__restrict__ q_out) {
    const int T = g.T, H = g.H;
    const float *__restrict__ vt = v_in + (long)blockIdx.z * 2 * T * g.ldv;
    float *__restrict__ qt = q_out + (long)blockIdx.z * T * H;
    // A: rows u and T + u of W2.  B: columns H .. ldv-1 of V were never written: staged as zeros
    paired_rows_body(w2, ldw2, T, 2 * T, vt, g.ldv, H, blockIdx.y * kTile, blockIdx.x * kTile,
                     [=](int u, int v, float x, float y) {
                         if (u < T && v < H) qt[(long)u * H + v] = __fmaf_rn(y, y, __fmul_rn(x, x));
                     });
}

// ---- the reduction: P (+)= the batch's Q in tile order ------------------------------------------------------------------
__global__ __launch_bounds__(256) void psd_sum_kernel(const float *__restrict__ q, int n, int nb, int first,
                                                      float *__restrict__ p) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float acc = first ? 0.0f : p[e];
    for (int t = 0; t < nb; ++t) acc = __fadd_rn(acc, q[(long)t * n + e]);
    p[e] = acc;
}

inline bool tile_ok(int T) { return T >= kMinTile && T <= kMaxTile && T % 16 == 0; }
inline bool sizes_ok(int ny, int nx, int T) { return T <= ny && ny <= kMaxSide && T <= nx && nx <= kMaxSide; }
inline long tiles_of(int ny, int nx, int T) { return (long)((ny - T) / (T / 2) + 1) * ((nx - T) / (T / 2) + 1); }
inline size_t v_bytes(int T) { return sprk::align16((size_t)2 * T * sprk::roundup4(T / 2 + 1) * sizeof(float)); }
inline size_t q_bytes(int T) { return sprk::align16((size_t)T * (T / 2 + 1) * sizeof(float)); }
// tiles per batch: the caller's, or as many as keep the workspace within kBudget (one at least)
inline int batch_of(long ntiles, int T, int max_batch) {
    long nb = max_batch > 0 ? max_batch : (long)(kBudget / (v_bytes(T) + q_bytes(T)));
    if (nb < 1) nb = 1;
    if (nb > kMaxBatch) nb = kMaxBatch;
    return (int)(nb < ntiles ? nb : ntiles);
}

template <typename S>
int launch_rows(const void *raw, const Tiling &g, int t0, int nb, const float *w1, int ldw1, float *v, hipStream_t s) {
    const dim3 grid(sprk::cdiv(2 * g.H, kTile), sprk::cdiv(g.T, kTile), nb);
    hipLaunchKernelGGL(psd_rows_kernel<S>, grid, dim3(kThreads), 0, s, (const S *)raw, g, t0, w1, ldw1, v);
    return sprk::check_launch("psd_tiles (rows)");
}

}  // namespace

extern "C" {

size_t sprk_psd_tiles_ws_bytes(int ny, int nx, int T, int max_batch) {
    if (!tile_ok(T) || !sizes_ok(ny, nx, T) || max_batch < 0) return 0;
    return (size_t)batch_of(tiles_of(ny, nx, T), T, max_batch) * (v_bytes(T) + q_bytes(T));
}

int sprk_psd_tiles(const void *raw, int mode, int ny, int nx, int T, const float *w1, int ldw1, const float *w2, int ldw2,
                   int max_batch, float *p_out, void *ws, size_t ws_bytes, void *stream) {
    SPRK_REQUIRE_MRC_MODE("psd_tiles", mode);
    SPRK_REQUIRE(tile_ok(T), "psd_tiles: tile side %d (a multiple of 16 in %d..%d)", T, kMinTile, kMaxTile);
    SPRK_REQUIRE(sizes_ok(ny, nx, T), "psd_tiles: a %dx%d image with tiles of %d (tile <= ny <= %d and tile <= nx <= %d)", ny,
                 nx, T, kMaxSide, kMaxSide);
    SPRK_REQUIRE(max_batch >= 0, "psd_tiles: max_batch %d (0 = the library's choice, or a positive number of tiles)",
                 max_batch);
    SPRK_REQUIRE(ldw1 >= T && ldw1 % 4 == 0, "psd_tiles: row stride ldw1 %d of W1 (a multiple of 4, at least the tile %d)",
                 ldw1, T);
    SPRK_REQUIRE(ldw2 >= 2 * T && ldw2 % 4 == 0,
                 "psd_tiles: row stride ldw2 %d of W2 (a multiple of 4, at least twice the tile = %d)", ldw2, 2 * T);
    SPRK_REQUIRE(raw && w1 && w2 && p_out, "psd_tiles: null pointer");
    SPRK_REQUIRE(sprk::aligned16(raw, w1, w2, p_out, ws),
                 "psd_tiles: the sample buffer, the matrices, the output and the workspace must start 16-byte aligned");
    if (int rc = sprk::check_ws("psd_tiles", ws, ws_bytes, sprk_psd_tiles_ws_bytes(ny, nx, T, max_batch))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int H = T / 2 + 1, n = T * H;
    const Tiling g{T, H, (nx - T) / (T / 2) + 1, nx, sprk::roundup4(T / 2 + 1)};
    const long ntiles = tiles_of(ny, nx, T);
    const int batch = batch_of(ntiles, T, max_batch);
    float *v = (float *)ws, *q = (float *)((char *)ws + (size_t)batch * v_bytes(T));
    // V and Q of a batch's tile k start k * 2T * ldv and k * T * H floats into their parts (the kernels' own strides)
    for (long t0 = 0; t0 < ntiles; t0 += batch) {
        const int nb = (int)(ntiles - t0 < batch ? ntiles - t0 : batch);
        int rc = dispatch_mrc(mode, [&](auto t) { return launch_rows<decltype(t)>(raw, g, (int)t0, nb, w1, ldw1, v, s); });
        if (rc) return rc;
        hipLaunchKernelGGL(psd_cols_kernel, dim3(sprk::cdiv(H, kTile), sprk::cdiv(T, kTile), nb), dim3(kThreads), 0, s, w2,
                           ldw2, v, g, q);
        if ((rc = sprk::check_launch("psd_tiles (columns)"))) return rc;
        hipLaunchKernelGGL(psd_sum_kernel, dim3(sprk::cdiv(n, 256)), dim3(256), 0, s, q, n, nb, t0 == 0 ? 1 : 0, p_out);
        if ((rc = sprk::check_launch("psd_tiles (sum)"))) return rc;
    }
    return SPRK_OK;
}

}  // extern "C"
