// CTF-corrected particle boxes: sprk_extract_filter (`joint extract --ctf_correct`).
//
// Per particle y = IDFT2(Phi . crop(DFT2(d))): d the B x B box of sprk_extract_scale (integer modes: minus its first sample,
// exact in fp32), Phi [Ku, Hs] the real, even filter of its micrograph over the kept frequencies k = -h .. h (rows, index
// kk = k + h) and v = 0 .. h (columns), h = S/2, Hs = h + 1, Ku = S + 1.  Four real fp32 GEMMs on v_mfma_f32_16x16x4_f32:
//   stage 1, K = B:    U[r, q]  = chain over c of D[r, c] * W1[q, c], q < 2Hs;   V = [U[:, :Hs] ; U[:, Hs:]]     [2B, Hs]
//   stage 2, K = 2B:   Re[kk, v] = chain over t of W2[kk, t] * V[t, v], Im with row Ku + kk;
//                      F = [Re * Phi ; Im * Phi] (one fp32 multiply each)                                        [2Ku, Hs]
//   stage 3, K = 2Ku:  Zr[i, v] = chain over t of W3[i, t] * F[t, v], Zi with row S + i;   Z = [Zr, Zi]          [S, 2Hs]
//   stage 4, K = 2Hs:  Y[i, j]  = chain over t of Z[i, t] * W4[j, t]                                             [S, S]
// every chain an fmaf chain over its K ascending from 0.0f, one accumulator per element and stage, K never split.  The four
// matrices come from the caller (spr_pick_amd.extract.filter_matrices; the weights of the Nyquist rows and 1/B^2 sit inside
// W3 and W4): nothing here knows any trigonometry.  K positions past K (padded to a multiple of 4), rows and columns past
// an operand are zeros formed in registers at staging, or values that only reach outputs nobody stores: the workspace may
// hold anything.
//
// Particles run in batches of nb (the workspace holds V, F and Z of one batch); a particle's bits depend on nothing but
// its own box.  Four launches per batch on the caller's stream, five with SPRK_EXTRACT_NORMALIZE; no host synchronisation,
// no atomics.  grid.z is the particle of the batch, and a box that is not entirely inside the image leaves every stage at
// once (stage 4 writes its zeros and its status 1): none of its samples is read.
//   filter_rows_kernel<T> (stage 1) and filter_out_kernel (stage 4): sample_rows_body and matrix_rows_body of
//     mfma_stage.h (a kernel is its index set-up, one call of a body and its store), one workgroup of four waves per
//     64 x 64 outputs, a wave on 16 rows with four accumulators; both operands in chunks of 64 K positions through LDS, two
//     chunks fetched ahead from clamped addresses (stage 1: sample rows against matrix rows; stage 4: matrix rows on both
//     sides).
//   filter_cols_kernel<kStage> (stages 2 and 3): the paired form of that pipeline (paired_rows_body), a wave holds the
//     accumulators of rows u and M + u of its 16 rows (Re and Im, Zr and Zi), so the filter is applied in the epilogue of
//     stage 2 without a second pass.
//   filter_norm_kernel: one workgroup per particle over its Y in `out`: normalize_box (box_dev.h), the background sums in
//     double and the final store that extract_scale_kernel ends with.
//
// Compiled with -ffp-contract=off (Makefile): the filter multiply, the anchor's fmaf and the normalisation are the
// operations the contract names and nothing else.
#include <cstdint>
#include <type_traits>

#include "common.h"
#include "box_dev.h"
#include "mfma_stage.h"
#include "mrc_host.h"

namespace {

constexpr int kMinSide = 16, kMaxBox = 1024;
constexpr int kThreads = kBoxThreads;            // four waves, every kernel
constexpr int kWaves = kBoxWaves;
constexpr int kTile = 64;                        // 64 x 64 outputs per workgroup, every stage
constexpr int kMaxBatch = 65535;                 // grid.z
constexpr size_t kBudget = (size_t)256 << 20;    // the library's own choice of a batch keeps the workspace near this

struct Geo {
    int B, S, Hs, Ku;                            // box, output side, S/2 + 1, S + 1
    int ldv, ldz;                                // floats per row of V and F: roundup(Hs, 4); of Z and W4: roundup(2Hs, 4)
    int ld1, ld3;                                // floats per row of W1: roundup(B, 4); of W3: roundup(2Ku, 4); W2 has 2B
    int ny, nx;
};

// the box of particle p: false when it is not entirely inside the image (in 64-bit: any int32 centre is safe)
__device__ __forceinline__ bool box_origin(const int *__restrict__ xy, int p, const Geo &g, long &offset) {
    const long x0 = (long)xy[2 * p] - g.B / 2, y0 = (long)xy[2 * p + 1] - g.B / 2;
    offset = y0 * g.nx + x0;
    return !(x0 < 0 || y0 < 0 || x0 + g.B > g.nx || y0 + g.B > g.ny);
}

// ---- stage 1: U of particle p0 + blockIdx.z, rows r0 .., columns q0 .., stored as V ------------------------------------
// grid (ceil(2Hs / 64), ceil(B / 64), nb)
template <typename T>
__global__ __launch_bounds__(kThreads) void filter_rows_kernel(const T *__restrict__ raw, Geo g, const int *__restrict__ xy,
                                                               int p0, const float *__restrict__ w1,
                                                               float *__restrict__ v_out) {
    const int B = g.B;
    long offset;
    if (!box_origin(xy, p0 + blockIdx.z, g, offset)) return;   // before any sample is addressed; the same in every lane
    const T *__restrict__ origin = raw + offset;               // samples read: origin[r*nx + q], 0 <= r, q < B
    const T first = origin[0];                                 // every lane the same address: a broadcast
    float *__restrict__ vp = v_out + (long)blockIdx.z * 2 * B * g.ldv;
    // rows and columns past the box are fetched from its last row / column; rows of W1 past 2Hs are staged as zeros
    sample_rows_body<false>(origin, g.nx, B, B, first, w1, g.ld1, 2 * g.Hs, blockIdx.y * kTile, blockIdx.x * kTile,
                            [=](int r, int q, float u) { store_v_split(vp, g.ldv, B, g.Hs, r, q, u); });
}

// ---- stages 2 and 3: rows u0 .. and M + u0 .. of W times the K-major operand of the workspace ---------------------------
// kStage 2: W = W2 [2Ku, 2B], the operand V [2B, ldv], out F [2Ku, ldv] = [Re * Phi ; Im * Phi]; M = Ku, K = 2B
// kStage 3: W = W3 [2S, ld3], the operand F [2Ku, ldv], out Z [S, ldz] = [Zr, Zi];            M = S,  K = 2Ku
// grid (ceil(Hs / 64), ceil(M / 64), nb)
template <int kStage>
__global__ __launch_bounds__(kThreads) void filter_cols_kernel(Geo g, const int *__restrict__ xy, int p0,
                                                               const float *__restrict__ w, const float *__restrict__ b_in,
                                                               const float *__restrict__ phi, float *__restrict__ c_out) {
    const int Hs = g.Hs, ldv = g.ldv;
    const int M = kStage == 2 ? g.Ku : g.S, K = kStage == 2 ? 2 * g.B : 2 * g.Ku, ldw = kStage == 2 ? 2 * g.B : g.ld3;
    long offset;
    if (!box_origin(xy, p0 + blockIdx.z, g, offset)) return;   // the same in every lane
    const float *__restrict__ bt = b_in + (long)blockIdx.z * K * ldv;
    float *__restrict__ ct = c_out + (long)blockIdx.z * (kStage == 2 ? 2 * g.Ku * ldv : g.S * g.ldz);
    // A: rows u and M + u of W, the K positions at or past K staged as zeros.  B: columns Hs .. ldv-1 of the operand were
    // never written: staged as zeros, like every row at or past K
    paired_rows_body(w, ldw, M, K, bt, ldv, Hs, blockIdx.y * kTile, blockIdx.x * kTile, [=](int u, int v, float x, float y) {
        if constexpr (kStage == 2) {
            if (u < M && v < Hs) {
                const float f = phi[u * Hs + v];
                ct[(long)u * ldv + v] = __fmul_rn(x, f);
                ct[(long)(M + u) * ldv + v] = __fmul_rn(y, f);
            }
        } else {
            store_zr_zi(ct, g.ldz, M, Hs, u, v, x, y);
        }
    });
}

// the box's first sample as the float the integer modes add back (times Phi at the origin); float32: not used
__device__ __forceinline__ float anchor_of(const void *__restrict__ raw, int mode, long offset) {
    switch (mode) {
        case SPRK_MRC_INT8: return (float)((const int8_t *)raw)[offset];
        case SPRK_MRC_INT16: return (float)((const int16_t *)raw)[offset];
        case SPRK_MRC_UINT16: return (float)((const uint16_t *)raw)[offset];
        default: return 0.0f;
    }
}

// ---- stage 4: Y of particle p0 + blockIdx.z, rows i0 .., columns j0 .., and the output stage without normalisation -------
// grid (ceil(S / 64), ceil(S / 64), nb)
__global__ __launch_bounds__(kThreads) void filter_out_kernel(const void *__restrict__ raw, int mode, Geo g,
                                                              const int *__restrict__ xy, int p0,
                                                              const float *__restrict__ z_in, const float *__restrict__ w4,
                                                              const float *__restrict__ phi, int flags,
                                                              float *__restrict__ out, int *__restrict__ status) {
    const int S = g.S, tid = threadIdx.x;
    const int p = p0 + blockIdx.z;
    const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
    const bool normalize = flags & SPRK_EXTRACT_NORMALIZE, invert = flags & SPRK_EXTRACT_INVERT;
    float *__restrict__ o = out + (long)p * S * S;
    long offset;
    if (!box_origin(xy, p, g, offset)) {                       // the same in every lane; no sample is addressed
        for (int e = tid; e < kTile * kTile; e += kThreads) {
            const int i = i0 + (e >> 6), j = j0 + (e & 63);
            if (i < S && j < S) o[i * S + j] = 0.0f;
        }
        if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) status[p] = 1;
        return;
    }
    const float *__restrict__ zt = z_in + (long)blockIdx.z * S * g.ldz;
    const float anchor = anchor_of(raw, mode, offset), phi0 = phi[(S / 2) * g.Hs];   // Phi at k = 0, v = 0
    // rows of Z and of W4 at or past S and the K positions at or past 2Hs are staged as zeros
    matrix_rows_body<false>(zt, g.ldz, S, w4, g.ldz, S, 2 * g.Hs, i0, j0, [=](int i, int j, float y) {
        if (i < S && j < S) {
            if (!normalize) {
                if (mode != SPRK_MRC_FLOAT32) y = __fmaf_rn(phi0, anchor, y);
                if (invert) y = -y;
            }
            o[i * S + j] = y;
        }
    });
    if (!normalize && tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) status[p] = 0;
}

// ---- normalisation of the Y that stage 4 left in `out` -----------------------------------------------------------------
// grid: nb workgroups
__global__ __launch_bounds__(kThreads) void filter_norm_kernel(Geo g, const int *__restrict__ xy, int p0, float inv_s, long R2,
                                                               int flags, float *__restrict__ out, int *__restrict__ status) {
    __shared__ __align__(16) unsigned char red[kWaves * 8];
    const int p = p0 + blockIdx.x;
    long offset;
    if (!box_origin(xy, p, g, offset)) return;                 // stage 4 wrote its zeros and its status
    normalize_box(out + (long)p * g.S * g.S, g.S, inv_s, R2, flags & SPRK_EXTRACT_INVERT, status + p, red);
}

inline bool sizes_ok(int B, int S) { return S >= kMinSide && S <= B && B <= kMaxBox && B % 2 == 0 && S % 2 == 0; }
inline Geo geo_of(int B, int S, int ny, int nx) {
    const int Hs = S / 2 + 1, Ku = S + 1;
    using sprk::roundup4;
    return Geo{B, S, Hs, Ku, roundup4(Hs), roundup4(2 * Hs), roundup4(B), roundup4(2 * Ku), ny, nx};
}
inline size_t v_bytes(const Geo &g) { return sprk::align16((size_t)2 * g.B * g.ldv * sizeof(float)); }
inline size_t f_bytes(const Geo &g) { return sprk::align16((size_t)2 * g.Ku * g.ldv * sizeof(float)); }
inline size_t z_bytes(const Geo &g) { return sprk::align16((size_t)g.S * g.ldz * sizeof(float)); }
// particles per batch: the caller's, or as many as keep the workspace within kBudget (one at least)
inline int batch_of(long P, const Geo &g, int max_batch) {
    long nb = max_batch > 0 ? max_batch : (long)(kBudget / (v_bytes(g) + f_bytes(g) + z_bytes(g)));
    if (nb < 1) nb = 1;
    if (nb > kMaxBatch) nb = kMaxBatch;
    return (int)(nb < P ? nb : P);
}

template <typename T>
int launch_rows(const void *raw, const Geo &g, const int *xy, int p0, int nb, const float *w1, float *v, hipStream_t s) {
    const dim3 grid(sprk::cdiv(2 * g.Hs, kTile), sprk::cdiv(g.B, kTile), nb);
    hipLaunchKernelGGL(filter_rows_kernel<T>, grid, dim3(kThreads), 0, s, (const T *)raw, g, xy, p0, w1, v);
    return sprk::check_launch("extract_filter (stage 1)");
}

}  // namespace

extern "C" {

size_t sprk_extract_filter_ws_bytes(int P, int box, int side, int max_batch) {
    if (!sizes_ok(box, side) || P < 1 || max_batch < 0) return 0;
    const Geo g = geo_of(box, side, 0, 0);
    return (size_t)batch_of(P, g, max_batch) * (v_bytes(g) + f_bytes(g) + z_bytes(g));
}

int sprk_extract_filter(const void *raw, int mode, int ny, int nx, const int *xy, int P, int box, int side, const float *w1,
                        const float *w2, const float *w3, const float *w4, const float *phi, int bg_radius, int flags,
                        int max_batch, float *out, int *status, void *ws, size_t ws_bytes, void *stream) {
    SPRK_REQUIRE_MRC_MODE("extract_filter", mode);
    SPRK_REQUIRE(sizes_ok(box, side),
                 "extract_filter: box %d with output side %d (both even, %d <= side <= box <= %d)", box, side, kMinSide,
                 kMaxBox);
    SPRK_REQUIRE(bg_radius >= 0, "extract_filter: background radius %d (>= 0)", bg_radius);
    SPRK_REQUIRE((flags & ~(SPRK_EXTRACT_NORMALIZE | SPRK_EXTRACT_INVERT)) == 0, "extract_filter: unknown flags 0x%x", flags);
    SPRK_REQUIRE(max_batch >= 0, "extract_filter: max_batch %d (0 = the library's choice, or a positive number of particles)",
                 max_batch);
    SPRK_REQUIRE(ny > 0 && nx > 0 && (long)ny * nx < (1L << 31), "extract_filter: bad image size %dx%d", ny, nx);
    SPRK_REQUIRE(P >= 0, "extract_filter: %d particles", P);
    if (P == 0) return SPRK_OK;
    SPRK_REQUIRE(raw && xy && w1 && w2 && w3 && w4 && phi && out && status, "extract_filter: null pointer");
    SPRK_REQUIRE(sprk::aligned16(raw, w1, w2, w3, w4, phi, out, ws),
                 "extract_filter: the sample buffer, the matrices, the filter, the output and the workspace must start "
                 "16-byte aligned");
    if (int rc = sprk::check_ws("extract_filter", ws, ws_bytes, sprk_extract_filter_ws_bytes(P, box, side, max_batch)))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    const Geo g = geo_of(box, side, ny, nx);
    const int batch = batch_of(P, g, max_batch);
    // V, F and Z of a batch's particle k start k * 2B * ldv, k * 2Ku * ldv and k * S * ldz floats into their parts
    float *v = (float *)ws, *f = (float *)((char *)ws + (size_t)batch * v_bytes(g)),
          *z = (float *)((char *)ws + (size_t)batch * (v_bytes(g) + f_bytes(g)));
    const dim3 block(kThreads);
    for (int p0 = 0; p0 < P; p0 += batch) {
        const int nb = P - p0 < batch ? P - p0 : batch;
        int rc = dispatch_mrc(mode, [&](auto t) { return launch_rows<decltype(t)>(raw, g, xy, p0, nb, w1, v, s); });
        if (rc) return rc;
        hipLaunchKernelGGL(filter_cols_kernel<2>, dim3(sprk::cdiv(g.Hs, kTile), sprk::cdiv(g.Ku, kTile), nb), block, 0, s, g,
                           xy, p0, w2, (const float *)v, phi, f);
        if ((rc = sprk::check_launch("extract_filter (stage 2)"))) return rc;
        hipLaunchKernelGGL(filter_cols_kernel<3>, dim3(sprk::cdiv(g.Hs, kTile), sprk::cdiv(g.S, kTile), nb), block, 0, s, g,
                           xy, p0, w3, (const float *)f, phi, z);
        if ((rc = sprk::check_launch("extract_filter (stage 3)"))) return rc;
        hipLaunchKernelGGL(filter_out_kernel, dim3(sprk::cdiv(g.S, kTile), sprk::cdiv(g.S, kTile), nb), block, 0, s, raw, mode,
                           g, xy, p0, (const float *)z, w4, phi, flags, out, status);
        if ((rc = sprk::check_launch("extract_filter (stage 4)"))) return rc;
        if (flags & SPRK_EXTRACT_NORMALIZE) {
            hipLaunchKernelGGL(filter_norm_kernel, dim3(nb), block, 0, s, g, xy, p0, 1.0f / (float)side,
                               (long)bg_radius * bg_radius, flags, out, status);
            if ((rc = sprk::check_launch("extract_filter (normalisation)"))) return rc;
        }
    }
    return SPRK_OK;
}

}  // extern "C"
