// Whole-frame motion correction of movies: sprk_align_corr and sprk_align_accumulate (`joint align`).
//
// Both entry points are fp32 GEMMs on v_mfma_f32_16x16x4_f32 by the pipeline of mfma_stage.h (the correlation on its K
// loop, multiply and accumulator walk with two loaders of its own; the two accumulate kernels each one call of a stage body
// and a store), and both keep its rule of the bits: one accumulator per output element, its K positions in ascending
// order, one rounding per product, K never split, so every tiling gives the bytes of the contract's fmaf chain
// (tests/align_model.py).
//
// sprk_align_corr: the cross-correlation window of every reduced frame a_f [Sy, Sx] against its reference r_f, both taken
// as periodic, for the row shifts i - R and the column shifts j - R, |shift| <= R:
//   cc[f, i, j] = fmaf chain, from 0.0f, over y' = 0 .. Sy-1 and then x = 0 .. Sx-1 ascending of
//                 a[f, (y' - (i-R)) mod Sy, x] * r[f, y', (x + (j-R)) mod Sx].
// As a GEMM per frame: M the 2R+1 row shifts, N the 2R+1 column shifts, K the Sy*Sx pixels.  Sx is a multiple of 64, so a
// chunk of 64 K positions never crosses an image row and K has no padding.  Row i of a chunk of the A operand is 64
// contiguous, 16-byte-aligned floats of a rolled image row (RolledRows: float4 fetches); column j of the B operand is 64
// contiguous floats that start at any element and wrap at the row end (WrappedCols: element loads, staged row-major as
// B^T).  Shift rows and columns past 2R+1 are fetched from the last shift and staged as zeros on both operands, and are not
// stored.  align_corr_kernel<WM, TN>: a workgroup of WM waves on 16*WM row shifts x 16*TN column shifts of one frame, grid
// (tiles, Z); 64 x 64 on four waves covers every window there is, 32 x 32 on two waves and 16 x 16 on one give more
// workgroups than frames when the frames alone would leave compute units idle.  The bytes do not depend on the choice.
//
// sprk_align_accumulate: one frame of a movie into the running sum, y (+)= My D Mx^T with D the [ny, nx] samples (integer
// modes: minus the anchor the caller passes, exact in fp32), My [by, ny] and Mx [bx, nx] the caller's matrices
// (align.shift_matrix: a sub-pixel shift and a Fourier crop in one):
//   U[r, j] = fmaf chain over c = 0 .. nx-1 ascending of D[r, c] * Mx[j, c], from 0.0f          (stage 1, U in the workspace);
//   y[i, j] = fmaf chain over r = 0 .. ny-1 ascending of My[i, r] * U[r, j],
//             from 0.0f if `first`, else from the y[i, j] already there                         (stage 2).
// Storing and reloading an fp32 accumulator is lossless, so Z calls give the bits of ONE chain over (frame, r) ascending.
// The kernels call the two stage bodies that resample.hip's call (mfma_stage.h: sample_rows_body, kmajor_rows_body), with
// the anchor as a kernel argument (no device read, nothing written back) and the accumulators of stage 2 loaded from y; no
// anchor add and no range.  Padding as there: every padded K position is
// a zero formed in registers on BOTH operands (the workspace is uninitialised memory), and with `first` y is not read.
// Two launches on the caller's stream, no host synchronisation, no atomics.
#include <cstdint>
#include <type_traits>

#include "common.h"
#include "mfma_stage.h"
#include "mrc_host.h"

namespace {

constexpr int kMaxSide = 16384;                  // a side of a frame at most: K = Sy * Sx and U's ny * roundup(bx, 4) stay below 2^31
constexpr int kMaxShift = 31;                    // R at most: the 63 x 63 window is one 64 x 64 tile
constexpr int kMaxFrames = 65535;                // the grid's second dimension
constexpr int kRowsThreads = 256;                // accumulate, stage 1: four waves
constexpr int kRowsTile = 64;                    // ... on 64 rows x 64 columns of U

// ---- the operands of the correlation --------------------------------------------------------------------------------------
// Both loaders take K position c0 = y' * Sx + x0 (a multiple of kKC; Sx is one as well) and keep mfma_stage.h's rule:
// a fetch is an unconditional load from a wrapped address inside the frame, and the zeros are formed at staging.

// Rolled rows: staged row rr is shift row i = i0 + rr, the floats x0 .. x0+63 of image row (y' - (i - R)) mod Sy, as float4
// (the frame 16-byte aligned) into dst [ROWS][kLd].  Sy may be smaller than the window (a roll by Sy is none): the shift is
// reduced modulo Sy first, a constant of the thread, and then one conditional add or subtract wraps the row.
template <int ROWS, int THREADS>
struct RolledRows {
    static constexpr int kPerThread = ROWS * kKC / 4 / THREADS;
    static_assert(ROWS * kKC / 4 % THREADS == 0, "whole float4 per thread");
    using Regs = float4[kPerThread];
    const float *__restrict__ img;               // the frame [Sy, Sx]
    int Sy, Sx, R, n, i0;                        // n = 2R+1 shifts
    lds_float *dst;

    __device__ __forceinline__ void fetch(Regs &v, int c0) const {
        const int y = c0 / Sx, x0 = c0 - y * Sx;
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int e = threadIdx.x + k * THREADS;
            int row = y - (min(i0 + (e >> 4), n - 1) - R) % Sy;  // the shift in (-Sy, Sy): the row in (-Sy, 2 Sy)
            row += row < 0 ? Sy : 0;
            row -= row >= Sy ? Sy : 0;
            v[k] = *reinterpret_cast<const float4 *>(img + (long)row * Sx + x0 + (e & 15) * 4);
        }
    }
    __device__ __forceinline__ void stage(const Regs &v, int) const {
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int e = threadIdx.x + k * THREADS;
            stage4(dst + (e >> 4) * kLd + (e & 15) * 4, zero4(v[k], i0 + (e >> 4) < n, 0, 4));
        }
    }
};

// Wrapped columns: staged row cc is shift column j = j0 + cc, the floats (x0 + k + (j - R)) mod Sx, k = 0 .. 63, of image
// row y', by element loads (a wave reads 64 adjacent floats of one row, split where they wrap) into dst [W][kLd], the
// BtRows layout.  R < Sx: one conditional add or subtract wraps the column.
template <int W, int THREADS>
struct WrappedCols {
    static constexpr int kPerThread = W * kKC / THREADS;
    static_assert(W * kKC % THREADS == 0, "whole elements per thread");
    using Regs = float[kPerThread];
    const float *__restrict__ img;               // the reference [Sy, Sx]
    int Sx, R, n, j0;
    lds_float *dst;

    __device__ __forceinline__ void fetch(Regs &v, int c0) const {
        const int y = c0 / Sx, x0 = c0 - y * Sx;
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int e = threadIdx.x + k * THREADS;
            int x = x0 + (e & 63) + (min(j0 + (e >> 6), n - 1) - R);
            x += x < 0 ? Sx : 0;
            x -= x >= Sx ? Sx : 0;
            v[k] = img[(long)y * Sx + x];
        }
    }
    __device__ __forceinline__ void stage(const Regs &v, int) const {
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int e = threadIdx.x + k * THREADS;
            dst[(e >> 6) * kLd + (e & 63)] = j0 + (e >> 6) < n ? v[k] : 0.0f;
        }
    }
};

// ---- cc[f, i0 .. i0+16*WM-1, j0 .. j0+16*TN-1] ------------------------------------------------------------------------------
// grid (ceil(n / (16*WM)) * ceil(n / (16*TN)), Z)
template <int WM, int TN>
__global__ __launch_bounds__(64 * WM) void align_corr_kernel(const float *__restrict__ a, const float *__restrict__ r,
                                                             long r_stride, int Sy, int Sx, int R,
                                                             float *__restrict__ cc) {
    constexpr int kThreads = 64 * WM, kRows = 16 * WM, W = 16 * TN;
    __shared__ __align__(16) float As[kRows * kLd];            // [row shifts][kLd]
    __shared__ __align__(16) float Bs[W * kLd];                // [column shifts][kLd]
    const int n = 2 * R + 1, tiles_x = (n + W - 1) / W;
    const int i0 = (int)(blockIdx.x / tiles_x) * kRows, j0 = (int)(blockIdx.x % tiles_x) * W;
    const long f = blockIdx.y, frame = (long)Sy * Sx;
    const int tid = threadIdx.x, wave = tid >> 6, lr = tid & 15, lk = (tid & 63) >> 4;

    const RolledRows<kRows, kThreads> la{a + f * frame, Sy, Sx, R, n, i0, lds_ptr(As)};
    const WrappedCols<W, kThreads> lb{r + f * r_stride, Sx, R, n, j0, lds_ptr(Bs)};
    const bool active = i0 + wave * 16 < n;                    // wave-uniform
    f32x4 acc[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    k_loop(Sy * Sx, la, lb, active,
           [&](int ks) { multiply<BtRows, true>(acc, a_frag(As, wave, lr, lk), BtRows::frag(Bs, lr, lk), ks); });
    if (active) {
        float *out = cc + f * n * n;
        for_each_output(acc, i0, j0, wave, lk, lr, [&](int i, int j, float v) {
            if (i < n && j < n) out[i * n + j] = v;
        });
    }
}

// ---- accumulate, stage 1: U[r0 .. r0+63, j0 .. j0+63] = D Mx^T ---------------------------------------------------------------
// resample_rows_kernel with the anchor as an argument: grid (ceil(bx / 64), ceil(ny / 64)); every row r < ny of U is written
// in columns 0 .. ldu-1 (columns bx .. ldu-1 are the products with zero rows of Mx: zeros)
template <typename T>
__global__ __launch_bounds__(kRowsThreads) void accumulate_rows_kernel(const T *__restrict__ raw, int ny, int nx, int bx,
                                                                       const float *__restrict__ mx, int ldmx, T first,
                                                                       float *__restrict__ u, int ldu) {
    sample_rows_body<true>(raw, nx, ny, nx, first, mx, ldmx, bx, blockIdx.y * kRowsTile, blockIdx.x * kRowsTile,
                           [=](int r, int j, float v) {
                               if (r < ny && j < ldu) u[(long)r * ldu + j] = v;
                           });
}

// ---- accumulate, stage 2: y[i0 .. i0+16*WM-1, j0 .. j0+16*TN-1] (+)= My U ----------------------------------------------------
// resample_cols_kernel with the accumulators loaded from y unless `first`: grid (ceil(bx / (16*TN)), ceil(by / (16*WM)))
template <int WM, int TN>
__global__ __launch_bounds__(64 * WM) void accumulate_cols_kernel(const float *__restrict__ my, int ldmy,
                                                                  const float *__restrict__ u, int ldu, int ny, int by,
                                                                  int bx, float *__restrict__ y, int first) {
    // the chain goes on where the frame before left it
    kmajor_rows_body<WM, TN>(my, ldmy, by, ny, u, ldu, bx, first ? nullptr : y, blockIdx.y * 16 * WM, blockIdx.x * 16 * TN,
                             [=](int i, int j, float v) {
                                 if (i < by && j < bx) y[(long)i * bx + j] = v;
                             });
}

inline bool sizes_ok(int ny, int nx, int by, int bx) {
    return 2 <= by && by <= ny && ny <= kMaxSide && 2 <= bx && bx <= nx && nx <= kMaxSide;
}

template <typename T>
int launch_rows(const void *raw, int ny, int nx, int bx, const float *mx, int ldmx, float anchor, float *u, hipStream_t s) {
    const dim3 grid(sprk::cdiv(bx, kRowsTile), sprk::cdiv(ny, kRowsTile));
    hipLaunchKernelGGL(accumulate_rows_kernel<T>, grid, dim3(kRowsThreads), 0, s, (const T *)raw, ny, nx, bx, mx, ldmx,
                       (T)anchor, u, sprk::roundup4(bx));
    return sprk::check_launch("align_accumulate (rows)");
}

template <int WM, int TN>
int launch_cols(const float *my, int ldmy, const float *u, int ny, int by, int bx, float *y, int first, hipStream_t s) {
    const dim3 grid(sprk::cdiv(bx, 16 * TN), sprk::cdiv(by, 16 * WM));
    hipLaunchKernelGGL((accumulate_cols_kernel<WM, TN>), grid, dim3(64 * WM), 0, s, my, ldmy, u, sprk::roundup4(bx), ny, by, bx, y,
                       first);
    return sprk::check_launch("align_accumulate (columns)");
}

template <int WM, int TN>
int launch_corr(const float *a, const float *r, long r_stride, int Z, int Sy, int Sx, int R, float *cc, hipStream_t s) {
    const int n = 2 * R + 1;
    const dim3 grid(sprk::cdiv(n, 16 * WM) * sprk::cdiv(n, 16 * TN), Z);
    hipLaunchKernelGGL((align_corr_kernel<WM, TN>), grid, dim3(64 * WM), 0, s, a, r, r_stride, Sy, Sx, R, cc);
    return sprk::check_launch("align_corr");
}

}  // namespace

extern "C" {

int sprk_align_corr(const float *a, const float *r, long r_stride, int Z, int Sy, int Sx, int R, int tile, float *cc,
                    void *stream) {
    SPRK_REQUIRE(1 <= R && R <= kMaxShift, "align_corr: window radius R %d (1..%d)", R, kMaxShift);
    SPRK_REQUIRE(1 <= Z && Z <= kMaxFrames, "align_corr: %d frames (1..%d)", Z, kMaxFrames);
    SPRK_REQUIRE(Sx >= 64 && Sx % 64 == 0 && Sx <= kMaxSide && 1 <= Sy && Sy <= kMaxSide,
                 "align_corr: frames of %dx%d (Sx a multiple of 64, Sy at least 1, both at most %d)", Sy, Sx, kMaxSide);
    SPRK_REQUIRE(r_stride == 0 || r_stride >= (long)Sy * Sx,
                 "align_corr: reference stride %ld (0 for one shared reference, or at least Sy*Sx = %ld floats)", r_stride,
                 (long)Sy * Sx);
    SPRK_REQUIRE(tile == 0 || tile == 16 || tile == 32 || tile == 64, "align_corr: tile %d (0 = the library's choice, 16, 32, 64)",
                 tile);
    SPRK_REQUIRE(a && r && cc, "align_corr: null pointer");
    SPRK_REQUIRE(((uintptr_t)a & 15) == 0 && ((uintptr_t)r & 3) == 0 && ((uintptr_t)cc & 3) == 0,
                 "align_corr: the frames must start 16-byte aligned, the references and the output 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (tile == 0) {                              // the largest tile that still gives every compute unit a workgroup
        const int n = 2 * R + 1;
        tile = 16;
        for (int t = 64; t > 16; t >>= 1)
            if ((long)sprk::cdiv(n, t) * sprk::cdiv(n, t) * Z >= sprk::num_cus()) {
                tile = t;
                break;
            }
    }
    switch (tile) {
        case 64: return launch_corr<4, 4>(a, r, r_stride, Z, Sy, Sx, R, cc, s);
        case 32: return launch_corr<2, 2>(a, r, r_stride, Z, Sy, Sx, R, cc, s);
        default: return launch_corr<1, 1>(a, r, r_stride, Z, Sy, Sx, R, cc, s);
    }
}

size_t sprk_align_accumulate_ws_bytes(int ny, int nx, int by, int bx) {
    if (!sizes_ok(ny, nx, by, bx)) return 0;
    return (size_t)ny * sprk::roundup4(bx) * sizeof(float);
}

int sprk_align_accumulate(const void *raw, int mode, int ny, int nx, int by, int bx, const float *my, int ldmy,
                          const float *mx, int ldmx, float anchor, float *y, int first, void *ws, size_t ws_bytes,
                          void *stream) {
    SPRK_REQUIRE_MRC_MODE("align_accumulate", mode);
    SPRK_REQUIRE(sizes_ok(ny, nx, by, bx),
                 "align_accumulate: a %dx%d frame resampled to %dx%d (2 <= by <= ny <= %d and 2 <= bx <= nx <= %d)", ny, nx, by,
                 bx, kMaxSide, kMaxSide);
    SPRK_REQUIRE(ldmy >= sprk::roundup4(ny) && ldmy % 4 == 0,
                 "align_accumulate: row stride ldmy %d of the row matrix (a multiple of 4, at least roundup(ny, 4) = %d)", ldmy,
                 sprk::roundup4(ny));
    SPRK_REQUIRE(ldmx >= sprk::roundup4(nx) && ldmx % 4 == 0,
                 "align_accumulate: row stride ldmx %d of the column matrix (a multiple of 4, at least roundup(nx, 4) = %d)",
                 ldmx, sprk::roundup4(nx));
    SPRK_REQUIRE(anchor_ok(mode, anchor),
                 "align_accumulate: anchor %g (a sample value of mode %d; 0 for float32)", (double)anchor, mode);
    SPRK_REQUIRE(raw && my && mx && y, "align_accumulate: null pointer");
    SPRK_REQUIRE(sprk::aligned16(raw, my, mx, y, ws),
                 "align_accumulate: the sample buffer, the matrices, the sum and the workspace must start 16-byte aligned");
    if (int rc = sprk::check_ws("align_accumulate", ws, ws_bytes, sprk_align_accumulate_ws_bytes(ny, nx, by, bx))) return rc;
    hipStream_t s = (hipStream_t)stream;
    float *u = (float *)ws;
    if (int rc = dispatch_mrc(mode, [&](auto t) { return launch_rows<decltype(t)>(raw, ny, nx, bx, mx, ldmx, anchor, u, s); }))
        return rc;
    // 64 x 64 tiles on four waves, unless they would leave compute units without a workgroup
    return (long)sprk::cdiv(by, 64) * sprk::cdiv(bx, 64) < sprk::num_cus()
               ? launch_cols<2, 2>(my, ldmy, u, ny, by, bx, y, first, s)
               : launch_cols<4, 4>(my, ldmy, u, ny, by, bx, y, first, s);
}

}  // extern "C"
