// Whole-frame motion correction of movies: sprk_align_corr and sprk_align_accumulate (`joint align`).
//
// Both entry points are fp32 GEMMs on v_mfma_f32_16x16x4_f32 by the pipeline of mfma_stage.h (its K loop, multiply and
// accumulator walk; a kernel here is its index set-up, two loader descriptions and an epilogue), and both keep its rule
// of the bits: one accumulator per output element, its K positions in ascending order, one rounding per product, K never
// split, so every tiling gives the bytes of the contract's fmaf chain (tests/align_model.py).
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
// The kernels are resample.hip's two stages with the anchor as a kernel argument (no device read, nothing written back)
// and the accumulators of stage 2 loaded from y; no anchor add and no range.  Padding as there: every padded K position is
// a zero formed in registers on BOTH operands (the workspace is uninitialised memory), and with `first` y is not read.
// Two launches on the caller's stream, no host synchronisation, no atomics.
#include <cstdint>
#include <limits>
#include <type_traits>

#include "common.h"
#include "mfma_stage.h"

namespace {

constexpr int kMaxSide = 16384;                  // a side of a frame at most: K = Sy * Sx and U's ny * roundup(bx, 4) stay below 2^31
constexpr int kMaxShift = 31;                    // R at most: the 63 x 63 window is one 64 x 64 tile
constexpr int kMaxFrames = 65535;                // the grid's second dimension
constexpr int kRowsThreads = 256;                // accumulate, stage 1: four waves
constexpr int kRowsTile = 64;                    // ... on 64 rows x 64 columns of U
constexpr int kRowsTN = kRowsTile / 16;

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
    __shared__ __align__(16) float As[kRowsTile * kLd];        // [64 rows of D][kLd]
    __shared__ __align__(16) float Ms[kRowsTile * kLd];        // [64 rows of Mx][kLd]
    const int r0 = blockIdx.y * kRowsTile, j0 = blockIdx.x * kRowsTile;
    const int tid = threadIdx.x, wave = tid >> 6, lr = tid & 15, lk = (tid & 63) >> 4;
    const int Kp4 = (nx + 3) & ~3;

    const SampleRows<T, kRowsThreads> d{raw, nx, ny, nx, r0, first, lds_ptr(As)};
    const MatrixRows<kRowsTile, kRowsThreads, RowsFrom> m{mx, ldmx, bx, Kp4, nx, RowsFrom{j0, bx}, lds_ptr(Ms)};
    const bool active = r0 + wave * 16 < ny;                   // wave-uniform
    f32x4 acc[kRowsTN];
#pragma unroll
    for (int t = 0; t < kRowsTN; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    k_loop(Kp4, d, m, active,
           [&](int ks) { multiply<BtRows, true>(acc, a_frag(As, wave, lr, lk), BtRows::frag(Ms, lr, lk), ks); });
    if (active) {
        for_each_output(acc, r0, j0, wave, lk, lr, [&](int r, int j, float v) {
            if (r < ny && j < ldu) u[(long)r * ldu + j] = v;
        });
    }
}

// ---- accumulate, stage 2: y[i0 .. i0+16*WM-1, j0 .. j0+16*TN-1] (+)= My U ----------------------------------------------------
// resample_cols_kernel with the accumulators loaded from y unless `first`: grid (ceil(bx / (16*TN)), ceil(by / (16*WM)))
template <int WM, int TN>
__global__ __launch_bounds__(64 * WM) void accumulate_cols_kernel(const float *__restrict__ my, int ldmy,
                                                                  const float *__restrict__ u, int ldu, int ny, int by,
                                                                  int bx, float *__restrict__ y, int first) {
    constexpr int kThreads = 64 * WM, kRows = 16 * WM, W = 16 * TN;
    using URows = KMajorRows<W, kThreads, false>;
    __shared__ __align__(16) float As[kRows * kLd];            // [rows of My][kLd]
    __shared__ __align__(16) float Bs[kKC * URows::kLdb];      // [rows of U = K][kLdb]
    const int i0 = blockIdx.y * kRows, j0 = blockIdx.x * W;
    const int tid = threadIdx.x, wave = tid >> 6, lr = tid & 15, lk = (tid & 63) >> 4;
    const int Kp4 = (ny + 3) & ~3;

    const MatrixRows<kRows, kThreads, RowsFrom> a{my, ldmy, by, Kp4, ny, RowsFrom{i0, by}, lds_ptr(As)};
    const URows b{u, ldu, ny, j0, ldu, lds_ptr(Bs)};
    const bool active = i0 + wave * 16 < by;                   // wave-uniform
    f32x4 acc[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (active && !first) {                                    // the chain goes on where the frame before left it
#pragma unroll
        for (int t = 0; t < TN; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = i0 + wave * 16 + lk * 4 + g, j = j0 + t * 16 + lr;
                if (i < by && j < bx) acc[t][g] = y[(long)i * bx + j];
            }
    }
    k_loop(Kp4, a, b, active,
           [&](int ks) { multiply<KMajor<W>, true>(acc, a_frag(As, wave, lr, lk), KMajor<W>::frag(Bs, lr, lk), ks); });
    if (active) {
        for_each_output(acc, i0, j0, wave, lk, lr, [&](int i, int j, float v) {
            if (i < by && j < bx) y[(long)i * bx + j] = v;
        });
    }
}

inline int ldu_of(int bx) { return (bx + 3) & ~3; }
inline bool sizes_ok(int ny, int nx, int by, int bx) {
    return 2 <= by && by <= ny && ny <= kMaxSide && 2 <= bx && bx <= nx && nx <= kMaxSide;
}

template <typename T>
int launch_rows(const void *raw, int ny, int nx, int bx, const float *mx, int ldmx, float anchor, float *u, hipStream_t s) {
    const dim3 grid(sprk::cdiv(bx, kRowsTile), sprk::cdiv(ny, kRowsTile));
    hipLaunchKernelGGL(accumulate_rows_kernel<T>, grid, dim3(kRowsThreads), 0, s, (const T *)raw, ny, nx, bx, mx, ldmx,
                       (T)anchor, u, ldu_of(bx));
    return sprk::check_launch("align_accumulate (rows)");
}

template <int WM, int TN>
int launch_cols(const float *my, int ldmy, const float *u, int ny, int by, int bx, float *y, int first, hipStream_t s) {
    const dim3 grid(sprk::cdiv(bx, 16 * TN), sprk::cdiv(by, 16 * WM));
    hipLaunchKernelGGL((accumulate_cols_kernel<WM, TN>), grid, dim3(64 * WM), 0, s, my, ldmy, u, ldu_of(bx), ny, by, bx, y,
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

// the anchor of an integer mode is a sample value: the kernel subtracts it in integers
template <typename T>
bool anchor_is_sample(float anchor) {
    return anchor >= (float)std::numeric_limits<T>::min() && anchor <= (float)std::numeric_limits<T>::max() &&
           (float)(T)anchor == anchor;
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
    return (size_t)ny * ldu_of(bx) * sizeof(float);
}

int sprk_align_accumulate(const void *raw, int mode, int ny, int nx, int by, int bx, const float *my, int ldmy,
                          const float *mx, int ldmx, float anchor, float *y, int first, void *ws, size_t ws_bytes,
                          void *stream) {
    SPRK_REQUIRE(mode == SPRK_MRC_INT8 || mode == SPRK_MRC_INT16 || mode == SPRK_MRC_FLOAT32 || mode == SPRK_MRC_UINT16,
                 "align_accumulate: unsupported MRC mode %d (0, 1, 2 and 6 are)", mode);
    SPRK_REQUIRE(sizes_ok(ny, nx, by, bx),
                 "align_accumulate: a %dx%d frame resampled to %dx%d (2 <= by <= ny <= %d and 2 <= bx <= nx <= %d)", ny, nx, by,
                 bx, kMaxSide, kMaxSide);
    SPRK_REQUIRE(ldmy >= ((ny + 3) & ~3) && ldmy % 4 == 0,
                 "align_accumulate: row stride ldmy %d of the row matrix (a multiple of 4, at least roundup(ny, 4) = %d)", ldmy,
                 (ny + 3) & ~3);
    SPRK_REQUIRE(ldmx >= ((nx + 3) & ~3) && ldmx % 4 == 0,
                 "align_accumulate: row stride ldmx %d of the column matrix (a multiple of 4, at least roundup(nx, 4) = %d)",
                 ldmx, (nx + 3) & ~3);
    SPRK_REQUIRE(mode == SPRK_MRC_INT8    ? anchor_is_sample<int8_t>(anchor)
                 : mode == SPRK_MRC_INT16 ? anchor_is_sample<int16_t>(anchor)
                 : mode == SPRK_MRC_UINT16 ? anchor_is_sample<uint16_t>(anchor)
                                           : anchor == 0.0f,
                 "align_accumulate: anchor %g (a sample value of mode %d; 0 for float32)", (double)anchor, mode);
    SPRK_REQUIRE(raw && my && mx && y, "align_accumulate: null pointer");
    SPRK_REQUIRE(((uintptr_t)raw & 15) == 0 && ((uintptr_t)my & 15) == 0 && ((uintptr_t)mx & 15) == 0 &&
                     ((uintptr_t)y & 15) == 0 && ((uintptr_t)ws & 15) == 0,
                 "align_accumulate: the sample buffer, the matrices, the sum and the workspace must start 16-byte aligned");
    if (int rc = sprk::check_ws("align_accumulate", ws, ws_bytes, sprk_align_accumulate_ws_bytes(ny, nx, by, bx))) return rc;
    hipStream_t s = (hipStream_t)stream;
    float *u = (float *)ws;
    int rc;
    switch (mode) {
        case SPRK_MRC_INT8: rc = launch_rows<int8_t>(raw, ny, nx, bx, mx, ldmx, anchor, u, s); break;
        case SPRK_MRC_INT16: rc = launch_rows<int16_t>(raw, ny, nx, bx, mx, ldmx, anchor, u, s); break;
        case SPRK_MRC_FLOAT32: rc = launch_rows<float>(raw, ny, nx, bx, mx, ldmx, anchor, u, s); break;
        default: rc = launch_rows<uint16_t>(raw, ny, nx, bx, mx, ldmx, anchor, u, s); break;
    }
    if (rc) return rc;
    // 64 x 64 tiles on four waves, unless they would leave compute units without a workgroup
    return (long)sprk::cdiv(by, 64) * sprk::cdiv(bx, 64) < sprk::num_cus()
               ? launch_cols<2, 2>(my, ldmy, u, ny, by, bx, y, first, s)
               : launch_cols<4, 4>(my, ldmy, u, ny, by, bx, y, first, s);
}

}  // extern "C"
