// Fourier-cropped micrograph ingest: sprk_ingest_resample (`joint eval --ftbin F`, `joint bin --ftbin F`).
//
// Y = My D Mx^T over ONE whole micrograph: D the [ny, nx] samples (integer modes: minus the first sample, exact in fp32),
// My [by, ny] and Mx [bx, nx] the Dirichlet-kernel resamplers of ingest.resample_matrix (IDFT_S . crop . DFT_B), as two
// fp32 GEMMs on v_mfma_f32_16x16x4_f32 with the operand layout of extract_scale_kernel (extract.hip):
//   U[r, j] = fmaf chain over c = 0 .. nx-1 ascending of D[r, c] * Mx[j, c], from 0.0f     (stage 1, U in the workspace);
//   Y[i, j] = fmaf chain over r = 0 .. ny-1 ascending of My[i, r] * U[r, j], from 0.0f     (stage 2);
// one accumulator per output element and stage, K never split: the MFMA adds its four k in ascending order into the
// accumulator it is given, one rounding per product, so every tiling gives the bytes of the two chains
// (tests/resample_model.py).  K is padded to a multiple of 4 and tiles to multiples of 16; every padded K position is a
// zero formed in registers on BOTH operands (the workspace is uninitialised memory, and fma(0, NaN, acc) is NaN), and
// nothing outside the sample block, the matrices' rows 0 .. S-1 / columns 0 .. roundup(B, 4)-1 or rows 0 .. ny-1 of U is read.
//
// Stage 1, resample_rows_kernel: one workgroup of four waves per 64 rows x 64 columns of U, a wave on 16 rows with four
// independent accumulators (a dependent 16x16x4 chain has 40 cycles of latency against 32 of issue).  K runs in chunks
// of 64 through LDS by the pipeline of mfma_stage.h (its loaders, K loop, multiply and accumulator walk; both kernels
// here are their index set-up, two loader descriptions and an epilogue): the samples by element loads of their own type
// (rows are not 16-byte aligned when nx is odd), converted once; the 64 rows of Mx as float4.  The next two chunks are
// in registers before the current one is multiplied: fetches are unconditional loads from clamped addresses that nothing
// touches until they are staged, and the zeros of the padding are formed at staging.  A staged row is 66 floats: lane
// (row, k) of a fragment read sits on bank 2*row + k.  A chunk's fragment reads run a group of four MFMA steps ahead
// (multiply<..., true>: mfma_chunk).
// Stage 2, resample_cols_kernel<WM, TN>: one workgroup of WM waves per 16*WM rows x 16*TN columns of Y; rows of My as
// float4, U [64 rows of K, 16*TN columns] as float4 into rows of 16*TN + 16 floats (the two k rows a half wave reads land
// on different banks).  The output is small (512^2 is 64 tiles of 64 x 64 on 256 CUs), so the tile drops to 32 x 32 on
// two waves when the larger one would leave CUs idle; the bytes do not depend on the choice.  Its epilogue adds the
// anchor (one fp32 add, integer modes), stores, and leaves the workgroup's min / max as an encoded pair.
// resample_range_kernel (the twin of ingest.hip's ingest_range_kernel) reduces the pairs.  Three launches on the caller's
// stream, no host synchronisation, no atomics.
#include <cstdint>
#include <type_traits>

#include "common.h"
#include "mfma_stage.h"

namespace {

constexpr int kMaxSide = 16384;                  // a side of the image at most: U is ny * roundup(bx, 4) <= 2^28 floats, indexed in long
constexpr int kRowsThreads = 256;                // stage 1: four waves
constexpr int kRowsTile = 64;                    // ... on 64 rows x 64 columns of U
constexpr int kRowsTN = kRowsTile / 16;
constexpr int kRangeThreads = 256;
constexpr size_t kHeadBytes = 16;                // the workspace starts with the anchor (one float), then the pairs, then U

struct Part {
    unsigned int min_enc, max_enc;               // order-preserving encodings of one workgroup's min / max (ingest.hip)
};

__device__ __forceinline__ unsigned int enc(float f) {
    const unsigned int b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float dec(unsigned int e) {
    return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}
__device__ __forceinline__ unsigned int wave_min(unsigned int v) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned int)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ __forceinline__ unsigned int wave_max(unsigned int v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned int)__shfl_xor((int)v, o, 64));
    return v;
}

// the workgroup's min / max (all threads must call); thread 0 returns true and holds the pair in lo / hi
template <int THREADS>
__device__ __forceinline__ bool block_reduce(unsigned int &lo, unsigned int &hi) {
    __shared__ unsigned int red[2][THREADS / 64];
    lo = wave_min(lo);
    hi = wave_max(hi);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][wave] = lo;
        red[1][wave] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < THREADS / 64; ++w) {
            lo = min(lo, red[0][w]);
            hi = max(hi, red[1][w]);
        }
        return true;
    }
    return false;
}

__global__ __launch_bounds__(kRangeThreads) void resample_range_kernel(const Part *__restrict__ parts, int nparts,
                                                                       float *__restrict__ range) {
    unsigned int lo = 0xffffffffu, hi = 0u;
    for (int k = threadIdx.x; k < nparts; k += kRangeThreads) {
        lo = min(lo, parts[k].min_enc);
        hi = max(hi, parts[k].max_enc);
    }
    if (block_reduce<kRangeThreads>(lo, hi)) {
        range[0] = dec(lo);
        range[1] = dec(hi);
    }
}

// ---- stage 1: U[r0 .. r0+63, j0 .. j0+63] = D Mx^T --------------------------------------------------------------------
// grid (ceil(bx / 64), ceil(ny / 64)); every row r < ny of U is written in columns 0 .. ldu-1 (ldu = roundup(bx, 4) <= the
// grid's columns; columns bx .. ldu-1 are the products with zero rows of Mx: zeros)
template <typename T>
__global__ __launch_bounds__(kRowsThreads) void resample_rows_kernel(const T *__restrict__ raw, int ny, int nx, int bx,
                                                                     const float *__restrict__ mx, int ldmx,
                                                                     float *__restrict__ u, int ldu,
                                                                     float *__restrict__ anchor_out) {
    constexpr bool kFloat = std::is_same<T, float>::value;
    __shared__ __align__(16) float As[kRowsTile * kLd];        // [64 rows of D][kLd]
    __shared__ __align__(16) float Ms[kRowsTile * kLd];        // [64 rows of Mx][kLd]
    const int r0 = blockIdx.y * kRowsTile, j0 = blockIdx.x * kRowsTile;
    const int tid = threadIdx.x, wave = tid >> 6, lr = tid & 15, lk = (tid & 63) >> 4;
    const int Kp4 = (nx + 3) & ~3;
    const T first = raw[0];                                    // every lane the same address: a broadcast
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) *anchor_out = kFloat ? 0.0f : (float)first;

    // positions past the image are fetched from its last row / column and staged as 0; rows of Mx past bx and its
    // columns past nx (mx and ldmx are 16-byte aligned) are staged as zeros
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

// ---- stage 2: Y[i0 .. i0+16*WM-1, j0 .. j0+16*TN-1] = My U, + anchor, store, partial range ------------------------------
// grid (ceil(bx / (16*TN)), ceil(by / (16*WM))); parts[blockIdx.y * gridDim.x + blockIdx.x] from every workgroup
template <int WM, int TN>
__global__ __launch_bounds__(64 * WM) void resample_cols_kernel(const float *__restrict__ my, int ldmy,
                                                                const float *__restrict__ u, int ldu, int ny, int by,
                                                                int bx, const float *__restrict__ anchor_in,
                                                                float *__restrict__ out, Part *__restrict__ parts) {
    constexpr int kThreads = 64 * WM, kRows = 16 * WM, W = 16 * TN;
    using URows = KMajorRows<W, kThreads, false>;
    __shared__ __align__(16) float As[kRows * kLd];            // [rows of My][kLd]
    __shared__ __align__(16) float Bs[kKC * URows::kLdb];      // [rows of U = K][kLdb]
    const int i0 = blockIdx.y * kRows, j0 = blockIdx.x * W;
    const int tid = threadIdx.x, wave = tid >> 6, lr = tid & 15, lk = (tid & 63) >> 4;
    const int Kp4 = (ny + 3) & ~3;

    // A: rows of My past by and columns past ny are staged as zeros (my and ldmy are 16-byte aligned).  B: rows of U at or
    // past ny were never written: fetched from row ny-1 instead and staged as zeros; every column below ldu was written
    const MatrixRows<kRows, kThreads, RowsFrom> a{my, ldmy, by, Kp4, ny, RowsFrom{i0, by}, lds_ptr(As)};
    const URows b{u, ldu, ny, j0, ldu, lds_ptr(Bs)};
    const bool active = i0 + wave * 16 < by;                   // wave-uniform
    f32x4 acc[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    k_loop(Kp4, a, b, active,
           [&](int ks) { multiply<KMajor<W>, true>(acc, a_frag(As, wave, lr, lk), KMajor<W>::frag(Bs, lr, lk), ks); });

    unsigned int lo = 0xffffffffu, hi = 0u;
    if (active) {
        const float anchor = anchor_in ? *anchor_in : 0.0f;
        for_each_output(acc, i0, j0, wave, lk, lr, [&](int i, int j, float y) {
            if (i < by && j < bx) {
                if (anchor_in) y = __fadd_rn(y, anchor);
                out[(long)i * bx + j] = y;
                const unsigned int k = enc(y);
                lo = min(lo, k);
                hi = max(hi, k);
            }
        });
    }
    // every workgroup stores its pair (each holds at least one output): nothing to initialise
    if (block_reduce<kThreads>(lo, hi)) parts[blockIdx.y * gridDim.x + blockIdx.x] = Part{lo, hi};
}

inline int ldu_of(int bx) { return (bx + 3) & ~3; }
// the most workgroups stage 2 can have (its smaller tile): the pairs' share of the workspace
inline size_t max_parts(int by, int bx) { return (size_t)sprk::cdiv(by, 32) * sprk::cdiv(bx, 32); }
inline bool sizes_ok(int ny, int nx, int by, int bx) {
    return 2 <= by && by <= ny && ny <= kMaxSide && 2 <= bx && bx <= nx && nx <= kMaxSide;
}

template <typename T>
int launch_rows(const void *raw, int ny, int nx, int bx, const float *mx, int ldmx, float *u, float *anchor, hipStream_t s) {
    const dim3 grid(sprk::cdiv(bx, kRowsTile), sprk::cdiv(ny, kRowsTile));
    hipLaunchKernelGGL(resample_rows_kernel<T>, grid, dim3(kRowsThreads), 0, s, (const T *)raw, ny, nx, bx, mx, ldmx, u,
                       ldu_of(bx), anchor);
    return sprk::check_launch("ingest_resample (rows)");
}

// -> the number of workgroups launched (= partial pairs written), or a negative error code
template <int WM, int TN>
int launch_cols(const float *my, int ldmy, const float *u, int ny, int by, int bx, const float *anchor, float *out,
                Part *parts, hipStream_t s) {
    const dim3 grid(sprk::cdiv(bx, 16 * TN), sprk::cdiv(by, 16 * WM));
    hipLaunchKernelGGL((resample_cols_kernel<WM, TN>), grid, dim3(64 * WM), 0, s, my, ldmy, u, ldu_of(bx), ny, by, bx, anchor,
                       out, parts);
    const int rc = sprk::check_launch("ingest_resample (columns)");
    return rc ? rc : (int)(grid.x * grid.y);
}

}  // namespace

extern "C" {

size_t sprk_ingest_resample_ws_bytes(int ny, int nx, int by, int bx) {
    if (!sizes_ok(ny, nx, by, bx)) return 0;
    return kHeadBytes + sprk::align16(max_parts(by, bx) * sizeof(Part)) + (size_t)ny * ldu_of(bx) * sizeof(float);
}

int sprk_ingest_resample(const void *raw, int mode, int ny, int nx, int by, int bx, const float *my, int ldmy,
                         const float *mx, int ldmx, float *out, float *range_out, void *ws, size_t ws_bytes, void *stream) {
    SPRK_REQUIRE(mode == SPRK_MRC_INT8 || mode == SPRK_MRC_INT16 || mode == SPRK_MRC_FLOAT32 || mode == SPRK_MRC_UINT16,
                 "ingest_resample: unsupported MRC mode %d (0, 1, 2 and 6 are)", mode);
    SPRK_REQUIRE(sizes_ok(ny, nx, by, bx),
                 "ingest_resample: a %dx%d image resampled to %dx%d (2 <= by <= ny <= %d and 2 <= bx <= nx <= %d)", ny, nx, by,
                 bx, kMaxSide, kMaxSide);
    SPRK_REQUIRE(ldmy >= ((ny + 3) & ~3) && ldmy % 4 == 0,
                 "ingest_resample: row stride ldmy %d of the row matrix (a multiple of 4, at least roundup(ny, 4) = %d)", ldmy,
                 (ny + 3) & ~3);
    SPRK_REQUIRE(ldmx >= ((nx + 3) & ~3) && ldmx % 4 == 0,
                 "ingest_resample: row stride ldmx %d of the column matrix (a multiple of 4, at least roundup(nx, 4) = %d)",
                 ldmx, (nx + 3) & ~3);
    SPRK_REQUIRE(raw && my && mx && out && range_out, "ingest_resample: null pointer");
    SPRK_REQUIRE(((uintptr_t)raw & 15) == 0 && ((uintptr_t)my & 15) == 0 && ((uintptr_t)mx & 15) == 0 &&
                     ((uintptr_t)out & 15) == 0 && ((uintptr_t)ws & 15) == 0,
                 "ingest_resample: the sample buffer, the matrices, the output and the workspace must start 16-byte aligned");
    if (int rc = sprk::check_ws("ingest_resample", ws, ws_bytes, sprk_ingest_resample_ws_bytes(ny, nx, by, bx))) return rc;
    hipStream_t s = (hipStream_t)stream;
    float *anchor = (float *)ws;
    Part *parts = (Part *)((char *)ws + kHeadBytes);
    float *u = (float *)((char *)parts + sprk::align16(max_parts(by, bx) * sizeof(Part)));
    int rc;
    switch (mode) {
        case SPRK_MRC_INT8: rc = launch_rows<int8_t>(raw, ny, nx, bx, mx, ldmx, u, anchor, s); break;
        case SPRK_MRC_INT16: rc = launch_rows<int16_t>(raw, ny, nx, bx, mx, ldmx, u, anchor, s); break;
        case SPRK_MRC_FLOAT32: rc = launch_rows<float>(raw, ny, nx, bx, mx, ldmx, u, anchor, s); break;
        default: rc = launch_rows<uint16_t>(raw, ny, nx, bx, mx, ldmx, u, anchor, s); break;
    }
    if (rc) return rc;
    const float *add = mode == SPRK_MRC_FLOAT32 ? nullptr : anchor;
    // 64 x 64 tiles on four waves, unless they would leave compute units without a workgroup
    const int grid = (long)sprk::cdiv(by, 64) * sprk::cdiv(bx, 64) < sprk::num_cus()
                         ? launch_cols<2, 2>(my, ldmy, u, ny, by, bx, add, out, parts, s)
                         : launch_cols<4, 4>(my, ldmy, u, ny, by, bx, add, out, parts, s);
    if (grid < 0) return grid;
    hipLaunchKernelGGL(resample_range_kernel, dim3(1), dim3(kRangeThreads), 0, s, parts, grid, range_out);
    return sprk::check_launch("ingest_resample (range)");
}

}  // extern "C"
