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
// of 64 through LDS by the pipeline of mfma_stage.h (both kernels here are their index set-up, one call of a stage body
// of its section 5 and the store): the samples by element loads of their own type
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
// ingest_range_kernel (range_dev.h, shared with ingest.hip) reduces the pairs.  Three launches on the caller's stream, no
// host synchronisation, no atomics.
#include <cstdint>
#include <type_traits>

#include "common.h"
#include "mfma_stage.h"
#include "mrc_host.h"
#include "range_dev.h"

namespace {

constexpr int kMaxSide = 16384;                  // a side of the image at most: U is ny * roundup(bx, 4) <= 2^28 floats, indexed in long
constexpr int kRowsThreads = 256;                // stage 1: four waves
constexpr int kRowsTile = 64;                    // ... on 64 rows x 64 columns of U
constexpr size_t kHeadBytes = 16;                // the workspace starts with the anchor (one float), then the pairs, then U

// ---- stage 1: U[r0 .. r0+63, j0 .. j0+63] = D Mx^T --------------------------------------------------------------------
// grid (ceil(bx / 64), ceil(ny / 64)); every row r < ny of U is written in columns 0 .. ldu-1 (ldu = roundup(bx, 4) <= the
// grid's columns; columns bx .. ldu-1 are the products with zero rows of Mx: zeros)
template <typename T>
__global__ __launch_bounds__(kRowsThreads) void resample_rows_kernel(const T *__restrict__ raw, int ny, int nx, int bx,
                                                                     const float *__restrict__ mx, int ldmx,
                                                                     float *__restrict__ u, int ldu,
                                                                     float *__restrict__ anchor_out) {
    constexpr bool kFloat = std::is_same<T, float>::value;
    const T first = raw[0];                                    // every lane the same address: a broadcast
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *anchor_out = kFloat ? 0.0f : (float)first;
    // positions past the image and rows of Mx past bx are staged as zeros (mx and ldmx are 16-byte aligned)
    sample_rows_body<true>(raw, nx, ny, nx, first, mx, ldmx, bx, blockIdx.y * kRowsTile, blockIdx.x * kRowsTile,
                           [=](int r, int j, float v) {
                               if (r < ny && j < ldu) u[(long)r * ldu + j] = v;
                           });
}

// ---- stage 2: Y[i0 .. i0+16*WM-1, j0 .. j0+16*TN-1] = My U, + anchor, store, partial range ------------------------------
// grid (ceil(bx / (16*TN)), ceil(by / (16*WM))); parts[blockIdx.y * gridDim.x + blockIdx.x] from every workgroup
template <int WM, int TN>
__global__ __launch_bounds__(64 * WM) void resample_cols_kernel(const float *__restrict__ my, int ldmy,
                                                                const float *__restrict__ u, int ldu, int ny, int by,
                                                                int bx, const float *__restrict__ anchor_in,
                                                                float *__restrict__ out, Part *__restrict__ parts) {
    const float anchor = anchor_in ? *anchor_in : 0.0f;
    unsigned int lo = 0xffffffffu, hi = 0u;
    // rows of My past by and columns past ny are staged as zeros (my and ldmy are 16-byte aligned), like the rows of U at
    // or past ny, which were never written
    kmajor_rows_body<WM, TN>(my, ldmy, by, ny, u, ldu, bx, nullptr, blockIdx.y * 16 * WM, blockIdx.x * 16 * TN,
                             [=, &lo, &hi](int i, int j, float y) {
                                 if (i < by && j < bx) {
                                     if (anchor_in) y = __fadd_rn(y, anchor);
                                     out[(long)i * bx + j] = y;
                                     const unsigned int k = enc(y);
                                     lo = min(lo, k);
                                     hi = max(hi, k);
                                 }
                             });
    // every workgroup stores its pair (each holds at least one output): nothing to initialise
    if (block_reduce<64 * WM>(lo, hi)) parts[blockIdx.y * gridDim.x + blockIdx.x] = Part{lo, hi};
}

// the most workgroups stage 2 can have (its smaller tile): the pairs' share of the workspace
inline size_t max_parts(int by, int bx) { return (size_t)sprk::cdiv(by, 32) * sprk::cdiv(bx, 32); }
inline bool sizes_ok(int ny, int nx, int by, int bx) {
    return 2 <= by && by <= ny && ny <= kMaxSide && 2 <= bx && bx <= nx && nx <= kMaxSide;
}

template <typename T>
int launch_rows(const void *raw, int ny, int nx, int bx, const float *mx, int ldmx, float *u, float *anchor, hipStream_t s) {
    const dim3 grid(sprk::cdiv(bx, kRowsTile), sprk::cdiv(ny, kRowsTile));
    hipLaunchKernelGGL(resample_rows_kernel<T>, grid, dim3(kRowsThreads), 0, s, (const T *)raw, ny, nx, bx, mx, ldmx, u,
                       sprk::roundup4(bx), anchor);
    return sprk::check_launch("ingest_resample (rows)");
}

// -> the number of workgroups launched (= partial pairs written), or a negative error code
template <int WM, int TN>
int launch_cols(const float *my, int ldmy, const float *u, int ny, int by, int bx, const float *anchor, float *out,
                Part *parts, hipStream_t s) {
    const dim3 grid(sprk::cdiv(bx, 16 * TN), sprk::cdiv(by, 16 * WM));
    hipLaunchKernelGGL((resample_cols_kernel<WM, TN>), grid, dim3(64 * WM), 0, s, my, ldmy, u, sprk::roundup4(bx), ny, by, bx,
                       anchor, out, parts);
    const int rc = sprk::check_launch("ingest_resample (columns)");
    return rc ? rc : (int)(grid.x * grid.y);
}

}  // namespace

extern "C" {

size_t sprk_ingest_resample_ws_bytes(int ny, int nx, int by, int bx) {
    if (!sizes_ok(ny, nx, by, bx)) return 0;
    return kHeadBytes + sprk::align16(max_parts(by, bx) * sizeof(Part)) + (size_t)ny * sprk::roundup4(bx) * sizeof(float);
}

int sprk_ingest_resample(const void *raw, int mode, int ny, int nx, int by, int bx, const float *my, int ldmy,
                         const float *mx, int ldmx, float *out, float *range_out, void *ws, size_t ws_bytes, void *stream) {
    SPRK_REQUIRE_MRC_MODE("ingest_resample", mode);
    SPRK_REQUIRE(sizes_ok(ny, nx, by, bx),
                 "ingest_resample: a %dx%d image resampled to %dx%d (2 <= by <= ny <= %d and 2 <= bx <= nx <= %d)", ny, nx, by,
                 bx, kMaxSide, kMaxSide);
    SPRK_REQUIRE(ldmy >= sprk::roundup4(ny) && ldmy % 4 == 0,
                 "ingest_resample: row stride ldmy %d of the row matrix (a multiple of 4, at least roundup(ny, 4) = %d)", ldmy,
                 sprk::roundup4(ny));
    SPRK_REQUIRE(ldmx >= sprk::roundup4(nx) && ldmx % 4 == 0,
                 "ingest_resample: row stride ldmx %d of the column matrix (a multiple of 4, at least roundup(nx, 4) = %d)",
                 ldmx, sprk::roundup4(nx));
    SPRK_REQUIRE(raw && my && mx && out && range_out, "ingest_resample: null pointer");
    SPRK_REQUIRE(sprk::aligned16(raw, my, mx, out, ws),
                 "ingest_resample: the sample buffer, the matrices, the output and the workspace must start 16-byte aligned");
    if (int rc = sprk::check_ws("ingest_resample", ws, ws_bytes, sprk_ingest_resample_ws_bytes(ny, nx, by, bx))) return rc;
    hipStream_t s = (hipStream_t)stream;
    float *anchor = (float *)ws;
    Part *parts = (Part *)((char *)ws + kHeadBytes);
    float *u = (float *)((char *)parts + sprk::align16(max_parts(by, bx) * sizeof(Part)));
    if (int rc = dispatch_mrc(mode, [&](auto t) { return launch_rows<decltype(t)>(raw, ny, nx, bx, mx, ldmx, u, anchor, s); }))
        return rc;
    const float *add = mode == SPRK_MRC_FLOAT32 ? nullptr : anchor;
    // 64 x 64 tiles on four waves, unless they would leave compute units without a workgroup
    const int grid = (long)sprk::cdiv(by, 64) * sprk::cdiv(bx, 64) < sprk::num_cus()
                         ? launch_cols<2, 2>(my, ldmy, u, ny, by, bx, add, out, parts, s)
                         : launch_cols<4, 4>(my, ldmy, u, ny, by, bx, add, out, parts, s);
    if (grid < 0) return grid;
    hipLaunchKernelGGL(ingest_range_kernel<kRangeThreads>, dim3(1), dim3(kRangeThreads), 0, s, parts, grid, range_out);
    return sprk::check_launch("ingest_resample (range)");
}

}  // extern "C"
