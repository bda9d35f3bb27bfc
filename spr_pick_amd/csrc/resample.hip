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
// of 64 through LDS: the samples by element loads of their own type (rows are not 16-byte aligned when nx is odd),
// converted once; the 64 rows of Mx as float4.  The next two chunks are in registers before the current one is
// multiplied: fetches are unconditional loads from clamped addresses that nothing touches until they are staged, and the
// zeros of the padding are formed at staging (fetch4 / zero4, mfma_stage.h).  A staged row is 66 floats: lane (row, k) of a
// fragment read sits on bank 2*row + k.  A chunk's fragment reads run a group of four MFMA steps ahead (mfma_chunk).
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
constexpr int kDPerThread = kRowsTile * kKC / kRowsThreads;        // 16 samples of a chunk per thread
constexpr int kMPerThread = kRowsTile * kKC / 4 / kRowsThreads;    // 4 float4 of a chunk of Mx per thread
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

// One whole chunk of K for a wave's TN accumulators: kKC / 4 MFMA steps per accumulator, k ascending.  The fragment reads
// of kGroup steps (ap[k]: A at this lane's row; bp[t * b_tile + k * b_step]: B of tile t) are issued a group ahead of
// the MFMAs that consume them, so that the LDS latency hides behind a group's MFMAs instead of standing before each step.
constexpr int kGroup = 4;
template <int TN>
__device__ __forceinline__ void mfma_chunk(f32x4 (&acc)[TN], const float *ap, const float *bp, int b_tile, int b_step) {
    constexpr int kGroups = kKC / 4 / kGroup;
    float a[2][kGroup], b[2][TN][kGroup];
    auto load = [&](int buf, int g) {
#pragma unroll
        for (int q = 0; q < kGroup; ++q) {
            const int k = (g * kGroup + q) * 4;
            a[buf][q] = ap[k];
#pragma unroll
            for (int t = 0; t < TN; ++t) b[buf][t][q] = bp[t * b_tile + k * b_step];
        }
    };
    load(0, 0);
#pragma unroll
    for (int g = 0; g < kGroups; ++g) {
        __builtin_amdgcn_sched_barrier(0);                     // the scheduler otherwise moves every read back to its MFMA
        if (g + 1 < kGroups) load((g + 1) & 1, g + 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < kGroup; ++q)
#pragma unroll
            for (int t = 0; t < TN; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g & 1][q], b[g & 1][t][q], acc[t], 0, 0, 0);
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
    // a fetched sample in its register: widened by the load itself (packed pairs of 16-bit samples would need an
    // operation on the loaded value right behind the load, and with it a wait)
    using R = typename std::conditional<kFloat, float, int>::type;
    __shared__ __align__(16) float As[kRowsTile * kLd];        // [64 rows of D][kLd]
    __shared__ __align__(16) float Ms[kRowsTile * kLd];        // [64 rows of Mx][kLd]
    const int r0 = blockIdx.y * kRowsTile, j0 = blockIdx.x * kRowsTile;
    const int tid = threadIdx.x, wave = tid >> 6, lr = tid & 15, lk = (tid & 63) >> 4;
    const int Kp4 = (nx + 3) & ~3;
    const T first = raw[0];                                    // every lane the same address: a broadcast
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) *anchor_out = kFloat ? 0.0f : (float)first;

    // the chunk of D at rows r0 .., columns c0 ..: thread t holds elements t, t + 256, ... of the [64][kKC] chunk (a wave
    // reads 64 adjacent samples of one row); positions past the image are fetched from its last row / column and staged as 0
    auto fetch_d = [&](R (&v)[kDPerThread], int c0) {
#pragma unroll
        for (int k = 0; k < kDPerThread; ++k) {
            const int e = tid + k * kRowsThreads, r = r0 + (e >> 6), q = c0 + (e & 63);
            v[k] = raw[(long)min(r, ny - 1) * nx + min(q, nx - 1)];
        }
    };
    auto stage_d = [&](const R (&v)[kDPerThread], int c0) {
#pragma unroll
        for (int k = 0; k < kDPerThread; ++k) {
            const int e = tid + k * kRowsThreads, r = r0 + (e >> 6), q = c0 + (e & 63);
            float d;
            if constexpr (kFloat) d = v[k];
            else d = (float)(v[k] - (int)first);               // |difference| < 2^17: exact
            As[(e >> 6) * kLd + (e & 63)] = (r < ny && q < nx) ? d : 0.0f;
        }
    };
    // rows j0 .. j0+63 of Mx, columns c0 .. c0+kKC-1, as float4 (mx and ldmx are 16-byte aligned); rows past bx and
    // columns past nx are staged as zeros
    auto fetch_m = [&](float4 (&v)[kMPerThread], int c0) {
#pragma unroll
        for (int k = 0; k < kMPerThread; ++k) {
            const int e = tid + k * kRowsThreads;
            v[k] = fetch4(mx, ldmx, bx, Kp4, j0 + (e >> 4), c0 + (e & 15) * 4);
        }
    };
    auto stage_m = [&](const float4 (&v)[kMPerThread], int c0) {
#pragma unroll
        for (int k = 0; k < kMPerThread; ++k) {
            const int e = tid + k * kRowsThreads;
            stage4(Ms + (e >> 4) * kLd + (e & 15) * 4, zero4(v[k], j0 + (e >> 4) < bx, c0 + (e & 15) * 4, nx));
        }
    };

    const bool active = r0 + wave * 16 < ny;                   // wave-uniform
    f32x4 acc[kRowsTN];
#pragma unroll
    for (int t = 0; t < kRowsTN; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    R dv[2][kDPerThread];
    float4 mv[2][kMPerThread];
    fetch_d(dv[0], 0);
    fetch_m(mv[0], 0);
    if (kKC < Kp4) {
        fetch_d(dv[1], kKC);
        fetch_m(mv[1], kKC);
    }
    auto chunk = [&](R (&d)[kDPerThread], float4 (&mm)[kMPerThread], int c0) {
        __syncthreads();                                       // the chunk before this one has been multiplied
        stage_d(d, c0);
        stage_m(mm, c0);
        __syncthreads();
        if (c0 + 2 * kKC < Kp4) {
            fetch_d(d, c0 + 2 * kKC);
            fetch_m(mm, c0 + 2 * kKC);
        }
        if (active) {
            const int ks = min(kKC, Kp4 - c0);
            const float *ap = As + (wave * 16 + lr) * kLd + lk, *bp = Ms + lr * kLd + lk;
            auto step = [&](int k) {
                const float a = ap[k];
#pragma unroll
                for (int t = 0; t < kRowsTN; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[t * 16 * kLd + k], acc[t], 0, 0, 0);
            };
            if (ks == kKC) {
                mfma_chunk<kRowsTN>(acc, ap, bp, 16 * kLd, 1);
            } else {
                for (int k = 0; k < ks; k += 4) step(k);
            }
        }
    };
    for (int c0 = 0; c0 < Kp4; c0 += 2 * kKC) {
        chunk(dv[0], mv[0], c0);
        if (c0 + kKC < Kp4) chunk(dv[1], mv[1], c0 + kKC);
    }
    if (active) {
#pragma unroll
        for (int t = 0; t < kRowsTN; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int r = r0 + wave * 16 + lk * 4 + g, j = j0 + t * 16 + lr;
                if (r < ny && j < ldu) u[(long)r * ldu + j] = acc[t][g];
            }
    }
}

// ---- stage 2: Y[i0 .. i0+16*WM-1, j0 .. j0+16*TN-1] = My U, + anchor, store, partial range ------------------------------
// grid (ceil(bx / (16*TN)), ceil(by / (16*WM))); parts[blockIdx.y * gridDim.x + blockIdx.x] from every workgroup
template <int WM, int TN>
__global__ __launch_bounds__(64 * WM) void resample_cols_kernel(const float *__restrict__ my, int ldmy,
                                                                const float *__restrict__ u, int ldu, int ny, int by,
                                                                int bx, const float *__restrict__ anchor_in,
                                                                float *__restrict__ out, Part *__restrict__ parts) {
    constexpr int kThreads = 64 * WM, kRows = 16 * WM, W = 16 * TN, kLdb = W + 16;
    constexpr int kAPerThread = kRows * kKC / 4 / kThreads;    // 4 float4 of a chunk of My per thread
    constexpr int kBPerThread = kKC * W / 4 / kThreads;        // float4 of a chunk of U per thread
    constexpr int kBRow4 = W / 4;                              // float4 per staged row of U
    static_assert(kRows * kKC / 4 % kThreads == 0 && kKC * W / 4 % kThreads == 0, "whole float4 per thread");
    __shared__ __align__(16) float As[kRows * kLd];            // [rows of My][kLd]
    __shared__ __align__(16) float Bs[kKC * kLdb];             // [rows of U = K][kLdb]
    const int i0 = blockIdx.y * kRows, j0 = blockIdx.x * W;
    const int tid = threadIdx.x, wave = tid >> 6, lr = tid & 15, lk = (tid & 63) >> 4;
    const int Kp4 = (ny + 3) & ~3;

    // rows i0 .. of My, columns c0 .. c0+kKC-1 (my and ldmy are 16-byte aligned); rows past by and columns past ny are
    // staged as zeros
    auto fetch_a = [&](float4 (&v)[kAPerThread], int c0) {
#pragma unroll
        for (int k = 0; k < kAPerThread; ++k) {
            const int e = tid + k * kThreads;
            v[k] = fetch4(my, ldmy, by, Kp4, i0 + (e >> 4), c0 + (e & 15) * 4);
        }
    };
    auto stage_a = [&](const float4 (&v)[kAPerThread], int c0) {
#pragma unroll
        for (int k = 0; k < kAPerThread; ++k) {
            const int e = tid + k * kThreads;
            stage4(As + (e >> 4) * kLd + (e & 15) * 4, zero4(v[k], i0 + (e >> 4) < by, c0 + (e & 15) * 4, ny));
        }
    };
    // rows c0 .. c0+kKC-1 of U, columns j0 .. j0+W-1 (u is 16-byte aligned, ldu and j0 multiples of 4).  Rows at or past
    // ny were never written: fetched from row ny-1 instead and staged as zeros.  Columns at or past ldu likewise; they
    // reach only output columns that are not stored
    auto fetch_b = [&](float4 (&v)[kBPerThread], int c0) {
#pragma unroll
        for (int k = 0; k < kBPerThread; ++k) {
            const int e = tid + k * kThreads;
            v[k] = fetch4(u, ldu, ny, ldu, c0 + e / kBRow4, j0 + (e % kBRow4) * 4);
        }
    };
    auto stage_b = [&](const float4 (&v)[kBPerThread], int c0) {
#pragma unroll
        for (int k = 0; k < kBPerThread; ++k) {
            const int e = tid + k * kThreads, j = j0 + (e % kBRow4) * 4;
            *reinterpret_cast<float4 *>(Bs + (e / kBRow4) * kLdb + (e % kBRow4) * 4) =
                zero4(v[k], c0 + e / kBRow4 < ny && j < ldu, 0, 4);
        }
    };

    const bool active = i0 + wave * 16 < by;                   // wave-uniform
    f32x4 acc[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float4 av[2][kAPerThread], bv[2][kBPerThread];
    fetch_a(av[0], 0);
    fetch_b(bv[0], 0);
    if (kKC < Kp4) {
        fetch_a(av[1], kKC);
        fetch_b(bv[1], kKC);
    }
    auto chunk = [&](float4 (&a4)[kAPerThread], float4 (&b4)[kBPerThread], int c0) {
        __syncthreads();                                       // the chunk before this one has been multiplied
        stage_a(a4, c0);
        stage_b(b4, c0);
        __syncthreads();
        if (c0 + 2 * kKC < Kp4) {
            fetch_a(a4, c0 + 2 * kKC);
            fetch_b(b4, c0 + 2 * kKC);
        }
        if (active) {
            const int ks = min(kKC, Kp4 - c0);
            const float *ap = As + (wave * 16 + lr) * kLd + lk, *bp = Bs + lk * kLdb + lr;
            auto step = [&](int k) {
                const float a = ap[k];
#pragma unroll
                for (int t = 0; t < TN; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[k * kLdb + t * 16], acc[t], 0, 0, 0);
            };
            if (ks == kKC) {
                mfma_chunk<TN>(acc, ap, bp, 16, kLdb);
            } else {
                for (int k = 0; k < ks; k += 4) step(k);
            }
        }
    };
    for (int c0 = 0; c0 < Kp4; c0 += 2 * kKC) {
        chunk(av[0], bv[0], c0);
        if (c0 + kKC < Kp4) chunk(av[1], bv[1], c0 + kKC);
    }

    unsigned int lo = 0xffffffffu, hi = 0u;
    if (active) {
        const float anchor = anchor_in ? *anchor_in : 0.0f;
#pragma unroll
        for (int t = 0; t < TN; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = i0 + wave * 16 + lk * 4 + g, j = j0 + t * 16 + lr;
                if (i < by && j < bx) {
                    float y = acc[t][g];
                    if (anchor_in) y = __fadd_rn(y, anchor);
                    out[(long)i * bx + j] = y;
                    const unsigned int k = enc(y);
                    lo = min(lo, k);
                    hi = max(hi, k);
                }
            }
    }
    // every workgroup stores its pair (each holds at least one output): nothing to initialise
    if (block_reduce<kThreads>(lo, hi)) parts[blockIdx.y * gridDim.x + blockIdx.x] = Part{lo, hi};
}

inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
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
    return kHeadBytes + align16(max_parts(by, bx) * sizeof(Part)) + (size_t)ny * ldu_of(bx) * sizeof(float);
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
    float *u = (float *)((char *)parts + align16(max_parts(by, bx) * sizeof(Part)));
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
