// The chunked K pipeline of the tiled fp32 GEMMs on v_mfma_f32_16x16x4_f32 whose K loop over one accumulator is a
// contract's fmaf chain (resample.hip, psd.hip, extractfilter.hip, align.hip, alignsum.hip, class2d.hip; extract.hip takes
// the staging helpers only).  Not part of the ABI.
//
// A workgroup of THREADS threads (64 per wave) multiplies A [rows, K] by B [K, columns] in chunks of kKC positions of K
// through LDS, a wave on 16 rows of A with TN accumulators of 16 x 16.  Top to bottom: the operand loaders (what a chunk
// of each operand is, fetched into registers and staged into LDS), multiply (one staged chunk for one wave), k_loop (the
// schedule that ties them together), for_each_output (where a wave's accumulators sit in the output) and the four stage
// bodies that put these together for one output tile, with the two stores that several kernels end with.
// The bits: every accumulator takes its K positions in ascending order, four per MFMA, one rounding per product, from
// 0.0f, K never split; every staged element outside an operand is a zero formed in registers, on BOTH operands wherever
// K is padded (the other operand may be uninitialised memory, and fma(0, NaN, acc) is NaN).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "common.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int kKC = 64;                          // columns of K staged per chunk
constexpr int kLd = kKC + 2;                     // floats per staged row of an A operand (and of a row-major B^T operand):
                                                 // lane (row, k) of a fragment read sits on bank 2*row + k
constexpr int kPairRows = 64;                    // the paired form: staged rows 0 .. 63 are rows u, 64 .. 127 rows M + u

// A loader's destination is the kernel's __shared__ array as a pointer that says so: lds_ptr(As).  (Through a plain
// float * the compiler learns the address space only after its first passes, and then forms and schedules the staging
// stores differently: the M operand's stores ahead of the samples', which costs 1.7 % at 4096^2 -> 512^2.)
using f32x2 = __attribute__((ext_vector_type(2))) float;
using lds_float = __attribute__((address_space(3))) float;
using lds_f32x2 = __attribute__((address_space(3))) f32x2;
using lds_f32x4 = __attribute__((address_space(3))) f32x4;
// The cast is not checked: `a` must be a __shared__ array, nothing else.
template <int N>
__device__ __forceinline__ lds_float *lds_ptr(float (&a)[N]) {
    return (lds_float *)a;
}

// ---- 1. operand loaders --------------------------------------------------------------------------------------------------
// A loader moves one chunk of its operand: fetch(regs, c0) loads K positions c0 .. c0+kKC-1 into this thread's registers,
// stage(regs, c0) writes them to LDS.  Fetching and zeroing are apart.  A fetch is an unconditional load from an address
// clamped into the part of its array that may be read, and nothing touches the value until the chunk is staged, two
// chunks later: only so are a chunk's loads in flight together and behind the MFMAs of the chunks before.  (With the
// load under a branch, or a select on its value next to it, the compiler waited for every load right behind its issue:
// one round trip to memory after the other.)  Staging then turns every element outside the operand into a zero formed in
// registers.  Thread t holds elements t, t + THREADS, ... of the chunk.

// fetch4: the float4 at row min(row, rows-1), columns min(q, cols4-4) .. +3 (cols4 a multiple of 4, at least 4)
__device__ __forceinline__ float4 fetch4(const float *__restrict__ m, int ld, int rows, int cols4, int row, int q) {
    return *reinterpret_cast<const float4 *>(m + (long)min(row, rows - 1) * ld + min(q, cols4 - 4));
}
// zero4: the elements at K positions q .. q+3 that lie at or past `end`, or all four unless `in`, become zeros
__device__ __forceinline__ float4 zero4(float4 v, bool in, int q, int end) {
    return make_float4(in && q < end ? v.x : 0.0f, in && q + 1 < end ? v.y : 0.0f, in && q + 2 < end ? v.z : 0.0f,
                       in && q + 3 < end ? v.w : 0.0f);
}
// a float4 into a staged row of kLd floats (8-byte aligned: kLd is even), through a loader's pointer or, for
// extract_scale_kernel's dynamic LDS, a plain one
__device__ __forceinline__ void stage4(float *d, float4 v) {
    *reinterpret_cast<float2 *>(d) = make_float2(v.x, v.y);
    *reinterpret_cast<float2 *>(d + 2) = make_float2(v.z, v.w);
}
__device__ __forceinline__ void stage4(lds_float *d, float4 v) {
    *(lds_f32x2 *)d = f32x2{v.x, v.y};
    *(lds_f32x2 *)(d + 2) = f32x2{v.z, v.w};
}

// Sample rows: 64 rows r0 .. of raw samples of type S, kKC columns each, by element loads of their own type (a row of
// samples is only itemsize-aligned; a wave reads 64 adjacent samples of one row) into dst [64][kLd].  A fetched sample
// is widened by the load itself (packed pairs of 16-bit samples would need an operation on the loaded value right behind
// the load, and with it a wait); integer samples are staged as (float)(v - first), |difference| < 2^17: exact.  Rows at
// or past `rows` and columns at or past `cols` are fetched from the last row / column and staged as zeros.
template <typename S, int THREADS>
struct SampleRows {
    static constexpr bool kFloat = std::is_same<S, float>::value;
    using R = typename std::conditional<kFloat, float, int>::type;
    static constexpr int kPerThread = 64 * kKC / THREADS;
    using Regs = R[kPerThread];
    const S *__restrict__ base;                  // the sample at row 0, column 0
    int pitch, rows, cols, r0;                   // samples per row in memory; the operand is [rows, cols]
    S first;                                     // what the integer modes subtract
    lds_float *dst;

    __device__ __forceinline__ void fetch(Regs &v, int c0) const {
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int e = threadIdx.x + k * THREADS, r = r0 + (e >> 6), q = c0 + (e & 63);
            v[k] = base[(long)min(r, rows - 1) * pitch + min(q, cols - 1)];
        }
    }
    __device__ __forceinline__ void stage(const Regs &v, int c0) const {
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int e = threadIdx.x + k * THREADS, r = r0 + (e >> 6), q = c0 + (e & 63);
            float d;
            if constexpr (kFloat) d = v[k];
            else d = (float)(v[k] - (int)first);
            dst[(e >> 6) * kLd + (e & 63)] = (r < rows && q < cols) ? d : 0.0f;
        }
    }
};

// Which row of a row-major matrix a staged row rr holds (src; fetch4 clamps it below the matrix's rows) and whether it is
// a row of the operand at all (in; otherwise it is staged as zeros).
struct RowsFrom {                                // rows row0 .. of a matrix whose operand rows end at `limit`
    int row0, limit;
    __device__ __forceinline__ int src(int rr) const { return row0 + rr; }
    __device__ __forceinline__ bool in(int rr) const { return row0 + rr < limit; }
};
struct RowPairs {                                // rows u0 .. in staged rows 0 .. 63, then rows M + u0 .. (u < M both)
    int u0, M;
    __device__ __forceinline__ int src(int rr) const {
        return (rr >= kPairRows ? M : 0) + min(u0 + (rr & (kPairRows - 1)), M - 1);
    }
    __device__ __forceinline__ bool in(int rr) const { return u0 + (rr & (kPairRows - 1)) < M; }
};

// Matrix rows: ROWS rows (by `map`) of a row-major fp32 matrix, kKC columns each, as float4 (m 16-byte aligned, ld a
// multiple of 4) into dst [ROWS][kLd].  Fetched from rows below `rows` and columns below `cols4`; rows that are not `in`
// and K positions at or past `kend` are staged as zeros.
template <int ROWS, int THREADS, typename Map>
struct MatrixRows {
    static constexpr int kPerThread = ROWS * kKC / 4 / THREADS;
    static_assert(ROWS * kKC / 4 % THREADS == 0, "whole float4 per thread");
    using Regs = float4[kPerThread];
    const float *__restrict__ m;
    int ld, rows, cols4, kend;
    Map map;
    lds_float *dst;

    __device__ __forceinline__ void fetch(Regs &v, int c0) const {
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int e = threadIdx.x + k * THREADS;
            v[k] = fetch4(m, ld, rows, cols4, map.src(e >> 4), c0 + (e & 15) * 4);
        }
    }
    __device__ __forceinline__ void stage(const Regs &v, int c0) const {
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int e = threadIdx.x + k * THREADS;
            stage4(dst + (e >> 4) * kLd + (e & 15) * 4, zero4(v[k], map.in(e >> 4), c0 + (e & 15) * 4, kend));
        }
    }
};

// K-major rows: rows c0 .. c0+kKC-1 of a row-major fp32 matrix whose ROWS are K, columns col0 .. col0+W-1, as float4 (m
// 16-byte aligned, ld and col0 multiples of 4) into dst [kKC][W + 16] (the two k rows a half wave reads land on different
// banks).  Rows at or past `rows` and columns at or past `ld` are fetched from the last row / float4 and staged as zeros;
// kRagged: only columns below `end` were ever written, and the rest of their float4 is staged as zeros too.  What is
// zeroed by column reaches only output columns that are not stored.
template <int W, int THREADS, bool kRagged>
struct KMajorRows {
    static constexpr int kLdb = W + 16, kRow4 = W / 4, kPerThread = kKC * W / 4 / THREADS;
    static_assert(kKC * W / 4 % THREADS == 0, "whole float4 per thread");
    using Regs = float4[kPerThread];
    const float *__restrict__ m;
    int ld, rows, col0, end;                     // end is read only when kRagged (pass ld otherwise: every column was written)
    lds_float *dst;

    __device__ __forceinline__ void fetch(Regs &v, int c0) const {
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int e = threadIdx.x + k * THREADS;
            v[k] = fetch4(m, ld, rows, ld, c0 + e / kRow4, col0 + (e % kRow4) * 4);
        }
    }
    __device__ __forceinline__ void stage(const Regs &v, int c0) const {
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int e = threadIdx.x + k * THREADS, j = col0 + (e % kRow4) * 4;
            const bool in = c0 + e / kRow4 < rows && j < ld;
            const float4 z = kRagged ? zero4(v[k], in, j, end) : zero4(v[k], in, 0, 4);
            *(lds_f32x4 *)(dst + (e / kRow4) * kLdb + (e % kRow4) * 4) = f32x4{z.x, z.y, z.z, z.w};
        }
    }
};

// ---- 2. one staged chunk for one wave ------------------------------------------------------------------------------------
// Lane (lr, lk) of a wave reads A at staged row wave*16 + lr (and, paired, kPairRows rows further), K position k + lk,
// and B of its 16-column tile t at column t*16 + lr, K position k + lk, in either staged layout of B:
__device__ __forceinline__ const float *a_frag(const float *As, int wave, int lr, int lk) {
    return As + (wave * 16 + lr) * kLd + lk;
}
struct BtRows {                                  // row-major B^T [columns][kLd]: the loaders SampleRows and MatrixRows
    static constexpr int kTileStride = 16 * kLd, kStep = 1;
    static __device__ __forceinline__ const float *frag(const float *Bs, int lr, int lk) { return Bs + lr * kLd + lk; }
};
template <int W>
struct KMajor {                                  // K-major B [kKC][W + 16]: the loader KMajorRows
    static constexpr int kTileStride = 16, kStep = W + 16;
    static __device__ __forceinline__ const float *frag(const float *Bs, int lr, int lk) { return Bs + lk * kStep + lr; }
};

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

// The ks (a multiple of 4, at most kKC) K positions of the staged chunk into acc[t], t the tile of B: k ascending in every
// accumulator.  A whole chunk is fully unrolled, with plain reads at each step or, kGrouped, mfma_chunk's read-ahead; a
// shorter one is a rolled loop.
template <typename B, bool kGrouped, int TN>
__device__ __forceinline__ void multiply(f32x4 (&acc)[TN], const float *ap, const float *bp, int ks) {
    auto step = [&](int k) {
        const float a = ap[k];
#pragma unroll
        for (int t = 0; t < TN; ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[t * B::kTileStride + k * B::kStep], acc[t], 0, 0, 0);
    };
    if (ks == kKC) {
        if constexpr (kGrouped) {
            mfma_chunk<TN>(acc, ap, bp, B::kTileStride, B::kStep);
        } else {
#pragma unroll
            for (int k = 0; k < kKC; k += 4) step(k);
        }
    } else {
        for (int k = 0; k < ks; k += 4) step(k);
    }
}
// The paired form: the lane's two rows of A (ap[k] and, kPairRows staged rows further, its partner) into re[t] and im[t]
// with one read of B per step and tile; plain reads only.
template <typename B, int TN>
__device__ __forceinline__ void multiply_pair(f32x4 (&re)[TN], f32x4 (&im)[TN], const float *ap, const float *bp, int ks) {
    auto step = [&](int k) {
        const float a_re = ap[k], a_im = ap[kPairRows * kLd + k];
#pragma unroll
        for (int t = 0; t < TN; ++t) {
            const float b = bp[t * B::kTileStride + k * B::kStep];
            re[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_re, b, re[t], 0, 0, 0);
            im[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_im, b, im[t], 0, 0, 0);
        }
    };
    if (ks == kKC) {
#pragma unroll
        for (int k = 0; k < kKC; k += 4) step(k);
    } else {
        for (int k = 0; k < ks; k += 4) step(k);
    }
}

// ---- 3. the K loop -------------------------------------------------------------------------------------------------------
// K positions 0 .. Kp-1 (Kp the padded K, a multiple of 4) in chunks of kKC, ascending: mul(ks) is called once per chunk
// with that chunk of both operands staged, in waves that are `active` (wave-uniform; the others fetch and stage only).
// Two chunks are fetched ahead into two register sets that alternate: chunk c's registers are refilled with chunk c + 2
// right behind its staging, and are touched by nothing until that chunk is staged in turn (see 1. for why).  The first
// barrier of a chunk says that the chunk before it has been multiplied, the second that this one is staged.
// k_chunk is a function inlined by force and not a lambda, and the accumulators are declared and zeroed in the kernel and
// reach mul by reference: behind a second closure, or zeroed by a helper, the compiler kept them as one wide vector and
// moved them between AGPRs and VGPRs in every chunk.
template <typename LA, typename LB, typename Mul>
__device__ __forceinline__ void k_chunk(int Kp, const LA &la, const LB &lb, bool active, const Mul &mul,
                                        typename LA::Regs &a, typename LB::Regs &b, int c0) {
    __syncthreads();
    la.stage(a, c0);
    lb.stage(b, c0);
    __syncthreads();
    if (c0 + 2 * kKC < Kp) {
        la.fetch(a, c0 + 2 * kKC);
        lb.fetch(b, c0 + 2 * kKC);
    }
    if (active) mul(min(kKC, Kp - c0));
}
template <typename LA, typename LB, typename Mul>
__device__ __forceinline__ void k_loop(int Kp, const LA &la, const LB &lb, bool active, const Mul &mul) {
    typename LA::Regs av[2];
    typename LB::Regs bv[2];
    la.fetch(av[0], 0);
    lb.fetch(bv[0], 0);
    if (kKC < Kp) {
        la.fetch(av[1], kKC);
        lb.fetch(bv[1], kKC);
    }
    for (int c0 = 0; c0 < Kp; c0 += 2 * kKC) {
        k_chunk(Kp, la, lb, active, mul, av[0], bv[0], c0);
        if (c0 + kKC < Kp) k_chunk(Kp, la, lb, active, mul, av[1], bv[1], c0 + kKC);
    }
}

// ---- 4. the accumulator walk ---------------------------------------------------------------------------------------------
// Element g of acc[t] in lane (lr, lk) is output row r0 + wave*16 + lk*4 + g, column c0 + t*16 + lr: f(row, column,
// value) for all of them, tiles in order and g ascending within a tile; the paired form calls f(row, column, re, im).
// Rows and columns past the output are the caller's to skip.
template <int TN, typename F>
__device__ __forceinline__ void for_each_output(const f32x4 (&acc)[TN], int r0, int c0, int wave, int lk, int lr, F f) {
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) f(r0 + wave * 16 + lk * 4 + g, c0 + t * 16 + lr, acc[t][g]);
}
template <int TN, typename F>
__device__ __forceinline__ void for_each_output(const f32x4 (&re)[TN], const f32x4 (&im)[TN], int r0, int c0, int wave, int lk,
                                                int lr, F f) {
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) f(r0 + wave * 16 + lk * 4 + g, c0 + t * 16 + lr, re[t][g], im[t][g]);
}

// ---- 5. the stage bodies -------------------------------------------------------------------------------------------------
// One output tile at rows r0 .., columns c0 .. from start to end: the two staged operands (each body owns its __shared__
// arrays: a kernel calls one body), the loaders, the wave-uniform `active`, the accumulators, the K loop and the walk.  K is
// the operands' own extent; it is padded here to Kp = sprk::roundup4(K), the zeros formed at staging on both operands.  A kernel
// is its index set-up, one call of a body and its store: store(row, column, value) or, paired, store(row, column, re, im),
// called by the active waves for every element of the tile, those past the output included (the store skips them).
// The accumulators are declared and zeroed in the body itself, which is inlined by force, and reach mul by reference (3.).
// A store captures what it needs BY VALUE ([=]; by reference only what it changes): behind captured references the compiler
// formed the output address anew for every element (60 instructions more in the epilogue of each V-split kernel).

// Sample rows x matrix rows^T, 64 x 64 on four waves: out[r, j] = chain over c < cols of (D[r, c] - first) * M[j, c], D the
// [rows, cols] samples at `base` (pitch samples per row), M [mrows, ldm] (ldm at least roundup4(cols)).
template <bool kGrouped, typename S, typename Store>
__device__ __forceinline__ void sample_rows_body(const S *__restrict__ base, int pitch, int rows, int cols, S first,
                                                 const float *__restrict__ m, int ldm, int mrows, int r0, int c0,
                                                 Store store) {
    constexpr int kThreads = 256, kTN = 4;
    __shared__ __align__(16) float As[64 * kLd];               // [64 rows of D][kLd]
    __shared__ __align__(16) float Ms[64 * kLd];               // [64 rows of M][kLd]
    const int tid = threadIdx.x, wave = tid >> 6, lr = tid & 15, lk = (tid & 63) >> 4;
    const int Kp = sprk::roundup4(cols);
    const SampleRows<S, kThreads> d{base, pitch, rows, cols, r0, first, lds_ptr(As)};
    const MatrixRows<64, kThreads, RowsFrom> b{m, ldm, mrows, Kp, cols, RowsFrom{c0, mrows}, lds_ptr(Ms)};
    const bool active = r0 + wave * 16 < rows;                 // wave-uniform
    f32x4 acc[kTN];
#pragma unroll
    for (int t = 0; t < kTN; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    k_loop(Kp, d, b, active,
           [&](int ks) { multiply<BtRows, kGrouped>(acc, a_frag(As, wave, lr, lk), BtRows::frag(Ms, lr, lk), ks); });
    if (active) for_each_output(acc, r0, c0, wave, lk, lr, store);
}

// Matrix rows x K-major rows, 16*WM x 16*TN on WM waves: out[i, j] = chain over r < K of A[i, r] * U[r, j], from 0.0f or,
// with `init`, from init[i * cols + j]; A [arows, lda], U [K, ldu] with every column below ldu written, cols <= ldu.
template <int WM, int TN, typename Store>
__device__ __forceinline__ void kmajor_rows_body(const float *__restrict__ a, int lda, int arows, int K,
                                                 const float *__restrict__ u, int ldu, int cols, const float *init, int r0,
                                                 int c0, Store store) {
    constexpr int kThreads = 64 * WM, kRows = 16 * WM, W = 16 * TN;
    using URows = KMajorRows<W, kThreads, false>;
    __shared__ __align__(16) float As[kRows * kLd];            // [rows of A][kLd]
    __shared__ __align__(16) float Bs[kKC * URows::kLdb];      // [rows of U = K][kLdb]
    const int tid = threadIdx.x, wave = tid >> 6, lr = tid & 15, lk = (tid & 63) >> 4;
    const int Kp = sprk::roundup4(K);
    // rows of U at or past K were never written: fetched from row K-1 instead and staged as zeros
    const MatrixRows<kRows, kThreads, RowsFrom> la{a, lda, arows, Kp, K, RowsFrom{r0, arows}, lds_ptr(As)};
    const URows lb{u, ldu, K, c0, ldu, lds_ptr(Bs)};
    const bool active = r0 + wave * 16 < arows;                // wave-uniform
    f32x4 acc[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (active && init) {                                      // the chain goes on where it was left
#pragma unroll
        for (int t = 0; t < TN; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = r0 + wave * 16 + lk * 4 + g, j = c0 + t * 16 + lr;
                if (i < arows && j < cols) acc[t][g] = init[(long)i * cols + j];
            }
    }
    k_loop(Kp, la, lb, active,
           [&](int ks) { multiply<KMajor<W>, true>(acc, a_frag(As, wave, lr, lk), KMajor<W>::frag(Bs, lr, lk), ks); });
    if (active) for_each_output(acc, r0, c0, wave, lk, lr, store);
}

// Paired rows x K-major rows, 64 x 64 on four waves: re[u, v] = chain over t < K of W[u, t] * B[t, v], im with row M + u;
// W [2M, ldw], B [K, ldb] of which only columns below `end` were ever written.
template <typename Store>
__device__ __forceinline__ void paired_rows_body(const float *__restrict__ w, int ldw, int M, int K,
                                                 const float *__restrict__ b, int ldb, int end, int r0, int c0,
                                                 Store store) {
    constexpr int kThreads = 256, kTN = 4;
    using BRows = KMajorRows<64, kThreads, true>;
    __shared__ __align__(16) float As[2 * kPairRows * kLd];    // [64 rows u, then 64 rows M + u][kLd]
    __shared__ __align__(16) float Bs[kKC * BRows::kLdb];      // [rows of B = K][kLdb]
    const int tid = threadIdx.x, wave = tid >> 6, lr = tid & 15, lk = (tid & 63) >> 4;
    const int Kp = sprk::roundup4(K);
    const MatrixRows<2 * kPairRows, kThreads, RowPairs> la{w, ldw, 2 * M, Kp, K, RowPairs{r0, M}, lds_ptr(As)};
    const BRows lb{b, ldb, K, c0, end, lds_ptr(Bs)};
    const bool active = r0 + wave * 16 < M;                    // wave-uniform
    f32x4 re[kTN], im[kTN];
#pragma unroll
    for (int t = 0; t < kTN; ++t) re[t] = im[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    k_loop(Kp, la, lb, active, [&](int ks) {
        multiply_pair<KMajor<64>>(re, im, a_frag(As, wave, lr, lk), KMajor<64>::frag(Bs, lr, lk), ks);
    });
    if (active) for_each_output(re, im, r0, c0, wave, lk, lr, store);
}

// Matrix rows x matrix rows^T, 64 x 64 on four waves: out[i, j] = chain over t < K of A[i, t] * B[j, t]; A [arows, lda],
// B [brows, ldb], both strides at least roundup4(K).
template <bool kGrouped, typename Store>
__device__ __forceinline__ void matrix_rows_body(const float *__restrict__ a, int lda, int arows,
                                                 const float *__restrict__ b, int ldb, int brows, int K, int r0, int c0,
                                                 Store store) {
    constexpr int kThreads = 256, kTN = 4;
    __shared__ __align__(16) float As[64 * kLd];               // [64 rows of A][kLd]
    __shared__ __align__(16) float Ms[64 * kLd];               // [64 rows of B][kLd]
    const int tid = threadIdx.x, wave = tid >> 6, lr = tid & 15, lk = (tid & 63) >> 4;
    const int Kp = sprk::roundup4(K);
    const MatrixRows<64, kThreads, RowsFrom> la{a, lda, arows, Kp, K, RowsFrom{r0, arows}, lds_ptr(As)};
    const MatrixRows<64, kThreads, RowsFrom> lb{b, ldb, brows, Kp, K, RowsFrom{c0, brows}, lds_ptr(Ms)};
    const bool active = r0 + wave * 16 < arows;                // wave-uniform
    f32x4 acc[kTN];
#pragma unroll
    for (int t = 0; t < kTN; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    k_loop(Kp, la, lb, active,
           [&](int ks) { multiply<BtRows, kGrouped>(acc, a_frag(As, wave, lr, lk), BtRows::frag(Ms, lr, lk), ks); });
    if (active) for_each_output(acc, r0, c0, wave, lk, lr, store);
}

// The two stores that more than one kernel ends with.
// U[r, q] of a [rows, 2H] tile product into V = [U[:, :H] ; U[:, H:]] [2 rows, ldv]: the sine half goes below the cosine
// half.  The address is formed outside the condition, so once per tile of the walk and not once per element.
__device__ __forceinline__ void store_v_split(float *v, int ldv, int rows, int H, int r, int q, float u) {
    const int part = q >= H;
    float *p = v + (long)(part * rows + r) * ldv + (q - part * H);
    if (r < rows && q < 2 * H) *p = u;
}
// (Zr, Zi)[u, v] of an [M, H] pair into Z = [Zr, Zi] [M, ldz]
__device__ __forceinline__ void store_zr_zi(float *z, int ldz, int M, int H, int u, int v, float zr, float zi) {
    if (u < M && v < H) {
        z[(long)u * ldz + v] = zr;
        z[(long)u * ldz + H + v] = zi;
    }
}

}  // namespace
