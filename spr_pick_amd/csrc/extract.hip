// Particle extraction: boxes cut out of the sample block of a 2-D MRC image, as it sits in the file, binned, background-
// normalised and optionally contrast-inverted (`joint extract`, spr_pick_amd/extract.py).
//
// raw: the buffer sprk_ingest_bin takes (modes 0 int8, 1 int16, 2 float32, 6 uint16).  xy [P, 2] int32 on the device:
// (x along nx, y along ny) of each centre in raw samples.  Particle p covers rows y0 .. y0+B-1 and columns x0 .. x0+B-1,
// x0 = x - B/2, y0 = y - B/2; output pixel (i, j) of its [b, b] image, b = B / N, is the N x N block at (y0 + iN, x0 + jN).
//   block value v: integer modes the exact int32 sum; float32 fp32 adds from 0.0f in row-major order within the block,
//       every add its own rounding (sprk_ingest_bin's order);
//   a box that is not entirely inside the image: status 1, all zeros, and NOT ONE sample of it is read — the coordinates
//       live in device memory, so this check is the kernel's (in 64-bit: any int32 centre is safe);
//   without SPRK_EXTRACT_NORMALIZE: out = float(v) / float(N*N), one correctly rounded division (sprk_ingest_bin's value);
//   with it: background = {(i, j): (i - b/2)^2 + (j - b/2)^2 > R^2}, n pixels; n == 0 -> status 2, zeros;
//       integer modes: d = v - v[0,0] (int32), S1 = sum_bg d, S2 = sum_bg d^2 exact in int64, mean = double(S1) / double(n),
//           var = double(S2) / double(n) - mean*mean (two roundings, no fma); !(var > 0) -> status 2, zeros; else
//           out = float((double(d) - mean) / sqrt(var));
//       float32: two passes in double over the fp32 v: mean = sum_bg v / n, var = sum_bg (v - mean)^2 / n, same rule and
//           formula with v in place of d;
//   SPRK_EXTRACT_INVERT negates the output.
//
// One workgroup per particle.  Phase 1: lanes stride over the output pixels (adjacent lanes read adjacent chunks of a
// row), kUnroll pixels per lane at a time, and form d or v and their share of the background sums.  Phase 2: the sums
// over the wave by an xor butterfly (both partners add the same two numbers, so every lane holds the same bits), over
// the workgroup through LDS with the waves added in index order — a fixed order, no atomics: the same call gives the
// same bytes.  Phase 3: write.  The box's d / v stay in LDS between the phases when 4*b*b bytes fit kResidentBytes; a
// larger box is formed again from global memory (its samples were just read: L2 serves them).  Every lane meets in
// phases 2 and 3 the pixels it formed in phase 1, so the resident values need no barrier of their own.
// Box rows start at an arbitrary x0 and are only itemsize-aligned: every sample is fetched by an element load of its
// own type, never by a wider one, and only samples of rows y0 .. y0+B-1, columns x0 .. x0+B-1 of an inside box are
// addressed.
//
// Compiled with -ffp-contract=off like ingest.hip (Makefile): mean*mean and the subtraction are separate roundings.
#include <cstdint>
#include <type_traits>

#include "common.h"
#include "box_dev.h"
#include "mfma_stage.h"
#include "mrc_host.h"

namespace {

constexpr int kThreads = kBoxThreads;
constexpr int kWaves = kBoxWaves;
constexpr int kUnroll = 8;                       // output pixels a lane forms together (for_each_pixel)
constexpr int kScratchBytes = 128;              // head of the dynamic LDS: kWaves slots of 8 bytes for the reductions
// LDS residency of a box: 4*b*b <= 64 KiB, b <= 128.  A workgroup may take all 160 KiB of a CU (b <= 202), but it
// would then be the CU's only one — four waves to hide the latency of phase 1's loads.  64 KiB keeps two workgroups
// (eight waves) on a CU at the largest resident box and more at the usual ones (b = 64: 16 KiB, nine workgroups).
constexpr int kResidentBytes = 64 * 1024;
constexpr int kMaxBox = 1024;

template <typename T>
struct Sum {                                    // the contract's block accumulator
    using value = int;
    int v = 0;
    __device__ __forceinline__ void add(T s) { v += (int)s; }
};
template <>
struct Sum<float> {
    using value = float;
    float v = 0.0f;
    __device__ __forceinline__ void add(float s) { v = __fadd_rn(v, s); }
};

// Calls f(e, i, j, v) for every output pixel e = i*b + j of this thread's share (e = tid, tid + kThreads, ...), v its
// block value.  kUnroll pixels are formed together: their loads do not depend on one another, so a lane keeps kUnroll
// of them in flight instead of one (a particle is one workgroup: with one load per lane in flight a 256 x 256 box
// is 256 dependent round trips to memory: measured 288 us for 1000 such boxes, 154 us with eight in flight).  Each pixel's own adds keep the
// contract's order.  A slot past the last pixel reads the box's first block (valid samples) and is dropped.
// Samples read: origin[r*nx + q], 0 <= r, q < b*N.
template <typename T, typename F>
__device__ __forceinline__ void for_each_pixel(const T *__restrict__ origin, int nx, int N, int b, float inv_b, F f) {
    const int npix = b * b;
    for (int e0 = threadIdx.x; e0 < npix; e0 += kUnroll * kThreads) {
        const T *p[kUnroll];
        int row[kUnroll];
        Sum<T> acc[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int e = e0 + u * kThreads;
            row[u] = e < npix ? fast_div(e, inv_b) : 0;                // exact: e < 2^20 (common.h; every b checked)
            const int col = e < npix ? e - row[u] * b : 0;
            p[u] = origin + (long)(row[u] * N) * nx + col * N;
        }
        for (int r = 0; r < N; ++r) {
            for (int q = 0; q < N; ++q) {
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) acc[u].add(p[u][q]);
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) p[u] += nx;
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int e = e0 + u * kThreads;
            if (e < npix) f(e, row[u], e - row[u] * b, acc[u].v);
        }
    }
}

// grid: P workgroups.  resident: the dynamic LDS holds kScratchBytes + 4*b*b bytes, else kScratchBytes.
template <typename T>
__global__ __launch_bounds__(kThreads) void extract_kernel(const T *__restrict__ raw, int ny, int nx,
                                                           const int *__restrict__ xy, int B, int N, float inv_b,
                                                           long R2, int flags, int resident, float *__restrict__ out,
                                                           int *__restrict__ status) {
    using V = typename Sum<T>::value;
    extern __shared__ __align__(16) unsigned char lds[];
    V *box = reinterpret_cast<V *>(lds + kScratchBytes);
    const int p = blockIdx.x, b = B / N, npix = b * b, c = b / 2;
    const bool invert = flags & SPRK_EXTRACT_INVERT;
    float *o = out + (long)p * npix;
    const long x0 = (long)xy[2 * p] - B / 2, y0 = (long)xy[2 * p + 1] - B / 2;
    if (x0 < 0 || y0 < 0 || x0 + B > nx || y0 + B > ny) {      // before any sample is addressed
        zero_box(o, npix, status + p, 1);
        return;
    }
    const T *origin = raw + y0 * nx + x0;                      // samples read: origin[r*nx + q], 0 <= r, q < B
    auto is_bg = [&](int i, int j) { return (long)((i - c) * (i - c) + (j - c) * (j - c)) > R2; };

    if (!(flags & SPRK_EXTRACT_NORMALIZE)) {
        const float nn = (float)(N * N);
        for_each_pixel(origin, nx, N, b, inv_b, [&](int e, int, int, V v) {
            const float m = __fdiv_rn((float)v, nn);           // |integer sum| <= 16^2 * 65535 < 2^24: exact
            o[e] = invert ? -m : m;
        });
        if (threadIdx.x == 0) status[p] = 0;
        return;
    }

    int n = 0;
    double mean, var;
    V anchor = 0;
    if constexpr (std::is_same<T, float>::value) {
        double s = 0.0;
        for_each_pixel(origin, nx, N, b, inv_b, [&](int e, int i, int j, float v) {
            if (resident) box[e] = v;
            if (is_bg(i, j)) {
                s += (double)v;
                ++n;
            }
        });
        n = block_sum(n, reinterpret_cast<int *>(lds));
        if (n == 0) {
            zero_box(o, npix, status + p, 2);
            return;
        }
        mean = block_sum(s, reinterpret_cast<double *>(lds)) / (double)n;
        double q = 0.0;
        auto square = [&](int, int i, int j, float v) {
            if (is_bg(i, j)) {
                const double t = (double)v - mean;
                q += t * t;
            }
        };
        if (resident) {
            for (int e = threadIdx.x; e < npix; e += kThreads) {
                const int i = fast_div(e, inv_b);
                square(e, i, e - i * b, box[e]);
            }
        } else {
            for_each_pixel(origin, nx, N, b, inv_b, square);   // the same pixels in the same order per lane
        }
        var = block_sum(q, reinterpret_cast<double *>(lds)) / (double)n;
    } else {
        // |d| <= 2 * N^2 * 65535 < 2^26 and S2 <= b^2 * d^2 = 4 * B^2 * N^2 * 65535^2 <= 4.6e18 < 2^63 at B = 1024,
        // N = 16: the int64 sums cannot overflow for any box sprk_extract_boxes admits (kMaxBox)
        Sum<T> first;                                          // v[0, 0]; every lane the same addresses: broadcasts
        for (int r = 0; r < N; ++r)
            for (int q = 0; q < N; ++q) first.add(origin[(long)r * nx + q]);
        anchor = first.v;
        long long s1 = 0, s2 = 0;
        for_each_pixel(origin, nx, N, b, inv_b, [&](int e, int i, int j, int v) {
            const int d = v - anchor;
            if (resident) box[e] = d;
            if (is_bg(i, j)) {
                s1 += d;
                s2 += (long long)d * d;
                ++n;
            }
        });
        n = block_sum(n, reinterpret_cast<int *>(lds));
        if (n == 0) {
            zero_box(o, npix, status + p, 2);
            return;
        }
        s1 = block_sum(s1, reinterpret_cast<long long *>(lds));
        s2 = block_sum(s2, reinterpret_cast<long long *>(lds));
        mean = (double)s1 / (double)n;
        var = __dsub_rn((double)s2 / (double)n, __dmul_rn(mean, mean));
    }
    if (!(var > 0.0)) {                                        // the same bits in every lane: a uniform branch
        zero_box(o, npix, status + p, 2);
        return;
    }
    const double sd = sqrt(var);
    auto write = [&](int e, V d) {
        const float r = (float)(((double)d - mean) / sd);
        o[e] = invert ? -r : r;
    };
    if (resident) {
        for (int e = threadIdx.x; e < npix; e += kThreads) write(e, box[e]);
    } else {
        for_each_pixel(origin, nx, N, b, inv_b, [&](int e, int, int, V v) {
            if constexpr (std::is_same<T, float>::value) write(e, v);
            else write(e, v - anchor);
        });
    }
    if (threadIdx.x == 0) status[p] = 0;
}

template <typename T>
int launch_extract(const void *raw, int ny, int nx, const int *xy, int P, int B, int N, int R, int flags, float *out,
                   int *status, hipStream_t s) {
    const int b = B / N;
    const size_t box_bytes = (size_t)4 * b * b;
    const int resident = (flags & SPRK_EXTRACT_NORMALIZE) && box_bytes <= (size_t)kResidentBytes;
    const size_t lds = kScratchBytes + (resident ? box_bytes : 0);
    if (int rc = sprk::lds_optin(extract_kernel<T>, kScratchBytes + kResidentBytes, "extract_boxes"))
        return rc;
    hipLaunchKernelGGL(extract_kernel<T>, dim3(P), dim3(kThreads), lds, s, (const T *)raw, ny, nx, xy, B, N,
                       1.0f / (float)b, (long)R * R, flags, resident, out, status);
    return sprk::check_launch("extract_boxes");
}

// ---- Fourier-cropped boxes: sprk_extract_scale ---------------------------------------------------------------------------
// Y = M D M^T per particle, M [S, B] the Dirichlet-kernel resampler of extract.crop_matrix (IDFT_S . crop . DFT_B), D the
// B x B box (integer modes: minus its first sample, exact in fp32), as two fp32 GEMMs on v_mfma_f32_16x16x4_f32:
//   U[r, j] = fmaf chain over c = 0 .. B-1 ascending of D[r, c] * M[j, c], from 0.0f;
//   Y[i, j] = fmaf chain over r = 0 .. B-1 ascending of M[i, r] * U[r, j], from 0.0f;
// one accumulator per output element and stage, K never split: the MFMA adds its four k in ascending order into the
// accumulator it is given, one rounding per product, so the bytes are those of the two chains (tests/extract_scale_model.py).
// Operands past the box (K padded to a multiple of 4, rows to a multiple of 16) are zeros formed in registers, never
// memory outside the box, and fma(0, d, acc) = acc.
//
// One workgroup per particle.  The output columns are cut into strips of 16*TN; per strip, stage 1 leaves U[:, strip] in
// LDS and stage 2 multiplies it by M.  Both stages walk blocks of kRows output rows, one 16-row tile per wave with its TN
// accumulators in registers over the whole K loop, and take their operands in chunks of kKC columns through LDS: the A
// operand (stage 1: samples by element loads of their own type, converted once; stage 2: rows of M) and, in stage 1, the
// strip's rows of M.  The next two chunks are fetched into registers before the current one is multiplied.  A staged row is
// kLd = kKC + 2 floats long (mfma_stage.h, whose chunk size and stage4 this kernel shares; its K loops stay its own: they
// run inside the kernel's strip and row-block loops, the fetch is predicated and U lives in LDS).
// U rows are 16*TN floats; when that is a multiple of 32, odd rows swap their 16-column halves, so that the two k rows a
// half wave reads land on different banks.
// Not normalised: the epilogue of stage 2 adds the anchor and stores.  Normalised: it stores Y, and after a workgroup
// barrier the workgroup reads its own Y back (L2) for the two double sums (block_sum: a fixed order) and the final store
// (normalize_box, box_dev.h).
constexpr int kRows = 16 * kWaves;               // output rows per row block
constexpr int kMaxTN = 4;                        // 16-column tiles per strip and wave: at most four accumulators
constexpr int kStripBytes = 64 * 1024;           // U[:, strip] in LDS: the strip narrows until roundup(B, 16) * 16*TN * 4 fits
constexpr int kDPerThread = kRows * kKC / kThreads;        // 16 samples of a chunk per thread
constexpr int kMPerThread = kRows * kKC / 4 / kThreads;    // 4 float4 of 64 rows of M per thread

__host__ __device__ constexpr size_t scale_lds_bytes(int B, int TN) {
    return kScratchBytes + sizeof(float) * ((size_t)kRows * kLd + (size_t)16 * TN * kLd + (size_t)((B + 15) & ~15) * 16 * TN);
}

template <typename T, int TN>
__global__ __launch_bounds__(kThreads) void extract_scale_kernel(const T *__restrict__ raw, int ny, int nx,
                                                                 const int *__restrict__ xy, int B, int S,
                                                                 const float *__restrict__ m, int ldm, float inv_s, long R2,
                                                                 int flags, float *__restrict__ out, int *__restrict__ status) {
    constexpr bool kFloat = std::is_same<T, float>::value;
    constexpr int W = 16 * TN;
    constexpr int kSwizzle = (W % 32 == 0) ? 16 : 0;
    extern __shared__ __align__(16) unsigned char lds[];
    float *As = reinterpret_cast<float *>(lds + kScratchBytes);        // [kRows][kLd]
    float *Ms = As + kRows * kLd;                                      // [W][kLd]
    float *U = Ms + W * kLd;                                           // [roundup(B, 16)][W]
    const int p = blockIdx.x, npix = S * S;
    const bool invert = flags & SPRK_EXTRACT_INVERT, normalize = flags & SPRK_EXTRACT_NORMALIZE;
    float *o = out + (long)p * npix;
    const long x0 = (long)xy[2 * p] - B / 2, y0 = (long)xy[2 * p + 1] - B / 2;
    if (x0 < 0 || y0 < 0 || x0 + B > nx || y0 + B > ny) {      // before any sample is addressed
        zero_box(o, npix, status + p, 1);
        return;
    }
    const T *origin = raw + y0 * nx + x0;                      // samples read: origin[r*nx + q], 0 <= r, q < B
    const int tid = threadIdx.x, wave = tid >> 6, lr = tid & 15, lk = (tid & 63) >> 4;
    const int Bp4 = sprk::roundup4(B), Bp16 = (B + 15) & ~15, Sp16 = (S + 15) & ~15;
    const T first = origin[0];                                 // every lane the same address: a broadcast
    const float anchor = kFloat ? 0.0f : (float)first;

    // the chunk of D at rows r0 .., columns c0 ..: thread t holds elements t, t + kThreads, ... of the [kRows][kKC] chunk
    // (a wave reads 64 adjacent samples of one row); positions past the box hold the anchor, whose D is 0
    auto fetch_d = [&](T (&v)[kDPerThread], int r0, int c0) {
#pragma unroll
        for (int u = 0; u < kDPerThread; ++u) {
            const int e = tid + u * kThreads, r = r0 + (e >> 6), q = c0 + (e & 63);
            v[u] = (r < B && q < B) ? origin[(long)r * nx + q] : (kFloat ? (T)0 : first);
        }
    };
    auto stage_d = [&](const T (&v)[kDPerThread]) {
#pragma unroll
        for (int u = 0; u < kDPerThread; ++u) {
            const int e = tid + u * kThreads;
            float d;
            if constexpr (kFloat) d = v[u];
            else d = (float)((int)v[u] - (int)first);          // |difference| < 2^17: exact
            As[(e >> 6) * kLd + (e & 63)] = d;
        }
    };
    // rows j0 .. j0+rows-1 of M, columns c0 .. c0+kKC-1, as float4 (m and ldm are 16-byte aligned); rows past S and
    // columns past roundup(B, 4) are zeros and are not read
    auto fetch_m = [&](float4 *v, int n4, int rows, int j0, int c0) {
#pragma unroll
        for (int u = 0; u < n4; ++u) {
            const int e = tid + u * kThreads, j = j0 + (e >> 4), q = c0 + (e & 15) * 4;
            v[u] = (e < rows * 16 && j < S && q < Bp4) ? *reinterpret_cast<const float4 *>(m + (long)j * ldm + q)
                                                      : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    };
    auto stage_m = [&](const float4 *v, int n4, int rows, float *dst) {
#pragma unroll
        for (int u = 0; u < n4; ++u) {
            const int e = tid + u * kThreads;
            if (e < rows * 16) stage4(dst + (e >> 4) * kLd + (e & 15) * 4, v[u]);
        }
    };
    auto u_at = [&](int r, int j) -> float & { return U[r * W + (j ^ ((r & 1) ? kSwizzle : 0))]; };

    for (int j0 = 0; j0 < Sp16; j0 += W) {
        // stage 1: U[:, j0 .. j0+W-1]
        for (int r0 = 0; r0 < Bp16; r0 += kRows) {
            const bool active = r0 + wave * 16 < Bp16;         // wave-uniform
            f32x4 acc[TN];
#pragma unroll
            for (int t = 0; t < TN; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            // two chunks are in flight: the samples come from HBM (every chunk is 64 rows of one cache line each), and
            // one chunk's MFMAs are shorter than that round trip
            T dv[2][kDPerThread];
            float4 mv[2][TN];
            fetch_d(dv[0], r0, 0);
            fetch_m(mv[0], TN, W, j0, 0);
            if (kKC < Bp4) {
                fetch_d(dv[1], r0, kKC);
                fetch_m(mv[1], TN, W, j0, kKC);
            }
            auto chunk = [&](T (&d)[kDPerThread], float4 (&mm)[TN], int c0) {
                __syncthreads();                               // the chunk before this one has been multiplied
                stage_d(d);
                stage_m(mm, TN, W, Ms);
                __syncthreads();
                if (c0 + 2 * kKC < Bp4) {
                    fetch_d(d, r0, c0 + 2 * kKC);
                    fetch_m(mm, TN, W, j0, c0 + 2 * kKC);
                }
                if (active) {
                    const int ks = min(kKC, Bp4 - c0);
                    const float *ap = As + (wave * 16 + lr) * kLd + lk, *bp = Ms + lr * kLd + lk;
                    auto step = [&](int k) {
                        const float a = ap[k];
#pragma unroll
                        for (int t = 0; t < TN; ++t)
                            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[t * 16 * kLd + k], acc[t], 0, 0, 0);
                    };
                    if (ks == kKC) {                           // a whole chunk: unrolled, its LDS reads run ahead
#pragma unroll
                        for (int k = 0; k < kKC; k += 4) step(k);
                    } else {
                        for (int k = 0; k < ks; k += 4) step(k);
                    }
                }
            };
            for (int c0 = 0; c0 < Bp4; c0 += 2 * kKC) {
                chunk(dv[0], mv[0], c0);
                if (c0 + kKC < Bp4) chunk(dv[1], mv[1], c0 + kKC);
            }
            if (active) {
#pragma unroll
                for (int t = 0; t < TN; ++t)
#pragma unroll
                    for (int g = 0; g < 4; ++g) u_at(r0 + wave * 16 + lk * 4 + g, t * 16 + lr) = acc[t][g];
            }
        }
        // stage 2: Y[:, j0 .. j0+W-1] = M . U
        for (int i0 = 0; i0 < Sp16; i0 += kRows) {
            const bool active = i0 + wave * 16 < Sp16;
            f32x4 acc[TN];
#pragma unroll
            for (int t = 0; t < TN; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            float4 av[2][kMPerThread];
            fetch_m(av[0], kMPerThread, kRows, i0, 0);
            if (kKC < Bp4) fetch_m(av[1], kMPerThread, kRows, i0, kKC);
            auto chunk = [&](float4 (&a4)[kMPerThread], int c0) {
                __syncthreads();                               // and, the first time, every wave's rows of U are written
                stage_m(a4, kMPerThread, kRows, As);
                __syncthreads();
                if (c0 + 2 * kKC < Bp4) fetch_m(a4, kMPerThread, kRows, i0, c0 + 2 * kKC);
                if (active) {
                    const int ks = min(kKC, Bp4 - c0);
                    const float *ap = As + (wave * 16 + lr) * kLd + lk;
                    auto step = [&](int k) {
                        const float a = ap[k];
                        const int r = c0 + k + lk;             // < roundup(B, 4): a row of U that stage 1 wrote
#pragma unroll
                        for (int t = 0; t < TN; ++t)
                            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, u_at(r, t * 16 + lr), acc[t], 0, 0, 0);
                    };
                    if (ks == kKC) {
#pragma unroll
                        for (int k = 0; k < kKC; k += 4) step(k);
                    } else {
                        for (int k = 0; k < ks; k += 4) step(k);
                    }
                }
            };
            for (int c0 = 0; c0 < Bp4; c0 += 2 * kKC) {
                chunk(av[0], c0);
                if (c0 + kKC < Bp4) chunk(av[1], c0 + kKC);
            }
            if (active) {
#pragma unroll
                for (int t = 0; t < TN; ++t)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int i = i0 + wave * 16 + lk * 4 + g, j = j0 + t * 16 + lr;
                        if (i < S && j < S) {
                            float y = acc[t][g];
                            if (!normalize) {
                                if constexpr (!kFloat) y = __fadd_rn(y, anchor);
                                if (invert) y = -y;
                            }
                            o[i * S + j] = y;
                        }
                    }
            }
        }
    }
    if (!normalize) {
        if (tid == 0) status[p] = 0;
        return;
    }

    __threadfence_block();
    __syncthreads();                                           // Y of every wave is in memory: each thread reads its pixels
    normalize_box(o, S, inv_s, R2, invert, status + p, lds);
}

// the strip width in 16-column tiles: the widest that keeps U[:, strip] within kStripBytes, then evened out over the strips
inline int scale_strip_tiles(int B, int S) {
    const int tiles = (S + 15) / 16, Bp16 = (B + 15) & ~15;
    static const size_t budget = (size_t)sprk::knob_env("SPRK_SCALE_STRIP_KB", kStripBytes / 1024) * 1024;   // DIAG builds: 16..128
    int tn = tiles < kMaxTN ? tiles : kMaxTN;
    while (tn > 1 && (size_t)Bp16 * 16 * tn * sizeof(float) > budget) --tn;
    const int strips = (tiles + tn - 1) / tn;
    return (tiles + strips - 1) / strips;
}

template <typename T, int TN>
int launch_scale_tn(const void *raw, int ny, int nx, const int *xy, int P, int B, int S, const float *m, int ldm, int R,
                    int flags, float *out, int *status, hipStream_t s) {
    const size_t lds = scale_lds_bytes(B, TN);
    if (int rc = sprk::lds_optin(extract_scale_kernel<T, TN>, lds, "extract_scale")) return rc;
    hipLaunchKernelGGL((extract_scale_kernel<T, TN>), dim3(P), dim3(kThreads), lds, s, (const T *)raw, ny, nx, xy, B, S, m,
                       ldm, 1.0f / (float)S, (long)R * R, flags, out, status);
    return sprk::check_launch("extract_scale");
}

template <typename T>
int launch_scale(const void *raw, int ny, int nx, const int *xy, int P, int B, int S, const float *m, int ldm, int R,
                 int flags, float *out, int *status, hipStream_t s) {
    switch (scale_strip_tiles(B, S)) {
        case 1: return launch_scale_tn<T, 1>(raw, ny, nx, xy, P, B, S, m, ldm, R, flags, out, status, s);
        case 2: return launch_scale_tn<T, 2>(raw, ny, nx, xy, P, B, S, m, ldm, R, flags, out, status, s);
        case 3: return launch_scale_tn<T, 3>(raw, ny, nx, xy, P, B, S, m, ldm, R, flags, out, status, s);
        default: return launch_scale_tn<T, 4>(raw, ny, nx, xy, P, B, S, m, ldm, R, flags, out, status, s);
    }
}

}  // namespace

extern "C" int sprk_extract_scale(const void *raw, int mode, int ny, int nx, const int *xy, int P, int box, int side,
                                  const float *m, int ldm, int bg_radius, int flags, float *out, int *status, void *stream) {
    SPRK_REQUIRE_MRC_MODE("extract_scale", mode);
    SPRK_REQUIRE(box >= 2 && box <= kMaxBox && side >= 2 && side <= box,
                 "extract_scale: box %d with output side %d (2 <= side <= box <= %d)", box, side, kMaxBox);
    SPRK_REQUIRE(ldm >= sprk::roundup4(box) && ldm % 4 == 0,
                 "extract_scale: row stride ldm %d of the matrix (a multiple of 4, at least roundup(box, 4) = %d)", ldm,
                 sprk::roundup4(box));
    SPRK_REQUIRE(bg_radius >= 0, "extract_scale: background radius %d (>= 0)", bg_radius);
    SPRK_REQUIRE((flags & ~(SPRK_EXTRACT_NORMALIZE | SPRK_EXTRACT_INVERT)) == 0, "extract_scale: unknown flags 0x%x", flags);
    SPRK_REQUIRE(ny > 0 && nx > 0 && (long)ny * nx < (1L << 31), "extract_scale: bad image size %dx%d", ny, nx);
    SPRK_REQUIRE(P >= 0, "extract_scale: %d particles", P);
    if (P == 0) return SPRK_OK;
    SPRK_REQUIRE(raw && xy && m && out && status, "extract_scale: null pointer");
    SPRK_REQUIRE(sprk::aligned16(raw), "extract_scale: the sample buffer must start 16-byte aligned");
    SPRK_REQUIRE(sprk::aligned16(m), "extract_scale: the matrix must start 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return dispatch_mrc(mode, [&](auto t) {
        return launch_scale<decltype(t)>(raw, ny, nx, xy, P, box, side, m, ldm, bg_radius, flags, out, status, s);
    });
}

extern "C" int sprk_extract_boxes(const void *raw, int mode, int ny, int nx, const int *xy, int P, int box, int bin,
                                  int bg_radius, int flags, float *out, int *status, void *stream) {
    SPRK_REQUIRE_MRC_MODE("extract_boxes", mode);
    SPRK_REQUIRE(bin >= 1 && bin <= SPRK_INGEST_MAX_BIN, "extract_boxes: bin factor %d (1..%d)", bin, SPRK_INGEST_MAX_BIN);
    // box <= 1024 is what keeps the int64 sum of squares of the integer modes below 2^63 (see the kernel)
    SPRK_REQUIRE(box >= 2 && box <= kMaxBox && box % bin == 0 && box / bin >= 2,
                 "extract_boxes: box %d with bin %d (2..%d, a multiple of the bin factor, at least 2 output pixels a side)",
                 box, bin, kMaxBox);
    SPRK_REQUIRE(bg_radius >= 0, "extract_boxes: background radius %d (>= 0)", bg_radius);
    SPRK_REQUIRE((flags & ~(SPRK_EXTRACT_NORMALIZE | SPRK_EXTRACT_INVERT)) == 0, "extract_boxes: unknown flags 0x%x", flags);
    SPRK_REQUIRE(ny > 0 && nx > 0 && (long)ny * nx < (1L << 31), "extract_boxes: bad image size %dx%d", ny, nx);
    SPRK_REQUIRE(P >= 0, "extract_boxes: %d particles", P);
    if (P == 0) return SPRK_OK;
    SPRK_REQUIRE(raw && xy && out && status, "extract_boxes: null pointer");
    SPRK_REQUIRE(sprk::aligned16(raw), "extract_boxes: the sample buffer must start 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return dispatch_mrc(mode, [&](auto t) {
        return launch_extract<decltype(t)>(raw, ny, nx, xy, P, box, bin, bg_radius, flags, out, status, s);
    });
}
