// Micrograph ingest: the sample block of a 2-D MRC image, as it sits in the file, to the network's input.
//
// Stage A (sprk_ingest_bin): decode (modes 0 int8, 1 int16, 2 float32, 6 uint16), bin N x N (N in 1..16, the binned
// area centred: by = ny / N, bx = nx / N, oy = (ny % N) / 2, ox = (nx % N) / 2) and find the range of the result.
//   integer modes: the block sum is an exact int32 (|sum| <= 16^2 * 65535 < 2^24, so float(sum) is exact too), then ONE
//       correctly rounded fp32 division by float(N*N);
//   float32: acc = 0.0f, the N*N samples added one at a time in row-major order within the block, every add its own
//       fp32 rounding, then one fp32 division by float(N*N);
//   N = 1: a plain conversion.
// One lane per output: it reads the N consecutive samples of each of its N rows, so adjacent lanes read adjacent chunks
// (coalesced) and the summation order is the contract's.  A chunk is fetched with the widest load (16, 8 or 4 bytes)
// that divides the chunk AND keeps every chunk of the image aligned (row pitch and the ox offset both multiples of
// that width; the buffer itself starts 16-byte aligned); otherwise sample by sample.  N = 1 is a flat conversion of
// 16 input bytes per lane whatever the row pitch is.
// The range: per lane an order-preserving integer encoding of the value, min / max over the wave by shuffles, over the
// workgroup through LDS, then one partial pair per workgroup in the workspace; a one-workgroup kernel reduces the (at
// most 2048) pairs and decodes the result to two floats.  (One atomicMin / atomicMax pair per workgroup on a shared
// address was measured first: 8192 same-address atomics cost 0.1 ms per image, more than the whole data pass.)  No
// host synchronisation.  Inputs are taken to be finite.
//
// Stage B (sprk_ingest_finish): micrograph_io.minmax_uint8 operation for operation (scale = 1 / (hi - lo) and
// shift = -lo * scale in double, 0 when hi - lo <= DBL_EPSILON, both rounded to fp32; norm = x*scale + shift as two
// fp32 roundings; q = (uint8) trunc(norm * 255.0f)), then either or both of
//   u8 [by, bx] = q                                        (what load_image returns for the binned image)
//   net [S, S]  = q[refl(b, by), refl(a, bx)] / 255.0f     (to_tensor, the CWH -> CHW transpose and the reflect padding
//                                                           of MicrographFeed; refl folds as often as np.pad does)
// in one launch: 32 x 32 tiles transposed through LDS, reads coalesced along the binned rows, writes along the net rows.
//
// No a*b+c of this file may be contracted into an FMA.  hipcc contracts by default, and HIP's __fmul_rn / __fadd_rn are
// plain operators that it contracts all the same (x*scale + shift came out as one v_fma_f32, and a file-scope
// `#pragma clang fp contract(off)` did not stop it), so the Makefile compiles this translation unit with
// -ffp-contract=off.  The intrinsics stay as markers of the operations the contract names; tests/test_gpu_ingest.py
// fails within a few pixels if the flag is lost.
#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <type_traits>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;
constexpr int kMaxBlocks = 2048;     // grid cap of the stage-A kernels = number of partial pairs in the workspace

struct Part {
    unsigned int min_enc, max_enc;   // order-preserving encodings of one workgroup's min / max
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
__device__ __forceinline__ bool block_reduce(unsigned int &lo, unsigned int &hi) {
    __shared__ unsigned int red[2][kThreads / 64];
    lo = wave_min(lo);
    hi = wave_max(hi);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][wave] = lo;
        red[1][wave] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kThreads / 64; ++w) {
            lo = min(lo, red[0][w]);
            hi = max(hi, red[1][w]);
        }
        return true;
    }
    return false;
}

// every workgroup stores its pair, also one without a single output (the neutral pair): nothing to initialise
__device__ __forceinline__ void block_range(unsigned int lo, unsigned int hi, Part *__restrict__ parts) {
    if (block_reduce(lo, hi)) parts[blockIdx.x] = Part{lo, hi};
}

__global__ __launch_bounds__(kThreads) void ingest_range_kernel(const Part *__restrict__ parts, int nparts,
                                                                float *__restrict__ range) {
    unsigned int lo = 0xffffffffu, hi = 0u;
    for (int k = threadIdx.x; k < nparts; k += kThreads) {
        lo = min(lo, parts[k].min_enc);
        hi = max(hi, parts[k].max_enc);
    }
    if (block_reduce(lo, hi)) {
        range[0] = dec(lo);
        range[1] = dec(hi);
    }
}

// the contract's accumulator: exact int32 for the integer modes, one fp32 add per sample for float32
template <typename T>
struct Sum {
    int v = 0;
    __device__ __forceinline__ void add(T s) { v += (int)s; }
    __device__ __forceinline__ float mean(float nn) const { return __fdiv_rn((float)v, nn); }
};
template <>
struct Sum<float> {
    float v = 0.0f;
    __device__ __forceinline__ void add(float s) { v = __fadd_rn(v, s); }
    __device__ __forceinline__ float mean(float nn) const { return __fdiv_rn(v, nn); }
};

// V: the load type of a chunk (T itself, or a 4 / 8 / 16-byte vector that the host found every chunk aligned for)
template <typename T, typename V>
__global__ __launch_bounds__(kThreads) void ingest_bin_kernel(const T *__restrict__ raw, int nx, int N, int oy, int ox,
                                                              int by, int bx, float *__restrict__ binned,
                                                              Part *__restrict__ parts) {
    constexpr int PER = sizeof(V) / sizeof(T);
    const int nvec = N / PER;                      // N % PER == 0 (host)
    const float nn = (float)(N * N);
    const int n = by * bx;                         // < 2^31 (host)
    unsigned int lo = 0xffffffffu, hi = 0u;
    for (long e = (long)blockIdx.x * kThreads + threadIdx.x; e < n; e += (long)gridDim.x * kThreads) {
        const int r = (int)e / bx, c = (int)e - r * bx;
        const T *p = raw + (long)(oy + r * N) * nx + ox + c * N;   // last sample read: (oy + by*N - 1, ox + bx*N - 1)
        Sum<T> acc;
        for (int i = 0; i < N; ++i, p += nx) {
            const V *pv = reinterpret_cast<const V *>(p);
            for (int k = 0; k < nvec; ++k) {
                const V v = pv[k];
                T s[PER];
                __builtin_memcpy(s, &v, sizeof(V));
#pragma unroll
                for (int j = 0; j < PER; ++j) acc.add(s[j]);
            }
        }
        const float m = acc.mean(nn);
        binned[e] = m;
        const unsigned int k = enc(m);
        lo = min(lo, k);
        hi = max(hi, k);
    }
    block_range(lo, hi, parts);
}

// N = 1: the image is one flat array; 16 input bytes per lane, the tail (n % PER samples) one sample per lane
template <typename T>
__global__ __launch_bounds__(kThreads) void ingest_convert_kernel(const T *__restrict__ raw, long n,
                                                                  float *__restrict__ binned, Part *__restrict__ parts) {
    constexpr int PER = 16 / sizeof(T);
    const long nvec = n / PER;
    unsigned int lo = 0xffffffffu, hi = 0u;
    for (long e = (long)blockIdx.x * kThreads + threadIdx.x; e < nvec; e += (long)gridDim.x * kThreads) {
        const uint4 v = reinterpret_cast<const uint4 *>(raw)[e];
        T s[PER];
        __builtin_memcpy(s, &v, 16);
        float f[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            f[j] = (float)s[j];
            const unsigned int k = enc(f[j]);
            lo = min(lo, k);
            hi = max(hi, k);
        }
        float4 *out = reinterpret_cast<float4 *>(binned + e * PER);
#pragma unroll
        for (int j = 0; j < PER / 4; ++j) out[j] = make_float4(f[4 * j], f[4 * j + 1], f[4 * j + 2], f[4 * j + 3]);
    }
    const long t = nvec * PER + (long)blockIdx.x * kThreads + threadIdx.x;
    if (t < n) {
        const float f = (float)raw[t];
        binned[t] = f;
        const unsigned int k = enc(f);
        lo = min(lo, k);
        hi = max(hi, k);
    }
    block_range(lo, hi, parts);
}

// np.pad(mode="reflect") index of position i on an axis of n samples, for any i >= 0
__device__ __forceinline__ int refl(int i, int n) {
    if (i < n) return i;
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    const int j = i % period;
    return j < n ? j : period - j;
}

// grid: (ceil(La / 32), ceil(Lb / 32)) tiles of the [La, Lb] = net frame (a = binned column, b = binned row); block
// (32, 8).  With net == nullptr the frame is the binned image itself (La = bx, Lb = by) and only u8 is written.
__global__ __launch_bounds__(kThreads) void ingest_finish_kernel(const float *__restrict__ binned, int by, int bx,
                                                                 const float *__restrict__ range,
                                                                 unsigned char *__restrict__ u8,
                                                                 float *__restrict__ net, int La, int Lb) {
    __shared__ unsigned char tile[kTile][kTile + 4];
    __shared__ float ab[2];
    const int tx = threadIdx.x, ty = threadIdx.y;
    if (tx == 0 && ty == 0) {
        const double lo = (double)range[0], hi = (double)range[1];
        const double scale = hi - lo > DBL_EPSILON ? 1.0 / (hi - lo) : 0.0;
        ab[0] = (float)scale;
        ab[1] = (float)(-lo * scale);
    }
    __syncthreads();
    const float scale = ab[0], shift = ab[1];
    const int a0 = blockIdx.x * kTile, b0 = blockIdx.y * kTile;
    for (int bb = ty; bb < kTile; bb += kThreads / kTile) {
        const int a = a0 + tx, b = b0 + bb;
        if (a < La && b < Lb) {
            const long src = (long)refl(b, by) * bx + refl(a, bx);
            const float norm = __fadd_rn(__fmul_rn(binned[src], scale), shift);
            const unsigned char q = (unsigned char)(int)__fmul_rn(norm, 255.0f);   // float -> int truncates
            tile[bb][tx] = q;
            if (u8 && a < bx && b < by) u8[(long)b * bx + a] = q;
        }
    }
    if (!net) return;
    __syncthreads();
    for (int aa = ty; aa < kTile; aa += kThreads / kTile) {
        const int a = a0 + aa, b = b0 + tx;
        if (a < La && b < Lb) net[(long)a * Lb + b] = __fdiv_rn((float)tile[tx][aa], 255.0f);
    }
}

int sample_bytes(int mode) {
    switch (mode) {
        case SPRK_MRC_INT8: return 1;
        case SPRK_MRC_INT16: return 2;
        case SPRK_MRC_FLOAT32: return 4;
        case SPRK_MRC_UINT16: return 2;
        default: return 0;
    }
}

// -> the number of workgroups launched (= partial pairs written), or a negative error code
template <typename T>
int launch_bin(const void *raw, int ny, int nx, int N, float *binned, Part *parts, hipStream_t s) {
    const int by = ny / N, bx = nx / N, oy = (ny % N) / 2, ox = (nx % N) / 2;
    const T *in = (const T *)raw;
    if (N == 1) {
        const long n = (long)ny * nx;
        const int grid = std::min(sprk::ew_blocks(n / (16 / sizeof(T)) + kThreads), kMaxBlocks);   // + the tail's lanes
        hipLaunchKernelGGL(ingest_convert_kernel<T>, dim3(grid), dim3(kThreads), 0, s, in, n, binned, parts);
        const int rc = sprk::check_launch("ingest_convert");
        return rc ? rc : grid;
    }
    const int grid = std::min(sprk::ew_blocks((long)by * bx), kMaxBlocks);
    // widest load that divides a chunk and keeps every chunk aligned: row pitch, column offset and chunk all multiples
    const size_t chunk = (size_t)N * sizeof(T), pitch = (size_t)nx * sizeof(T), off = (size_t)ox * sizeof(T);
    auto fits = [&](size_t w) { return w > sizeof(T) && chunk % w == 0 && pitch % w == 0 && off % w == 0; };
#define SPRK_BIN(V) \
    hipLaunchKernelGGL((ingest_bin_kernel<T, V>), dim3(grid), dim3(kThreads), 0, s, in, nx, N, oy, ox, by, bx, binned, parts)
    if (fits(16)) SPRK_BIN(uint4);
    else if (fits(8)) SPRK_BIN(uint2);
    else if (fits(4)) SPRK_BIN(uint32_t);
    else SPRK_BIN(T);
#undef SPRK_BIN
    const int rc = sprk::check_launch("ingest_bin");
    return rc ? rc : grid;
}

}  // namespace

extern "C" {

size_t sprk_ingest_ws_bytes(int ny, int nx, int bin) {
    if (ny < 1 || nx < 1 || bin < 1 || bin > SPRK_INGEST_MAX_BIN || ny / bin < 1 || nx / bin < 1) return 0;
    return (size_t)kMaxBlocks * sizeof(Part);
}

int sprk_ingest_bin(const void *raw, int mode, int ny, int nx, int bin, float *binned_out, float *range_out, void *ws,
                    size_t ws_bytes, void *stream) {
    SPRK_REQUIRE(raw && binned_out && range_out, "ingest_bin: null pointer");
    SPRK_REQUIRE(sample_bytes(mode) > 0, "ingest_bin: unsupported MRC mode %d (0, 1, 2 and 6 are)", mode);
    SPRK_REQUIRE(bin >= 1 && bin <= SPRK_INGEST_MAX_BIN, "ingest_bin: bin factor %d (1..%d)", bin, SPRK_INGEST_MAX_BIN);
    SPRK_REQUIRE(ny > 0 && nx > 0 && (long)ny * nx < (1L << 31), "ingest_bin: bad image size %dx%d", ny, nx);
    SPRK_REQUIRE(ny / bin >= 1 && nx / bin >= 1, "ingest_bin: a %dx%d image has no %dx%d block", ny, nx, bin, bin);
    SPRK_REQUIRE(((uintptr_t)raw & 15) == 0 && ((uintptr_t)binned_out & 15) == 0,
                 "ingest_bin: the sample buffer and the output must start 16-byte aligned");
    if (int rc = sprk::check_ws("ingest_bin", ws, ws_bytes, sprk_ingest_ws_bytes(ny, nx, bin))) return rc;
    hipStream_t s = (hipStream_t)stream;
    Part *parts = (Part *)ws;
    int grid;
    switch (mode) {
        case SPRK_MRC_INT8: grid = launch_bin<int8_t>(raw, ny, nx, bin, binned_out, parts, s); break;
        case SPRK_MRC_INT16: grid = launch_bin<int16_t>(raw, ny, nx, bin, binned_out, parts, s); break;
        case SPRK_MRC_FLOAT32: grid = launch_bin<float>(raw, ny, nx, bin, binned_out, parts, s); break;
        default: grid = launch_bin<uint16_t>(raw, ny, nx, bin, binned_out, parts, s); break;
    }
    if (grid < 0) return grid;
    hipLaunchKernelGGL(ingest_range_kernel, dim3(1), dim3(kThreads), 0, s, parts, grid, range_out);
    return sprk::check_launch("ingest_range");
}

int sprk_ingest_finish(const float *binned, int by, int bx, const float *range, uint8_t *u8_out, float *net_out, int S,
                       void *stream) {
    SPRK_REQUIRE(binned && range, "ingest_finish: null pointer");
    SPRK_REQUIRE(u8_out || net_out, "ingest_finish: null pointer (neither u8_out nor net_out)");
    SPRK_REQUIRE(by > 0 && bx > 0 && (long)by * bx < (1L << 31), "ingest_finish: bad image size %dx%d", by, bx);
    int La = bx, Lb = by;
    if (net_out) {
        SPRK_REQUIRE(S >= by && S >= bx && S % 32 == 0 && (long)S * S < (1L << 31),
                     "ingest_finish: network size %d for a %dx%d image (a multiple of 32, >= both)", S, by, bx);
        La = Lb = S;
    }
    hipLaunchKernelGGL(ingest_finish_kernel, dim3(sprk::cdiv(La, kTile), sprk::cdiv(Lb, kTile)),
                       dim3(kTile, kThreads / kTile), 0, (hipStream_t)stream, binned, by, bx, range, u8_out, net_out, La,
                       Lb);
    return sprk::check_launch("ingest_finish");
}

}  // extern "C"
