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
// Optional, between the two (sprk_ingest_clip): the binned image clamped to two of its own order statistics, which then
// are the range stage B normalises by.  A radix select on d = key(x) - key(min) (min / max: stage A's range, read on the
// device): three passes of at most 11 bits, taken from the highest set bit of key(max) - key(min) downward — a
// micrograph's values share sign, exponent and leading mantissa bits, so digits at fixed positions would put every pixel
// in one bin.  A pass: every workgroup (at most 256, grid-stride, 16-byte loads) counts the elements whose higher digits
// match each rank's prefix into 2048-bin LDS histograms, one per rank while the prefixes differ, aggregated inside the
// wave first, and stores its whole partial (nothing to zero, no same-address global atomics: see the note on stage A's
// range); a second kernel sums the partials; a one-workgroup kernel scans the sums, picks each rank's bin and updates
// (prefix, k) in the workspace.  Then the clamp x < lo ? lo : (x > hi ? hi : x) and the new range.  Exact: lo and hi are
// elements of the image.  No host synchronisation.
//
// Optional too (sprk_ingest_flatten; with the clip: clip, flatten, clip again): the mean over a (2R+1)^2 window, clamped
// at the edges, subtracted from every pixel — a slow gradient across the micrograph otherwise takes most of the 256
// levels.  The window sums are integers: t = floor((x - lo) * 2^(30 - ilogb(hi - lo))) < 2^31, summed in uint64, so that
// any order of summation, running updates included, gives the same bits as the NumPy model (include/sprk.h has the
// contract).  A row pass (LDS prefix sums per row segment, windows reaching across segment boundaries) writes the
// horizontal sums, a column pass runs a window sum down each column, lanes on adjacent columns, and stores
// float((x - lo) - mean) with per-workgroup ranges for ingest_range_kernel.  Three launches, no host synchronisation.
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
#include "mrc_host.h"
#include "range_dev.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;
constexpr int kMaxBlocks = 2048;     // grid cap of the stage-A kernels = number of partial pairs in the workspace

// every workgroup stores its pair, also one without a single output (the neutral pair): nothing to initialise
__device__ __forceinline__ void block_range(unsigned int lo, unsigned int hi, Part *__restrict__ parts) {
    if (block_reduce<kThreads>(lo, hi)) parts[blockIdx.x] = Part{lo, hi};
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

// ---- sprk_ingest_clip: two order statistics of the binned image by radix select, then the clamp --------------------
constexpr int kClipBins = 2048;      // an 11-bit digit
constexpr int kClipPasses = 3;       // 11 + 11 + 10 bits cover any span of keys
constexpr int kClipBlocks = 256;     // grid cap of the histogram kernel = partial histograms in the workspace
constexpr int kClipThreads = 1024;   // ... whose workgroups are large instead: four waves per SIMD at one workgroup per CU
constexpr int kPeelRounds = 4;

// workspace: ClipState | sums [2][kClipBins] | partials [grid][2][kClipBins] (uint32); index 0 = the low rank, 1 = the high
struct ClipState {
    unsigned int prefix[2];   // the bits of d = key(x) - key(min) of each rank's element above the digits still to come
    unsigned int k[2];        // its rank among the elements that share that prefix
    float lohi[2];            // after the last pass: the two elements themselves
    unsigned int pad[2];
};

// pass p takes bits [shift, top) of d, at most 11 from the highest set bit of the span down; top == shift: none left
struct ClipDigits {
    int top, shift;
    unsigned int mask;
};
__device__ __forceinline__ ClipDigits clip_digits(unsigned int span, int pass) {
    const int nbits = span ? 32 - __clz((int)span) : 0;
    ClipDigits g;
    g.top = max(nbits - 11 * pass, 0);
    g.shift = max(g.top - 11, 0);
    g.mask = (1u << (g.top - g.shift)) - 1u;
    return g;
}

// One count per active lane into hist[digit].  Lanes that hold the same digit elect one lane, which adds their number:
// a tied, two-valued or near-constant image puts a whole wave on one bin, and same-address LDS atomics serialise.  A
// few rounds peel the wave's most common digits; what is left is spread over bins and adds lane by lane.  Every lane
// of the wave must call (inactive ones with active == false).
__device__ __forceinline__ void wave_count(unsigned int *hist, bool active, unsigned int digit) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(active);
    for (int round = 0; round < kPeelRounds && todo; ++round) {
        const int leader = __ffsll(todo) - 1;
        const unsigned int dl = (unsigned int)__shfl((int)digit, leader, 64);
        const unsigned long long same = __ballot(active && digit == dl);
        if (lane == leader) atomicAdd(&hist[dl], (unsigned int)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1) atomicAdd(&hist[digit], 1u);
}

// vec: x starts 16-byte aligned (float4 loads, the next one in flight while this one is counted; the n % 4 tail one
// element per lane).  Loop bounds are uniform over the workgroup, so that every lane reaches wave_count.
__global__ __launch_bounds__(kClipThreads) void clip_hist_kernel(const float *__restrict__ x, long n, int vec,
                                                             const float *__restrict__ range, int pass,
                                                             const ClipState *__restrict__ st,
                                                             unsigned int *__restrict__ partials) {
    __shared__ unsigned int hist[2 * kClipBins];
    const unsigned int kmin = enc(range[0]);
    const ClipDigits g = clip_digits(enc(range[1]) - kmin, pass);
    if (g.top == g.shift) return;
    const unsigned int p0 = pass ? st->prefix[0] : 0u, p1 = pass ? st->prefix[1] : 0u;
    const bool two = p0 != p1;                     // else both ranks share histogram 0
    const int used = (two ? 2 : 1) * kClipBins;
    for (int i = threadIdx.x; i < used; i += kClipThreads) hist[i] = 0u;
    __syncthreads();
    auto count = [&](bool in, float v) {
        const unsigned int d = enc(v) - kmin;
        const unsigned int pre = (unsigned int)((unsigned long long)d >> g.top);
        const unsigned int digit = (d >> g.shift) & g.mask;                  // < kClipBins whatever v is
        wave_count(hist, in && pre == p0, digit);
        if (two) wave_count(hist + kClipBins, in && pre == p1, digit);
    };
    const long nvec = vec ? n / 4 : 0;
    const long stride = (long)gridDim.x * kClipThreads;
    auto load = [&](long e) {
        return e < nvec ? reinterpret_cast<const float4 *>(x)[e] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    };
    float4 v = load((long)blockIdx.x * kClipThreads + threadIdx.x);
    for (long base = (long)blockIdx.x * kClipThreads; base < nvec; base += stride) {
        const long e = base + threadIdx.x;
        const float4 ahead = load(e + stride);
        const bool in = e < nvec;
        count(in, v.x);
        count(in, v.y);
        count(in, v.z);
        count(in, v.w);
        v = ahead;
    }
    for (long base = nvec * 4 + (long)blockIdx.x * kClipThreads; base < n; base += stride) {
        const long e = base + threadIdx.x;
        const bool in = e < n;
        count(in, in ? x[e] : 0.0f);
    }
    __syncthreads();
    unsigned int *out = partials + (size_t)blockIdx.x * 2 * kClipBins;       // the whole partial: nothing to initialise
    for (int i = threadIdx.x; i < used; i += kClipThreads) out[i] = hist[i];
}

// grid (kClipBins / 64, 2): 64 bins of one histogram per workgroup, the partials dealt to its four waves
__global__ __launch_bounds__(kThreads) void clip_sum_kernel(const unsigned int *__restrict__ partials, int nparts,
                                                            const float *__restrict__ range, int pass,
                                                            const ClipState *__restrict__ st,
                                                            unsigned int *__restrict__ sums) {
    __shared__ unsigned int red[kThreads / 64][64];
    const ClipDigits g = clip_digits(enc(range[1]) - enc(range[0]), pass);
    if (g.top == g.shift) return;
    const int h = blockIdx.y;
    if (h == 1 && (pass == 0 || st->prefix[0] == st->prefix[1])) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bin = blockIdx.x * 64 + lane;
    unsigned int s = 0;
    for (int i = wave; i < nparts; i += kThreads / 64) s += partials[((size_t)i * 2 + h) * kClipBins + bin];
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0) {
        for (int w = 1; w < kThreads / 64; ++w) s += red[w][lane];
        sums[h * kClipBins + bin] = s;
    }
}

// one workgroup: for both ranks, the bin of the summed histogram that holds the rank -> the next (prefix, k).  Thread
// t owns bins 8t .. 8t+7.  Pass 0 starts from (0, k_lo), (0, k_hi); a pass without bits hands the state on as it is.
__global__ __launch_bounds__(kThreads) void clip_pick_kernel(const unsigned int *__restrict__ sums,
                                                             const float *__restrict__ range, int pass,
                                                             unsigned int k_lo, unsigned int k_hi, ClipState *st) {
    constexpr int PER = kClipBins / kThreads;
    __shared__ unsigned int wtot[kThreads / 64];
    __shared__ ClipState next;
    const unsigned int kmin = enc(range[0]);
    const ClipDigits g = clip_digits(enc(range[1]) - kmin, pass);
    if (threadIdx.x == 0) {
        if (pass) {
            next = *st;
        } else {
            next.prefix[0] = next.prefix[1] = 0u;
            next.k[0] = k_lo;
            next.k[1] = k_hi;
            next.lohi[0] = next.lohi[1] = 0.0f;
            next.pad[0] = next.pad[1] = 0u;
        }
    }
    __syncthreads();
    const unsigned int prefix[2] = {next.prefix[0], next.prefix[1]}, rank[2] = {next.k[0], next.k[1]};
    const bool two = prefix[0] != prefix[1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (g.top != g.shift) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const unsigned int *h = sums + (two && r ? kClipBins : 0);
            unsigned int c[PER], t = 0;
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                c[j] = h[threadIdx.x * PER + j];
                t += c[j];
            }
            unsigned int inc = t;                                  // inclusive scan of t over the workgroup
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned int u = (unsigned int)__shfl_up((int)inc, o, 64);
                if (lane >= o) inc += u;
            }
            __syncthreads();                                       // wtot of the other rank has been read
            if (lane == 63) wtot[wave] = inc;
            __syncthreads();
            unsigned int cum = inc - t;
            for (int w = 0; w < wave; ++w) cum += wtot[w];
            const unsigned int k = rank[r];
            if (k >= cum && k - cum < t) {                         // the one thread whose bins hold rank k
                bool done = false;
#pragma unroll
                for (int j = 0; j < PER; ++j) {
                    if (!done) {
                        if (k - cum < c[j]) {
                            next.prefix[r] = (prefix[r] << (g.top - g.shift)) | (unsigned int)(threadIdx.x * PER + j);
                            next.k[r] = k - cum;
                            done = true;
                        } else {
                            cum += c[j];
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (pass == kClipPasses - 1) {                             // shift == 0 by now: the prefix is all of d
            next.lohi[0] = dec(kmin + next.prefix[0]);
            next.lohi[1] = dec(kmin + next.prefix[1]);
        }
        *st = next;
    }
}

// y may be x (every element is read and written by the same lane); vec: both start 16-byte aligned
__global__ __launch_bounds__(kThreads) void clip_clamp_kernel(const float *x, float *y, long n, int vec,
                                                              const ClipState *__restrict__ st, float *range_out) {
    const float lo = st->lohi[0], hi = st->lohi[1];
    auto clamp = [&](float v) { return v < lo ? lo : (v > hi ? hi : v); };
    const long nvec = vec ? n / 4 : 0;
    const long stride = (long)gridDim.x * kThreads;
    for (long e = (long)blockIdx.x * kThreads + threadIdx.x; e < nvec; e += stride) {
        const float4 v = reinterpret_cast<const float4 *>(x)[e];
        reinterpret_cast<float4 *>(y)[e] = make_float4(clamp(v.x), clamp(v.y), clamp(v.z), clamp(v.w));
    }
    for (long e = nvec * 4 + (long)blockIdx.x * kThreads + threadIdx.x; e < n; e += stride) y[e] = clamp(x[e]);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        range_out[0] = lo;
        range_out[1] = hi;
    }
}

// ---- sprk_ingest_flatten: the mean over a clamped (2R+1)^2 window subtracted, in exact integer sums ------------------
constexpr int kFlatSeg = 1024;                        // output columns of one row segment
constexpr int kFlatRowBlocks = 2048;                  // grid cap of the row pass (grid-stride over the segments)
constexpr int kFlatStrip = 64;                        // columns of a column-pass tile: one per lane of a wave
constexpr int kFlatBatch = 8;                         // rows the column pass fetches ahead of their use

// workspace: Part [kMaxBlocks] | H [by, bx] uint64, the horizontal window sums
struct FlatScale {
    double lo;
    int e;          // ilogb(hi - lo)
    bool flat;      // hi == lo: the output is +0.0f everywhere
};
__device__ __forceinline__ FlatScale flat_scale(const float *range) {
    FlatScale s;
    s.lo = (double)range[0];
    const double span = (double)range[1] - s.lo;      // >= 2^-149 or 0: never a subnormal double
    s.flat = !(span > 0.0);
    s.e = s.flat ? 0 : (int)((__double_as_longlong(span) >> 52) & 0x7ff) - 1023;
    return s;
}
// t = floor((x - lo) * 2^(30 - e)): 0 <= t < 2^31 for lo <= x <= hi, the scaling exact
__device__ __forceinline__ unsigned int flat_fixed(float x, const FlatScale &s) {
    return (unsigned int)(long long)floor(ldexp((double)x - s.lo, 30 - s.e));
}

// Row pass.  A workgroup takes row segments of kFlatSeg columns: t of the segment and of the R columns either side of
// it (as far as the row goes) into LDS, an exclusive prefix sum P over them (thread i sums `per` consecutive elements,
// the threads' totals are scanned through the waves), then H[r][c] = P[right end of c's window + 1] - P[left end].
// Dynamic LDS, flatten_row_lds(R) bytes for span = kFlatSeg + 2R elements: P [span + 1] | wtot [4] | t [span] — a small
// radius leaves room for eight workgroups on a CU, the largest (36.9 KB) for four.
__global__ __launch_bounds__(kThreads) void flatten_row_kernel(const float *__restrict__ x, int by, int bx, int R,
                                                               const float *__restrict__ range,
                                                               unsigned long long *__restrict__ H) {
    extern __shared__ unsigned long long flat_lds[];
    const int span = kFlatSeg + 2 * R;
    unsigned long long *P = flat_lds, *wtot = P + span + 1;
    unsigned int *t = (unsigned int *)(wtot + kThreads / 64);
    const FlatScale sc = flat_scale(range);
    const int nseg = (bx + kFlatSeg - 1) / kFlatSeg;
    const long total = (long)by * nseg;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long w = blockIdx.x; w < total; w += gridDim.x) {
        const int r = (int)(w / nseg), c0 = (int)(w - (long)r * nseg) * kFlatSeg;
        const int cols = min(kFlatSeg, bx - c0);
        const int base = max(c0 - R, 0);
        const int len = min(c0 + cols - 1 + R, bx - 1) - base + 1;        // <= span
        const float *row = x + (long)r * bx;
        for (int i = threadIdx.x; i < len; i += kThreads) t[i] = sc.flat ? 0u : flat_fixed(row[base + i], sc);
        __syncthreads();
        const int per = (len + kThreads - 1) / kThreads;
        const int first = min((int)threadIdx.x * per, len), last = min(first + per, len);
        unsigned long long mine = 0;
        for (int i = first; i < last; ++i) mine += t[i];
        unsigned long long inc = mine;                                    // inclusive scan over the wave
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long u = __shfl_up(inc, o, 64);
            if (lane >= o) inc += u;
        }
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        unsigned long long run = inc - mine;
        for (int k = 0; k < wave; ++k) run += wtot[k];
        if (threadIdx.x == 0) P[0] = 0;
        for (int i = first; i < last; ++i) {
            run += t[i];
            P[i + 1] = run;
        }
        __syncthreads();
        unsigned long long *out = H + (long)r * bx + c0;
        for (int i = threadIdx.x; i < cols; i += kThreads) {
            const int c = c0 + i;
            out[i] = P[min(c + R, bx - 1) - base + 1] - P[max(c - R, 0) - base];
        }
        __syncthreads();                                                  // t, P and wtot are free again
    }
}

// Column pass.  A wave takes tiles of kFlatStrip columns (one per lane: adjacent lanes on adjacent columns) by `chunk`
// rows.  It primes S with the window of the tile's first row and then moves it down a row at a time: + the row that
// enters, - the row that leaves.  Integers: the running sum is the window's sum, exactly.  y may be x (an element is
// read and written by the same lane, and H holds everything else this pass reads).
__global__ __launch_bounds__(kThreads) void flatten_col_kernel(const float *x, float *y, int by, int bx, int R, int chunk,
                                                               const float *__restrict__ range,
                                                               const unsigned long long *__restrict__ H,
                                                               Part *__restrict__ parts) {
    const FlatScale sc = flat_scale(range);
    const int strips = (bx + kFlatStrip - 1) / kFlatStrip, chunks = (by + chunk - 1) / chunk;
    const long tiles = (long)strips * chunks;
    const int lane = threadIdx.x & 63;
    const long nwaves = (long)gridDim.x * (kThreads / 64);
    unsigned int lo = 0xffffffffu, hi = 0u;
    for (long tile = (long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); tile < tiles; tile += nwaves) {
        const int c = (int)(tile % strips) * kFlatStrip + lane;           // neighbouring waves: neighbouring strips
        const int r0 = (int)(tile / strips) * chunk, r1 = min(r0 + chunk, by);
        if (c >= bx) continue;
        const unsigned long long *Hc = H + c;
        const int ncols = min(c + R, bx - 1) - max(c - R, 0) + 1;
        unsigned long long S = 0;
#pragma unroll 8
        for (int q = max(r0 - R, 0); q <= min(r0 + R, by - 1); ++q) S += Hc[(long)q * bx];
        // kFlatBatch rows at a time: their pixels and the rows that enter and leave are all fetched before the first
        // is used (every load unconditional, from a clamped row; what lies outside the image is dropped afterwards),
        // or each row would wait a whole memory latency for its own three loads
        for (int rb = r0; rb < r1; rb += kFlatBatch) {
            float px[kFlatBatch];
            unsigned long long in[kFlatBatch], out[kFlatBatch];
#pragma unroll
            for (int j = 0; j < kFlatBatch; ++j) {
                const int r = rb + j;
                px[j] = x[(long)min(r, r1 - 1) * bx + c];
                in[j] = Hc[(long)min(r + 1 + R, by - 1) * bx];
                out[j] = Hc[(long)max(r - R, 0) * bx];
            }
#pragma unroll
            for (int j = 0; j < kFlatBatch; ++j) {
                const int r = rb + j;
                if (r < r1) {
                    float f = 0.0f;
                    if (!sc.flat) {
                        const int cnt = (min(r + R, by - 1) - max(r - R, 0) + 1) * ncols;    // <= 2047^2
                        const double bg = ldexp((double)S / (double)cnt, sc.e - 30);          // S < 2^53: exact
                        f = (float)(((double)px[j] - sc.lo) - bg);
                    }
                    y[(long)r * bx + c] = f;
                    const unsigned int k = enc(f);
                    lo = min(lo, k);
                    hi = max(hi, k);
                }
                S += r + 1 + R <= by - 1 ? in[j] : 0ull;
                S -= r - R >= 0 ? out[j] : 0ull;
            }
        }
    }
    block_range(lo, hi, parts);
}

size_t flatten_row_lds(int R) {
    const size_t span = kFlatSeg + 2 * (size_t)R;
    return (span + 1 + kThreads / 64) * sizeof(unsigned long long) + span * sizeof(unsigned int);
}

// Rows of a column-pass tile.  Priming reads 2R+1 rows of H per tile, so R rows and more keep H's traffic at most four
// times its size; an image too small to give 2048 such tiles takes shorter ones, down to 32 rows (its H stays in the
// L2).  Speed only: the sums are integers, any tiling gives the same bits.
int flatten_chunk(int R, int by, int bx) {
    const long fill = (long)by * sprk::cdiv(bx, kFlatStrip) / 2048;
    return (int)std::max<long>(32, std::min<long>(R, fill));
}
constexpr size_t kFlatPartBytes = (size_t)kMaxBlocks * sizeof(Part);     // 16 KiB: H starts 16-byte aligned

int clip_grid(long n) { return (int)std::min<long>(kClipBlocks, sprk::cdiv(sprk::cdiv(n, 4), kClipThreads)); }

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
    SPRK_REQUIRE_MRC_MODE("ingest_bin", mode);
    SPRK_REQUIRE(bin >= 1 && bin <= SPRK_INGEST_MAX_BIN, "ingest_bin: bin factor %d (1..%d)", bin, SPRK_INGEST_MAX_BIN);
    SPRK_REQUIRE(ny > 0 && nx > 0 && (long)ny * nx < (1L << 31), "ingest_bin: bad image size %dx%d", ny, nx);
    SPRK_REQUIRE(ny / bin >= 1 && nx / bin >= 1, "ingest_bin: a %dx%d image has no %dx%d block", ny, nx, bin, bin);
    SPRK_REQUIRE(sprk::aligned16(raw, binned_out),
                 "ingest_bin: the sample buffer and the output must start 16-byte aligned");
    if (int rc = sprk::check_ws("ingest_bin", ws, ws_bytes, sprk_ingest_ws_bytes(ny, nx, bin))) return rc;
    hipStream_t s = (hipStream_t)stream;
    Part *parts = (Part *)ws;
    const int grid = dispatch_mrc(
        mode, [&](auto t) { return launch_bin<decltype(t)>(raw, ny, nx, bin, binned_out, parts, s); });
    if (grid < 0) return grid;
    hipLaunchKernelGGL(ingest_range_kernel<kRangeThreads>, dim3(1), dim3(kRangeThreads), 0, s, parts, grid, range_out);
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

size_t sprk_ingest_clip_ws_bytes(int by, int bx) {
    if (by < 1 || bx < 1 || (long)by * bx >= (1L << 31)) return 0;
    return sizeof(ClipState) + (size_t)(2 + 2 * clip_grid((long)by * bx)) * kClipBins * sizeof(unsigned int);
}

int sprk_ingest_clip(const float *binned_in, float *binned_out, int by, int bx, long long k_lo, long long k_hi,
                     const float *range_in, float *range_out, void *ws, size_t ws_bytes, void *stream) {
    SPRK_REQUIRE(binned_in && binned_out && range_in && range_out, "ingest_clip: null pointer");
    SPRK_REQUIRE(by > 0 && bx > 0 && (long)by * bx < (1L << 31), "ingest_clip: bad image size %dx%d", by, bx);
    const long n = (long)by * bx;
    SPRK_REQUIRE(k_lo >= 0 && k_lo <= k_hi && k_hi <= n - 1,
                 "ingest_clip: ranks %lld, %lld of %ld elements (0 <= k_lo <= k_hi <= n-1)", k_lo, k_hi, n);
    if (int rc = sprk::check_ws("ingest_clip", ws, ws_bytes, sprk_ingest_clip_ws_bytes(by, bx))) return rc;
    SPRK_REQUIRE(sprk::aligned16(ws), "ingest_clip: the workspace must start 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    ClipState *st = (ClipState *)ws;
    unsigned int *sums = (unsigned int *)(st + 1), *partials = sums + 2 * kClipBins;
    const int grid = clip_grid(n);
    const int vec_in = sprk::aligned16(binned_in), vec_out = vec_in && sprk::aligned16(binned_out);
    for (int pass = 0; pass < kClipPasses; ++pass) {
        hipLaunchKernelGGL(clip_hist_kernel, dim3(grid), dim3(kClipThreads), 0, s, binned_in, n, vec_in, range_in, pass, st,
                           partials);
        if (int rc = sprk::check_launch("ingest_clip_hist")) return rc;
        hipLaunchKernelGGL(clip_sum_kernel, dim3(kClipBins / 64, 2), dim3(kThreads), 0, s, partials, grid, range_in, pass,
                           st, sums);
        if (int rc = sprk::check_launch("ingest_clip_sum")) return rc;
        hipLaunchKernelGGL(clip_pick_kernel, dim3(1), dim3(kThreads), 0, s, sums, range_in, pass, (unsigned int)k_lo,
                           (unsigned int)k_hi, st);
        if (int rc = sprk::check_launch("ingest_clip_pick")) return rc;
    }
    const int grid_clamp = std::min(sprk::ew_blocks(sprk::cdiv(n, 4)), kMaxBlocks);      // plain streaming: no partials
    hipLaunchKernelGGL(clip_clamp_kernel, dim3(grid_clamp), dim3(kThreads), 0, s, binned_in, binned_out, n, vec_out, st,
                       range_out);
    return sprk::check_launch("ingest_clip_clamp");
}

size_t sprk_ingest_flatten_ws_bytes(int by, int bx, int R) {
    if (by < 1 || bx < 1 || (long)by * bx >= (1L << 31) || R < 1 || R > SPRK_INGEST_MAX_FLATTEN) return 0;
    return kFlatPartBytes + (size_t)by * bx * sizeof(unsigned long long);
}

int sprk_ingest_flatten(const float *binned_in, float *binned_out, int by, int bx, int R, const float *range_in,
                        float *range_out, void *ws, size_t ws_bytes, void *stream) {
    SPRK_REQUIRE(binned_in && binned_out && range_in && range_out, "ingest_flatten: null pointer");
    SPRK_REQUIRE(by > 0 && bx > 0 && (long)by * bx < (1L << 31), "ingest_flatten: bad image size %dx%d", by, bx);
    // a window holds at most 2047^2 values below 2^31: their integer sum stays below 2^53, exact as a double
    SPRK_REQUIRE(R >= 1 && R <= SPRK_INGEST_MAX_FLATTEN, "ingest_flatten: radius %d (1..%d)", R, SPRK_INGEST_MAX_FLATTEN);
    if (int rc = sprk::check_ws("ingest_flatten", ws, ws_bytes, sprk_ingest_flatten_ws_bytes(by, bx, R))) return rc;
    SPRK_REQUIRE(sprk::aligned16(ws), "ingest_flatten: the workspace must start 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    Part *parts = (Part *)ws;
    unsigned long long *H = (unsigned long long *)((char *)ws + kFlatPartBytes);
    const int grid_row = (int)std::min<long>((long)by * sprk::cdiv(bx, kFlatSeg), kFlatRowBlocks);
    hipLaunchKernelGGL(flatten_row_kernel, dim3(grid_row), dim3(kThreads), flatten_row_lds(R), s, binned_in, by, bx, R,
                       range_in, H);
    if (int rc = sprk::check_launch("ingest_flatten_row")) return rc;
    const int chunk = flatten_chunk(R, by, bx);
    const long tiles = (long)sprk::cdiv(bx, kFlatStrip) * sprk::cdiv(by, chunk);
    const int grid = (int)std::min<long>(sprk::cdiv(tiles, kThreads / 64), kMaxBlocks);
    hipLaunchKernelGGL(flatten_col_kernel, dim3(grid), dim3(kThreads), 0, s, binned_in, binned_out, by, bx, R, chunk,
                       range_in, H, parts);
    if (int rc = sprk::check_launch("ingest_flatten_col")) return rc;
    hipLaunchKernelGGL(ingest_range_kernel<kRangeThreads>, dim3(1), dim3(kRangeThreads), 0, s, parts, grid, range_out);
    return sprk::check_launch("ingest_flatten_range");
}

}  // extern "C"
