// Reference-free 2-D classification: sprk_class_transform, sprk_class_score and sprk_class_average (`joint class2d`;
// DESIGN §4.3l).  The contracts are stated in include/sprk.h and modelled in tests/class2d_model.py.
//
// The rigid transform (class_value below, shared by the transform and the averaging kernel): the output pixel (i, j) is the
// bilinear sample of the source at the rotated position plus an integer shift,
//   y = (float)(i - c),  x = (float)(j - c),  c = S / 2;
//   u = fmaf(ct, y, -(st * x)),  v = fmaf(st, y, ct * x)            (the inner product rounded first);
//   fu = floorf(u),  tu = u - fu;   fv = floorf(v),  tv = v - fv;
//   the first tap at (i0, j0) = ((int)fu + c + dy, (int)fv + c + dx);  s[a][b] = src[i0 + a, j0 + b], a zero formed in
//   registers (never a read) wherever the tap lies outside [0, S): the edges are not periodic;
//   r_a = fmaf(tv, s[a][1], (1.0f - tv) * s[a][0]);   out = fmaf(tu, r_1, (1.0f - tu) * r_0).
// Every index that comes from device memory (source, angle, shift, pixel list, class offsets, members) is clamped into its
// array before it addresses anything: no content of those arrays makes a kernel read or write out of bounds.
//
// class_transform_kernel: one workgroup of 256 threads per output image, the source image staged once in LDS.  With
// SPRK_CLASS_NORMALIZE the masked values of the whole image are kept in a second LDS image and the two statistics are
// formed in fp64 in a fixed order (thread t its pixels t, t + 256, ... ascending, then a halving tree over the 256 partials),
// whatever the output form: packed and unpacked calls give the same values.
//
// class_score_kernel: s = Q B^T on v_mfma_f32_16x16x4_f32 by matrix_rows_body of mfma_stage.h (both operands MatrixRows, B
// as the BtRows operand), once per column tile, K never split: every score is the fmaf chain over d ascending from 0.0f.
// A workgroup of four waves owns 64 rows of Q and walks the column tiles of 64 bank rows in ascending order; a lane keeps
// the running best of its four rows over its own columns (ascending, a strictly greater score replaces: the lowest index
// of a tie stays), and at the end the 16 lanes that share a row are combined, the lower index winning a tie.  Padded rows
// and columns are staged as zeros and never compared or stored.
//
// class_average_kernel: one workgroup per (class, 256 output pixels); a thread owns one pixel and adds the transform value
// of the class's members in list order (one fp32 add each, from 0.0f), read straight from memory, then multiplies once by
// 1.0f / (float)count.  An empty class is not written.
// No atomics, no host synchronisation, no workspace.
//
// Compiled with -ffp-contract=off (Makefile): the fmaf above are the only fused operations.
#include <cstdint>

#include "common.h"
#include "mfma_stage.h"

namespace {

constexpr int kMaxSide = 128;                    // two LDS images of 128 x 128 fp32 and the tree fit a workgroup's LDS
constexpr int kMaxAngles = 720;
constexpr int kMaxShiftAbs = 256;                // a shift is clamped here: past +-S every tap is outside anyway
constexpr int kThreads = 256;
constexpr int kTile = 64;                        // score: rows of Q per workgroup, bank rows per column tile
constexpr int kMaxBank = 65536;
constexpr int kMaxD = 16384;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// the transform value at output pixel (i, j): img [S, S] in LDS or in memory
__device__ __forceinline__ float class_value(const float *img, int S, float ct, float st, int dy, int dx, int i, int j) {
    const int c = S / 2;
    const float y = (float)(i - c), x = (float)(j - c);
    const float u = __fmaf_rn(ct, y, -(st * x)), v = __fmaf_rn(st, y, ct * x);
    const float fu = floorf(u), fv = floorf(v);
    const float tu = u - fu, tv = v - fv;
    const int i0 = (int)fu + c + dy, j0 = (int)fv + c + dx;
    float r[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int ii = i0 + a;
        const bool row_in = ii >= 0 && ii < S;
        const float s0 = row_in && j0 >= 0 && j0 < S ? img[ii * S + j0] : 0.0f;
        const float s1 = row_in && j0 + 1 >= 0 && j0 + 1 < S ? img[ii * S + j0 + 1] : 0.0f;
        r[a] = __fmaf_rn(tv, s1, (1.0f - tv) * s0);
    }
    return __fmaf_rn(tu, r[1], (1.0f - tu) * r[0]);
}

// the sum of the 256 partials by a halving tree, returned to every thread (all threads must call)
__device__ __forceinline__ double tree_sum(double v, double *red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int h = kThreads / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    const double t = red[0];
    __syncthreads();                             // red is used again
    return t;
}

struct Transform {
    const float *src;                            // [n_src, S, S]
    const int *idx, *ang, *shift;                // [M], [M], [M, 2]
    const float *cs;                             // [A_n, 2]
    int n_src, S, A_n;
    int r2, masked, count;                       // radius^2; the mask applies; pixels inside it (normalisation)
    const int *pix;                              // [D] or null
    int D, ldo;
    float *out;
};

// grid: M workgroups; dynamic LDS: S*S floats, and with kNorm S*S floats and 256 doubles more
template <bool kNorm>
__global__ __launch_bounds__(kThreads) void class_transform_kernel(Transform t) {
    extern __shared__ __align__(16) unsigned char lds[];
    float *img = reinterpret_cast<float *>(lds);
    const int S = t.S, npix = S * S, c = S / 2, tid = threadIdx.x;
    const long m = blockIdx.x;
    const int source = clampi(t.idx[m], 0, t.n_src - 1), a = clampi(t.ang[m], 0, t.A_n - 1);
    const int dy = clampi(t.shift[2 * m], -kMaxShiftAbs, kMaxShiftAbs);
    const int dx = clampi(t.shift[2 * m + 1], -kMaxShiftAbs, kMaxShiftAbs);
    const float ct = t.cs[2 * a], st = t.cs[2 * a + 1];
    const float4 *__restrict__ p = reinterpret_cast<const float4 *>(t.src + (long)source * npix);
    for (int e = tid; e < npix / 4; e += kThreads) reinterpret_cast<float4 *>(img)[e] = p[e];   // S is even: whole float4
    __syncthreads();

    auto value = [&](int e) {                                  // the masked transform value at linear pixel e
        const int i = e / S, j = e - i * S;
        if (t.masked && (i - c) * (i - c) + (j - c) * (j - c) > t.r2) return 0.0f;
        return class_value(img, S, ct, st, dy, dx, i, j);
    };
    if constexpr (!kNorm) {
        if (t.pix) {
            float *__restrict__ o = t.out + m * t.ldo;
            for (int q = tid; q < t.ldo; q += kThreads) o[q] = q < t.D ? value(clampi(t.pix[q], 0, npix - 1)) : 0.0f;
        } else {
            float *__restrict__ o = t.out + m * npix;
            for (int e = tid; e < npix; e += kThreads) o[e] = value(e);
        }
    } else {
        auto inside = [&](int e) {
            const int i = e / S, j = e - i * S;
            return (i - c) * (i - c) + (j - c) * (j - c) <= t.r2;
        };
        float *vals = img + npix;
        double *red = reinterpret_cast<double *>(vals + npix);  // 8-byte aligned: 2 * npix floats, npix a multiple of 4
        double s = 0.0;
        for (int e = tid; e < npix; e += kThreads) {
            const float v = value(e);
            vals[e] = v;
            s += (double)v;
        }
        const double sum = tree_sum(s, red);
        const float mean = t.count > 0 ? (float)(sum / (double)t.count) : 0.0f;
        double q2 = 0.0;
        for (int e = tid; e < npix; e += kThreads) {
            const float w = inside(e) ? vals[e] - mean : 0.0f;
            vals[e] = w;
            q2 += (double)w * (double)w;
        }
        const float norm = sqrtf((float)tree_sum(q2, red));    // correctly rounded (__fsqrt_rn is the native, approximate one)
        const bool ok = t.count > 0 && norm > 0.0f;            // the same bits in every lane
        for (int e = tid; e < npix; e += kThreads) vals[e] = ok ? __fdiv_rn(vals[e], norm) : 0.0f;
        __syncthreads();
        if (t.pix) {
            float *__restrict__ o = t.out + m * t.ldo;
            for (int q = tid; q < t.ldo; q += kThreads) o[q] = q < t.D ? vals[clampi(t.pix[q], 0, npix - 1)] : 0.0f;
        } else {
            float *__restrict__ o = t.out + m * npix;
            for (int e = tid; e < npix; e += kThreads) o[e] = vals[e];
        }
    }
}

// ---- scores of rows r0 .. r0+63 of Q against every bank row, and their best ----------------------------------------------------
// grid: ceil(N / 64) workgroups
__global__ __launch_bounds__(kThreads) void class_score_kernel(const float *__restrict__ Q, int ldq, int N,
                                                               const float *__restrict__ B, int ldb, int Mb, int D,
                                                               float *__restrict__ scores, long lds,
                                                               float *__restrict__ best_score, int *__restrict__ best_index) {
    const int r0 = blockIdx.x * kTile;
    const int tid = threadIdx.x, wave = tid >> 6, lr = tid & 15, lk = (tid & 63) >> 4;
    const bool active = r0 + wave * 16 < N;                    // wave-uniform
    float bv[4];                                               // the running best of rows r0 + wave*16 + lk*4 + g
    int bi[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        bv[g] = -__builtin_inff();
        bi[g] = 0x7fffffff;
    }
    // rows of Q at or past N and bank rows at or past Mb are staged as zeros; D is a multiple of 4: no K position is padded
    for (int c0 = 0; c0 < Mb; c0 += kTile) {
        int walk = 0;                                          // for_each_output: tiles in order, g ascending within a tile
        matrix_rows_body<true>(Q, ldq, N, B, ldb, Mb, D, r0, c0, [=, &walk, &bv, &bi](int n, int m, float v) {
            const int g = walk++ & 3;
            if (n < N && m < Mb) {
                if (scores) scores[(long)n * lds + m] = v;
                if (v > bv[g]) {                               // this lane's columns come in ascending order
                    bv[g] = v;
                    bi[g] = m;
                }
            }
        });
    }
    if (!active) return;
    // the 16 lanes lr of a row: the greater score, and of equal scores the lower index
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const float ov = __shfl_xor(bv[g], o, 64);
            const int oi = __shfl_xor(bi[g], o, 64);
            if (ov > bv[g] || (ov == bv[g] && oi < bi[g])) {
                bv[g] = ov;
                bi[g] = oi;
            }
        }
        const int n = r0 + wave * 16 + lk * 4 + g;
        if (lr == 0 && n < N) {
            best_score[n] = bv[g];
            best_index[n] = bi[g];
        }
    }
}

struct Average {
    const float *src;                            // [n_src, S, S]
    const int *ang, *shift;                      // [n_src], [n_src, 2]: by particle
    const float *cs;                             // [A_n, 2]
    const int *members, *offsets;                // [N], [K + 1]
    int n_src, S, A_n, N;
    float *out;                                  // [K, S, S]
};

// grid (ceil(S*S / 256), K)
__global__ __launch_bounds__(kThreads) void class_average_kernel(Average t) {
    const int S = t.S, npix = S * S, k = blockIdx.y;
    const int beg = clampi(t.offsets[k], 0, t.N), end = clampi(t.offsets[k + 1], 0, t.N);
    if (end <= beg) return;                                    // an empty class keeps what it has
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= npix) return;
    const int i = e / S, j = e - i * S;
    auto member = [&](int n) {                                 // the transform value of list entry n at this pixel
        const int p = clampi(t.members[n], 0, t.n_src - 1), a = clampi(t.ang[p], 0, t.A_n - 1);
        const int dy = clampi(t.shift[2 * (long)p], -kMaxShiftAbs, kMaxShiftAbs);
        const int dx = clampi(t.shift[2 * (long)p + 1], -kMaxShiftAbs, kMaxShiftAbs);
        return class_value(t.src + (long)p * npix, S, t.cs[2 * a], t.cs[2 * a + 1], dy, dx, i, j);
    };
    // kAhead members' taps are in flight together (one at a time, a member is three dependent round trips to memory); the
    // adds stay in list order
    constexpr int kAhead = 4;
    float sum = 0.0f;
    int n = beg;
    for (; n + kAhead <= end; n += kAhead) {
        float v[kAhead];
#pragma unroll
        for (int b = 0; b < kAhead; ++b) v[b] = member(n + b);
#pragma unroll
        for (int b = 0; b < kAhead; ++b) sum = sum + v[b];
    }
    for (; n < end; ++n) sum = sum + member(n);
    t.out[(long)k * npix + e] = sum * (1.0f / (float)(end - beg));
}

inline bool side_ok(int S) { return 2 <= S && S <= kMaxSide && S % 2 == 0; }
inline bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" {

int sprk_class_transform(const float *src, int n_src, int S, const int *idx, const int *ang, const int *shift, int M,
                         const float *cs, int A_n, int radius, int flags, const int *pix, int D, int ldo, float *out,
                         void *stream) {
    SPRK_REQUIRE(side_ok(S), "class_transform: images of side %d (even, 2..%d)", S, kMaxSide);
    SPRK_REQUIRE(n_src >= 1 && M >= 1, "class_transform: %d source images and %d outputs (at least 1 each)", n_src, M);
    SPRK_REQUIRE(1 <= A_n && A_n <= kMaxAngles, "class_transform: an angle table of %d entries (1..%d)", A_n, kMaxAngles);
    SPRK_REQUIRE((flags & ~(SPRK_CLASS_MASK | SPRK_CLASS_NORMALIZE)) == 0, "class_transform: unknown flags 0x%x", flags);
    SPRK_REQUIRE(flags == 0 || (0 <= radius && radius <= S), "class_transform: mask radius %d (0..%d)", radius, S);
    SPRK_REQUIRE(src && idx && ang && shift && cs && out, "class_transform: null pointer");
    SPRK_REQUIRE(aligned(src, 16) && aligned(out, 16) && aligned(idx, 4) && aligned(ang, 4) && aligned(shift, 4) &&
                     aligned(cs, 4) && aligned(pix, 4),
                 "class_transform: src and out must start 16-byte aligned, the index arrays and the table 4-byte aligned");
    if (pix)
        SPRK_REQUIRE(1 <= D && D <= S * S && ldo >= D && ldo % 4 == 0,
                     "class_transform: a packed output of %d pixels with row stride %d (1 <= D <= S*S = %d, ldo a multiple "
                     "of 4, at least D)", D, ldo, S * S);
    Transform t{src, idx, ang, shift, cs, n_src, S, A_n, radius * radius, flags != 0, 0, pix, D, ldo, out};
    const bool norm = flags & SPRK_CLASS_NORMALIZE;
    const int c = S / 2;
    if (norm)
        for (int i = 0; i < S; ++i)
            for (int j = 0; j < S; ++j) t.count += (i - c) * (i - c) + (j - c) * (j - c) <= t.r2;
    const size_t image = (size_t)S * S * sizeof(float);
    const size_t lds = norm ? 2 * image + kThreads * sizeof(double) : image;
    auto *kernel = norm ? class_transform_kernel<true> : class_transform_kernel<false>;
    if (int rc = sprk::lds_optin(kernel, lds, "class_transform")) return rc;
    hipLaunchKernelGGL(kernel, dim3(M), dim3(kThreads), lds, (hipStream_t)stream, t);
    return sprk::check_launch("class_transform");
}

int sprk_class_score(const float *Q, int ldq, int N, const float *B, int ldb, int Mb, int D, float *scores, long lds,
                     float *best_score, int *best_index, void *stream) {
    SPRK_REQUIRE(N >= 1 && (long)sprk::cdiv(N, kTile) <= 0x7fffffffL, "class_score: %d rows (at least 1)", N);
    SPRK_REQUIRE(1 <= Mb && Mb <= kMaxBank, "class_score: a bank of %d rows (1..%d)", Mb, kMaxBank);
    SPRK_REQUIRE(4 <= D && D <= kMaxD && D % 4 == 0, "class_score: %d columns (a multiple of 4 in 4..%d)", D, kMaxD);
    SPRK_REQUIRE(ldq >= D && ldq % 4 == 0 && ldb >= D && ldb % 4 == 0,
                 "class_score: row strides %d and %d (multiples of 4, at least D = %d)", ldq, ldb, D);
    SPRK_REQUIRE(Q && B && best_score && best_index, "class_score: null pointer");
    SPRK_REQUIRE(!scores || lds >= Mb, "class_score: row stride %ld of the score matrix (at least Mb = %d)", lds, Mb);
    SPRK_REQUIRE(aligned(Q, 16) && aligned(B, 16) && aligned(scores, 4) && aligned(best_score, 4) && aligned(best_index, 4),
                 "class_score: Q and B must start 16-byte aligned, the outputs 4-byte aligned");
    hipLaunchKernelGGL(class_score_kernel, dim3(sprk::cdiv(N, kTile)), dim3(kThreads), 0, (hipStream_t)stream, Q, ldq, N, B,
                       ldb, Mb, D, scores, lds, best_score, best_index);
    return sprk::check_launch("class_score");
}

int sprk_class_average(const float *src, int n_src, int S, const int *ang, const int *shift, const float *cs, int A_n,
                       const int *members, int N, const int *offsets, int K, float *out, void *stream) {
    SPRK_REQUIRE(side_ok(S), "class_average: images of side %d (even, 2..%d)", S, kMaxSide);
    SPRK_REQUIRE(n_src >= 1 && 1 <= N, "class_average: %d particles and %d members (at least 1 each)", n_src, N);
    SPRK_REQUIRE(1 <= K && K <= 65535, "class_average: %d classes (1..65535)", K);
    SPRK_REQUIRE(1 <= A_n && A_n <= kMaxAngles, "class_average: an angle table of %d entries (1..%d)", A_n, kMaxAngles);
    SPRK_REQUIRE(src && ang && shift && cs && members && offsets && out, "class_average: null pointer");
    SPRK_REQUIRE(aligned(src, 4) && aligned(out, 4) && aligned(ang, 4) && aligned(shift, 4) && aligned(cs, 4) &&
                     aligned(members, 4) && aligned(offsets, 4),
                 "class_average: every array must start 4-byte aligned");
    SPRK_REQUIRE(src != out, "class_average: out must not be src");
    const Average t{src, ang, shift, cs, members, offsets, n_src, S, A_n, N, out};
    hipLaunchKernelGGL(class_average_kernel, dim3(sprk::cdiv(S * S, kThreads), K), dim3(kThreads), 0, (hipStream_t)stream, t);
    return sprk::check_launch("class_average");
}

}  // extern "C"
