// Contamination mask: the reference's find_contamination (utils/algorithms.py:24-57), on the device.
//
// The reference min-max normalises the denoised micrograph to uint8 (cv2.normalize), box-blurs the crop
// u[c:H-c, c:W-c] (cv2.blur), flags blurred pixels below mean - k_low*std or above mean + k_high*std of the WHOLE
// uint8 image, and adds, for every flagged pixel (i, j) and every disk offset di^2 + dj^2 <= r^2, the flat index
// clip(i+di, 0, Hb) * Wb + clip(j+dj, 0, Wb) to a set (Hb = H-2c, Wb = W-2c: the crop's frame).
//
// The set as a dilation.  Clipping at 0 only re-adds points that the disk already holds at row / column 0 (the
// disk is convex and the seed lies inside the frame), and clipping at Hb / Wb likewise only re-adds the disk's own
// points on the virtual row Hb / column Wb.  So the set is exactly
//     C = { y*Wb + x : 0 <= y <= Hb, 0 <= x <= Wb, some seed (i, j) has (y-i)^2 + (x-j)^2 <= r^2 }
// on a grid one row and one column larger than the crop; a point of the virtual column x = Wb is the flat index
// (y+1)*Wb, column 0 of the next row.  Evaluated as a gather: per seed row i and column x the distance hd(i, x) to
// the nearest seed of that row (capped at r+1), and D(y, x) = OR_i [hd(i, x) <= floor(sqrt(r^2 - (y-i)^2))].
// Nothing scatters: the cost does not depend on how many pixels are seeds.
//
// Output frames.  set_bitmap[f], f in [0, (Hb+1)*Wb], is 1 iff f is in C (the reference's own frame).  mask[H, W]
// holds C in the score map's frame: f masks pixel (f / Wb + c, f % Wb + c) — un-flatten where the index was made,
// then undo the crop.  So mask[y+c][x+c] = set_bitmap[y*Wb + x] for 0 <= x < Wb, 0 <= y <= Hb+1, and 0
// elsewhere.
//
// Restatements, not pinned by a cv2 run (cv2 is not a dependency of this project): the normalisation is
// u = rint_half_even(fl32(fl32(x*a) + b)) saturated to [0, 255], a = float(255/(max-min)), b = float(-min*255/(max-min))
// with the quotient in double, no FMA contraction (u = 0 everywhere when max - min <= DBL_EPSILON); the blur is
// (sum + K*K/2) / (K*K) over a KxK window (K*K is odd: no ties), BORDER_REFLECT_101 at the crop's edges (cv2's
// borderInterpolate loop, a NumPy view being a whole image to cv2).
//
// Non-finite input: min and max are taken over the finite pixels; a NaN pixel normalises to 0, +-inf saturate to
// 255 / 0.  A map with no finite pixel normalises to all zeros and yields an empty mask (stats min = max = NaN).
#include <cfloat>

#include "common.h"
#include "range_dev.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxR = 31;          // 2r+1 <= 63: a seed window fits one 64-bit word
constexpr int kMaxHalfK = 7;       // blur windows up to 15x15
constexpr int kBlurRows = 16;      // blur tile: 16 rows x 64 columns (one 64-bit seed word per wave and row)
constexpr int kDilRows = 32;       // dilation tile: 32 mask rows x 64 columns

// control block at the head of the workspace
struct Ctl {
    unsigned int min_enc, max_enc;     // order-preserving encodings of the finite min / max
    unsigned int hist[256];
    unsigned long long seeds, covered;
    double thr_lo, thr_hi;
};

// cv2::borderInterpolate(p, len, BORDER_REFLECT_101)
__device__ __forceinline__ int reflect101(int p, int len) {
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    do {
        p = p < 0 ? -p : 2 * len - 2 - p;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}

__global__ void contam_init_kernel(Ctl *__restrict__ ctl) {
    const int t = threadIdx.x;
    ctl->hist[t] = 0;
    if (t == 0) {
        ctl->min_enc = 0xffffffffu;
        ctl->max_enc = 0u;
        ctl->seeds = 0;
        ctl->covered = 0;
    }
}

__global__ __launch_bounds__(kThreads) void contam_minmax_kernel(const float *__restrict__ img, long n,
                                                                 Ctl *__restrict__ ctl) {
    unsigned int lo = 0xffffffffu, hi = 0u;
    for (long e = (long)blockIdx.x * kThreads + threadIdx.x; e < n; e += (long)gridDim.x * kThreads) {
        const float f = img[e];
        if (isfinite(f)) {
            const unsigned int k = enc(f);
            lo = min(lo, k);
            hi = max(hi, k);
        }
    }
    if (block_reduce<kThreads>(lo, hi) && lo != 0xffffffffu) {
        atomicMin(&ctl->min_enc, lo);
        atomicMax(&ctl->max_enc, hi);
    }
}

// u = saturate(rint(x*a + b)) with a, b from the finite min / max (header); 256-bin histogram of u
__global__ __launch_bounds__(kThreads) void contam_normalise_kernel(const float *__restrict__ img, long n,
                                                                    unsigned char *__restrict__ u, Ctl *__restrict__ ctl) {
    __shared__ unsigned int hist[4][256];   // one sub-histogram per wave: a flat image puts every add on one bin
    __shared__ float ab[2];
    for (int k = threadIdx.x; k < 4 * 256; k += kThreads) (&hist[0][0])[k] = 0;
    if (threadIdx.x == 0) {
        float a = 0.f, b = 0.f;
        const unsigned int le = ctl->min_enc, he = ctl->max_enc;
        if (le != 0xffffffffu) {
            const double lo = (double)dec(le), hi = (double)dec(he);
            if (hi - lo > DBL_EPSILON) {
                const double s = 255.0 / (hi - lo);
                a = (float)s;
                b = (float)(-lo * s);
            }
        }
        ab[0] = a;
        ab[1] = b;
    }
    __syncthreads();
    const float a = ab[0], b = ab[1];
    unsigned int *h = hist[threadIdx.x >> 6];
    for (long e = (long)blockIdx.x * kThreads + threadIdx.x; e < n; e += (long)gridDim.x * kThreads) {
        const float v = rintf(__fadd_rn(__fmul_rn(img[e], a), b));
        const int q = v != v ? 0 : (int)fminf(fmaxf(v, 0.f), 255.f);
        u[e] = (unsigned char)q;
        atomicAdd(&h[q], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 256; k += kThreads) {
        const unsigned int c = hist[0][k] + hist[1][k] + hist[2][k] + hist[3][k];
        if (c) atomicAdd(&ctl->hist[k], c);
    }
}

// mean / population std of u from the exact counts (np.mean / np.std), thresholds, stats[0..5]
__global__ __launch_bounds__(kThreads) void contam_stats_kernel(Ctl *__restrict__ ctl, long n, double k_low,
                                                                double k_high, double *__restrict__ stats) {
    __shared__ double red[kThreads];
    __shared__ unsigned long long isum[kThreads];
    const int t = threadIdx.x;
    const unsigned int c = ctl->hist[t];
    isum[t] = (unsigned long long)c * (unsigned long long)t;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (t < s) isum[t] += isum[t + s];
        __syncthreads();
    }
    const double mean = (double)isum[0] / (double)n;   // the sum is exact: np.mean's pairwise sum of integers is too
    const double d = (double)t - mean;
    red[t] = (double)c * (d * d);
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) {
        const double sd = sqrt(red[0] / (double)n);
        ctl->thr_lo = mean - sd * k_low;
        ctl->thr_hi = mean + sd * k_high;
        const bool any = ctl->min_enc != 0xffffffffu;
        stats[0] = any ? (double)dec(ctl->min_enc) : __builtin_nan("");
        stats[1] = any ? (double)dec(ctl->max_enc) : __builtin_nan("");
        stats[2] = mean;
        stats[3] = sd;
        stats[4] = ctl->thr_lo;
        stats[5] = ctl->thr_hi;
    }
}

// KxK box blur of the crop (reflect-101 inside it) and the thresholds: one bit per crop pixel, rows of WW 64-bit
// words (bit b of word q = column 64q + b; columns >= Wb are 0).  Tile: kBlurRows rows x 64 columns, wave w takes
// rows w, w+4, ...
__global__ __launch_bounds__(kThreads) void contam_seed_kernel(const unsigned char *__restrict__ u, int W, int crop,
                                                               int Hb, int Wb, int WW, int half,
                                                               const Ctl *__restrict__ ctl,
                                                               unsigned long long *__restrict__ bits,
                                                               unsigned long long *__restrict__ seeds) {
    constexpr int TW = 64 + 2 * kMaxHalfK;
    __shared__ unsigned char tile[kBlurRows + 2 * kMaxHalfK][TW];
    const int i0 = blockIdx.y * kBlurRows, j0 = blockIdx.x * 64;
    const int rows = kBlurRows + 2 * half, cols = 64 + 2 * half;
    for (int e = threadIdx.x; e < rows * cols; e += kThreads) {
        const int ly = e / cols, lx = e - ly * cols;
        const int i = reflect101(min(i0 - half + ly, Hb - 1 + half), Hb);   // rows past the tile's last useful one:
        const int j = reflect101(min(j0 - half + lx, Wb - 1 + half), Wb);   // any in-range pixel (never read)
        tile[ly][lx] = u[(long)(i + crop) * W + (j + crop)];
    }
    __syncthreads();
    const double lo = ctl->thr_lo, hi = ctl->thr_hi;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = 2 * half + 1, KK = K * K;
    int found = 0;
    for (int ly = wave; ly < kBlurRows; ly += kThreads / 64) {
        const int i = i0 + ly, j = j0 + lane;
        bool seed = false;
        if (i < Hb && j < Wb) {
            int sum = 0;
            for (int dy = 0; dy < K; ++dy)
                for (int dx = 0; dx < K; ++dx) sum += tile[ly + dy][lane + dx];
            const double v = (double)((sum + KK / 2) / KK);
            seed = v < lo || v > hi;
        }
        const unsigned long long m = __ballot(seed);
        if (i < Hb && lane == 0) {
            bits[(long)i * WW + blockIdx.x] = m;
            found += __popcll(m);
        }
    }
    if (lane == 0 && found) atomicAdd(seeds, (unsigned long long)found);
}

// distance from column x (0 <= x <= Wb) to the nearest seed of row `row`, r+1 if none is within r
__device__ __forceinline__ int row_dist(const unsigned long long *__restrict__ row, int WW, int x, int r) {
    const int c = x - r;                       // window: columns x-r .. x+r, bit k = column c+k
    const int q = c >= 0 ? c >> 6 : -1;        // c >= -31
    const int sh = c - 64 * q;
    const unsigned long long w0 = (q >= 0 && q < WW) ? row[q] : 0ull;
    const unsigned long long w1 = (q + 1 >= 0 && q + 1 < WW) ? row[q + 1] : 0ull;
    unsigned long long v = sh ? (w0 >> sh) | (w1 << (64 - sh)) : w0;
    v &= (2ull << (2 * r)) - 1;                // 2r+1 bits
    const unsigned long long right = v >> r;   // bit 0 = column x
    const unsigned long long left = v & ((2ull << r) - 1);   // bit r = column x
    const int dr = right ? __ffsll((long long)right) - 1 : r + 1;
    const int dl = left ? r - (63 - __clzll((long long)left)) : r + 1;
    return min(dl, dr);
}

// D(y, x) from global seed bits (the virtual column's wrap term, one lane per mask row)
__device__ bool covered_global(const unsigned long long *__restrict__ bits, int WW, int Hb, int y, int x, int r,
                               const unsigned char *__restrict__ reach) {
    for (int i = max(0, y - r); i <= min(Hb - 1, y + r); ++i)
        if (row_dist(bits + (long)i * WW, WW, x, r) <= reach[abs(y - i)]) return true;
    return false;
}

// mask[H, W] (score-map frame) and, if set_bitmap, C in the reference's frame.  Tile: kDilRows mask rows x 64 mask
// columns; LDS holds hd for the seed rows the tile's disks reach.
__global__ __launch_bounds__(kThreads) void contam_dilate_kernel(const unsigned long long *__restrict__ bits, int H,
                                                                 int W, int crop, int Hb, int Wb, int WW, int r,
                                                                 unsigned char *__restrict__ mask,
                                                                 unsigned char *__restrict__ set_bitmap,
                                                                 unsigned long long *__restrict__ covered) {
    __shared__ unsigned char hd[kDilRows + 2 * kMaxR][64];
    __shared__ unsigned char reach[kMaxR + 1];
    __shared__ unsigned int count;
    const int r0 = blockIdx.y * kDilRows, c0 = blockIdx.x * 64;
    const int y0 = r0 - crop, x0 = c0 - crop;          // extended-grid coordinates of the tile's corner
    if (threadIdx.x <= r) {
        const int a = threadIdx.x;
        int d = (int)sqrtf((float)(r * r - a * a));
        while ((d + 1) * (d + 1) + a * a <= r * r) ++d;
        while (d * d + a * a > r * r) --d;
        reach[a] = (unsigned char)d;
    }
    if (threadIdx.x == 0) count = 0;
    const int rows = kDilRows + 2 * r;
    for (int e = threadIdx.x; e < rows * 64; e += kThreads) {
        const int ly = e >> 6, lx = e & 63;
        const int i = y0 - r + ly, x = x0 + lx;
        hd[ly][lx] = (i >= 0 && i < Hb && x >= 0 && x <= Wb) ? (unsigned char)row_dist(bits + (long)i * WW, WW, x, r)
                                                                : (unsigned char)(r + 1);
    }
    __syncthreads();
    const int lx = threadIdx.x & 63;
    const int c = c0 + lx, x = x0 + lx;
    unsigned int mine = 0;
    for (int ly = threadIdx.x >> 6; ly < kDilRows; ly += kThreads / 64) {
        const int rr = r0 + ly, y = y0 + ly;
        if (rr >= H || c >= W) continue;
        // the crop grid's rows 0..Hb, and of row Hb+1 only column 0: the last index (Hb+1)*Wb
        const bool inside = x >= 0 && x < Wb && y >= 0 && (y <= Hb || (y == Hb + 1 && x == 0));
        bool m = false;
        if (inside && y <= Hb)
            for (int d = -r; d <= r && !m; ++d) m = hd[ly + r + d][lx] <= reach[abs(d)];
        if (inside && x == 0 && y >= 1 && !m) m = covered_global(bits, WW, Hb, y - 1, Wb, r, reach);
        mask[(long)rr * W + c] = (unsigned char)m;
        if (inside && set_bitmap) set_bitmap[(long)y * Wb + x] = (unsigned char)m;
        mine += m;
    }
    if (mine) atomicAdd(&count, mine);
    __syncthreads();
    if (threadIdx.x == 0 && count) atomicAdd(covered, (unsigned long long)count);
}

__global__ void contam_finish_kernel(const Ctl *__restrict__ ctl, double *__restrict__ stats) {
    stats[6] = (double)ctl->seeds;
    stats[7] = (double)ctl->covered;
}

struct ContamWs {
    size_t off_u, off_bits, total;
    int WW;
};

ContamWs contam_layout(int H, int W, int crop) {
    ContamWs L{};
    const int Hb = H - 2 * crop, Wb = W - 2 * crop;
    L.WW = (Wb + 63) / 64;
    L.off_u = 4096;
    static_assert(sizeof(Ctl) <= 4096, "control block");
    L.off_bits = L.off_u + (((size_t)H * W + 255) & ~(size_t)255);
    L.total = L.off_bits + (size_t)Hb * L.WW * 8;
    return L;
}

}  // namespace

extern "C" {

size_t sprk_contam_ws_bytes(int H, int W) {
    if (H < 1 || W < 1) return 0;
    // the crop only shrinks the seed bitmap: size for crop 0, any valid crop then fits
    return contam_layout(H, W, 0).total;
}

int sprk_contam_mask(const float *img, int H, int W, int crop, int ksize, double k_low, double k_high, int radius,
                     uint8_t *mask_out, uint8_t *set_bitmap_out, double *stats_out, void *ws, size_t ws_bytes,
                     void *stream) {
    SPRK_REQUIRE(img && mask_out && stats_out, "contam_mask: null pointer");
    SPRK_REQUIRE(H > 0 && W > 0 && (long)H * W < (1L << 31), "contam_mask: bad map size %dx%d", H, W);
    // crop >= 2: the last index of C, (Hb+1)*Wb, maps to mask row H-crop+1, which must lie inside the map
    SPRK_REQUIRE(crop >= 2 && H - 2 * crop >= 1 && W - 2 * crop >= 1, "contam_mask: crop %d (>= 2) on a %dx%d map",
                 crop, H, W);
    SPRK_REQUIRE(ksize >= 1 && ksize <= 2 * kMaxHalfK + 1 && (ksize & 1), "contam_mask: ksize %d (odd, <= %d)", ksize,
                 2 * kMaxHalfK + 1);
    SPRK_REQUIRE(radius >= 0 && radius <= kMaxR, "contam_mask: radius %d (0..%d)", radius, kMaxR);
    const size_t need = sprk_contam_ws_bytes(H, W);
    if (!ws || ws_bytes < need) {
        sprk::set_error("contam_mask: workspace %zu < %zu", ws_bytes, need);
        return SPRK_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const ContamWs L = contam_layout(H, W, crop);
    unsigned char *base = (unsigned char *)ws;
    Ctl *ctl = (Ctl *)base;
    unsigned char *u = base + L.off_u;
    unsigned long long *bits = (unsigned long long *)(base + L.off_bits);
    const int Hb = H - 2 * crop, Wb = W - 2 * crop;
    const long n = (long)H * W;
    const int grid = std::min(sprk::ew_blocks(n), 2048);

    hipLaunchKernelGGL(contam_init_kernel, dim3(1), dim3(256), 0, s, ctl);
    if (int rc = sprk::check_launch("contam_init")) return rc;
    hipLaunchKernelGGL(contam_minmax_kernel, dim3(grid), dim3(kThreads), 0, s, img, n, ctl);
    if (int rc = sprk::check_launch("contam_minmax")) return rc;
    hipLaunchKernelGGL(contam_normalise_kernel, dim3(grid), dim3(kThreads), 0, s, img, n, u, ctl);
    if (int rc = sprk::check_launch("contam_normalise")) return rc;
    hipLaunchKernelGGL(contam_stats_kernel, dim3(1), dim3(kThreads), 0, s, ctl, n, k_low, k_high, stats_out);
    if (int rc = sprk::check_launch("contam_stats")) return rc;
    hipLaunchKernelGGL(contam_seed_kernel, dim3(L.WW, sprk::cdiv(Hb, kBlurRows)), dim3(kThreads), 0, s, u, W, crop, Hb,
                       Wb, L.WW, ksize / 2, ctl, bits, &ctl->seeds);
    if (int rc = sprk::check_launch("contam_seed")) return rc;
    hipLaunchKernelGGL(contam_dilate_kernel, dim3(sprk::cdiv(W, 64), sprk::cdiv(H, kDilRows)), dim3(kThreads), 0, s,
                       bits, H, W, crop, Hb, Wb, L.WW, radius, mask_out, set_bitmap_out, &ctl->covered);
    if (int rc = sprk::check_launch("contam_dilate")) return rc;
    hipLaunchKernelGGL(contam_finish_kernel, dim3(1), dim3(1), 0, s, ctl, stats_out);
    return sprk::check_launch("contam_finish");
}

}  // extern "C"
