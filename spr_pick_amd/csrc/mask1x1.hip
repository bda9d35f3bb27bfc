// Backward-data of the 1x1 layers of the U-Nets' heads with the activation backward of the layer in front in its store.
//
//   gin[n][c][p] = act'(mask[n][c][p]) * sum_k gy[n][k][p] * w[k][c],    K <= 96
//
// A plain GEMM [pixels x K] . [K x N] per image plane: no halo, no taps, no tables of input offsets.  conv_mfma_kernel
// writes the unmasked product and act_bwd_kernel then reads it back, reads the mask and writes it again; here the
// mask is multiplied in before the only store.  The sums are conv_mfma_kernel's (chunk_mma), operation for operation:
// every output element has ONE accumulator that starts at 0 and takes one v_mfma_f32_16x16x4_f32 per k-step, pixels in
// the A operand and weights in the B operand, lane group lq holding K row 4q + lq of step q, steps in increasing q
// chunk by chunk, rows past a chunk's end as (first channel of the chunk) x (zero weight row) — read from the very
// slab transform_weights wrote for that kernel.  Its epilogue computes acc * 1 + 0 (no bias, no scale), which turns a
// -0 into +0: the + 0.f below.  Then act_bwd_kernel's m > 0 ? v : v * 0.1f (or 0).
//
// Decomposition: grid (workgroups, slabs of NT * 16 output channels).  A workgroup keeps its slab in LDS for its whole
// life and walks tiles of kTP = 128 consecutive pixels of one image plane, t = blockIdx.x, + gridDim.x, ...: the
// [K][128] block of gy arrives by 16-byte LDS-DMA, double buffered (the next tile's block is in flight under this tile's
// MFMAs), each of the 4 waves owns 32 pixels x NT * 16 channels, fetches its part of the mask before the MFMAs (the
// loads are in flight under them) and stores float4 (4 consecutive pixels of one channel).  The workgroups of one
// pixel tile (blockIdx.y = 0 .. nblkN - 1) are gridDim.x apart in launch order, a multiple of 8: they share an XCD and
// its L2, so gy comes from HBM once.
#include "mask1x1.h"

#include "conv_dev.h"

namespace {

constexpr int kTP = 128;            // pixels per tile
constexpr int kMaxSteps = 30;       // k-steps of a call (K = 96 in chunks of 16: 24)
constexpr int kTabEntries = kMaxSteps + 2;

struct M1Args {
    const float *gy, *wT, *mask;
    float *gin;
    int N, K, Cn, HW;
    int CK, R4, rows, ldw;
    int act, steps, tilesPerImg, nTiles;
};

using i32x2 = __attribute__((ext_vector_type(2))) int;
typedef const __attribute__((address_space(3))) i32x2 *lds_ci2p;

template <int NT>
__global__ __launch_bounds__(256) void mask1x1_kernel(const M1Args a) {
    // LDS: step table [kTabEntries][4] of (A byte offset, B byte offset) | weights [rows][ldw] | stage 0, 1: gy [K][kTP]
    extern __shared__ __attribute__((aligned(16))) float smem[];
    i32x2 *tab = reinterpret_cast<i32x2 *>(smem);
    float *w_lds = smem + kTabEntries * 4 * 2;
    const int wFloats = a.rows * a.ldw;
    float *stage = w_lds + wFloats;
    const int stageFloats = a.K * kTP;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    const int nb = blockIdx.y;
    const long HW = a.HW;

    {   // this workgroup's slab, once
        const float *wsrc = a.wT + (long)nb * wFloats;
        const int total4 = wFloats >> 2;
        for (int gi = wave; gi * 64 < total4; gi += 4) {
            const int idx = gi * 64 + lane;
            if (idx < total4) dma16(wsrc + idx * 4, w_lds + gi * 256);
        }
    }
    // the [K][kTP] block of gy of tile t into stage b: one wave instruction moves two channel rows of 32 16-byte pieces;
    // pieces past the end of a ragged last tile re-read the plane's last piece (their pixels are never stored)
    auto issue = [&](int t, int b) {
        const int n = t / a.tilesPerImg, p0 = (t - n * a.tilesPerImg) * kTP;
        const int chl = lane >> 5;
        const int px = min(p0 + (lane & 31) * 4, a.HW - 4);
        const float *src = a.gy + (long)n * a.K * HW + px;
        float *dst = stage + b * stageFloats;
        for (int c = wave * 2; c < a.K; c += 8) {
            const int ch = c + chl;
            if (ch < a.K) dma16(src + (long)ch * HW, dst + c * kTP);   // (odd K: the upper half-wave must not write)
        }
    };
    int t = blockIdx.x;
    issue(t, 0);
    // step s, lane group l: K row 4q + l of chunk ci.  A: the channel's row of the stage; B: the slab row.  Rows past the
    // chunk's end are zero weight rows, paired with the chunk's first channel as in conv_mfma_kernel (k-row offset 0).
    // Two more entries repeat the last step: the software pipeline below reads ahead.
    if (tid < kTabEntries * 4) {
        const int s = min(tid >> 2, a.steps - 1), l = tid & 3;
        int c0 = 0, ci = 0, q = s;
        for (;;) {
            const int nkq = (min(a.CK, a.K - c0) + 3) >> 2;
            if (q < nkq) break;
            q -= nkq;
            c0 += a.CK;
            ++ci;
        }
        const int cke = min(a.CK, a.K - c0), kk = 4 * q + l;
        tab[tid] = i32x2{(c0 + (kk < cke ? kk : 0)) * (kTP * 4), (ci * a.R4 + kk) * (a.ldw * 4)};
    }
    const int abase = lds_addr(stage) + (wave * 32 + l15) * 4;
    const int bbase = lds_addr(w_lds) + l15 * 4;
    lds_ci2p tp = (lds_ci2p)(__SIZE_TYPE__)(unsigned)lds_addr(tab + lq);
    const bool leaky = a.act == SPRK_ACT_LEAKY;

    // Barriers order LDS traffic only (lds_only_barrier): a wave's stores of one tile drain under the MFMAs of the next.
    // What must have landed is waited for explicitly: the slab and the first block here, the next block (and the mask)
    // by the s_waitcnt in front of a tile's stores, i.e. before the wave reaches the barrier that publishes it.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int i = 0; t < a.nTiles; t += gridDim.x, ++i) {
        // every wave's part of this tile's block (the first time also of the slab, and the table) is in LDS, and every
        // wave is done with the other stage
        lds_only_barrier();
        if (t + (int)gridDim.x < a.nTiles) issue(t + gridDim.x, (i + 1) & 1);
        const int n = t / a.tilesPerImg, p0 = (t - n * a.tilesPerImg) * kTP;
        const int pix = p0 + wave * 32 + lq * 4;     // this lane's 4 pixels of pixel tile mt: pix + 16 mt
        // the mask of this tile's outputs: in flight under the MFMAs.  Every lane loads (a branch around a load makes the
        // compiler wait for it at the join, one memory round trip per load): channels past the last and pixels past the
        // plane's end re-read the last valid ones and are never stored
        float4 mk[2][NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int co = min(nb * (NT * 16) + nt * 16 + l15, a.Cn - 1);
            const float *mp = a.mask + ((long)n * a.Cn + co) * HW;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) mk[mt][nt] = *reinterpret_cast<const float4 *>(mp + min(pix + 16 * mt, a.HW - 4));
        }
        f32x4 acc[2][NT];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int sa = abase + (i & 1) * stageFloats * 4;
        float av[2], bv[NT];
        i32x2 e1 = tp[4];
        {
            const i32x2 e0 = tp[0];
            lds_cfp ap = lds_f(sa + e0.x);
            av[0] = ap[0];
            av[1] = ap[16];
            lds_cfp bp = lds_f(bbase + e0.y);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bv[nt] = bp[16 * nt];
        }
        for (int s = 0; s < a.steps; ++s) {
            const i32x2 e2 = tp[(s + 2) * 4];
            float an[2], bn[NT];
            lds_cfp ap = lds_f(sa + e1.x);
            an[0] = ap[0];
            an[1] = ap[16];
            lds_cfp bp = lds_f(bbase + e1.y);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bn[nt] = bp[16 * nt];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
            av[0] = an[0];
            av[1] = an[1];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bv[nt] = bn[nt];
            e1 = e2;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the next tile's block and this tile's mask (no store is pending
                                                           // but the previous tile's, issued a whole MFMA phase ago)
        // (the compiler does not see that wait: naming every mask register here makes it place its own wait for the
        // mask loads in front of the stores, not between them, where it would drain each store before the next)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
                asm volatile("" : "+v"(mk[mt][nt].x), "+v"(mk[mt][nt].y), "+v"(mk[mt][nt].z), "+v"(mk[mt][nt].w));
        // D layout: col (channel) = lane & 15, row (pixel) = (lane >> 4) * 4 + reg
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int co = nb * (NT * 16) + nt * 16 + l15;
            if (co >= a.Cn) continue;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                if (pix + 16 * mt >= a.HW) continue;
                const f32x4 c = acc[mt][nt];
                const float4 m = mk[mt][nt];
                float4 v = make_float4(c[0] + 0.f, c[1] + 0.f, c[2] + 0.f, c[3] + 0.f);
                v.x = m.x > 0.f ? v.x : (leaky ? v.x * kLeak : 0.f);
                v.y = m.y > 0.f ? v.y : (leaky ? v.y * kLeak : 0.f);
                v.z = m.z > 0.f ? v.z : (leaky ? v.z * kLeak : 0.f);
                v.w = m.w > 0.f ? v.w : (leaky ? v.w * kLeak : 0.f);
                *reinterpret_cast<float4 *>(a.gin + ((long)n * a.Cn + co) * HW + pix + 16 * mt) = v;
            }
        }
    }
}

template <int NT>
int launch(const M1Args &a, dim3 grid, size_t lds, hipStream_t s) {
    if (int rc = sprk::lds_optin(mask1x1_kernel<NT>, lds, "mask1x1")) return rc;
    hipLaunchKernelGGL(mask1x1_kernel<NT>, grid, dim3(256), lds, s, a);
    return SPRK_OK;
}

}  // namespace

namespace sprk {

int mask1x1_steps(int K, int CK) {
    if (K < 1 || K > kMask1x1MaxK || CK < 1) return 0;
    int steps = 0;
    for (int c0 = 0; c0 < K; c0 += CK) steps += (std::min(CK, K - c0) + 3) >> 2;
    return steps <= kMaxSteps ? steps : 0;
}

int mask1x1_run(const Mask1x1Call &c, hipStream_t s) {
    M1Args a{};
    a.gy = c.gy; a.wT = c.wT; a.mask = c.mask; a.gin = c.gin;
    a.N = c.N; a.K = c.K; a.Cn = c.Cn; a.HW = c.HW;
    a.CK = c.CK; a.R4 = c.R4; a.rows = c.rows; a.ldw = c.ldw;
    a.act = c.act;
    a.steps = mask1x1_steps(c.K, c.CK);
    a.tilesPerImg = cdiv(c.HW, kTP);
    a.nTiles = c.N * a.tilesPerImg;
    SPRK_REQUIRE(a.steps > 0 && c.HW >= 4 && c.HW % 4 == 0 && (long)c.N * a.tilesPerImg < (1L << 30) &&
                     (c.rows * c.ldw) % 4 == 0 && (c.act == SPRK_ACT_LEAKY || c.act == SPRK_ACT_RELU),
                 "mask1x1: call outside the kernel's limits");
    const size_t lds = ((size_t)kTabEntries * 8 + (size_t)c.rows * c.ldw + 2 * (size_t)c.K * kTP) * sizeof(float);
    SPRK_REQUIRE(lds <= 160 * 1024, "mask1x1: %zu bytes of LDS", lds);
    // one workgroup per CU over all slabs; the workgroups of one pixel tile on one XCD (see above)
    int wgs = std::max(1, num_cus() / c.nblkN);
    if (wgs >= 8) wgs &= ~7;
    const dim3 grid(std::min(a.nTiles, wgs), c.nblkN);
    int rc;
    switch (c.NT) {
        case 1: rc = launch<1>(a, grid, lds, s); break;
        case 2: rc = launch<2>(a, grid, lds, s); break;
        case 3: rc = launch<3>(a, grid, lds, s); break;
        case 4: rc = launch<4>(a, grid, lds, s); break;
        case 6: rc = launch<6>(a, grid, lds, s); break;
        default: set_error("mask1x1: no kernel for %d channel tiles per slab", c.NT); return SPRK_EINVAL;
    }
    if (rc) return rc;
    g_mask1x1_launches.fetch_add(1, std::memory_order_relaxed);
    return SPRK_OK;
}

}  // namespace sprk
