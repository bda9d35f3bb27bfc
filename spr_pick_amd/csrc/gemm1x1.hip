// The wide 1x1 layers of the U-Nets' heads (384 -> 384, 384 -> 96 at 64 x 64, forward and backward-data) as a streaming GEMM.
//
//   y[n][c][p] = act(scale[c] * sum_k x[n][k][p] * w[k][c] + shift[c]),    K >= 192
//
// A plain GEMM [pixels x K] . [K x N] per image plane: no halo, no taps, no tables of input or k-row offsets.  The sums
// are conv_mfma_kernel<4, 6>'s (chunk_mma), operation for operation: every output element has ONE accumulator that starts
// at 0 and takes one v_mfma_f32_16x16x4_f32 per k-step, pixels in the A operand and weights in the B operand, lane group
// lq holding K row 4q + lq of step q, steps in increasing q; rows past the end of a ragged K are the zero weight rows of
// the slab paired with the first channel of the last 16-channel chunk — read from the very slabs transform_weights wrote
// for that kernel (chunks of 16 rows in 16 rows: slab row = reduced channel).  The epilogue is conv_epilogue.inc's
// apply_act(c * sc + sh, act), compiled with the same contraction setting.
//
// Decomposition: persistent workgroups of 4 waves, at most one per CU.  An item is a tile of kTP = 256 consecutive pixels
// of one image plane x NB slabs of 96 output channels (NB = 2 when the layer has two or more slabs: x is staged once
// per 192 channels instead of once per 96); wave w owns pixels 64 w .. 64 w + 63 x all NB * 96 channels (4 x NB * 6
// accumulator tiles).  K is walked in chunks of kKC = 32 rows, double buffered across items: the DMA of the next chunk
// (the next item's first chunk at an item's end) is issued after the barrier that publishes the current one, between the
// MFMAs of its first k-step, a whole chunk of MFMAs (8 k-steps x 24 NB per wave) before it is needed.  Operand addresses
// are base + q * constant.  LDS
// row strides (272 and 112 floats) are = 16 (mod 32): the two K rows a 32-lane ds_read group holds fall on disjoint banks.
// Barriers order LDS only; a tile's stores drain under the next item's MFMAs.  The items of one pixel tile run at the
// same time on workgroups of one XCD (id % 8), so x comes from HBM once.
#include "gemm1x1.h"

#include <type_traits>

#include "conv_dev.h"

namespace {

constexpr int kTP = 256;                    // pixels per tile
constexpr int kXS = kTP + 16;               // row stride of the x block in LDS
constexpr int kKC = 32;                     // K rows per chunk
constexpr int kLdw = sprk::kGemm1x1Ldw;     // row stride of a slab
constexpr int kWInstr = kKC * kLdw / 256;   // 16-byte wave DMAs per slab chunk
static_assert(kKC * kLdw % 256 == 0 && kXS % 32 == 16 && kLdw % 32 == 16, "LDS layout");

struct G1Args {
    const float *x, *wT, *scp, *shp;
    float *y;
    int N, K, Cn, HW;
    int rows, nblkN;
    int act, hasSc, hasSh;
    int steps, nch, c0last;
    int tilesPerImg, nTiles, nh, xcd;
};

template <int NB>
__global__ __launch_bounds__(256) void gemm1x1_kernel(const G1Args a) {
    // LDS: stage 0, 1: x [kKC][kXS] | weights [NB][kKC][kLdw]
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NTT = NB * 6;
    constexpr int stageFloats = kKC * kXS + NB * kKC * kLdw;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    const int G = gridDim.x;

    // the item of this workgroup in round r: pixel tile t, channel part h.  XCD order: the nh parts of a tile on
    // workgroups 8 apart
    auto decode = [&](int r, int &t, int &h) {
        const int b = blockIdx.x;
        if (a.xcd) {
            const int j = b >> 3;
            h = j % a.nh;
            t = r * (G / a.nh) + (j / a.nh) * 8 + (b & 7);
        } else {
            const int it = r * G + b;
            t = it / a.nh;
            h = it - t * a.nh;
        }
        // (uniform, but divisions are vector instructions: back into scalar registers, or every buffer load that
        // takes its descriptor from them is wrapped in a waterfall loop)
        t = __builtin_amdgcn_readfirstlane(t);
        h = __builtin_amdgcn_readfirstlane(h);
        return t < a.nTiles;
    };
    const rsrc_t wr = make_rsrc(a.wT);
    // chunk ci of item (t, h) into stage b.  Every wave issues the same instructions whatever the chunk: rows past K
    // re-read the last chunk's first channel (the rows up to the next multiple of 4 are the zero-weight pairing, the rest
    // is never read), pieces past the plane's or the slab's end re-read the last valid piece
    auto issue = [&](int t, int h, int ci, int b) {
        const int n = __builtin_amdgcn_readfirstlane(t / a.tilesPerImg), p0 = (t - n * a.tilesPerImg) * kTP;
        float *xs = smem + b * stageFloats;
        float *ws = xs + kKC * kXS;
        const rsrc_t xr = make_rsrc(a.x + (long)n * a.K * a.HW);
        const int xv = min(p0 + lane * 4, a.HW - 4) * 4;
        const int r0 = ci * kKC;
#pragma unroll
        for (int i = 0; i < kKC / 4; ++i) {
            const int r = r0 + wave + 4 * i;
            const int ch = r < a.K ? r : a.c0last;
            bdma16(xr, xv, ch * a.HW * 4, xs + (wave + 4 * i) * kXS);
        }
        const int valid = min(kKC, a.rows - r0) * kLdw * 4 - 16;
#pragma unroll
        for (int i0 = 0; i0 < NB * kWInstr; i0 += 4) {
            // (no branch: where the pieces do not divide by the four waves, the last one is copied twice)
            const int i = min(i0 + wave, NB * kWInstr - 1);
            const int nbi = i / kWInstr, ii = i - nbi * kWInstr;
            const int nb = min(h * NB + nbi, a.nblkN - 1);
            bdma16(wr, min(ii * 1024 + lane * 16, valid), (nb * a.rows + r0) * (kLdw * 4), ws + nbi * (kKC * kLdw) + ii * 256);
        }
    };
    constexpr int kDmaPerWave = kKC / 4 + (NB * kWInstr + 3) / 4;   // buffer_load ... lds of one wave and chunk

    int t, h;
    bool ok = decode(0, t, h);
    if (!ok) return;
    issue(t, h, 0, 0);
    const int abase = lds_addr(smem) + (lq * kXS + wave * 64 + l15) * 4;
    const int bbase = lds_addr(smem + kKC * kXS) + (lq * kLdw + l15) * 4;
    int g = 0;   // chunks walked so far: chunk g lives in stage g & 1
    for (int r = 0; ok; ++r) {
        int tn, hn;
        const bool okn = decode(r + 1, tn, hn);
        const int n = __builtin_amdgcn_readfirstlane(t / a.tilesPerImg), p0 = (t - n * a.tilesPerImg) * kTP;
        const int pix = p0 + wave * 64 + lq * 4;     // this lane's 4 pixels of pixel tile mt: pix + 16 mt
        // the epilogue's per-channel constants: in flight under the MFMAs.  Every lane loads, from a clamped index (a
        // branch around a load makes the compiler wait for it at the join); a call without them reads the zero block
        float vsc[NTT], vsh[NTT];
#pragma unroll
        for (int j = 0; j < NTT; ++j) {
            const int idx = min(h * (NB * 96) + j * 16 + l15, a.Cn - 1);
            vsc[j] = a.scp[a.hasSc ? idx : 0];
            vsh[j] = a.shp[a.hasSh ? idx : 0];
        }
        f32x4 acc[4][NTT];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int j = 0; j < NTT; ++j) acc[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};

        for (int ci = 0; ci < a.nch; ++ci, ++g) {
            // this wave's part of chunk g has landed (an item's first chunk was waited for in front of the previous
            // item's stores, which stay in flight); after the barrier every wave's has, and every wave is done with
            // the other stage
            if (ci > 0 || r == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            lds_only_barrier();
            const bool lastc = ci + 1 == a.nch;
            const int nq = min(kKC / 4, a.steps - ci * (kKC / 4));
            const int sa = abase + (g & 1) * (stageFloats * 4), sb = bbase + (g & 1) * (stageFloats * 4);
            // two operand register sets, alternating: the operands of step q + 1 are fetched under the MFMAs of step q
            float a0[4], b0[NTT], a1[4], b1[NTT];
            auto ld = [&](float (&av)[4], float (&bv)[NTT], int q) {
                lds_cfp ap = lds_f(sa + q * (4 * kXS * 4));
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) av[mt] = ap[16 * mt];
                lds_cfp bp = lds_f(sb + q * (4 * kLdw * 4));
#pragma unroll
                for (int j = 0; j < NTT; ++j) bv[j] = bp[(j / 6) * (kKC * kLdw) + 16 * (j % 6)];
            };
            auto mm = [&](const float (&av)[4], const float (&bv)[NTT]) {
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int j = 0; j < NTT; ++j)
                        acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], bv[j], acc[mt][j], 0, 0, 0);
            };
            const int last = nq - 1;
            ld(a0, b0, 0);
            ld(a1, b1, min(1, last));
            // The DMA of the next chunk (the next item's first chunk at an item's end; after the very last chunk the
            // item's first one again, which nobody reads) goes out between the MFMAs of step 0: no branch around it, so
            // that it shares their scheduling region, and a few MFMAs per load asked of the scheduler.  Issued as a
            // block in front of them it would leave the pipes idle for its whole length, once per chunk.
            {
                const bool own = !lastc || !okn;
                issue(own ? t : tn, own ? h : hn, lastc ? 0 : ci + 1, (g + 1) & 1);
            }
            mm(a0, b0);
#pragma unroll
            for (int i = 0; i < kDmaPerWave; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 4 * NTT / kDmaPerWave, 0);   // MFMA
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                       // VMEM
            }
            // steps 1 .. nq - 1; a1 holds step 1 (a re-read of the last step is unused)
            for (int q = 1; q + 1 < nq; q += 2) {
                ld(a0, b0, q + 1);
                mm(a1, b1);
                ld(a1, b1, min(q + 2, last));
                mm(a0, b0);
            }
            if (!(nq & 1)) mm(a1, b1);
        }
        // the next item's first chunk (issued a whole chunk of MFMAs ago) and this item's constants; no store is
        // pending but the previous item's
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // (the compiler does not see that wait: naming the constants here makes it place its own wait for their loads
        // in front of the stores, not between them)
#pragma unroll
        for (int j = 0; j < NTT; ++j) asm volatile("" : "+v"(vsc[j]), "+v"(vsh[j]));
        // D layout: col (channel) = lane & 15, row (pixel) = (lane >> 4) * 4 + reg.  One copy of the stores per
        // activation (a wave-uniform choice made once per item, not once per value)
        auto stores = [&](auto actc) {
            constexpr int ACT = decltype(actc)::value;
#pragma unroll
            for (int j = 0; j < NTT; ++j) {
                const int co = h * (NB * 96) + j * 16 + l15;
                if (co >= a.Cn) continue;
                const float sc = a.hasSc ? vsc[j] : 1.f, sh = vsh[j];
                float *yc = a.y + ((long)n * a.Cn + co) * a.HW + pix;
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    if (pix + 16 * mt >= a.HW) continue;
                    const f32x4 c = acc[mt][j];
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = apply_act(c[e] * sc + sh, ACT);
                    *reinterpret_cast<float4 *>(yc + 16 * mt) = make_float4(v[0], v[1], v[2], v[3]);
                }
            }
        };
        if (a.act == SPRK_ACT_LEAKY)
            stores(std::integral_constant<int, SPRK_ACT_LEAKY>{});
        else if (a.act == SPRK_ACT_RELU)
            stores(std::integral_constant<int, SPRK_ACT_RELU>{});
        else
            stores(std::integral_constant<int, SPRK_ACT_NONE>{});
        t = tn;
        h = hn;
        ok = okn;
    }
}

inline int slabs_per_item(int nblkN) { return nblkN >= 2 ? 2 : 1; }

template <int NB>
int launch(const G1Args &a, int grid, hipStream_t s) {
    const size_t lds = 2 * (size_t)(kKC * kXS + NB * kKC * kLdw) * sizeof(float);
    if (int rc = sprk::lds_optin(gemm1x1_kernel<NB>, lds, "gemm1x1")) return rc;
    hipLaunchKernelGGL(gemm1x1_kernel<NB>, dim3(grid), dim3(256), lds, s, a);
    return SPRK_OK;
}

}  // namespace

namespace sprk {

std::atomic<long> g_gemm1x1_launches{0};
std::atomic<int> g_gemm1x1_on{1};

bool gemm1x1_fits(int N, int K, int HW) {
    return K >= kGemm1x1MinK && HW >= 4 && HW % 4 == 0 && (long)K * HW * 4 < (1L << 31) &&
           (long)N * cdiv(HW, kTP) < (1L << 28);
}

int gemm1x1_grid(int N, int HW, int nblkN) {
    const int nh = cdiv(nblkN, slabs_per_item(nblkN));
    const long items = (long)N * cdiv(HW, kTP) * nh;
    int G = (int)std::min<long>(items, num_cus());
    if (G >= 8 * nh) G -= G % (8 * nh);   // XCD order needs whole groups of 8 * nh workgroups
    return std::max(G, 1);
}

int gemm1x1_run(const Gemm1x1Call &c, hipStream_t s) {
    SPRK_REQUIRE(gemm1x1_fits(c.N, c.K, c.HW) && c.ldw == kLdw && c.rows == cdiv(c.K, 16) * 16 && c.nblkN >= 1 &&
                     c.nblkN == cdiv(c.Cn, 96) && (long)c.nblkN * c.rows * kLdw * 4 < (1L << 31),
                 "gemm1x1: call outside the kernel's limits");
    const int NB = slabs_per_item(c.nblkN);
    G1Args a{};
    a.x = c.x; a.wT = c.wT; a.y = c.y;
    a.scp = c.scale ? c.scale : c.zeros;
    a.shp = c.scale ? c.shift : (c.bias ? c.bias : c.zeros);
    a.hasSc = c.scale != nullptr;
    a.hasSh = (c.scale || c.bias) ? 1 : 0;
    a.N = c.N; a.K = c.K; a.Cn = c.Cn; a.HW = c.HW;
    a.rows = c.rows; a.nblkN = c.nblkN;
    a.act = c.act;
    a.steps = cdiv(c.K, 4);
    a.nch = cdiv(a.steps, kKC / 4);
    a.c0last = (c.K - 1) / 16 * 16;
    a.tilesPerImg = cdiv(c.HW, kTP);
    a.nTiles = c.N * a.tilesPerImg;
    a.nh = cdiv(c.nblkN, NB);
    const int grid = gemm1x1_grid(c.N, c.HW, c.nblkN);
    a.xcd = (grid % (8 * a.nh) == 0) ? 1 : 0;
    if (int rc = NB == 2 ? launch<2>(a, grid, s) : launch<1>(a, grid, s)) return rc;
    g_gemm1x1_launches.fetch_add(1, std::memory_order_relaxed);
    return SPRK_OK;
}

}  // namespace sprk
