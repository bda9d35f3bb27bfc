// Convolution kernels of libsprk.so (gfx950 / MI355X).
//
// All convolutions of the hot path are implicit GEMMs on the fp32 matrix cores
// (v_mfma_f32_16x16x4_f32: exact fp32, k-ordered fma chain) over NCHW tensors:
//
//   forward / backward-data :  Out[pixel][cout] += A[pixel][k] * Wt[k][cout],  k = (tap, cin)
//        A-fragment lane l -> pixel l&15, k l>>4 : 16 consecutive pixels of a row, straight
//        from an LDS copy of the input tile (with halo, zero-filled outside the image), so
//        the im2col matrix is never formed;  B-fragment from an LDS copy of the
//        pre-transposed weight rows.
//   backward-weight         :  dW[k][cout] += X[k][pixel] * G[pixel][cout]  (pixels are the
//        reduced dimension; per-block partials + a deterministic reduction pass).
//
// LDS plane strides are chosen per kernel so that the two k-values (fwd) / two pixels (bwd-w)
// held by one 32-lane ds_read group fall on disjoint banks (MI355X_MICROARCH.md §LDS).
// The "direct" kernels at the end are the plain per-output-element statement of the same
// maths: they serve strided backward-data (tiny detector layers) and as an on-device
// cross-check (SPRK_DT_NAIVE in sprk_conv_geom.dtype).
#include "common.h"
#include "conv16.h"
#include "gemm1x1.h"
#include "mask1x1.h"
#include "wgrad16.h"
#include "wgrad1x1.h"
#include "wgrad3x3.h"
#include "wino.h"
#include "wprep_dev.h"

#include <cstdlib>

#include "conv_dev.h"
#include "io_dev.h"


namespace {

// per-call switch: SPRK_DT_NAIVE in sprk_conv_geom.dtype routes the call to the plain (non-MFMA) kernels
inline bool naive_of(const sprk_conv_geom *g) { return (g->dtype & SPRK_DT_NAIVE) != 0; }

// ------------------------------------------------------------------------------------------
// weight transform:  W[Cout][Cin][KHW]  ->  Wt[nblk][rows][ldw]   (rows = k in chunked order)
//   mode 0 (forward):        GEMM-k channel = cin,  n = cout, tap as is
//   mode 1 (backward-data):  GEMM-k channel = cout, n = cin,  tap flipped
// Row order: chunks of CK k-channels; inside a chunk row = tap * cke + cl (cke = channels
// actually present in the chunk); every chunk occupies R4 = roundup(CK*KHW, 4) rows (16 for MT = 1).
// Each N-block (NT*16 output channels) is stored as its own [rows][ldw] slab with the LDS row
// stride ldw (zero padded), so a chunk of a slab is one contiguous run that LDS-DMA copies 1:1.
// The first 256 floats of the workspace are zeroed: the DMA source of out-of-image lanes.
// ------------------------------------------------------------------------------------------
constexpr int kZeroFloats = 256;
__device__ __attribute__((aligned(64))) float g_zero_block[kZeroFloats];  // zero-initialised; source of out-of-image DMA lanes

// nch channel planes from one source tensor: `base` points at channel 0 of image 0 of the staged
// channel range; imgStride / cs are the image / channel strides in floats; (Hs, Ws) the source plane
// size; up: source is half resolution, nearest-upsampled on load.
__device__ __forceinline__ void stage_planes(float *dst, const float *base, long imgStride, long cs, int nch, int N,
                                             int Hin, int Win, int Ws, int up, int vec, const float *zeros,
                                             const PlaneGeom &g, int n0, int iy0, int ixa, int lw, int lane) {
    const int imgElems = g.inRows * g.pitch;
    const int planeElems = g.NI * imgElems;
    const int per = vec ? 256 : 64;
    const int nGroups = (planeElems + per - 1) / per;
    // work items (group, channel) are dealt round-robin to the issuing waves: every wave walks all
    // groups but only every kIssuers-th channel, so the issue load is even whatever nGroups is
    const int nw = g.nw;
    const int gstart = g.deal ? 0 : lw, gstep = g.deal ? 1 : nw, cstep = g.deal ? nw : 1;
    for (int gi = gstart; gi < nGroups; gi += gstep) {
        const int e = vec ? gi * 256 + lane * 4 : gi * 64 + lane;
        const int il = fast_div(e, g.invImg);
        const int rem = e - il * imgElems;
        const int r = fast_div(rem, g.invPitch);
        const int j = rem - r * g.pitch;
        const int n = n0 + il, iy = iy0 + r, ix = ixa + j;
        const bool inb = e < planeElems;
        const bool ok = inb && n < N && (unsigned)iy < (unsigned)Hin && (unsigned)ix < (unsigned)Win;
        const int cl0 = g.deal ? (lw + nw - (gi % nw)) % nw : 0;
        const float *p = base + (long)n * imgStride + (up ? (long)(iy >> 1) * Ws + (ix >> 1) : (long)iy * Ws + ix) +
                         (long)cl0 * cs;
        long step = (long)cstep * cs;
        if (!ok) {  // lanes outside the image read the zero block
            p = zeros + lane * 4;
            step = 0;
        }
        float *d = dst + gi * per + cl0 * g.cplane;
        for (int cl = cl0; cl < nch; cl += cstep) {
            if (inb) {
                if (vec)
                    dma16(p, d);
                else
                    dma4(p, d);
            }
            p += step;
            d += cstep * g.cplane;
        }
    }
}

// Source of the (virtual) conv input: channel concat of x (optionally 2x nearest-upsampled on the
// fly) and x2, zero outside the image.
struct TileSrc {
    const float *x, *x2, *zeros;
    int N, C1, C2, Hin, Win, up1, H1, W1;
    int vec1, vec2;  // 16-byte DMA allowed for source 1 / source 2
};

// channels [c0, c0+cke) of the concatenated input
__device__ __forceinline__ void stage_input_dma(float *in_lds, const TileSrc &s, const PlaneGeom &g, int n0, int iy0,
                                                int ix0, int c0, int cke, int lw, int lane) {
    const int ixa = ix0 - g.colOff;
    const int n1 = max(0, min(c0 + cke, s.C1) - c0);  // channels taken from x
    if (n1 > 0) {
        const long cs1 = (long)s.H1 * s.W1;
        stage_planes(in_lds, s.x + (long)c0 * cs1, (long)s.C1 * cs1, cs1, n1, s.N, s.Hin, s.Win, s.W1, s.up1, s.vec1,
                     s.zeros, g, n0, iy0, ixa, lw, lane);
    }
    if (n1 < cke) {
        const long cs2 = (long)s.Hin * s.Win;
        const int cb = max(c0, s.C1) - s.C1;
        stage_planes(in_lds + n1 * g.cplane, s.x2 + (long)cb * cs2, (long)s.C2 * cs2, cs2, cke - n1, s.N, s.Hin, s.Win,
                     s.Win, 0, s.vec2, s.zeros, g, n0, iy0, ixa, lw, lane);
    }
}

// The K loop of one staged chunk.  Non-MFMA VALU instructions take issue time from the MFMA stream (about a
// quarter of an fp32 16x16x4 MFMA each), so a k-step is written to need few of them: all operand addresses
// are absolute LDS byte addresses; the RB row bases of this wave's MT pixel tiles take one add each (tiles
// of one row are 16 floats apart: immediates), the weight row one add (cout tiles: immediates), the k-row
// offset one add for its table address.  The operands of step kq+1 are fetched under the MFMAs of step kq.
//   abase[r]: address of this lane's pixel of row base r at channel 0, tap 0 of the stage
//   kaddr:    address of koff[lq] (byte offsets of k rows 4kq+lq);   baddr: address of w[lq][l15]
template <int MT, int NT, int RB>
__device__ __forceinline__ void chunk_mma(f32x4 (&acc)[MT][NT], const int (&abase)[RB], int kaddr, int baddr,
                                          int bstep, int nkq) {
    constexpr int MPR = MT / RB;
    float av[MT], bv[NT];
    {
        const int ko = *lds_i(kaddr);
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            lds_cfp ap = lds_f(abase[r] + ko);
#pragma unroll
            for (int j = 0; j < MPR; ++j) av[r * MPR + j] = ap[16 * j];
        }
        lds_cfp bp = lds_f(baddr);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = bp[16 * nt];
    }
    const int last = nkq - 1;
    for (int kq = 0; kq < nkq; ++kq) {
        const int kn = min(kq + 1, last);   // the last step re-reads itself (unused)
        const int ko = lds_i(kaddr)[kn * 4];
        float an[MT], bn[NT];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            lds_cfp ap = lds_f(abase[r] + ko);
#pragma unroll
            for (int j = 0; j < MPR; ++j) an[r * MPR + j] = ap[16 * j];
        }
        lds_cfp bp = lds_f(baddr + kn * bstep);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bn[nt] = bp[16 * nt];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) av[mt] = an[mt];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = bn[nt];
    }
}

// MT = 1, NT <= 3 (planes of a few pixels: the U-Net levels <= 16x16 and the detector's patch layers): one pixel tile per wave
// means 1..6 MFMAs per k-step, far less than the two LDS round trips (k-row offset -> operand) a step of chunk_mma
// exposes, and these launches are latency-bound (8..512 workgroups, each alone on its CU).  Here a wave walks the
// chunk in groups of U k-steps: the offsets of group g+2 and the operands of group g+1 are in flight under the MFMAs
// of group g (U = 4, or 2 with three cout tiles), and with one or two cout tiles the steps of a group alternate
// between two accumulator sets (half the dependent-MFMA chain).  nkq is a multiple of U (the plan rounds a chunk's
// rows to 16: zero weight rows).
template <int NT>
__device__ __forceinline__ void chunk_mma_small(f32x4 (&acc)[1][NT], int abase, int kaddr, int baddr, int bstep, int nkq) {
    static_assert(NT <= 3, "four or more cout tiles: chunk_mma hides the latencies under its MFMAs (measured: this form is slower)");
    constexpr int U = NT <= 2 ? 4 : 2;
    constexpr bool TWO = NT <= 2;
    const int ng = nkq / U, lastg = ng - 1;
    int ko[U];
    float av[U], bv[U][NT];
    f32x4 acc2[TWO ? NT : 1];
#pragma unroll
    for (int nt = 0; nt < (TWO ? NT : 1); ++nt) acc2[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < U; ++u) ko[u] = lds_i(kaddr)[u * 4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        av[u] = *lds_f(abase + ko[u]);
        lds_cfp bp = lds_f(baddr + u * bstep);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[u][nt] = bp[16 * nt];
    }
    {
        const int g1 = min(1, lastg);
#pragma unroll
        for (int u = 0; u < U; ++u) ko[u] = lds_i(kaddr)[(g1 * U + u) * 4];
    }
    for (int g = 0; g < ng; ++g) {
        const int gn = min(g + 1, lastg), gnn = min(g + 2, lastg);   // the last groups re-read themselves (unused)
        float an[U], bn[U][NT];
        int kn[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            an[u] = *lds_f(abase + ko[u]);
            lds_cfp bp = lds_f(baddr + (gn * U + u) * bstep);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bn[u][nt] = bp[16 * nt];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) kn[u] = lds_i(kaddr)[(gnn * U + u) * 4];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                if (TWO && (u & 1))
                    acc2[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u][nt], acc2[nt], 0, 0, 0);
                else
                    acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u][nt], acc[0][nt], 0, 0, 0);
            }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            av[u] = an[u];
            ko[u] = kn[u];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bv[u][nt] = bn[u][nt];
        }
    }
    if (TWO) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[0][nt] += acc2[nt];
    }
}

// RB: row bases per wave (1: the wave's MT pixel tiles lie in one tile row, ... MT: one base per tile).
// XTAB: inputs staged by buffer loads through the per-tile offset tables (the normal case); the other
// instantiation keeps the pointer-arithmetic staging for geometries the tables do not cover (rows that are
// not 16-byte aligned).  Two kernels instead of a run-time branch: the K-chunk loop is short on scalar
// registers, and every spilled scalar comes back through a v_readlane, i.e. a VALU instruction.
#ifdef SPRK_DIAG
__device__ long long sprk_diag_conv_clk[40];   // phase time stamps of workgroup 0 (wall_clock64: 10 ns units)
#define SPRK_DIAG_STAMP(i) do { if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) sprk_diag_conv_clk[i] = wall_clock64(); } while (0)
#else
#define SPRK_DIAG_STAMP(i)
#endif

template <int MT, int NT, int RB, bool XTAB>
__global__ __launch_bounds__(kBlock, 2) void conv_mfma_kernel(const ConvArgs a) {
    SPRK_DIAG_STAMP(0);
    // LDS: koff[2][R4] (full chunk | last chunk) | xtab1[nG1*64] xtab2[nG2*64] | stage 0: input[CK*cplane]
    //      weights[R4*ldw] | stage 1: ...
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int stageFloats = a.CK * a.cplane + a.R4 * a.ldw;
    int *koff_base = reinterpret_cast<int *>(smem);
    int *xtab1 = koff_base + 2 * a.R4;
    int *xtab2 = xtab1 + a.nG1 * 64;
    float *stage_base = smem + 2 * a.R4 + (a.nG1 + a.nG2) * 64;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    constexpr int TM = 64 * MT;
    constexpr int kRowUnit = (MT == 1 && NT <= 3) ? 16 : 4;   // a chunk's k rows are rounded to this (plan_fwd: R4)
    const int lgT = a.lgTC + a.lgTR;
    const int NI = TM >> lgT;
    // XCD-aware tile order: workgroups are dealt round-robin to the 8 XCDs (each with its own L2), so
    // give every XCD a contiguous run of tiles — vertically adjacent tiles share their halo rows in L2.
    // (bijective remap; only a speed matter, see cdna_hip_programming.md T1)
    int bid = blockIdx.x;
    if (a.xcdRemap) {
        const int nwg = gridDim.x, q = nwg >> 3, rr = nwg & 7, xcd = bid & 7;
        bid = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (bid >> 3);
    }
    const int tx = bid % a.tilesX;
    bid /= a.tilesX;
    const int ty = bid % a.tilesY;
    const int ig = bid / a.tilesY;
    const int nb = blockIdx.y;
    const int oy0 = ty << a.lgTR, ox0 = tx << a.lgTC, n0 = ig * NI;
    const int iy0 = oy0 * a.stride - a.padT, ix0 = ox0 * a.stride - a.padL;
    const int KHW = a.KH * a.KW, Cin = a.C1 + a.C2;
    const int TCm = (1 << a.lgTC) - 1, TRm = (1 << a.lgTR) - 1;
    const int lw = wave;

    int abase[RB];   // byte offset of this lane's pixel (row base r) inside a stage's input image
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        const int p = (wave * MT + r * (MT / RB)) * 16 + l15;
        const int il = p >> lgT, rr = (p >> a.lgTC) & TRm, c = p & TCm;
        abase[r] = ((il * a.inRows + rr * a.stride) * a.pitch + c * a.stride + a.colOff) * 4;
    }
    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    const PlaneGeom pg{NI, a.inRows, a.pitch, a.colOff, a.cplane, a.invImg, a.invPitch, a.deal, 4};
    if (XTAB) {
        const int ixa = ix0 - a.colOff;
        if (a.nG1)
            build_xtab(xtab1, a.nG1, a.vec1, a.up1, a.W1, (long)a.C1 * a.H1 * a.W1, a.N, a.Hin, a.Win, pg, n0, iy0, ixa,
                       tid, kBlock);
        if (a.nG2)
            build_xtab(xtab2, a.nG2, a.vec2, 0, a.Win, (long)a.C2 * a.Hin * a.Win, a.N, a.Hin, a.Win, pg, n0, iy0, ixa,
                       tid, kBlock);
    }
    const float *wslab = a.wT + (long)nb * a.rows * a.ldw;

    // issue the DMA of the chunk starting at channel c0 into stage `b`
    auto issue = [&](int c0, int b) {
        const int cke = min(a.CK, Cin - c0);
        const int kchunk = (cke * KHW + kRowUnit - 1) & ~(kRowUnit - 1);
        float *in_lds = stage_base + b * stageFloats;
        float *w_lds = in_lds + a.CK * a.cplane;
        const float *wsrc = wslab + (long)(c0 / a.CK) * a.R4 * a.ldw;
        const int total4 = (kchunk * a.ldw) >> 2;
        if (XTAB) {
            const int n1 = max(0, min(c0 + cke, a.C1) - c0);   // channels of this chunk taken from x
            if (n1 > 0) {
                const int cs1 = a.H1 * a.W1;
                stage_planes_buf<4>(in_lds, make_rsrc(a.x + ((long)n0 * a.C1 + c0) * cs1), cs1 * 4, n1, xtab1, a.nG1,
                                    a.vec1, a.cplane, lw, lane);
            }
            if (n1 < cke) {
                const int cs2 = a.Hin * a.Win;
                const int cb = max(c0, a.C1) - a.C1;
                stage_planes_buf<4>(in_lds + n1 * a.cplane, make_rsrc(a.x2 + ((long)n0 * a.C2 + cb) * cs2), cs2 * 4,
                                    cke - n1, xtab2, a.nG2, a.vec2, a.cplane, lw, lane);
            }
            const rsrc_t wr = make_rsrc(wsrc);
            const int wv = lane * 16, room = total4 - lane;   // lanes past the slab must not write (next stage)
            for (int gi = lw; gi * 64 < total4; gi += 4)
                if (gi * 64 < room) bdma16(wr, wv, gi * 1024, w_lds + gi * 256);
        } else {
            const TileSrc src{a.x, a.x2, a.zeros, a.N, a.C1, a.C2, a.Hin, a.Win, a.up1, a.H1, a.W1, a.vec1, a.vec2};
            stage_input_dma(in_lds, src, pg, n0, iy0, ix0, c0, cke, lw, lane);
            for (int gi = lw; gi * 64 < total4; gi += 4) {
                const int idx = gi * 64 + lane;
                if (idx < total4) dma16(wsrc + idx * 4, w_lds + gi * 256);
            }
        }
    };

    SPRK_DIAG_STAMP(1);
    __syncthreads();   // tables visible
    SPRK_DIAG_STAMP(2);
    issue(0, 0);
    SPRK_DIAG_STAMP(3);
    // k-row byte offsets (tap-major inside a chunk) for a full chunk and for the last, possibly shorter one; built
    // under the first chunk's DMA (the chunk loop's first barrier publishes them)
    const int ckeLast = Cin - ((Cin - 1) / a.CK) * a.CK;
    for (int idx = tid; idx < 2 * a.R4; idx += kBlock) {
        const int which = idx >= a.R4, k = idx - which * a.R4;
        const int cke = which ? ckeLast : a.CK;
        int v = 0;
        if (k < cke * KHW) {
            const int tap = k / cke, cl = k - tap * cke;
            const int ky = tap / a.KW, kx = tap - ky * a.KW;
            v = (cl * a.cplane + (ky * a.pitch + kx) * a.dil) * 4;
        }
        koff_base[idx] = v;
    }

    const int baddr0 = lds_addr(stage_base + a.CK * a.cplane + lq * a.ldw + l15);
    const int kaddr0 = lds_addr(koff_base + lq);
    const int abyte0 = lds_addr(stage_base);
    const int bstep = a.ldw * 16;
    int ci = 0;
    for (int c0 = 0; c0 < Cin; c0 += a.CK, ++ci) {
        // every wave's DMA of this chunk has landed (vmcnt(0)) and every wave is done reading the
        // other stage (previous chunk) once all have passed the barrier
        __syncthreads();
        if (c0 == 0) SPRK_DIAG_STAMP(4);
        if (ci < 8) SPRK_DIAG_STAMP(8 + 3 * ci);
        if (c0 + a.CK < Cin) issue(c0 + a.CK, (ci + 1) & 1);
        if (c0 == 0) SPRK_DIAG_STAMP(5);
        if (ci < 8) SPRK_DIAG_STAMP(9 + 3 * ci);
        const int cke = min(a.CK, Cin - c0);
        const int nkq = ((cke * KHW + kRowUnit - 1) & ~(kRowUnit - 1)) >> 2;
        const int soff = (ci & 1) * stageFloats * 4;
        int ab[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) ab[r] = abyte0 + soff + abase[r];
        if constexpr (MT == 1 && NT <= 3)
            chunk_mma_small<NT>(acc, ab[0], kaddr0 + (cke == a.CK ? 0 : a.R4 * 4), baddr0 + soff, bstep, nkq);
        else
            chunk_mma<MT, NT, RB>(acc, ab, kaddr0 + (cke == a.CK ? 0 : a.R4 * 4), baddr0 + soff, bstep, nkq);
        if (c0 == 0) SPRK_DIAG_STAMP(6);
        if (ci < 8) SPRK_DIAG_STAMP(10 + 3 * ci);
    }
    SPRK_DIAG_STAMP(7);

#include "conv_epilogue.inc"
}

// ------------------------------------------------------------------------------------------
// backward-weight MFMA kernel:  partial[group][k = c*KHW + tap][CoutP]
//   D[k-row][cout] += X[k-row][pixel] * G[pixel][cout] over the block's 64-pixel tiles; both
//   operands arrive by LDS-DMA, double buffered, so the next tile streams in under the MFMAs.
//   The G tile is stored [cout][64 pixels] with its 16 16-byte chunks XOR-swizzled by (cout & 15)
//   (applied on the DMA source address; the image itself is lane-linear): the 16 couts x 4 pixels one
//   B-operand read touches fall into 64 distinct words.
// ------------------------------------------------------------------------------------------
struct WgArgs {
    const float *x, *x2, *gy, *zeros;
    float *partial;
    int N, C1, C2, Hin, Win, up1, H1, W1;
    int Cout, CoutP, Hout, Wout;
    int KH, KW, stride, dil, padT, padL;
    int lgTC, lgTR;          // 64-pixel tile
    int tilesX, tilesY, nTiles, tilesPerGroup;
    int CKW;                 // input channels per blockIdx.y
    int ioffN;               // ints reserved for the k-row offset table
    int inRows, inCols, pitch, cplane, colOff;
    int xrow, g4, vec1, vec2, deal;
    int xtab;                // buffer-load staging of the row tiles (G, and x for 1x1)
    int nG1, nG2;            // MODE 2: 256-float groups per staged x plane (source 1 / 2): table staging
    float invImg, invPitch;
    int diag;                // timing experiments only (SPRK_WG_DIAG): 1 = stage the first tile of a group only
};

// one 64-pixel tile: 16 k-steps of MFMAs on NIT k-tiles x NT cout-tiles, software pipelined by hand: the LDS
// operands of step ks+1 are fetched into a second register set before the MFMAs of step ks are issued.
// The reduced dimension of this GEMM is the pixel, so which pixel feeds which (k-step, k-lane) slot is free as
// long as both operands agree:  k-step 4j+s, k-lane lq  <-  pixel 16j + 4lq + s.  Then the four G values a lane
// needs for steps 4j..4j+3 are one 16-byte chunk of its cout row: one ds_read_b128 per cout tile and 4 steps
// instead of four ds_read_b32, and the 8 lanes a b128 read serves per cycle hit 8 different swizzled chunks (no
// bank conflicts; the per-step b32 form was 2-way conflicted).
// Operand addresses are absolute LDS byte addresses and cost as few VALU instructions as possible (each one
// takes issue time from the MFMA stream):
//   MODE 2 (stride-1 tiles, rows of >= 4 pixels): A operand of k-tile t at  ab[t] + 4*(16j+s)  — an immediate —
//          where ab[t] is re-based per 16-pixel group from rowd (byte delta of a tile row against a straight run);
//   MODE 1 (1x1: the x tile is staged as swizzled 64-pixel rows like the G tile);
//   MODE 0 (any stride): pixel offsets from the pixoff table, one add per k-tile and step.
//   B operand: chunk ((4j+lq) ^ gsw) of the swizzled G row of this lane's cout, + nt * 4096 bytes.
template <int NIT, int IT, int NT, int MODE, bool DB>
__device__ __forceinline__ void wgrad_tile(f32x4 (&acc)[IT][NT], int xaddr, const int (&ioffb)[IT], int gaddr,
                                           lds_cip pixoffp, lds_cip rowdp, int lgTC, int gsw, int lq) {
    typedef const __attribute__((address_space(3))) f32x4 *lds_c4p;
    float a0[NIT], a1[NIT];
    f32x4 b0[NT], b1[DB ? NT : 1];   // DB: a second G register set (workgroups with one wave per SIMD)
    int ab[NIT];
    const int lsw = lq ^ gsw;
    auto loadB = [&](int j, f32x4 (&bv)[NT]) {
        const int q = ((4 * j) ^ lsw) << 4;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = *(lds_c4p)(__SIZE_TYPE__)(unsigned)(gaddr + q + nt * 4096);
    };
    auto baseA = [&](int j) {   // MODE 2: row base of this lane's 4-pixel chunk of group j
        if (MODE == 2 && (j == 0 || lgTC < 6)) {
            const int d = rowdp[(16 * j + 4 * lq) >> lgTC];
#pragma unroll
            for (int t = 0; t < NIT; ++t) ab[t] = xaddr + ioffb[t] + d;
        }
    };
    auto loadA = [&](int j, int sx, float (&av)[NIT]) {
        if (MODE == 2) {
#pragma unroll
            for (int t = 0; t < NIT; ++t) av[t] = lds_f(ab[t])[16 * j + sx];
        } else {
            const int xo = MODE == 1 ? ((((4 * j) ^ lsw) << 4) + 4 * sx) : pixoffp[16 * j + 4 * lq + sx];
#pragma unroll
            for (int t = 0; t < NIT; ++t) av[t] = *lds_f(xaddr + ioffb[t] + xo);
        }
    };
    auto mma = [&](const float (&av)[NIT], const f32x4 (&bv)[NT], int sx) {
#pragma unroll
        for (int t = 0; t < NIT; ++t)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[t][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], bv[nt][sx], acc[t][nt], 0, 0, 0);
    };
    loadB(0, b0);
    baseA(0);
    loadA(0, 0, a0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if constexpr (DB) {
            if (j + 1 < 4) {
                if (j & 1) loadB(j + 1, b0); else loadB(j + 1, b1);
            }
        }
#pragma unroll
        for (int sx = 0; sx < 4; ++sx) {
            const int ks = 4 * j + sx;
            if (ks + 1 < 16) {            // A operands of the next step
                const int jn = (ks + 1) >> 2, sn = (ks + 1) & 3;
                if (sn == 0) baseA(jn);
                if (ks & 1) loadA(jn, sn, a0); else loadA(jn, sn, a1);
            }
            if constexpr (DB) {
                if (ks & 1) {
                    if (j & 1) mma(a1, b1, sx); else mma(a1, b0, sx);
                } else {
                    if (j & 1) mma(a0, b1, sx); else mma(a0, b0, sx);
                }
            } else {
                if (ks & 1) mma(a1, b0, sx); else mma(a0, b0, sx);
            }
        }
        // eight-wave workgroups: the G chunk of the next four steps goes into the same registers (a second set
        // does not fit next to 84 accumulators at two waves per SIMD; the SIMD partner covers the wait)
        if constexpr (!DB) {
            if (j + 1 < 4) loadB(j + 1, b0);
        }
    }
}

// (A first version of MODE 2's table staging of the x planes kept the per-group offsets in a small register
// array and was slower than pointer arithmetic: the array cost more VALU — initialisation, guarded reads,
// indexed access — than it saved.  Written as plain loops that read each table entry where it is used, it wins.)

// WJ = 2: eight waves (two per SIMD); wave (wi, wj) owns k-tiles wi, wi+4, ... x the wj-th half of the
// NT cout tiles, so that one wave's LDS latency and barrier skew are covered by its SIMD partner.
// MODE: operand addressing of wgrad_tile.  1 (1x1 convolutions: x staged as rows) and 2 also mean that the row
// tiles are staged by buffer loads (16-byte aligned rows, 32-bit offsets: the host checks); 0 is the general
// form with pointer-arithmetic staging.  Separate instantiations rather than run-time branches: spilled scalar
// registers come back as v_readlane, i.e. VALU instructions in the tile loop.
template <int IT, int NT, int WJ, int MODE>
__global__ __launch_bounds__(256 * WJ) void conv_wgrad_mfma_kernel(const WgArgs a) {
    constexpr bool XROW = MODE == 1;
    constexpr bool FAST = MODE != 0;
    constexpr int NTW = NT / WJ;          // cout tiles per wave
    constexpr int kWgThreads = 256 * WJ;
    constexpr int kWgWaves = 4 * WJ;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // LDS: ioff[ioffN] | pixoff[64] | rowd[16] | xp[(nG1+nG2)*64] xv[(nG1+nG2)*64] (MODE 2) | 2 x { x, g }
    int *ioff = reinterpret_cast<int *>(smem);
    int *pixoff = ioff + a.ioffN;
    int *rowd = pixoff + 64;
    int *xp = rowd + 16, *xv = xp + (a.nG1 + a.nG2) * 64;
    float *stage_base = smem + a.ioffN + 64 + 16 + 2 * (a.nG1 + a.nG2) * 64;
    const int stageFloats = a.CKW * a.cplane + NT * 16 * 64;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    const int lgT = a.lgTC + a.lgTR;
    const int NI = 64 >> lgT;
    const int TCm = (1 << a.lgTC) - 1, TRm = (1 << a.lgTR) - 1;
    const int KHW = a.KH * a.KW, Cin = a.C1 + a.C2;
    const int c0 = blockIdx.y * a.CKW;
    const int cke = min(a.CKW, Cin - c0);
    const int kvalid = cke * KHW;
    const int nIT = (kvalid + 15) >> 4;
    const int co0 = blockIdx.z * (NT * 16);
    const long planeO = (long)a.Hout * a.Wout;
    const long planeI = (long)a.Hin * a.Win;
    const int wi = wave & 3, wj = wave >> 2;
    const int lw = wave;

    for (int k = tid; k < nIT * 16; k += kWgThreads) {
        int v = 0;
        if (k < kvalid) {
            const int tap = k / cke, cl = k - tap * cke;
            const int ky = tap / a.KW, kx = tap - ky * a.KW;
            v = (cl * a.cplane + (ky * a.pitch + kx) * a.dil) * 4;   // bytes
        }
        ioff[k] = v;
    }
    if (tid < 64) {
        const int il = tid >> lgT, r = (tid >> a.lgTC) & TRm, c = tid & TCm;
        const int off = (il * a.inRows + r * a.stride) * a.pitch + c * a.stride + a.colOff;
        pixoff[tid] = off * 4;   // bytes
        // byte delta of the tile row holding pixel `tid` against a straight 4-bytes-per-pixel run from pixel 0
        if (c == 0) rowd[tid >> a.lgTC] = (off - tid) * 4;
    }
    const PlaneGeom pg{NI, a.inRows, a.pitch, a.colOff, a.cplane, a.invImg, a.invPitch, a.deal, kWgWaves};
    if (MODE == 2) {
        // x planes by buffer loads: per lane and 256-float group of a plane, the packed in-tile coordinates
        // (-1: past the plane) and the byte offset against the tile origin; sources 1 and 2 back to back
        const int imgElems = a.inRows * a.pitch, planeElems = NI * imgElems;
        for (int idx = tid; idx < (a.nG1 + a.nG2) * 64; idx += kWgThreads) {
            const int second = idx >= a.nG1 * 64;
            const int gi = (idx - (second ? a.nG1 * 64 : 0)) >> 6, ln = idx & 63;
            const int e = gi * 256 + ln * 4;
            const int il = fast_div(e, a.invImg);
            const int rem = e - il * imgElems;
            const int r = fast_div(rem, a.invPitch);
            const int j = rem - r * a.pitch;
            const long imgStride = second ? (long)a.C2 * planeI : (long)a.C1 * planeI;
            xp[idx] = e < planeElems ? (il << 20) | (r << 10) | j : -1;
            xv[idx] = (int)((il * imgStride + (long)r * a.Win + j) * 4);
        }
    }
    // G rows (and, for 1x1, x rows): lane -> (row within the item's 4 rows, swizzled 16-byte chunk) -> pixel
    const int rowl = lane >> 4;
    int gpk, gvo, xvo;
    {
        const int rsw = ((lw & 3) << 2) | rowl;             // (row & 15) of every item this wave stages
        const int p = ((lane & 15) ^ rsw) << 2;
        const int il = p >> lgT, r = (p >> a.lgTC) & TRm, c = p & TCm;
        gpk = (il << 20) | (r << 10) | c;
        gvo = (int)((((long)il * a.Cout + rowl) * planeO + (long)r * a.Wout + c) * 4);
        xvo = (int)((((long)il * a.C1 + rowl) * planeI + (long)r * a.Win + c) * 4);
    }
    const TileSrc src{a.x, a.x2, a.zeros, a.N, a.C1, a.C2, a.Hin, a.Win, a.up1, a.H1, a.W1, a.vec1, a.vec2};

    // rows of 64 pixels, 16-byte chunks XOR-swizzled by (row & 15): LDS chunk (row, qs) <- pixels
    // 4q..4q+3, q = qs ^ (row & 15).  base: tensor [N][C][H*W]; row r is channel ch0 + r.
    auto stage_rows16 = [&](float *dst, const float *base, int C, long plane, int W, int H, int ch0, int nrows,
                            int chlim, int n0, int oy0, int ox0) {
        for (int gi = lw; gi * 4 < nrows; gi += kWgWaves) {
            const int idx = gi * 64 + lane;
            const int row = idx >> 4, qs = idx & 15;
            const int p = (qs ^ (row & 15)) << 2;
            const int il = p >> lgT, r = (p >> a.lgTC) & TRm, c = p & TCm;
            const int n = n0 + il, oy = oy0 + r, ox = ox0 + c, ch = ch0 + row;
            const float *s = a.zeros + lane * 4;
            if (ch < chlim && n < a.N && oy < H && ox < W) s = base + ((long)n * C + ch) * plane + (long)oy * W + ox;
            if (row < nrows) dma16(s, dst + gi * 256);
        }
    };
    // the same through buffer loads: the pixel part of the address is this lane's fixed offset against the
    // tile origin (vo), made invalid (zero fill) per tile; the channel part is wave-uniform
    auto stage_rows_buf = [&](float *dst, const float *base, int C, long plane, int W, int ch0, int nrows, int chlim,
                              int n0, int oy0, int ox0, int vo, bool inside) {
        const rsrc_t r = make_rsrc(base + ((long)n0 * C + ch0) * plane + (long)oy0 * W + ox0);
        const int v = inside ? vo : kXZero;
        const int rowBytes4 = (int)(plane * 16);
        for (int gi = lw; gi * 4 < nrows; gi += kWgWaves) {
            int vv = v;
            if (ch0 + gi * 4 + 3 >= chlim) vv = (ch0 + gi * 4 + rowl < chlim) ? v : kXZero;   // ragged last cout block
            if (gi * 4 + rowl < nrows) bdma16(r, vv, gi * rowBytes4, dst + gi * 256);
        }
    };
    auto issue = [&](int tile, int b) {
        if (a.diag && tile != (int)blockIdx.x * a.tilesPerGroup) return;
        int t = tile;
        const int tx = t % a.tilesX;
        t /= a.tilesX;
        const int ty = t % a.tilesY;
        const int ig = t / a.tilesY;
        const int oy0 = ty << a.lgTR, ox0 = tx << a.lgTC, n0 = ig * NI;
        float *x_lds = stage_base + b * stageFloats;
        float *g_lds = x_lds + a.CKW * a.cplane;
        bool inside = false;
        if (FAST) {
            const int r = (gpk >> 10) & 1023, c = gpk & 1023, il = gpk >> 20;
            inside = n0 + il < a.N && oy0 + r < a.Hout && ox0 + c < a.Wout;
        }
        if (XROW) {
            stage_rows_buf(x_lds, a.x, a.C1, planeI, a.Win, c0, cke, Cin, n0, oy0, ox0, xvo, inside);
        } else {
            if (MODE == 2) {
                // table + buffer-load staging: one validity pass per 256-float group and tile, then a
                // wave-uniform channel offset per DMA; lanes outside the image read zeros by range check
                const int iy0 = oy0 - a.padT, ixa = ox0 - a.padL - a.colOff;
                const int n1 = max(0, min(c0 + cke, a.C1) - c0);   // channels of this chunk taken from x
                auto planes = [&](const float *base, int nch, int nG, int tb, float *dstp) {
                    const rsrc_t r = make_rsrc(base + (long)iy0 * a.Win + ixa);
                    for (int gi = 0; gi < nG; ++gi) {
                        const int pk = xp[tb + gi * 64 + lane], vo = xv[tb + gi * 64 + lane];
                        const int rr = (pk >> 10) & 1023, jj = pk & 1023, il = pk >> 20;
                        const bool ok = n0 + il < a.N && (unsigned)(iy0 + rr) < (unsigned)a.Hin &&
                                        (unsigned)(ixa + jj) < (unsigned)a.Win;
                        const int o = ok ? vo : kXZero;
                        const int cl0 = (lw + kWgWaves - (gi % kWgWaves)) % kWgWaves;
                        float *d = dstp + gi * 256 + cl0 * a.cplane;
                        int soff = cl0 * (int)planeI * 4;
                        if (pk >= 0) {
                            for (int cl = cl0; cl < nch; cl += kWgWaves) {
                                bdma16(r, o, soff, d);
                                soff += kWgWaves * (int)planeI * 4;
                                d += kWgWaves * a.cplane;
                            }
                        }
                    }
                };
                if (n1 > 0) planes(a.x + ((long)n0 * a.C1 + c0) * planeI, n1, a.nG1, 0, x_lds);
                if (n1 < cke)
                    planes(a.x2 + ((long)n0 * a.C2 + (max(c0, a.C1) - a.C1)) * planeI, cke - n1, a.nG2, a.nG1 * 64,
                           x_lds + n1 * a.cplane);
            } else {
                stage_input_dma(x_lds, src, pg, n0, oy0 * a.stride - a.padT, ox0 * a.stride - a.padL, c0, cke, lw, lane);
            }
        }
        if (FAST) {
            stage_rows_buf(g_lds, a.gy, a.Cout, planeO, a.Wout, co0, NT * 16, a.Cout, n0, oy0, ox0, gvo, inside);
        } else if (a.g4) {
            stage_rows16(g_lds, a.gy, a.Cout, planeO, a.Wout, a.Hout, co0, NT * 16, a.Cout, n0, oy0, ox0);
        } else {
            for (int col = lw; col < NT * 16; col += kWgWaves) {
                const int p = (((lane >> 2) ^ (col & 15)) << 2) | (lane & 3);
                const int il = p >> lgT, r = (p >> a.lgTC) & TRm, c = p & TCm;
                const int n = n0 + il, oy = oy0 + r, ox = ox0 + c, co = co0 + col;
                const float *s = a.zeros + lane;
                if (co < a.Cout && n < a.N && oy < a.Hout && ox < a.Wout)
                    s = a.gy + ((long)n * a.Cout + co) * planeO + (long)oy * a.Wout + ox;
                dma4(s, g_lds + col * 64);
            }
        }
    };

    const int t_begin = blockIdx.x * a.tilesPerGroup;
    const int t_end = min(a.nTiles, t_begin + a.tilesPerGroup);
    __syncthreads();  // tables visible
    if (t_begin < t_end) issue(t_begin, 0);
    int ioffb[IT];   // byte offset of this lane's k row (k-tile t) inside a stage's x image (+ its pixel quad)
#pragma unroll
    for (int t = 0; t < IT; ++t) {
        const int it = wi + 4 * t;
        ioffb[t] = (it < nIT ? ioff[it * 16 + l15] : 0) + (MODE == 2 ? lq * 16 : 0);
    }
    f32x4 acc[IT][NTW];
#pragma unroll
    for (int t = 0; t < IT; ++t)
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) acc[t][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int gsw = l15;   // rows are multiples of 16 apart per cout tile: row & 15 == l15
    const int myIT = nIT > wi ? (nIT - wi + 3) >> 2 : 0;  // k-tiles owned by this wave (uniform)
    const int xaddr0 = lds_addr(stage_base);
    const int gaddr0 = lds_addr(stage_base + a.CKW * a.cplane + wj * (NTW * 16 * 64) + l15 * 64);
    const lds_cip pixoffp = lds_i(lds_addr(pixoff)), rowdp = lds_i(lds_addr(rowd));

    // The tile loop is written once per k-tile count of this wave (a wave-uniform choice made once): with the
    // choice inside the loop the three variants get different accumulator registers and the compiler copies
    // all 84 of them at every join — 36-72 v_mov per tile, each costing MFMA issue time.
    auto tiles = [&](auto body) {
        int bsel = 0;
        for (int tile = t_begin; tile < t_end; ++tile, bsel ^= 1) {
            __syncthreads();  // this tile landed everywhere; previous tile fully consumed
            if (tile + 1 < t_end) issue(tile + 1, bsel ^ 1);
            const int soff = bsel * stageFloats * 4;
            body(xaddr0 + soff, gaddr0 + soff);
        }
    };
    if (myIT >= IT) {
        tiles([&](int xaddr, int gaddr) {
            wgrad_tile<IT, IT, NTW, MODE, WJ == 1>(acc, xaddr, ioffb, gaddr, pixoffp, rowdp, a.lgTC, gsw, lq);
        });
    } else if (IT > 1 && myIT == IT - 1) {
        tiles([&](int xaddr, int gaddr) {
            wgrad_tile<(IT > 1 ? IT - 1 : 1), IT, NTW, MODE, WJ == 1>(acc, xaddr, ioffb, gaddr, pixoffp, rowdp, a.lgTC, gsw,
                                                                      lq);
        });
    } else {
        // short tail chunk: predicate per k-tile (rare: last channel chunk of a layer); same pixel order.
        // (waves without k-tiles still take part in the staging and the barriers)
        tiles([&](int xaddr, int gaddr) {
            if (myIT <= 0) return;
#pragma unroll 1
            for (int ks = 0; ks < 16; ++ks) {
                const int j = ks >> 2, sx = ks & 3;
                const int q = ((4 * j) ^ lq ^ gsw) << 4;
                const int p = 16 * j + 4 * lq + sx;
                const int xo = MODE == 1 ? q + 4 * sx : MODE == 2 ? (16 * j + sx) * 4 + rowdp[p >> a.lgTC] : pixoffp[p];
                float bv[NTW];
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt) bv[nt] = lds_f(gaddr + q + 4 * sx)[nt * 1024];
#pragma unroll
                for (int t = 0; t < IT; ++t) {
                    if (t < myIT) {
                        const float av = *lds_f(xaddr + ioffb[t] + xo);
#pragma unroll
                        for (int nt = 0; nt < NTW; ++nt)
                            acc[t][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[nt], acc[t][nt], 0, 0, 0);
                    }
                }
            }
        });
    }
    // partial slab of this group: rows = global k (c*KHW + tap), cols = cout (64-byte runs per store)
    float *dst = a.partial + (long)blockIdx.x * Cin * KHW * a.CoutP;
#pragma unroll
    for (int t = 0; t < IT; ++t) {
        const int it = wi + 4 * t;
        if (it >= nIT) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = it * 16 + lq * 4 + j;
            if (k >= kvalid) continue;
            const int tap = k / cke, cl = k - tap * cke;
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) {
                const int co = co0 + (wj * NTW + nt) * 16 + l15;
                if (co < a.CoutP) dst[((long)(c0 + cl) * KHW + tap) * a.CoutP + co] = acc[t][nt][j];
            }
        }
    }
}


// ------------------------------------------------------------------------------------------
// direct kernels (plain statement of the maths)
// ------------------------------------------------------------------------------------------
struct DirectArgs {
    const float *x, *x2, *w, *gy;
    float *y;
    sprk_conv_geom g;
    sprk_conv_epilogue ep;
};

__device__ __forceinline__ float fetch_in(const DirectArgs &a, int n, int c, int iy, int ix) {
    const sprk_conv_geom &g = a.g;
    if ((unsigned)iy >= (unsigned)g.Hin || (unsigned)ix >= (unsigned)g.Win) return 0.f;
    if (c < g.C1) {
        if (g.up1) return a.x[(((long)n * g.C1 + c) * (g.Hin >> 1) + (iy >> 1)) * (g.Win >> 1) + (ix >> 1)];
        return a.x[(((long)n * g.C1 + c) * g.Hin + iy) * g.Win + ix];
    }
    return a.x2[(((long)n * g.C2 + (c - g.C1)) * g.Hin + iy) * g.Win + ix];
}

__global__ void conv_fwd_direct_kernel(const DirectArgs a) {
    const sprk_conv_geom &g = a.g;
    const int Cin = g.C1 + g.C2;
    const long total = (long)g.N * g.Cout * g.Hout * g.Wout;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        long t = e;
        const int ox = (int)(t % g.Wout); t /= g.Wout;
        const int oy = (int)(t % g.Hout); t /= g.Hout;
        const int co = (int)(t % g.Cout);
        const int n = (int)(t / g.Cout);
        float s = 0.f;
        for (int c = 0; c < Cin; ++c)
            for (int ky = 0; ky < g.KH; ++ky)
                for (int kx = 0; kx < g.KW; ++kx)
                    s += fetch_in(a, n, c, oy * g.stride - g.pad_top + ky * g.dil, ox * g.stride - g.pad_left + kx * g.dil) *
                         a.w[(((long)co * Cin + c) * g.KH + ky) * g.KW + kx];
        if (a.ep.res) s += a.ep.res[(((long)n * g.Cout + co) * a.ep.res_h + oy + a.ep.res_off) * a.ep.res_w + ox + a.ep.res_off];
        if (a.ep.scale)
            s = s * a.ep.scale[co] + a.ep.shift[co];
        else if (a.ep.bias)
            s += a.ep.bias[co];
        const float v = apply_act(s, a.ep.act);
        if (a.ep.up2) {
            float *q = a.y + (((long)n * g.Cout + co) * (2 * g.Hout) + 2 * oy) * (2L * g.Wout) + 2 * ox;
            q[0] = v;
            q[1] = v;
            q[2L * g.Wout] = v;
            q[2L * g.Wout + 1] = v;
        } else {
            a.y[e] = v;
        }
    }
}

// y here is gin [N,Cin,Hin,Win]
__global__ void conv_bwd_data_direct_kernel(const DirectArgs a) {
    const sprk_conv_geom &g = a.g;
    const int Cin = g.C1 + g.C2;
    const long total = (long)g.N * Cin * g.Hin * g.Win;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        long t = e;
        const int ix = (int)(t % g.Win); t /= g.Win;
        const int iy = (int)(t % g.Hin); t /= g.Hin;
        const int c = (int)(t % Cin);
        const int n = (int)(t / Cin);
        float s = 0.f;
        for (int ky = 0; ky < g.KH; ++ky) {
            const int ny = iy + g.pad_top - ky * g.dil;
            if (ny < 0 || ny % g.stride) continue;
            const int oy = ny / g.stride;
            if (oy >= g.Hout) continue;
            for (int kx = 0; kx < g.KW; ++kx) {
                const int nx = ix + g.pad_left - kx * g.dil;
                if (nx < 0 || nx % g.stride) continue;
                const int ox = nx / g.stride;
                if (ox >= g.Wout) continue;
                for (int co = 0; co < g.Cout; ++co)
                    s += a.gy[(((long)n * g.Cout + co) * g.Hout + oy) * g.Wout + ox] *
                         a.w[(((long)co * Cin + c) * g.KH + ky) * g.KW + kx];
            }
        }
        a.y[e] = s;
    }
}

// Strided backward-data of a layer whose weights fit LDS (the detector's 7x7 stride-2 stem): the sums of
// conv_bwd_data_direct_kernel — the same loops in the same order, one chain s += gy * w from 0 per element, so the
// results are equal bit for bit — with both operands read from LDS instead of global memory.  A workgroup owns a
// kStemTW x kStemTH tile of input pixels of one image; it stages the weights [Cout][Cin][KH][KW] and the window of gy
// its pixels can reach ([Cout][wr][wc], zero outside the image: never used) once, then each thread walks the input
// channels of its pixel.
constexpr int kStemTW = 32, kStemTH = 8;
constexpr size_t kStemLdsLimit = 64 * 1024;   // no LDS opt-in

struct StemPlan {
    int wr, wc, tilesX, tilesY;
    size_t ldsBytes;
};

// false: the weights and a tile's gradient window do not fit LDS (conv_bwd_data_direct_kernel runs)
bool plan_stem_bwd(const sprk_conv_geom *g, StemPlan *p) {
    if (g->stride < 1 || g->dil < 1) return false;
    const long Cin = g->C1 + g->C2;
    p->wr = (kStemTH - 1 + (g->KH - 1) * g->dil) / g->stride + 1;
    p->wc = (kStemTW - 1 + (g->KW - 1) * g->dil) / g->stride + 1;
    p->tilesX = sprk::cdiv(g->Win, kStemTW);
    p->tilesY = sprk::cdiv(g->Hin, kStemTH);
    const long floats = (long)g->Cout * Cin * g->KH * g->KW + (long)g->Cout * p->wr * p->wc;
    p->ldsBytes = (size_t)floats * sizeof(float);
    return p->ldsBytes <= kStemLdsLimit && (long)g->N * p->tilesX * p->tilesY < (1L << 31);
}

__global__ __launch_bounds__(kStemTW * kStemTH) void conv_bwd_data_stem_kernel(const DirectArgs a, int wr, int wc,
                                                                               int tilesX, int tilesY) {
    extern __shared__ __attribute__((aligned(16))) float stem_lds[];
    const sprk_conv_geom &g = a.g;
    const int Cin = g.C1 + g.C2, KHW = g.KH * g.KW;
    const int nW = g.Cout * Cin * KHW;
    float *wl = stem_lds, *gl = stem_lds + nW;
    int bid = blockIdx.x;
    const int tx = bid % tilesX; bid /= tilesX;
    const int ty = bid % tilesY;
    const int n = bid / tilesY;
    const int iy0 = ty * kStemTH, ix0 = tx * kStemTW;
    // first output row / column any pixel of the tile reaches: ceil((i0 + pad - (K - 1) * dil) / stride), at least 0
    const int ylo = iy0 + g.pad_top - (g.KH - 1) * g.dil, xlo = ix0 + g.pad_left - (g.KW - 1) * g.dil;
    const int oyLo = ylo <= 0 ? 0 : (ylo + g.stride - 1) / g.stride;
    const int oxLo = xlo <= 0 ? 0 : (xlo + g.stride - 1) / g.stride;
    const int tid = threadIdx.x;
    for (int i = tid; i < nW; i += kStemTW * kStemTH) wl[i] = a.w[i];
    const int win = wr * wc;
    for (int i = tid; i < g.Cout * win; i += kStemTW * kStemTH) {
        const int co = i / win, rem = i - co * win;
        const int r = rem / wc, oy = oyLo + r, ox = oxLo + rem - r * wc;
        gl[i] = (oy < g.Hout && ox < g.Wout) ? a.gy[(((long)n * g.Cout + co) * g.Hout + oy) * g.Wout + ox] : 0.f;
    }
    __syncthreads();
    const int iy = iy0 + tid / kStemTW, ix = ix0 + tid % kStemTW;
    if (iy >= g.Hin || ix >= g.Win) return;
    for (int c = 0; c < Cin; ++c) {
        float s = 0.f;
        for (int ky = 0; ky < g.KH; ++ky) {
            const int ny = iy + g.pad_top - ky * g.dil;
            if (ny < 0 || ny % g.stride) continue;
            const int oy = ny / g.stride;
            if (oy >= g.Hout) continue;
            for (int kx = 0; kx < g.KW; ++kx) {
                const int nx = ix + g.pad_left - kx * g.dil;
                if (nx < 0 || nx % g.stride) continue;
                const int ox = nx / g.stride;
                if (ox >= g.Wout) continue;
                const float *gp = gl + (oy - oyLo) * wc + (ox - oxLo);
                const float *wp = wl + (c * g.KH + ky) * g.KW + kx;
                for (int co = 0; co < g.Cout; ++co) s += gp[co * win] * wp[co * Cin * KHW];
            }
        }
        a.y[(((long)n * Cin + c) * g.Hin + iy) * g.Win + ix] = s;
    }
}

// one block per (co, c); y here is gw
__global__ __launch_bounds__(256) void conv_bwd_weight_direct_kernel(const DirectArgs a) {
    const sprk_conv_geom &g = a.g;
    const int Cin = g.C1 + g.C2;
    const int co = blockIdx.x / Cin, c = blockIdx.x % Cin;
    __shared__ float red[256];
    const long npix = (long)g.N * g.Hout * g.Wout;
    for (int ky = 0; ky < g.KH; ++ky)
        for (int kx = 0; kx < g.KW; ++kx) {
            float s = 0.f;
            for (long p = threadIdx.x; p < npix; p += 256) {
                long t = p;
                const int ox = (int)(t % g.Wout); t /= g.Wout;
                const int oy = (int)(t % g.Hout);
                const int n = (int)(t / g.Hout);
                s += fetch_in(a, n, c, oy * g.stride - g.pad_top + ky * g.dil, ox * g.stride - g.pad_left + kx * g.dil) *
                     a.gy[(((long)n * g.Cout + co) * g.Hout + oy) * g.Wout + ox];
            }
            red[threadIdx.x] = s;
            __syncthreads();
            for (int w = 128; w > 0; w >>= 1) {
                if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
                __syncthreads();
            }
            if (threadIdx.x == 0) a.y[(((long)co * Cin + c) * g.KH + ky) * g.KW + kx] = red[0];
            __syncthreads();
        }
}

// ------------------------------------------------------------------------------------------
// activation backward (+ bias gradient) and concat/upsample gradient split
// ------------------------------------------------------------------------------------------
// grid (C, nsplit): block (c, s) walks images n = s, s+nsplit, ... of channel c.
// up2: g and y are the 2x upsampled tensors [N,C,2H,2W] written by a conv with the fused upsample
// epilogue; the incoming gradient is first summed over each 2x2 block (backward of nn.Upsample).
// gstride: elements between consecutive images of g (a channel slice of a wider tensor: the backward-data output of
// a concat layer is handed on as views, not copied); y and gpre are dense.
// TG / TY / TO: element types of g, y and gpre (fp32 or the 16-bit storage type, io_dev.h); arithmetic and the bias
// sums are fp32.
template <typename TG, typename TY, typename TO>
__global__ __launch_bounds__(256) void act_bwd_kernel(const TG *g, const TY *__restrict__ y, TO *gpre,
                                                      float *__restrict__ partial, int act, int N, int C, int HW,
                                                      int W, int up2, int nsplit, long gstride) {
    const int c = blockIdx.x, s = blockIdx.y;
    float sum = 0.f;
    const bool al16 = (((uintptr_t)g | (uintptr_t)y | (uintptr_t)gpre) & 15) == 0 && (gstride & 3) == 0;
    const bool v4 = !up2 && (HW & 3) == 0 && al16;
    const bool v2u = up2 && (W & 1) == 0 && al16;
    for (int n = s; n < N; n += nsplit) {
        const long base = ((long)n * C + c) * HW;
        const long gbase = (long)n * gstride + (long)c * (up2 ? 4L * HW : HW);     // first element of g's plane
        if (v4) {  // four elements per lane
            for (int i = threadIdx.x * 4; i < HW; i += 1024) {
                float4 v = IO<TG>::ld4(g + gbase + i);
                if (act != SPRK_ACT_NONE) {
                    const float4 yv = IO<TY>::ld4(y + base + i);
                    const bool lk = act == SPRK_ACT_LEAKY;
                    v.x = yv.x > 0.f ? v.x : (lk ? v.x * kLeak : 0.f);
                    v.y = yv.y > 0.f ? v.y : (lk ? v.y * kLeak : 0.f);
                    v.z = yv.z > 0.f ? v.z : (lk ? v.z * kLeak : 0.f);
                    v.w = yv.w > 0.f ? v.w : (lk ? v.w * kLeak : 0.f);
                    IO<TO>::st4(gpre + base + i, v);
                } else if (IO<TG>::code != IO<TO>::code && gpre) {
                    IO<TO>::st4(gpre + base + i, v);       // a pure change of storage type on the way (+ the bias sum)
                }
                sum += (v.x + v.y) + (v.z + v.w);
            }
            continue;
        }
        if (v2u) {  // two outputs per lane: four elements from each of the two source rows
            for (int i = threadIdx.x * 2; i < HW; i += 512) {
                const int oy = i / W, ox = i - oy * W;
                const long q = base * 4 + (long)(2 * oy) * (2 * W) + 2 * ox;
                const long gq = gbase + (long)(2 * oy) * (2 * W) + 2 * ox;
                const float4 a = IO<TG>::ld4(g + gq);
                const float4 b = IO<TG>::ld4(g + gq + 2 * W);
                float2 v = make_float2((a.x + a.y) + (b.x + b.y), (a.z + a.w) + (b.z + b.w));
                if (act != SPRK_ACT_NONE) {
                    const float4 yv = IO<TY>::ld4(y + q);
                    const bool lk = act == SPRK_ACT_LEAKY;
                    v.x = yv.x > 0.f ? v.x : (lk ? v.x * kLeak : 0.f);
                    v.y = yv.z > 0.f ? v.y : (lk ? v.y * kLeak : 0.f);
                }
                IO<TO>::st2(gpre + base + i, v);
                sum += v.x + v.y;
            }
            continue;
        }
        for (int i = threadIdx.x; i < HW; i += 256) {
            float v, yv = 0.f;
            if (up2) {
                const int oy = i / W, ox = i - oy * W;
                const long q = base * 4 + (long)(2 * oy) * (2 * W) + 2 * ox;
                const long gq = gbase + (long)(2 * oy) * (2 * W) + 2 * ox;
                v = (IO<TG>::ld(g + gq) + IO<TG>::ld(g + gq + 1)) + (IO<TG>::ld(g + gq + 2 * W) + IO<TG>::ld(g + gq + 2 * W + 1));
                if (act != SPRK_ACT_NONE) yv = IO<TY>::ld(y + q);
            } else {
                v = IO<TG>::ld(g + gbase + i);
                if (act != SPRK_ACT_NONE) yv = IO<TY>::ld(y + base + i);
            }
            if (act == SPRK_ACT_LEAKY)
                v = yv > 0.f ? v : v * kLeak;
            else if (act == SPRK_ACT_RELU)
                v = yv > 0.f ? v : 0.f;
            if (act != SPRK_ACT_NONE || up2 || (IO<TG>::code != IO<TO>::code && gpre)) IO<TO>::st(gpre + base + i, v);
            sum += v;
        }
    }
    if (partial) {
        __shared__ float red[256];
        red[threadIdx.x] = sum;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) partial[c * nsplit + s] = red[0];
    }
}

// Backward of Shift2d + chunk + rotate + concat (elem.hip: unrot4_tile64_kernel<false>) and the activation backward of
// the layer in front of it in one pass, P = 64, fp32 (sprk_unrot_act_bwd).  gf [B,4C,P,P] is the gradient of the
// un-rotated tensor f [B,4C,P,P], which is itself the mask: f at gf's address is y at the position the gradient goes
// to, so plane (n = kB + b, c) of gpre [4B,C,P,P] reads gf and f at plane (b, kC + c) along its rows, masks there, and
// turns the plane through LDS.  The decomposition is act_bwd_kernel's, so that the bias sums are the same additions in
// the same order: grid (C, nsplit), workgroup (c, s) walks images s, s + nsplit, ..., thread t owns elements
// 4t + 1024p of each plane.  Row P-1 of every gpre plane is +0 (Shift2d dropped it).
__global__ __launch_bounds__(256) void unrot_act_bwd64_kernel(const float *__restrict__ gf, const float *__restrict__ f,
                                                              float *__restrict__ gpre, float *__restrict__ partial,
                                                              int act, int B, int C, int nsplit) {
    constexpr int P = 64;
    __shared__ float tile[P][P + 1];
    const int c = blockIdx.x, s = blockIdx.y, N = 4 * B;
    const int j4 = (threadIdx.x & 15) << 2, r0 = threadIdx.x >> 4;
    const bool lk = act == SPRK_ACT_LEAKY;
    float sum = 0.f;
    for (int n = s; n < N; n += nsplit) {
        const int k = n / B, b = n - k * B, rot = (4 - k) & 3;
        const long src = (((long)b * 4 + k) * C + c) * (P * P);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int i = r0 + 16 * p;
            float4 v = *reinterpret_cast<const float4 *>(gf + src + i * P + j4);
            const float4 yv = *reinterpret_cast<const float4 *>(f + src + i * P + j4);
            v.x = yv.x > 0.f ? v.x : (lk ? v.x * kLeak : 0.f);
            v.y = yv.y > 0.f ? v.y : (lk ? v.y * kLeak : 0.f);
            v.z = yv.z > 0.f ? v.z : (lk ? v.z * kLeak : 0.f);
            v.w = yv.w > 0.f ? v.w : (lk ? v.w * kLeak : 0.f);
            tile[i][j4] = v.x;
            tile[i][j4 + 1] = v.y;
            tile[i][j4 + 2] = v.z;
            tile[i][j4 + 3] = v.w;
        }
        __syncthreads();
        float *dst = gpre + ((long)n * C + c) * (P * P);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int r = r0 + 16 * p;
            float o[4] = {0.f, 0.f, 0.f, 0.f};
            if (r + 1 < P) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    // gd (r, j) <- gf at rot_dst(rot; r + 1, j)   (elem.hip)
                    const int u = r + 1, w = j4 + q;
                    const int i = rot == 0 ? u : rot == 1 ? P - 1 - w : rot == 2 ? P - 1 - u : w;
                    const int j = rot == 0 ? w : rot == 1 ? u : rot == 2 ? P - 1 - w : P - 1 - u;
                    o[q] = tile[i][j];
                }
            }
            const float4 v = make_float4(o[0], o[1], o[2], o[3]);
            *reinterpret_cast<float4 *>(dst + r * P + j4) = v;
            sum += (v.x + v.y) + (v.z + v.w);
        }
        __syncthreads();
    }
    if (partial) {
        __shared__ float red[256];
        red[threadIdx.x] = sum;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) partial[c * nsplit + s] = red[0];
    }
}

__global__ void concat_up_bwd_kernel(const float *__restrict__ gin, float *__restrict__ ga, float *__restrict__ gb,
                                     int N, int C1, int C2, int H, int W, int up1) {
    const int Cin = C1 + C2;
    const int H1 = up1 ? H >> 1 : H, W1 = up1 ? W >> 1 : W;
    const long nA = (long)N * C1 * H1 * W1, nB = (long)N * C2 * H * W;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < nA + nB; e += (long)gridDim.x * blockDim.x) {
        if (e < nA) {
            long t = e;
            const int x = (int)(t % W1); t /= W1;
            const int y = (int)(t % H1); t /= H1;
            const int c = (int)(t % C1);
            const int n = (int)(t / C1);
            const float *p = gin + (((long)n * Cin + c) * H) * W;
            float v;
            if (up1) {
                const float *q = p + (long)(2 * y) * W + 2 * x;
                v = (q[0] + q[1]) + (q[W] + q[W + 1]);
            } else {
                v = p[(long)y * W + x];
            }
            ga[e] = v;
        } else {
            long t = e - nA;
            const int x = (int)(t % W); t /= W;
            const int y = (int)(t % H); t /= H;
            const int c = (int)(t % C2);
            const int n = (int)(t / C2);
            gb[e - nA] = gin[(((long)n * Cin + C1 + c) * H + y) * W + x];
        }
    }
}

// ------------------------------------------------------------------------------------------
// host-side planning
// ------------------------------------------------------------------------------------------
constexpr size_t kLdsLimit = 160 * 1024;

struct FwdPlan {
    int MT, NT, lgTC, lgTR, tilesX, tilesY, imgGroups, nblkN;
    int CK, R4, rows;
    int inRows, inCols, pitch, cplane, colOff, ldw, NI;
    int xtab, nG1, nG2;   // table-driven input staging (conv_mfma_kernel): groups per plane, source 1 / 2
    int latency;          // the latency-bound branch below re-chunked K (fewer, longer chunks than the throughput rule)
    long blocks;
    size_t ldsBytes, wsBytes;
};

// The stage of conv_dispatch / wgrad_dispatch that takes a call (sprk.h: SPRK_STAGE_*), and everything the MFMA
// launchers and the kernels' run-time branches are chosen by.  One function per family fills it (fwd_route /
// wg_route): the dispatchers, the launchers, the argument blocks and sprk_conv2d_variant all read it and decide
// nothing themselves.
struct FwdVariant {
    int stage;
    int MT, NT, RB, XTAB;            // conv_mfma_kernel<MT, NT, RB, XTAB>
    int small;                       // chunk_mma_small (MT == 1 and NT <= 3) instead of chunk_mma
    int stages, ragged_k, latency;   // K stages in LDS (1: all of K in one chunk), a shorter last chunk, FwdPlan::latency
    int vec1, vec2, vec4;            // 16-byte DMA of source 1 / 2, 16-byte stores
    int colOff, up1, c2, taps;       // colOff != 0, source 1 up-sampled on load, a second source, Corr::taps
    int CK, nChunks;                 // channels per K-chunk, K-chunks
    int blocks;                      // workgroups of the launch (FwdPlan::blocks: what plan_fwd's thresholds compare)
    sprk::WinoVariant wino;          // stage SPRK_STAGE_WINOGRAD: the kernel, grid and loop shapes of wino.hip (wino.h)
    int32_t rec16[SPRK_VARIANT_INTS];   // stage SPRK_STAGE_16BIT: the record as conv16_variant fills it (conv16.h)
};
struct WgVariant {
    int stage;
    int IT, NT, WJ, MODE;            // conv_wgrad_mfma_kernel<IT, NT, WJ, MODE>, MODE as the tensors allow it
    int xrow, xtab, g4, vec1, vec2;
    int chunks, groups;              // nChunks > 1, groups > 1
    int up1, c2;
    int tiles;                       // 64-pixel tiles one workgroup sums over (WgPlan::tilesPerGroup)
    sprk::WinoWgVariant wino;        // stage SPRK_STAGE_WINOGRAD: the launches of wino_wgrad (wino.h)
    int32_t rec16[SPRK_VARIANT_INTS];   // stage SPRK_STAGE_16BIT: the record as wgrad16_variant fills it (wgrad16.h)
};
thread_local FwdVariant t_last_fwd[2] = {{SPRK_STAGE_NONE}, {SPRK_STAGE_NONE}};   // [0] forward, [1] backward-data
thread_local WgVariant t_last_wg = {SPRK_STAGE_NONE};

int pad_to_residue(int raw, int residue) {  // smallest v >= raw with v % 32 == residue
    return raw + ((residue - raw % 32) + 32) % 32;
}

int pick_nt(int ntile) {
    // N tiles per block: every block re-stages the input tile, so fewer, wider blocks win; the
    // last block may be ragged (its surplus columns are zero weights, never stored)
    int NT = 1, best = 1 << 30;
    for (int cand : {6, 4, 3, 2, 1}) {
        const int cost = sprk::cdiv(ntile, cand) * (cand + 2);
        if (cost < best) {
            best = cost;
            NT = cand;
        }
    }
    return NT;
}

// Ck: channels along GEMM-k; Nn: GEMM-n extent; output spatial dims Ho x Wo over Nimg images
bool plan_fwd(const sprk::Corr &c, FwdPlan *p) {
    const int Nimg = c.N, Ck = c.C1 + c.C2, Nn = c.Cout, Ho = c.Hout, Wo = c.Wout, KH = c.KH, KW = c.KW;
    const int stride = c.stride, dil = c.dil, padL = c.padL, up1 = c.up1, hasC2 = c.C2 > 0, WinSrc = c.Win;
    const int KHW = KH * KW;
    const int ntile = sprk::cdiv(Nn, 16);
    int NT = pick_nt(ntile);
    int MT = 4;
    auto geometry = [&](int mt, int nt) {
        const int TM = 64 * mt;
        int TC = std::min(sprk::pow2_ceil(Wo), 64);
        if (dil * (KW - 1) >= 8 && TM >= 256) TC = std::min(TC, 16);
        TC = std::min(TC, TM);
        int TR = std::min(TM / TC, sprk::pow2_ceil(Ho));
        int NI = TM / (TC * TR);
        p->MT = mt;
        p->NT = nt;
        p->NI = NI;
        p->lgTC = sprk::ilog2(TC);
        p->lgTR = sprk::ilog2(TR);
        p->tilesX = sprk::cdiv(Wo, TC);
        p->tilesY = sprk::cdiv(Ho, TR);
        p->imgGroups = sprk::cdiv(Nimg, NI);
        p->nblkN = sprk::cdiv(ntile, nt);
        p->inRows = (TR - 1) * stride + (KH - 1) * dil + 1;
        p->inCols = (TC - 1) * stride + (KW - 1) * dil + 1;
        // image column 0 sits on a 16-byte boundary of the global rows (tile origins are multiples of 4)
        p->colOff = ((TC * stride) % 4 == 0) ? (((-padL) % 4) + 4) % 4 : 0;
        p->pitch = sprk::roundup(p->colOff + p->inCols, 4);
        p->cplane = pad_to_residue(NI * p->inRows * p->pitch, 16);
        return (long)p->imgGroups * p->tilesX * p->tilesY * p->nblkN;
    };
    long blocks = geometry(MT, NT);
    p->latency = 0;
    while (blocks < 512 && MT > 1) {
        MT >>= 1;
        blocks = geometry(MT, NT);
    }
    static const int kNtBlocks = sprk::knob_env("SPRK_FWD_NTBLK", 512);   // sweeps
    while (blocks < kNtBlocks && NT > 1) {
        NT = (NT == 6) ? 3 : (NT == 4) ? 2 : 1;
        blocks = geometry(MT, NT);
    }
    p->ldw = (NT % 2) ? NT * 16 : NT * 16 + 16;
    // per-tile source-offset tables (one entry per DMA lane and 256- or 64-float group of a channel plane):
    // source 1 by 16-byte DMA, or dword DMA when it is upsampled on load; source 2 by 16-byte DMA
    {
        const int planeElems = p->NI * p->inRows * p->pitch;
        const bool vecGeo = (((1 << p->lgTC) * stride) % 4 == 0) && (WinSrc % 4 == 0);
        p->nG1 = up1 ? sprk::cdiv(planeElems, 64) : sprk::cdiv(planeElems, 256);
        p->nG2 = hasC2 ? sprk::cdiv(planeElems, 256) : 0;
        p->xtab = (vecGeo && p->nG1 <= kMaxXG && p->nG2 <= kMaxXG) ? 1 : 0;
        if (!p->xtab) p->nG1 = p->nG2 = 0;
    }
    // channels per K-chunk: two stages (double buffer) should leave room for 3 workgroups per CU
    const int rowUnit = (MT == 1 && NT <= 3) ? 16 : 4;   // chunk_mma_small walks a chunk in groups of 4 k-steps
    auto lds = [&](int ck) {
        const int r4 = sprk::roundup(ck * KHW, rowUnit);
        const int stages = ck >= Ck ? 1 : 2;   // the whole of K in one chunk: nothing to double-buffer
        return (size_t)(2 * r4 + (p->nG1 + p->nG2) * 64 + stages * (ck * p->cplane + r4 * p->ldw)) * 4;
    };
    int CK = std::max(1, std::min(Ck, KHW == 1 ? 16 : std::max(1, 36 / KHW)));
    while (CK > 1 && lds(CK) > 52 * 1024) CK >>= 1;
    // small tiles: longer K-chunks (fewer barriers) while the stages stay small
    while (CK * 2 <= Ck && CK * 2 * KHW <= 288 && lds(CK * 2) <= (size_t)(MT == 1 ? 64 : 24) * 1024) CK *= 2;
    if (MT == 1 && blocks <= 2 * sprk::num_cus()) {
        // planes of a few pixels on a grid the CUs hold at once: these launches are latency-bound (a workgroup's serial
        // preamble -> DMA -> MFMA -> store chain, not the machine's throughput), and every chunk adds a DMA issue, a
        // landing wait and a barrier to that chain: as few chunks as the LDS allows — all of K in one stage when it
        // fits.  One workgroup per CU is all a grid of <= 256 workgroups needs, two up to 512; larger grids keep the
        // smaller stages (more resident workgroups hide more latency than fewer chunks save: measured).
        const size_t room = blocks <= sprk::num_cus() ? 156 * 1024 : 78 * 1024;
        for (int nCh = 1; nCh <= Ck; ++nCh) {
            const int ck = sprk::cdiv(Ck, nCh);
            if (ck <= CK) break;
            if (lds(ck) <= room) {
                CK = ck;
                p->latency = 1;
                break;
            }
        }
    }
    if (lds(CK) > kLdsLimit) return false;
    p->CK = CK;
    p->blocks = blocks;
    p->R4 = sprk::roundup(CK * KHW, rowUnit);
    p->rows = sprk::cdiv(Ck, CK) * p->R4;
    p->ldsBytes = lds(CK);
    p->wsBytes = ((size_t)kZeroFloats + (size_t)p->nblkN * p->rows * p->ldw) * sizeof(float);
    return true;
}

template <int MT, int NT, int RB>
int launch_fwd_one(const ConvArgs &a, const FwdPlan &p, const FwdVariant &v, dim3 grid, hipStream_t s) {
    auto go = [&](auto kernel) {
        if (int rc = sprk::lds_optin(kernel, p.ldsBytes, "conv_mfma")) return rc;
        hipLaunchKernelGGL(kernel, grid, dim3(kBlock), p.ldsBytes, s, a);
        return (int)SPRK_OK;
    };
    return v.XTAB ? go(conv_mfma_kernel<MT, NT, RB, true>) : go(conv_mfma_kernel<MT, NT, RB, false>);
}

template <int MT, int RB>
int launch_fwd_nt(const ConvArgs &a, const FwdPlan &p, const FwdVariant &v, dim3 grid, hipStream_t s) {
    switch (v.NT) {
        case 1: return launch_fwd_one<MT, 1, RB>(a, p, v, grid, s);
        case 2: return launch_fwd_one<MT, 2, RB>(a, p, v, grid, s);
        case 3: return launch_fwd_one<MT, 3, RB>(a, p, v, grid, s);
        case 4: return launch_fwd_one<MT, 4, RB>(a, p, v, grid, s);
        default: return launch_fwd_one<MT, 6, RB>(a, p, v, grid, s);
    }
}

int launch_fwd(const ConvArgs &a, const FwdPlan &p, const FwdVariant &v, hipStream_t s) {
    dim3 grid(p.imgGroups * p.tilesX * p.tilesY, p.nblkN);
    switch (v.MT) {
        case 1: return launch_fwd_nt<1, 1>(a, p, v, grid, s);
        case 2: return v.RB == 1 ? launch_fwd_nt<2, 1>(a, p, v, grid, s) : launch_fwd_nt<2, 2>(a, p, v, grid, s);
        default:
            return v.RB == 1 ? launch_fwd_nt<4, 1>(a, p, v, grid, s)
                             : v.RB == 2 ? launch_fwd_nt<4, 2>(a, p, v, grid, s) : launch_fwd_nt<4, 4>(a, p, v, grid, s);
    }
}

bool aligned16(const void *p) {
    static const bool novec = sprk::knob_env("SPRK_NOVEC", 0) != 0;  // 1 = force the 4-byte DMA path
    return !novec && (((uintptr_t)p) & 15) == 0;
}

// The variant of conv_mfma_kernel that correlation c takes under plan p with these tensors (only their alignment is
// looked at); `stage` is left to fwd_route.
FwdVariant fwd_variant(const sprk::Corr &c, const FwdPlan &p, const void *x, const void *x2, const void *y) {
    FwdVariant v{};
    v.MT = p.MT;
    v.NT = p.NT;
    // pixel tiles of a wave that lie in one tile row are 16 floats apart in LDS (stride 1): one address
    // base per row instead of one per tile
    const int rows = (c.stride == 1) ? std::max(1, (p.MT * 16) >> p.lgTC) : p.MT;
    v.RB = p.MT == 1 ? 1 : p.MT == 2 ? (rows == 1 ? 1 : 2) : (rows == 1 ? 1 : rows == 2 ? 2 : 4);
    v.small = (p.MT == 1 && p.NT <= 3) ? 1 : 0;
    const int Ck = c.C1 + c.C2;
    v.CK = p.CK;
    v.nChunks = sprk::cdiv(Ck, p.CK);
    v.blocks = (int)std::min<long>(p.blocks, 1L << 30);
    v.stages = p.CK >= Ck ? 1 : 2;
    v.ragged_k = (Ck % p.CK) ? 1 : 0;
    v.latency = p.latency;
    v.colOff = p.colOff != 0;
    v.up1 = c.up1 ? 1 : 0;
    v.c2 = c.C2 > 0;
    v.taps = c.taps;
    v.vec4 = ((c.Wout % 4 == 0) && (p.lgTC >= 2) && (((uintptr_t)y & 15) == 0)) ? 1 : 0;
    // 16-byte DMA: tile origins on 4-column boundaries, rows 16-byte aligned, source at full resolution
    const bool geo = ((1 << p.lgTC) * c.stride) % 4 == 0 && (c.Win % 4) == 0;
    v.vec1 = (geo && !c.up1 && aligned16(x)) ? 1 : 0;
    v.vec2 = (geo && x2 && aligned16(x2)) ? 1 : 0;
    // the tables hold byte offsets (image within the tile's group + in-plane part) below 2^31 and were sized
    // for the expected DMA widths; a chunk's channel offset (soffset) stays below 2^32 bytes
    const long H1 = c.up1 ? c.Hin / 2 : c.Hin, W1 = c.up1 ? c.Win / 2 : c.Win;
    const long NIm1 = p.NI - 1;
    const bool small1 = (NIm1 * c.C1 + 1) * H1 * W1 < (1L << 29) && (long)p.CK * H1 * W1 < (1L << 29);
    const bool small2 = (NIm1 * c.C2 + 1) * c.Hin * c.Win < (1L << 29) && (long)p.CK * c.Hin * c.Win < (1L << 29);
    static const int tabmode = sprk::knob_env("SPRK_XTAB", 2);   // 0 = pointer-arithmetic staging, 1 = not for 1x1
    const bool want = tabmode == 2 || (tabmode == 1 && c.KH * c.KW > 1);
    v.XTAB = (p.xtab && want && small1 && small2 && (c.up1 || v.vec1) && (c.C2 == 0 || v.vec2)) ? 1 : 0;
    return v;
}

// conv_mfma_kernel's argument block for correlation c under plan p and variant v; wsf: the call's workspace (zero
// block, then the transformed weights)
ConvArgs conv_args(const sprk::Corr &c, const FwdPlan &p, const FwdVariant &v, const float *x, const float *x2, float *wsf,
                   float *y) {
    ConvArgs a{};
    a.x = x; a.x2 = x2; a.zeros = wsf; a.wT = wsf + kZeroFloats;
    a.bias = c.ep.bias; a.scale = c.ep.scale; a.shift = c.ep.shift; a.res = c.ep.res;
    a.y = y;
    a.N = c.N; a.C1 = c.C1; a.C2 = c.C2; a.Hin = c.Hin; a.Win = c.Win; a.up1 = c.up1;
    a.H1 = c.up1 ? c.Hin / 2 : c.Hin;
    a.W1 = c.up1 ? c.Win / 2 : c.Win;
    a.Cout = c.Cout; a.Hout = c.Hout; a.Wout = c.Wout;
    a.KH = c.KH; a.KW = c.KW; a.stride = c.stride; a.dil = c.dil; a.padT = c.padT; a.padL = c.padL;
    a.act = c.ep.act;
    a.resH = c.ep.res_h; a.resW = c.ep.res_w; a.resOff = c.ep.res_off;
    a.up2 = c.ep.up2;
    a.vec4 = v.vec4;
    a.lgTC = p.lgTC;
    a.lgTR = p.lgTR;
    a.tilesX = p.tilesX;
    a.tilesY = p.tilesY;
    a.CK = p.CK;
    a.R4 = p.R4;
    a.rows = p.rows;
    a.inRows = p.inRows;
    a.inCols = p.inCols;
    a.pitch = p.pitch;
    a.cplane = p.cplane;
    a.colOff = p.colOff;
    a.ldw = p.ldw;
    a.invImg = 1.0f / (float)(p.inRows * p.pitch);
    a.invPitch = 1.0f / (float)p.pitch;
    a.vec1 = v.vec1;
    a.vec2 = v.vec2;
    a.deal = 1;
    a.xcdRemap = 1;
    a.xtab = v.XTAB;
    a.nG1 = p.nG1;
    a.nG2 = p.nG2;
    return a;
}

int transform_weights(const float *w, float *ws, int Cout, int Cin, int KHW, int mode, const FwdPlan &p,
                      hipStream_t s) {
    const long total = (long)p.nblkN * p.rows * p.ldw + kZeroFloats;
    return sprk::wprep_site(sprk::wprep_item(sprk::WPREP_DIRECT, w, ws, total,
                                             {Cout, Cin, KHW, mode, p.CK, p.R4, p.rows, p.NT * 16, p.ldw, p.nblkN}), s);
}

int check_geom(const sprk_conv_geom *g) {
    SPRK_REQUIRE(g, "conv: null geometry");
    SPRK_REQUIRE(g->N > 0 && g->C1 >= 0 && g->C2 >= 0 && g->C1 + g->C2 > 0 && g->Cout > 0, "conv: bad channel/batch counts");
    SPRK_REQUIRE(g->Hin > 0 && g->Win > 0 && g->Hout > 0 && g->Wout > 0, "conv: bad spatial dims");
    SPRK_REQUIRE(g->KH > 0 && g->KW > 0 && g->stride > 0 && g->dil > 0, "conv: bad kernel params");
    SPRK_REQUIRE(!g->up1 || (g->Hin % 2 == 0 && g->Win % 2 == 0), "conv: up1 needs even Hin/Win");
    SPRK_REQUIRE((long)g->N * (g->C1 + g->C2) * g->Hin * g->Win < (1L << 40), "conv: tensor too large");
    return SPRK_OK;
}

struct WgPlan {
    int IT, NT, lgTC, lgTR, tilesX, tilesY, nTiles, tilesPerGroup, groups;
    int CKW, nChunks, nblkN, ioffN, CoutP;
    int inRows, inCols, pitch, cplane, colOff, xrow;
    int mode, nG1, nG2;
    size_t ldsBytes, wsBytes;
};

bool plan_wgrad(const sprk_conv_geom *g, WgPlan *p) {
    const int KHW = g->KH * g->KW, Cin = g->C1 + g->C2;
    const int ntile = sprk::cdiv(g->Cout, 16);
    const int NT = pick_nt(ntile);
    p->NT = NT;
    p->nblkN = sprk::cdiv(ntile, NT);
    p->CoutP = p->nblkN * NT * 16;
    const int TM = 64;
    int TC = std::min(sprk::pow2_ceil(g->Wout), 64);
    if (g->dil * (g->KW - 1) >= 8) TC = std::min(TC, 8);
    int TR = std::min(TM / TC, sprk::pow2_ceil(g->Hout));
    int NI = TM / (TC * TR);
    p->lgTC = sprk::ilog2(TC);
    p->lgTR = sprk::ilog2(TR);
    p->tilesX = sprk::cdiv(g->Wout, TC);
    p->tilesY = sprk::cdiv(g->Hout, TR);
    p->nTiles = sprk::cdiv(g->N, NI) * p->tilesX * p->tilesY;
    p->inRows = (TR - 1) * g->stride + (g->KH - 1) * g->dil + 1;
    p->inCols = (TC - 1) * g->stride + (g->KW - 1) * g->dil + 1;
    p->colOff = ((TC * g->stride) % 4 == 0) ? (((-g->pad_left) % 4) + 4) % 4 : 0;
    p->pitch = sprk::roundup(p->colOff + p->inCols, 4);
    // channel stride: 16-byte DMA needs a multiple of 4 floats (then 16 channels x 2 pixels of one A read
    // share banks pairwise: 2-way); the 4-byte DMA fallback can use the conflict-free stride = 2 (mod 32)
    const bool vecGeo = (TC * g->stride) % 4 == 0 && (g->Win % 4) == 0;
    p->cplane = pad_to_residue(NI * p->inRows * p->pitch, vecGeo ? 4 : 2);
    // 1x1, stride 1, unpadded, single full-resolution source: the x tile is 64 contiguous pixels per
    // channel, staged like the G tile (swizzled 64-float rows, 16-byte DMA)
    p->xrow = (KHW == 1 && g->stride == 1 && g->pad_top == 0 && g->pad_left == 0 && !g->up1 && g->C2 == 0 &&
               TC >= 4 && (g->Win % 4) == 0 && g->Hin == g->Hout && g->Win == g->Wout)
                  ? 1
                  : 0;
    if (p->xrow) {
        p->cplane = 64;
        p->colOff = 0;
    }
    // channel chunks: each wave (wi = 0..3) owns k-tiles wi, wi+4, ... of a chunk's ceil(CKW*KHW/16) k-tiles, at
    // most kMaxIT of them.  Cost of a split = chunks x busiest wave's k-tiles (+ a little per chunk for staging
    // the G tile again); equal-sized chunks so every workgroup carries the same load.
    constexpr int kMaxIT = 7;
    // operand addressing of the tile loop: 1 = 1x1 rows, 2 = stride-1 tiles with rows of >= 4 pixels, 0 = any
    // (MODE 2 also stages the x planes through offset tables and 16-byte buffer loads: aligned rows, no upsampling)
    p->mode = p->xrow ? 1 : (g->stride == 1 && TC >= 4 && vecGeo && !g->up1) ? 2 : 0;
    {
        const int planeElems = NI * p->inRows * p->pitch;
        p->nG1 = p->mode == 2 ? sprk::cdiv(planeElems, 256) : 0;
        p->nG2 = (p->mode == 2 && g->C2 > 0) ? sprk::cdiv(planeElems, 256) : 0;
        if (p->inRows >= 1024 || p->pitch >= 1024) p->mode = p->xrow ? 1 : 0, p->nG1 = p->nG2 = 0;
    }
    auto lds = [&](int ck) {
        const int ioffN = sprk::roundup(sprk::roundup(ck * KHW, 16), 4);
        return (size_t)(ioffN + 64 + 16 + 2 * (p->nG1 + p->nG2) * 64 + 2 * (ck * p->cplane + NT * 16 * 64)) * 4;
    };
    // The cost of a split is the time of ONE workgroup (they all run at once: never more workgroups than CUs, see
    // below): tiles per workgroup x (the busiest wave's k-tiles + a little for staging the G tile again).  With many
    // tiles that is proportional to chunks x k-tiles, the total work; with few tiles (the U-Net levels <= 16x16: every
    // workgroup has one tile whatever the split) it is the k-tiles alone, so small planes are cut into more, shorter
    // chunks on more CUs (96->96 at 64x8x8: 2 chunks of 7 k-tiles per wave -> 4 of 4).
    static const int kWgKnob = sprk::knob_env("SPRK_WG_BLOCKS", 0);   // sweeps; default: one workgroup per CU
    const int kWgBlocks = kWgKnob > 0 ? kWgKnob : sprk::num_cus();
    int CKW = 0;
    long bestCost = 1L << 60;
    for (int nCh = 1; nCh <= Cin; ++nCh) {
        const int ck = sprk::cdiv(Cin, nCh);
        if (sprk::cdiv(Cin, ck) != nCh) continue;
        const int itw = sprk::cdiv(sprk::cdiv(ck * KHW, 16), 4);
        if (itw > kMaxIT || lds(ck) > 150 * 1024 || (p->xrow && ck > 192)) continue;
        const int g = std::max(1, std::min(p->nTiles, kWgBlocks / (nCh * p->nblkN)));
        const long cost = (long)sprk::cdiv(p->nTiles, g) * (4 * itw + 1);
        if (cost < bestCost) {
            bestCost = cost;
            CKW = ck;
        }
        if (itw == 1) break;
    }
    if (CKW == 0 || lds(CKW) > kLdsLimit) return false;
    p->CKW = CKW;
    p->nChunks = sprk::cdiv(Cin, CKW);
    p->ioffN = sprk::roundup(sprk::roundup(CKW * KHW, 16), 4);
    p->IT = sprk::cdiv(sprk::cdiv(CKW * KHW, 16), 4);
    p->ldsBytes = lds(CKW);
    // one workgroup per CU (the stages fill most of the LDS): never more workgroups than CUs, or the
    // surplus runs as a second, nearly empty round
    const int per = p->nChunks * p->nblkN;
    int groups = std::max(1, std::min(p->nTiles, kWgBlocks / per));
    p->tilesPerGroup = sprk::cdiv(p->nTiles, groups);
    p->groups = sprk::cdiv(p->nTiles, p->tilesPerGroup);
    p->wsBytes = ((size_t)kZeroFloats + (size_t)p->groups * Cin * KHW * p->CoutP) * sizeof(float);
    return true;
}

template <int IT, int NT, int MODE>
int launch_wg_one(const WgArgs &a, const WgPlan &p, dim3 grid, hipStream_t s) {
    constexpr int WJ = (NT % 2 == 0) ? 2 : 1;   // two waves per SIMD whenever the cout tiles split evenly (wg_variant: WJ)
    if (int rc = sprk::lds_optin(conv_wgrad_mfma_kernel<IT, NT, WJ, MODE>, p.ldsBytes, "conv_wgrad_mfma")) return rc;
    hipLaunchKernelGGL((conv_wgrad_mfma_kernel<IT, NT, WJ, MODE>), grid, dim3(256 * WJ), p.ldsBytes, s, a);
    return SPRK_OK;
}

template <int IT, int MODE>
int launch_wg_nt(const WgArgs &a, const WgPlan &p, const WgVariant &v, dim3 grid, hipStream_t s) {
    switch (v.NT) {
        case 1: return launch_wg_one<IT, 1, MODE>(a, p, grid, s);
        case 2: return launch_wg_one<IT, 2, MODE>(a, p, grid, s);
        case 3: return launch_wg_one<IT, 3, MODE>(a, p, grid, s);
        case 4: return launch_wg_one<IT, 4, MODE>(a, p, grid, s);
        default: return launch_wg_one<IT, 6, MODE>(a, p, grid, s);
    }
}

template <int MODE>
int launch_wg_it(const WgArgs &a, const WgPlan &p, const WgVariant &v, dim3 grid, hipStream_t s) {
    switch (v.IT) {
        case 1: return launch_wg_nt<1, MODE>(a, p, v, grid, s);
        case 2: return launch_wg_nt<2, MODE>(a, p, v, grid, s);
        case 3: return launch_wg_nt<3, MODE>(a, p, v, grid, s);
    }
    if constexpr (MODE != 1) {   // the row-staged 1x1 form never needs more than 192 channels = 3 k-tiles per wave
        switch (v.IT) {
            case 4: return launch_wg_nt<4, MODE>(a, p, v, grid, s);
            case 5: return launch_wg_nt<5, MODE>(a, p, v, grid, s);
            case 6: return launch_wg_nt<6, MODE>(a, p, v, grid, s);
            case 7: return launch_wg_nt<7, MODE>(a, p, v, grid, s);
        }
    }
    sprk::set_error("conv2d_bwd_weight: no kernel for %d k-tiles per wave", v.IT);
    return SPRK_EINVAL;
}

int launch_wg(const WgArgs &a, const WgPlan &p, const WgVariant &v, hipStream_t s) {
    dim3 grid(p.groups, p.nChunks, p.nblkN);
    return v.MODE == 1 ? launch_wg_it<1>(a, p, v, grid, s)
                       : v.MODE == 2 ? launch_wg_it<2>(a, p, v, grid, s) : launch_wg_it<0>(a, p, v, grid, s);
}

// The variant of conv_wgrad_mfma_kernel that layer g takes under plan p with these tensors (only their alignment is
// looked at): the kernel's MODE is the plan's, or the general kernel's 0 where the tensors' alignment or size rules the
// plan's staging out.  `stage` is left to wg_route; *refused: the 1x1 row form has no staging for these tensors.
WgVariant wg_variant(const sprk_conv_geom *g, const WgPlan &p, const void *x, const void *x2, const void *gy, bool *refused) {
    WgVariant v{};
    const int Cin = g->C1 + g->C2;
    v.IT = p.IT;
    v.NT = p.NT;
    v.WJ = (p.NT % 2 == 0) ? 2 : 1;
    {
        const bool geo = ((1 << p.lgTC) * g->stride) % 4 == 0 && (g->Win % 4) == 0;
        v.vec1 = (geo && !g->up1 && aligned16(x)) ? 1 : 0;
        v.vec2 = (geo && x2 && aligned16(x2)) ? 1 : 0;
    }
    v.xrow = p.xrow;
    v.g4 = (p.lgTC >= 2 && (g->Wout % 4) == 0 && ((uintptr_t)gy & 15) == 0) ? 1 : 0;
    // buffer-load staging of the row tiles needs 16-byte aligned rows and 32-bit byte offsets inside one tile
    // group and one channel block; otherwise the general kernel (MODE 0) runs
    const long planeI = (long)g->Hin * g->Win, planeO = (long)g->Hout * g->Wout;
    const int NIw = 64 >> (p.lgTC + p.lgTR);
    const bool fits = (long)NIw * Cin * planeI < (1L << 28) && (long)NIw * g->Cout * planeO < (1L << 28) &&
                      (long)p.CKW * planeI < (1L << 28) && (long)p.NT * 16 * planeO < (1L << 28);
    static const int rowbuf = sprk::knob_env("SPRK_WG_ROWBUF", 1);
    const bool fast = rowbuf && fits && v.g4;
    v.xtab = fast ? 1 : 0;
    *refused = v.xrow && (!fast || (((uintptr_t)x & 15) != 0));
    // MODE 2 additionally needs 16-byte aligned x / x2 (the general kernel ignores the table area in LDS)
    const bool planesOk = v.vec1 && (g->C2 == 0 || v.vec2);
    v.MODE = !fast ? 0 : (p.mode == 2 && !planesOk) ? 0 : p.mode;
    v.chunks = p.nChunks > 1;
    v.groups = p.groups > 1;
    v.up1 = g->up1 ? 1 : 0;
    v.c2 = g->C2 > 0;
    v.tiles = p.tilesPerGroup;
    return v;
}

// conv_wgrad_mfma_kernel's argument block for layer g under plan p and variant v; wsf: the call's workspace (a
// zero-block-sized gap, then the partial sums)
int wgrad_args(const sprk_conv_geom *g, const WgPlan &p, const WgVariant &v, const float *x, const float *x2,
               const float *gy, float *wsf, WgArgs &a) {
    const float *zeros = nullptr;  // device-resident, never written: no per-call memset
    if (hipGetSymbolAddress((void **)&zeros, HIP_SYMBOL(g_zero_block)) != hipSuccess || !zeros) {
        sprk::set_error("conv2d_bwd_weight: zero block unavailable");
        return SPRK_ELAUNCH;
    }
    a = WgArgs{};
    a.x = x; a.x2 = x2; a.gy = gy; a.zeros = zeros; a.partial = wsf + kZeroFloats;
    a.N = g->N; a.C1 = g->C1; a.C2 = g->C2; a.Hin = g->Hin; a.Win = g->Win; a.up1 = g->up1;
    a.H1 = g->up1 ? g->Hin / 2 : g->Hin;
    a.W1 = g->up1 ? g->Win / 2 : g->Win;
    a.Cout = g->Cout; a.CoutP = p.CoutP; a.Hout = g->Hout; a.Wout = g->Wout;
    a.KH = g->KH; a.KW = g->KW; a.stride = g->stride; a.dil = g->dil; a.padT = g->pad_top; a.padL = g->pad_left;
    a.lgTC = p.lgTC; a.lgTR = p.lgTR; a.tilesX = p.tilesX; a.tilesY = p.tilesY; a.nTiles = p.nTiles;
    a.tilesPerGroup = p.tilesPerGroup;
    a.CKW = p.CKW; a.ioffN = p.ioffN;
    a.inRows = p.inRows; a.inCols = p.inCols; a.pitch = p.pitch; a.cplane = p.cplane; a.colOff = p.colOff;
    a.invImg = 1.0f / (float)(p.inRows * p.pitch);
    a.invPitch = 1.0f / (float)p.pitch;
    a.vec1 = v.vec1;
    a.vec2 = v.vec2;
    a.deal = 1;
    a.xrow = v.xrow;
    a.g4 = v.g4;
    a.xtab = v.xtab;
    static const int wg_diag = sprk::diag_env("SPRK_WG_DIAG");
    a.diag = wg_diag;
    a.nG1 = p.nG1;
    a.nG2 = p.nG2;
    return SPRK_OK;
}

// the calls whose activation tensors are 16-bit tensors (SPRK_DT_X16 / SPRK_DT_Y16) end here when no 16-bit kernel took them
int check_storage32(const char *who, int dtype) {
    SPRK_REQUIRE(!(dtype & (SPRK_DT_X16 | SPRK_DT_Y16)),
                 "%s: no kernel takes this geometry with 16-bit activation tensors (ask sprk_conv2d_storage16 first)", who);
    return SPRK_OK;
}

}  // namespace

// ==========================================================================================
// C ABI
// ==========================================================================================
extern "C" {

#ifdef SPRK_DIAG
// diagnostic builds only: the phase time stamps workgroup 0 of the last conv_mfma_kernel launch left (10 ns units)
int sprk_diag_conv_clock(long long *out8) {
    return hipMemcpyFromSymbol(out8, HIP_SYMBOL(sprk_diag_conv_clk), 40 * sizeof(long long)) == hipSuccess ? SPRK_OK : SPRK_ELAUNCH;
}
#endif

// Which calls of a layer exist for 16-bit ACTIVATION tensors (SPRK_DT_X16 / SPRK_DT_Y16)?  Bit 0: forward, bit 1:
// backward-data, bit 2: backward-weight.  g->dtype carries the operand type; the storage bits are ignored (every
// input / output storage combination of an eligible call exists).  ep: the forward call's epilogue (may be null).
int sprk_conv2d_storage16(const sprk_conv_geom *g, const sprk_conv_epilogue *ep) {
    if (!g || check_geom(g) != SPRK_OK) return 0;
    const int dt = g->dtype & SPRK_DT_MASK;
    if ((dt != SPRK_DT_BF16 && dt != SPRK_DT_F16) || naive_of(g) || g->stride != 1) return 0;
    sprk_conv_geom q = *g;
    q.dtype = (g->dtype & ~(SPRK_DT_WPREP | SPRK_DT_WPREP_KIND(7))) | SPRK_DT_X16 | SPRK_DT_Y16;
    int r = 0;
    if (sprk::conv16_kind(sprk::Corr(q, ep)) >= 2) r |= 1;
    if (sprk::conv16_kind(sprk::Corr(q)) >= 2) r |= 2;   // (never for an up1 layer: Corr::mfma_only)
    if (sprk::wgrad16_eligible(q)) r |= 4;
    return r;
}

// What a dispatch of c can ask for: the maximum over the stages of conv_dispatch that could take it (0: the MFMA plan
// does not fit LDS).  ops.WeightPrep keeps workspaces of this size for the life of a stepper.
static size_t corr_ws_bytes(const sprk::Corr &c) {
    FwdPlan p;
    if (!plan_fwd(c, &p)) return 0;
    size_t need = p.wsBytes;
    if (sprk::wino_eligible(c)) need = std::max(need, sprk::wino_ws_bytes(c));
    if (c.dt() != SPRK_DT_F32) need = std::max(need, sprk::conv16_ws_bytes(c));
    return need;
}

size_t sprk_conv2d_fwd_ws_bytes(const sprk_conv_geom *g) {
    if (!g) return 0;
    // the query does not know the epilogue the call will carry (fused up-sampling and a residual exclude some kernels,
    // and the remaining one may need more): the maximum over the four cases
    size_t need = 0;
    for (int v = 0; v < 4; ++v) {
        sprk_conv_epilogue e = sprk::kNoEpilogue;
        e.up2 = v & 1;
        e.res = (v & 2) ? (const float *)g : nullptr;   // any non-null pointer: never read
        need = std::max(need, corr_ws_bytes(sprk::Corr(*g, &e)));
    }
    return need;
}

size_t sprk_conv2d_bwd_data_ws_bytes(const sprk_conv_geom *g) {
    return (g && g->stride == 1) ? corr_ws_bytes(sprk::Corr(*g)) : 0;
}

// in-place mask of a finished gradient (the layers whose backward-data kernel has no masked epilogue)
// (with SPRK_DT_Y16 the gradient and the mask — the consumer's saved 16-bit input — are tensors of the operand type)
static int mask_in_place(float *gin, const float *mask_y, int mask_act, const sprk_conv_geom *g, hipStream_t s) {
    const int t = (g->dtype & SPRK_DT_Y16) ? (g->dtype & SPRK_DT_MASK) : 0;
    return sprk_act_bwd(gin, mask_y, gin, nullptr, mask_act, g->N, g->C1 + g->C2, g->Hin, g->Win, 0, 0, SPRK_IO3(t, t, t),
                        nullptr, 0, s);
}

// Stage 5's narrow case: may the masked backward-data of layer g, planned as p, run on mask1x1_kernel (mask1x1.hip)
// instead of conv_mfma_kernel + mask_in_place?  A 1x1 GEMM over few reduced channels whose plan walks its chunks with
// chunk_mma (MT >= 2; chunk_mma_small of the MT = 1 plans sums in another order).  The one predicate of the dispatcher
// and of sprk_conv2d_bwd_data_mask_fused.
static bool mask1x1_takes(const sprk_conv_geom *g, const sprk::Corr &c, const FwdPlan &p) {
    return g->KH == 1 && g->KW == 1 && g->stride == 1 && g->dil == 1 && g->pad_top == 0 && g->pad_left == 0 && !g->up1 &&
           g->C2 == 0 && g->Hin == g->Hout && g->Win == g->Wout && c.dt() == SPRK_DT_F32 && !c.x16() && !c.y16() &&
           ((long)g->Hin * g->Win) % 4 == 0 && (long)g->Hin * g->Win < (1L << 30) && p.MT >= 2 &&
           sprk::mask1x1_steps(g->Cout, p.CK) > 0;
}

// Stage 6: may the unmasked call c, planned as p, run on gemm1x1_kernel (gemm1x1.hip) instead of conv_mfma_kernel?  A 1x1
// GEMM over many reduced channels on the plan of the launches that fill the machine (MT = 4, NT = 6: slabs of 96
// channels whose 16-row chunks make slab row = reduced channel), nothing fused that the streaming kernel has no code
// for.  The one predicate of the dispatcher and of sprk_conv2d_variant; the tensors' alignment is the caller's part.
static bool gemm1x1_takes(const sprk::Corr &c, const FwdPlan &p) {
    return sprk::g_gemm1x1_on.load(std::memory_order_relaxed) && c.KH == 1 && c.KW == 1 && c.stride == 1 && c.dil == 1 &&
           c.padT == 0 && c.padL == 0 && !c.up1 && !c.mfma_only && c.C2 == 0 && !c.ep.up2 && !c.ep.res &&
           c.Hin == c.Hout && c.Win == c.Wout && c.dt() == SPRK_DT_F32 && !c.x16() && !c.y16() && p.MT == 4 && p.NT == 6 &&
           p.CK == 16 && p.R4 == 16 && p.ldw == sprk::kGemm1x1Ldw && sprk::gemm1x1_fits(c.N, c.C1, c.Hin * c.Win);
}

// Which stage of conv_dispatch takes the call, by the stages' own predicates in the dispatcher's order, and for the
// stages that plan (mask1x1, MFMA) the plan and the kernel variant.  The dispatcher acts on this answer and
// sprk_conv2d_variant returns it; the tensors are looked at for their alignment only.  x / x2 / y as conv_dispatch
// takes them (backward-data: x = gy, y = gin); mask_y null: an unmasked call.
static FwdVariant fwd_route(bool bwd, const sprk_conv_geom *g, const sprk_conv_epilogue *ep, const void *x, const void *x2,
                            const void *y, const void *mask_y, FwdPlan *p, bool unrot = false) {
    FwdVariant v{};
    if (naive_of(g) || (bwd && g->stride != 1)) {
        StemPlan sp;
        v.stage = (bwd && !naive_of(g) && plan_stem_bwd(g, &sp)) ? SPRK_STAGE_STEM : SPRK_STAGE_DIRECT;
        return v;
    }
    const sprk::Corr c = bwd ? sprk::Corr(*g) : sprk::Corr(*g, ep);
    if (c.dt() != SPRK_DT_F32 && sprk::conv16_eligible(c)) {
        v.stage = SPRK_STAGE_16BIT;
        sprk::conv16_variant(c, v.rec16);
    } else if (c.dtype & (SPRK_DT_X16 | SPRK_DT_Y16)) {
        v.stage = SPRK_STAGE_REFUSED;   // the storage guard
    } else if (sprk::wino_eligible(c)) {
        v.stage = SPRK_STAGE_WINOGRAD;
        v.wino = sprk::wino_variant(c, mask_y != nullptr, unrot ? g->N / 4 : 0);
    } else if (!plan_fwd(c, p)) {
        v.stage = SPRK_STAGE_REFUSED;   // no plan fits LDS
    } else {
        v = fwd_variant(c, *p, x, x2, y);
        v.stage = (bwd && mask_y && mask1x1_takes(g, c, *p) && aligned16(x) && aligned16(y) && aligned16(mask_y))
                      ? SPRK_STAGE_MASK1X1
                      : SPRK_STAGE_MFMA;
        if (v.stage == SPRK_STAGE_MFMA && !mask_y && !unrot && gemm1x1_takes(c, *p) && aligned16(x) && aligned16(y))
            v.stage = SPRK_STAGE_GEMM1X1;
    }
    return v;
}

// The one place where a forward or (bwd) backward-data call meets its kernel; a new convolution kernel is plugged in
// here and in fwd_route ("The convolution dispatcher").  g / ep: the layer as the caller gave it; for
// backward-data x = gy, x2 = null, y = gin, and mask_y / mask_act the optional mask of sprk_conv2d_bwd_data_masked.
// The stages, in order:
//   direct kernels (SPRK_DT_NAIVE; strided backward-data) -> 16-bit operands -> storage guard -> Winograd -> MFMA
// unrot (forward only): y is the un-rotated tensor f [N/4, 4*Cout, H, W] of sprk_unrot4_shift_concat_fwd, stored by the
// kernel itself (sprk_conv2d_fwd_unrot); only the fp32 Winograd stage has such a store, any other stage refuses.
static int conv_dispatch(bool bwd, const float *x, const float *x2, const float *w, float *y, const sprk_conv_geom *g,
                         const sprk_conv_epilogue *ep, const float *mask_y, int mask_act, void *ws, size_t ws_bytes,
                         void *stream, bool unrot = false) {
    const char *who = bwd ? "conv2d_bwd_data" : unrot ? "conv2d_fwd_unrot" : "conv2d_fwd";
    if (int rc = check_geom(g)) return rc;
    SPRK_REQUIRE(!unrot || sprk_conv2d_fwd_unrot_eligible(g, ep), "conv2d_fwd_unrot: no kernel with an un-rotated store for this layer");
    SPRK_REQUIRE(x && w && y, "%s: null tensor", who);
    if (bwd) {
        SPRK_REQUIRE(mask_act == SPRK_ACT_NONE || (mask_y && !g->up1), "conv2d_bwd_data: mask needs the saved input, no upsampling");
        if (mask_act == SPRK_ACT_NONE) mask_y = nullptr;
    } else {
        SPRK_REQUIRE(g->C2 == 0 || x2, "conv2d_fwd: C2 > 0 but x2 is null");
        SPRK_REQUIRE(!ep || !ep->scale || ep->shift, "conv2d_fwd: scale without shift");
    }
    hipStream_t s = (hipStream_t)stream;
    // the kernels without a masked epilogue: the mask is an in-place pass over the finished gradient
    auto masked = [&](int rc) { return (rc || !mask_y) ? rc : mask_in_place(y, mask_y, mask_act, g, s); };

    FwdPlan p;
    const FwdVariant v = fwd_route(bwd, g, ep, x, x2, y, mask_y, &p, unrot);
    if (!sprk::wprep_describing()) t_last_fwd[bwd ? 1 : 0] = v;   // (a describing call launches nothing)

    if (v.stage == SPRK_STAGE_DIRECT || v.stage == SPRK_STAGE_STEM) {
        if (sprk::wprep_describing()) return SPRK_OK;   // no weight transform on this path
        if (bwd) {
            DirectArgs a{nullptr, nullptr, w, x, y, *g, sprk::kNoEpilogue};
            StemPlan sp;
            if (v.stage == SPRK_STAGE_STEM && plan_stem_bwd(g, &sp)) {   // the same sums from LDS copies of both operands
                hipLaunchKernelGGL(conv_bwd_data_stem_kernel, dim3(g->N * sp.tilesX * sp.tilesY), dim3(kStemTW * kStemTH),
                                   sp.ldsBytes, s, a, sp.wr, sp.wc, sp.tilesX, sp.tilesY);
                return masked(sprk::check_launch("conv_bwd_data_stem"));
            }
            const long total = (long)g->N * (g->C1 + g->C2) * g->Hin * g->Win;
            hipLaunchKernelGGL(conv_bwd_data_direct_kernel, dim3(sprk::ew_blocks(total)), dim3(256), 0, s, a);
            return masked(sprk::check_launch("conv_bwd_data_direct"));
        }
        DirectArgs a{x, x2, w, nullptr, y, *g, ep ? *ep : sprk::kNoEpilogue};
        const long total = (long)g->N * g->Cout * g->Hout * g->Wout;
        hipLaunchKernelGGL(conv_fwd_direct_kernel, dim3(sprk::ew_blocks(total)), dim3(256), 0, s, a);
        return sprk::check_launch("conv_fwd_direct");
    }
    const sprk::Corr c = bwd ? sprk::Corr(*g) : sprk::Corr(*g, ep);

    // (a masked epilogue in conv16_tile_kernel<6> takes it from 231 to 256 VGPRs + 92 bytes of scratch — the next
    // tile's fetch is in flight during the stores — and the bf16 step from 11.22 to 11.27 ms: in-place pass)
    if (v.stage == SPRK_STAGE_16BIT) return masked(sprk::conv16_run(c, x, x2, w, y, ws, ws_bytes, s));
    if (int rc = check_storage32(who, c.dtype)) return rc;

    if (v.stage == SPRK_STAGE_WINOGRAD) {
        if (int rc = sprk::check_ws(who, ws, ws_bytes, sprk::wino_ws_bytes(c))) return rc;
        // the mask is d act / d y of the layer that produced this conv's input, applied in the output transform: gin
        // leaves the kernel as that layer's pre-activation gradient
        if (int rc = sprk::wino_conv(c, v.wino, x, x2, w, y, (float *)ws, mask_y, mask_act, s)) return rc;
        return sprk::check_launch(bwd ? "wino_conv(bwd_data)" : "wino_conv");
    }
    SPRK_REQUIRE(!unrot, "conv2d_fwd_unrot: the call left the Winograd stage");

    SPRK_REQUIRE(v.stage != SPRK_STAGE_REFUSED, "%s: geometry does not fit LDS", who);
    if (int rc = sprk::check_ws(who, ws, ws_bytes, p.wsBytes)) return rc;
    float *wsf = (float *)ws;
    if (int rc = transform_weights(w, wsf, g->Cout, g->C1 + g->C2, g->KH * g->KW, c.taps, p, s)) return rc;
    if (v.stage == SPRK_STAGE_MASK1X1) {
        // few reduced channels, 1x1: a streaming kernel of its own with the mask in its store, on the same slabs
        const sprk::Mask1x1Call m{x, wsf + kZeroFloats, mask_y, y, g->N, g->Cout, g->C1, g->Hin * g->Win,
                                  p.CK, p.R4, p.rows, p.ldw, p.NT, p.nblkN, mask_act};
        if (int rc = sprk::mask1x1_run(m, s)) return rc;
        return sprk::check_launch("mask1x1(bwd_data)");
    }
    if (v.stage == SPRK_STAGE_GEMM1X1) {
        // many reduced channels, 1x1, nothing fused: the streaming GEMM on the same slabs (timed with conv_mfma_kernel<4, 6>)
        const sprk::Gemm1x1Call m{x, wsf + kZeroFloats, wsf, c.ep.bias, c.ep.scale, c.ep.shift, y, c.N, c.C1, c.Cout,
                                  c.Hin * c.Win, p.rows, p.ldw, p.nblkN, c.ep.act};
        sprk::prof_begin(0, c.flops, s);
        if (int rc = sprk::gemm1x1_run(m, s)) return rc;
        sprk::prof_end(0, s);
        return sprk::check_launch(bwd ? "gemm1x1(bwd_data)" : "gemm1x1");
    }
    const ConvArgs a = conv_args(c, p, v, x, x2, wsf, y);
    // (a masked epilogue in this kernel costs 26 VGPRs — 160 -> 186, two workgroups per CU instead of three — for
    // every call, masked or not: measured in round 1 and again in round 3; the mask is applied by an in-place pass)
    const int kclass = (v.MT == 4 && v.NT == 6) ? 0 : 2;   // 0: the dominant instantiation conv_mfma_kernel<4, 6>
    sprk::prof_begin(kclass, c.flops, s);
    if (int rc = launch_fwd(a, p, v, s)) return rc;
    sprk::prof_end(kclass, s);
    return masked(sprk::check_launch(bwd ? "conv_mfma(bwd_data)" : "conv_mfma"));
}

int sprk_conv2d_fwd(const float *x, const float *x2, const float *w, float *y, const sprk_conv_geom *g,
                    const sprk_conv_epilogue *ep, void *ws, size_t ws_bytes, void *stream) {
    sprk::WprepScope scope(nullptr, g ? g->dtype : 0);
    return scope.verify(conv_dispatch(false, x, x2, w, y, g, ep, nullptr, SPRK_ACT_NONE, ws, ws_bytes, stream));
}

// 1: sprk_conv2d_fwd_unrot runs for this layer — the call would reach the fp32 Winograd stage of conv_dispatch (no
// SPRK_DT_NAIVE, fp32 operands and tensors) and the kernel has the store (wino_unrot_eligible: a 4-rotation stack of
// 64 x 64 planes, 49..96 output channels, no fused up-sampling or residual)
int sprk_conv2d_fwd_unrot_eligible(const sprk_conv_geom *g, const sprk_conv_epilogue *ep) {
    if (!g || check_geom(g) || naive_of(g)) return 0;
    const sprk::Corr c(*g, ep);
    if (c.dt() != SPRK_DT_F32 || c.x16() || c.y16()) return 0;
    return sprk::wino_unrot_eligible(c) ? 1 : 0;
}

int sprk_conv2d_fwd_unrot(const float *x, const float *x2, const float *w, float *f, const sprk_conv_geom *g,
                          const sprk_conv_epilogue *ep, void *ws, size_t ws_bytes, void *stream) {
    sprk::WprepScope scope(nullptr, g ? g->dtype : 0);
    return scope.verify(conv_dispatch(false, x, x2, w, f, g, ep, nullptr, SPRK_ACT_NONE, ws, ws_bytes, stream, true));
}

int sprk_conv2d_fwd_wprep(const float *w, const sprk_conv_geom *g, const sprk_conv_epilogue *ep, void *ws,
                          size_t ws_bytes, sprk_wprep_item *item) {
    SPRK_REQUIRE(item && w && ws, "conv2d_fwd_wprep: null argument");
    *item = sprk_wprep_item{};
    sprk::WprepScope scope(item, 0);
    // the tensors are never touched in describe mode: the call ends at its weight-transform site
    const float *dummy = (const float *)ws;
    const int rc = conv_dispatch(false, dummy, g && g->C2 ? dummy : nullptr, w, (float *)ws, g, ep, nullptr, SPRK_ACT_NONE,
                                 ws, ws_bytes, nullptr);
    return rc == sprk::kWprepDescribed ? (int)SPRK_OK : rc;
}

int sprk_conv2d_bwd_data(const float *gy, const float *w, float *gin, const sprk_conv_geom *g, void *ws,
                         size_t ws_bytes, void *stream) {
    return sprk_conv2d_bwd_data_masked(gy, w, gin, g, nullptr, SPRK_ACT_NONE, ws, ws_bytes, stream);
}

int sprk_conv2d_bwd_data_masked(const float *gy, const float *w, float *gin, const sprk_conv_geom *g,
                                const float *mask_y, int mask_act, void *ws, size_t ws_bytes, void *stream) {
    sprk::WprepScope scope(nullptr, g ? g->dtype : 0);
    return scope.verify(conv_dispatch(true, gy, nullptr, w, gin, g, nullptr, mask_y, mask_act, ws, ws_bytes, stream));
}

// conv_dispatch's stages for a masked backward-data call of g, by their own predicates, in their order
int sprk_conv2d_bwd_data_mask_fused(const sprk_conv_geom *g) {
    if (!g || check_geom(g) != SPRK_OK || naive_of(g) || g->stride != 1 || g->up1) return 0;
    const sprk::Corr c(*g);
    if (c.dt() != SPRK_DT_F32 && sprk::conv16_eligible(c)) return 0;
    if (c.dtype & (SPRK_DT_X16 | SPRK_DT_Y16)) return 0;
    if (sprk::wino_eligible(c)) return 1;
    FwdPlan p;
    return (plan_fwd(c, &p) && mask1x1_takes(g, c, p)) ? 1 : 0;
}

int sprk_conv2d_bwd_data_wprep(const float *w, const sprk_conv_geom *g, void *ws, size_t ws_bytes, sprk_wprep_item *item) {
    SPRK_REQUIRE(item && w && ws, "conv2d_bwd_data_wprep: null argument");
    *item = sprk_wprep_item{};
    sprk::WprepScope scope(item, 0);
    const int rc = conv_dispatch(true, (const float *)ws, nullptr, w, (float *)ws, g, nullptr, nullptr, SPRK_ACT_NONE, ws,
                                 ws_bytes, nullptr);
    return rc == sprk::kWprepDescribed ? (int)SPRK_OK : rc;
}

// What a backward-weight call of g can ask for: the maximum over the stages of wgrad_dispatch that take a workspace,
// by the predicates and sizes the dispatcher itself uses.  SPRK_DT_NAIVE is ignored (the direct kernel needs none):
// ops.py and the graph stepper size long-lived buffers by this, whatever flags a later call carries.
static size_t wgrad_ws_bytes(const sprk_conv_geom &g) {
    size_t need = sprk::wgrad16_ws_bytes(g);
    WgPlan p;
    if (sprk::wino_wgrad_eligible(g)) need = std::max(need, sprk::wino_wgrad_ws_bytes(g));
    if (plan_wgrad(&g, &p)) need = std::max(need, p.wsBytes);
    return need;
}

size_t sprk_conv2d_bwd_weight_ws_bytes(const sprk_conv_geom *g) { return g ? wgrad_ws_bytes(*g) : 0; }

// Stage 7: may the call of layer g, planned as p and routed to conv_wgrad_mfma_kernel as v, run on wgrad1x1_kernel
// (wgrad1x1.hip) instead?  An fp32 1x1 call in the row form (MODE 1: x and gy 16-byte aligned, 32-bit offsets) on the plan
// of the wide heads (3 k-tiles per wave, blocks of 6 output tiles), over planes whose 64-pixel tiles are 64 consecutive
// floats of one plane.  The one predicate of wg_route, and so of the dispatcher and of sprk_conv2d_variant.
static bool wgrad1x1_takes(const sprk_conv_geom *g, const WgPlan &p, const WgVariant &v) {
    const int W = g->Wout, H = g->Hout;
    const bool rows64 = W % 64 == 0 || ((W == 4 || W == 8 || W == 16 || W == 32) && H % (64 / W) == 0 && H * W >= 64);
    return sprk::g_wgrad1x1_on.load(std::memory_order_relaxed) && (g->dtype & SPRK_DT_MASK) == SPRK_DT_F32 &&
           !(g->dtype & (SPRK_DT_X16 | SPRK_DT_Y16)) && !naive_of(g) && g->KH == 1 && g->KW == 1 && g->stride == 1 &&
           g->pad_top == 0 && g->pad_left == 0 && g->C2 == 0 && !g->up1 && g->Hin == g->Hout && g->Win == g->Wout &&
           v.stage == SPRK_STAGE_MFMA && p.xrow && v.MODE == 1 && p.IT == 3 && p.NT == 6 && p.CKW <= sprk::kWgrad1x1Rows &&
           rows64 && (long)sprk::kWgrad1x1Rows * H * W * 4 < (1L << 31);
}

// Stage 8: may the call of layer g, planned as p and routed to conv_wgrad_mfma_kernel as v, run on wgrad3x3_kernel
// (wgrad3x3.hip) instead?  An fp32 3x3 stride-1 same-size call in MODE 2 (x, x2 and gy 16-byte aligned, 32-bit offsets)
// whose plan has chunks of 48 input channels (27 k-tiles: IT = 7; none straddles the two sources) and blocks of 3 or 6
// output tiles, over planes of 16, 32 or 64 columns and whole tiles of 4, 2 or 1 rows.
static bool wgrad3x3_takes(const sprk_conv_geom *g, const WgPlan &p, const WgVariant &v) {
    return sprk::g_wgrad3x3_on.load(std::memory_order_relaxed) && (g->dtype & SPRK_DT_MASK) == SPRK_DT_F32 &&
           !(g->dtype & (SPRK_DT_X16 | SPRK_DT_Y16)) && !naive_of(g) && g->KH == 3 && g->KW == 3 && g->stride == 1 &&
           g->dil == 1 && !g->up1 && g->Hin == g->Hout && g->Win == g->Wout && g->pad_top >= 0 && g->pad_top <= 2 &&
           g->pad_left >= 0 && g->pad_left <= 2 && v.stage == SPRK_STAGE_MFMA && v.MODE == 2 && p.IT == 7 &&
           (p.NT == 3 || p.NT == 6) && p.CKW == sprk::kWgrad3x3Chunk && g->C1 % p.CKW == 0 && g->C2 % p.CKW == 0 &&
           sprk::wgrad3x3_plane(g->Hout, g->Wout) && (1 << p.lgTC) == g->Wout && (64 >> p.lgTC) == (1 << p.lgTR);
}

// Which stage of wgrad_dispatch takes the call, by the stages' own predicates in the dispatcher's order, and for the
// MFMA stage the plan and the kernel variant: the twin of fwd_route.
static WgVariant wg_route(const sprk_conv_geom *g, const void *x, const void *x2, const void *gy, WgPlan *p) {
    WgVariant v{};
    const bool naive = naive_of(g);   // skips the kernels, not the storage guard: the direct kernel reads fp32 tensors
    if (!naive && sprk::wgrad16_ws_bytes(*g)) {   // eligible (never with fp32 operands)
        v.stage = SPRK_STAGE_16BIT;
        sprk::wgrad16_variant(*g, v.rec16);
    } else if (g->dtype & (SPRK_DT_X16 | SPRK_DT_Y16)) {
        v.stage = SPRK_STAGE_REFUSED;   // the storage guard
    } else if (!naive && sprk::wino_wgrad_eligible(*g)) {
        v.stage = SPRK_STAGE_WINOGRAD;
        v.wino = sprk::wino_wgrad_variant(*g);
    } else if (naive || !plan_wgrad(g, p)) {
        v.stage = SPRK_STAGE_DIRECT;
    } else {
        bool refused;
        v = wg_variant(g, *p, x, x2, gy, &refused);
        v.stage = refused ? SPRK_STAGE_REFUSED : SPRK_STAGE_MFMA;
        if (wgrad1x1_takes(g, *p, v)) v.stage = SPRK_STAGE_WGRAD1X1;
        else if (wgrad3x3_takes(g, *p, v)) v.stage = SPRK_STAGE_WGRAD3X3;
    }
    return v;
}

// The one place where a backward-weight call meets its kernel, the twin of conv_dispatch; the layer's sprk_conv_geom is
// the common description, and a kernel family is a predicate, a workspace size and a run function over it (DESIGN.md,
// "The convolution dispatcher").  item == nullptr: finish the sum over the partial buffers now; otherwise describe it in
// *item (sprk.h).  The stages, in order:
//   direct kernel (SPRK_DT_NAIVE) -> 16-bit operands -> storage guard -> Winograd -> MFMA (-> direct: no plan fits LDS),
//   whose wide 1x1 row-form calls leave for wgrad1x1_kernel on the same plan (SPRK_STAGE_WGRAD1X1), and whose 3x3 calls
//   on chunks of 48 channels for wgrad3x3_kernel (SPRK_STAGE_WGRAD3X3)
static int wgrad_dispatch(const float *x, const float *x2, const float *gy, float *gw, const sprk_conv_geom *g, void *ws,
                          size_t ws_bytes, sprk_reduce_item *item, void *stream) {
    const char *who = "conv2d_bwd_weight";
    if (item) *item = sprk_reduce_item{nullptr, nullptr, SPRK_RED_NONE, 0, 0, 0, 0, 0};
    if (int rc = check_geom(g)) return rc;
    SPRK_REQUIRE(x && gy && gw, "conv2d_bwd_weight: null tensor");
    SPRK_REQUIRE(g->C2 == 0 || x2, "conv2d_bwd_weight: C2 > 0 but x2 is null");
    hipStream_t s = (hipStream_t)stream;

    WgPlan p;
    const WgVariant v = wg_route(g, x, x2, gy, &p);
    t_last_wg = v;

    if (v.stage == SPRK_STAGE_16BIT) {
        if (int rc = sprk::check_ws(who, ws, ws_bytes, sprk::wgrad16_ws_bytes(*g))) return rc;
        return sprk::wgrad16_run(*g, x, x2, gy, gw, ws, item, s);
    }
    if (int rc = check_storage32(who, g->dtype)) return rc;

    if (v.stage == SPRK_STAGE_WINOGRAD) {
        if (int rc = sprk::check_ws(who, ws, ws_bytes, sprk::wino_wgrad_ws_bytes(*g))) return rc;
        return sprk::wino_wgrad(*g, v.wino, x, x2, gy, gw, ws, item, s);
    }

    if (v.stage == SPRK_STAGE_DIRECT) {
        DirectArgs a{x, x2, nullptr, gy, gw, *g, sprk::kNoEpilogue};
        hipLaunchKernelGGL(conv_bwd_weight_direct_kernel, dim3(g->Cout * (g->C1 + g->C2)), dim3(256), 0, s, a);
        return sprk::check_launch("conv_bwd_weight_direct");
    }
    if (int rc = sprk::check_ws(who, ws, ws_bytes, p.wsBytes)) return rc;
    SPRK_REQUIRE(v.stage != SPRK_STAGE_REFUSED,
                 "conv2d_bwd_weight: 1x1 row staging needs 16-byte aligned x / gy and < 2^28-element tiles");
    float *wsf = (float *)ws;
    if (v.stage == SPRK_STAGE_WGRAD1X1) {
        // the same split, slabs and reduction item as the MFMA stage below
        const sprk::Wgrad1x1Call c{x, gy, wsf + kZeroFloats, g->N, g->C1, g->Cout, p.CoutP, g->Hout * g->Wout,
                                   p.nTiles, p.tilesPerGroup, p.groups, p.CKW, p.nChunks, p.nblkN};
        sprk::prof_begin(1, sprk::conv_flops(*g), s);
        if (int rc = sprk::wgrad1x1_run(c, s)) return rc;
        sprk::prof_end(1, s);
        if (int rc2 = sprk::check_launch("wgrad1x1")) return rc2;
    } else if (v.stage == SPRK_STAGE_WGRAD3X3) {
        // the same split, slabs and reduction item as the MFMA stage below
        const sprk::Wgrad3x3Call c{x, x2, gy, wsf + kZeroFloats, g->N, g->C1, g->C2, g->Cout, p.CoutP, g->Hout, g->Wout,
                                   g->pad_top, g->pad_left, p.NT, p.nTiles, p.tilesPerGroup, p.groups, p.nChunks, p.nblkN};
        sprk::prof_begin(1, sprk::conv_flops(*g), s);
        if (int rc = sprk::wgrad3x3_run(c, s)) return rc;
        sprk::prof_end(1, s);
        if (int rc2 = sprk::check_launch("wgrad3x3")) return rc2;
    } else {
        WgArgs a;
        if (int rc = wgrad_args(g, p, v, x, x2, gy, wsf, a)) return rc;
        sprk::prof_begin(1, sprk::conv_flops(*g), s);
        if (int rc = launch_wg(a, p, v, s)) return rc;
        sprk::prof_end(1, s);
        if (int rc2 = sprk::check_launch("conv_wgrad_mfma")) return rc2;
    }
    const int K = (g->C1 + g->C2) * g->KH * g->KW;
    const sprk_reduce_item it{wsf + kZeroFloats, gw, SPRK_RED_WGRAD, p.groups, 0, K, g->Cout, p.CoutP};
    return sprk::finish_or_defer(it, item, s);
}

// ---- which kernel variant: the query and the record of the last call --------------------------------------------------
static void variant_out(const FwdVariant &v, int32_t *out) {
    if (v.stage == SPRK_STAGE_16BIT) {
        out[0] = v.stage;
        for (int i = 1; i < SPRK_VARIANT_INTS; ++i) out[i] = v.rec16[i];
        return;
    }
    if (v.stage == SPRK_STAGE_WINOGRAD) {
        const sprk::WinoVariant &w = v.wino;
        const int f[] = {v.stage, w.NT, w.SQ, w.UNROT, w.groups, w.lastCh, w.nc1, w.nch, w.r1, w.r2, w.pairs, w.sw, w.gridX,
                         w.ntiles, w.tpwMin, w.tpwMax, w.xcd, w.tilesX, w.tilesY, w.padT, w.padL, w.mode};
        static_assert(sizeof(f) / sizeof(f[0]) <= SPRK_VARIANT_INTS, "the record fits");
        for (int i = 0; i < SPRK_VARIANT_INTS; ++i) out[i] = i < (int)(sizeof(f) / sizeof(f[0])) ? f[i] : 0;
        return;
    }
    const int f[] = {v.stage, v.MT, v.NT, v.RB, v.XTAB, v.small, v.stages, v.ragged_k, v.latency, v.vec1, v.vec2, v.vec4,
                     v.colOff, v.up1, v.c2, v.taps, v.CK, v.nChunks, v.blocks};
    for (int i = 0; i < SPRK_VARIANT_INTS; ++i) out[i] = i < (int)(sizeof(f) / sizeof(f[0])) ? f[i] : 0;
}
static void variant_out(const WgVariant &v, int32_t *out) {
    if (v.stage == SPRK_STAGE_16BIT) {
        out[0] = v.stage;
        for (int i = 1; i < SPRK_VARIANT_INTS; ++i) out[i] = v.rec16[i];
        return;
    }
    if (v.stage == SPRK_STAGE_WINOGRAD) {
        const sprk::WinoWgVariant &w = v.wino;
        int f[SPRK_VARIANT_INTS] = {v.stage, w.launches};
        for (int i = 0; i < w.launches; ++i) f[2 + 3 * i] = w.l[i].MT, f[3 + 3 * i] = w.l[i].ch, f[4 + 3 * i] = w.l[i].parts;
        int srcMask = 0;
        for (int i = 0; i < w.launches; ++i) srcMask |= w.l[i].src << i;
        const int t[] = {w.regionsX, w.regionsY, w.cx, w.cy, w.padT, w.padL, w.Cout, w.xcdMask, srcMask};
        static_assert(14 + sizeof(t) / sizeof(t[0]) <= SPRK_VARIANT_INTS, "the record fits");
        for (int i = 0; i < (int)(sizeof(t) / sizeof(t[0])); ++i) f[14 + i] = t[i];
        for (int i = 0; i < SPRK_VARIANT_INTS; ++i) out[i] = f[i];
        return;
    }
    const int f[] = {v.stage, v.IT, v.NT, v.WJ, v.MODE, v.xrow, v.xtab, v.g4, v.vec1, v.vec2, v.chunks, v.groups, v.up1, v.c2,
                     v.tiles};
    for (int i = 0; i < SPRK_VARIANT_INTS; ++i) out[i] = i < (int)(sizeof(f) / sizeof(f[0])) ? f[i] : 0;
}

int sprk_conv2d_variant(int which, const sprk_conv_geom *g, const sprk_conv_epilogue *ep, const void *x, const void *x2,
                        const void *y_or_gy, int32_t *out) {
    SPRK_REQUIRE(out && which >= 0 && which <= 2, "conv2d_variant: which is 0 (forward), 1 (backward-data) or 2 (backward-weight)");
    if (int rc = check_geom(g)) return rc;
    if (which == 2) {
        WgPlan p;
        variant_out(wg_route(g, x, x2, y_or_gy, &p), out);
    } else {
        FwdPlan p;
        // backward-data: the correlation reads gy and writes gin (here: x)
        variant_out(which == 0 ? fwd_route(false, g, ep, x, x2, y_or_gy, nullptr, &p)
                               : fwd_route(true, g, nullptr, y_or_gy, nullptr, x, nullptr, &p), out);
    }
    return SPRK_OK;
}

int sprk_conv2d_last_variant(int which, int32_t *out) {
    SPRK_REQUIRE(out && which >= 0 && which <= 2, "conv2d_last_variant: which is 0 (forward), 1 (backward-data) or 2 (backward-weight)");
    if (which == 2)
        variant_out(t_last_wg, out);
    else
        variant_out(t_last_fwd[which], out);
    return SPRK_OK;
}

int sprk_conv2d_bwd_weight(const float *x, const float *x2, const float *gy, float *gw, const sprk_conv_geom *g,
                           void *ws, size_t ws_bytes, void *stream) {
    return wgrad_dispatch(x, x2, gy, gw, g, ws, ws_bytes, nullptr, stream);
}

int sprk_conv2d_bwd_weight_partial(const float *x, const float *x2, const float *gy, float *gw, const sprk_conv_geom *g,
                                   void *ws, size_t ws_bytes, sprk_reduce_item *item, void *stream) {
    return wgrad_dispatch(x, x2, gy, gw, g, ws, ws_bytes, item, stream);
}

static int act_nsplit(int N, int C) {
    int ns = 1;
    while (ns < N && (long)C * ns < 1024) ns <<= 1;
    return std::min(ns, N);
}

size_t sprk_act_bwd_ws_bytes(int N, int C, int HW) {
    (void)HW;
    return (size_t)C * act_nsplit(N, C) * sizeof(float);
}

int sprk_act_bwd(const void *g, const void *y, void *gpre, float *gbias, int act, int N, int C, int H, int W,
                 int up2, long g_image_stride, int io, void *ws, size_t ws_bytes, void *stream) {
    return sprk_act_bwd_partial(g, y, gpre, gbias, act, N, C, H, W, up2, g_image_stride, io, ws, ws_bytes, nullptr, stream);
}

int sprk_act_bwd_partial(const void *g, const void *y, void *gpre, float *gbias, int act, int N, int C, int H, int W,
                         int up2, long g_image_stride, int io, void *ws, size_t ws_bytes, sprk_reduce_item *item,
                         void *stream) {
    if (item) *item = sprk_reduce_item{nullptr, nullptr, SPRK_RED_NONE, 0, 0, 0, 0, 0};
    SPRK_REQUIRE(g && N > 0 && C > 0 && H > 0 && W > 0, "act_bwd: bad arguments");
    SPRK_REQUIRE(act == SPRK_ACT_NONE || (y && gpre), "act_bwd: activation needs the saved output and gpre");
    SPRK_REQUIRE(!up2 || (gpre && gpre != g), "act_bwd: up2 needs a separate low-resolution gpre");
    hipStream_t s = (hipStream_t)stream;
    const bool retype = gpre && (io & 15) != ((io >> 8) & 15);    // gpre has another storage type than gy
    SPRK_REQUIRE(!retype || gpre != g, "act_bwd: a change of storage type needs a separate gpre");
    if (act == SPRK_ACT_NONE && !gbias && !up2 && !retype) return SPRK_OK;
    const int ns = act_nsplit(N, C);
    if (gbias && (ws_bytes < (size_t)C * ns * sizeof(float) || !ws)) {
        sprk::set_error("act_bwd: workspace too small");
        return SPRK_EWORKSPACE;
    }
    const long dense = (long)C * H * W * (up2 ? 4 : 1);
    const long gs = g_image_stride ? g_image_stride : dense;
    SPRK_REQUIRE(gs >= dense, "act_bwd: image stride of gy smaller than one image");
    SPRK_REQUIRE(gs == dense || (gpre && gpre != g), "act_bwd: a strided gy needs a separate gpre");
    const int drc = dispatch_io3(io, [&](auto tg, auto ty, auto to) {
        using TG = decltype(tg);
        using TY = decltype(ty);
        using TO = decltype(to);
        hipLaunchKernelGGL((act_bwd_kernel<TG, TY, TO>), dim3(C, ns), dim3(256), 0, s, (const TG *)g, (const TY *)y, (TO *)gpre,
                           gbias ? (float *)ws : nullptr, act, N, C, H * W, W, up2, ns, gs);
        return 0;
    });
    SPRK_REQUIRE(drc == 0, "act_bwd: bad storage types (io)");
    if (int rc = sprk::check_launch("act_bwd")) return rc;
    if (gbias) {
        const sprk_reduce_item it{(const float *)ws, gbias, SPRK_RED_COLS, ns, C, 0, 0, 0};
        return sprk::finish_or_defer(it, item, s);
    }
    return SPRK_OK;
}

int sprk_unrot_act_bwd_eligible(int B, int C, int P, int act) {
    return B > 0 && C > 0 && P == 64 && (act == SPRK_ACT_LEAKY || act == SPRK_ACT_RELU);
}

int sprk_unrot_act_bwd(const float *gf, const float *f, float *gpre, float *gbias, int act, int B, int C, int P,
                       void *ws, size_t ws_bytes, sprk_reduce_item *item, void *stream) {
    if (item) *item = sprk_reduce_item{nullptr, nullptr, SPRK_RED_NONE, 0, 0, 0, 0, 0};
    SPRK_REQUIRE(gf && f && gpre && gpre != gf && gpre != f, "unrot_act_bwd: null or aliased tensor");
    SPRK_REQUIRE(sprk_unrot_act_bwd_eligible(B, C, P, act), "unrot_act_bwd: needs P == 64 and an activation (B %d, C %d, P %d, act %d)",
                 B, C, P, act);
    SPRK_REQUIRE((((uintptr_t)gf | (uintptr_t)f | (uintptr_t)gpre) & 15) == 0, "unrot_act_bwd: tensors must be 16-byte aligned");
    const int N = 4 * B, ns = act_nsplit(N, C);
    if (gbias && (ws_bytes < (size_t)C * ns * sizeof(float) || !ws)) {
        sprk::set_error("unrot_act_bwd: workspace too small");
        return SPRK_EWORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(unrot_act_bwd64_kernel, dim3(C, ns), dim3(256), 0, s, gf, f, gpre, gbias ? (float *)ws : nullptr, act,
                       B, C, ns);
    if (int rc = sprk::check_launch("unrot_act_bwd")) return rc;
    if (gbias) {
        const sprk_reduce_item it{(const float *)ws, gbias, SPRK_RED_COLS, ns, C, 0, 0, 0};
        return sprk::finish_or_defer(it, item, s);
    }
    return SPRK_OK;
}

int sprk_concat_up_bwd(const float *gin, float *ga, float *gb, int N, int C1, int C2, int H, int W, int up1,
                       void *stream) {
    SPRK_REQUIRE(gin && N > 0 && C1 >= 0 && C2 >= 0 && H > 0 && W > 0, "concat_up_bwd: bad arguments");
    SPRK_REQUIRE((C1 == 0 || ga) && (C2 == 0 || gb), "concat_up_bwd: null output");
    SPRK_REQUIRE(!up1 || (H % 2 == 0 && W % 2 == 0), "concat_up_bwd: odd size with upsampling");
    const long total = (long)N * C1 * (up1 ? (H / 2) * (W / 2) : H * W) + (long)N * C2 * H * W;
    hipLaunchKernelGGL(concat_up_bwd_kernel, dim3(sprk::ew_blocks(total)), dim3(256), 0, (hipStream_t)stream, gin, ga,
                       gb, N, C1, C2, H, W, up1);
    return sprk::check_launch("concat_up_bwd");
}

}  // extern "C"
