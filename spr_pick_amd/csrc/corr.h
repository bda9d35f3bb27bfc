// One forward-shaped correlation: what the convolution dispatcher of conv.hip (conv_dispatch) and the kernel families
// behind it (conv16.hip, wino.hip, the MFMA kernels of conv.hip) are handed.  Host only, not part of the ABI.
#pragma once
#include "common.h"

namespace sprk {

constexpr sprk_conv_epilogue kNoEpilogue = {nullptr, nullptr, nullptr, nullptr, 0, 0, 0, SPRK_ACT_NONE, 0};

// y[N,Cout,Hout,Wout] = epilogue(correlation of cat(x[N,C1], x2[N,C2]) with the taps)
struct Corr {
    int N, C1, C2, Hin, Win, up1, Cout, Hout, Wout, KH, KW, stride, dil, padT, padL;
    int taps;       // layout of w: 0 = w[Cout][C1+C2][KH][KW]; 1 = the FORWARD layer's w[C1][Cout][KH][KW] (this call's k
                    // channels are its output channels), read channel-transposed with the taps flipped
    int dtype;      // the call's sprk_conv_geom.dtype, flag bits included
    int mfma_only;  // backward-data of a layer that up-samples its input: the 16-bit and Winograd kernels do not take it
    sprk_conv_epilogue ep;   // empty for backward-data
    double flops;   // conv_flops() of the layer

    // a forward call (ep may be null)
    Corr(const sprk_conv_geom &g, const sprk_conv_epilogue *e)
        : N(g.N), C1(g.C1), C2(g.C2), Hin(g.Hin), Win(g.Win), up1(g.up1), Cout(g.Cout), Hout(g.Hout), Wout(g.Wout),
          KH(g.KH), KW(g.KW), stride(g.stride), dil(g.dil), padT(g.pad_top), padL(g.pad_left), taps(0), dtype(g.dtype),
          mfma_only(0), ep(e ? *e : kNoEpilogue), flops(conv_flops(g)) {}
    // backward-data of a stride-1 layer: gin is the correlation of gy with the flipped, channel-transposed taps, the
    // padding mirrored.  The only place that knows this mapping.  A strided layer has no such view: the
    // dispatcher sends it to the direct kernel first, and the stride is carried through so that the 16-bit and Winograd
    // stages decline it like any other strided correlation.
    explicit Corr(const sprk_conv_geom &g)
        : N(g.N), C1(g.Cout), C2(0), Hin(g.Hout), Win(g.Wout), up1(0), Cout(g.C1 + g.C2), Hout(g.Hin), Wout(g.Win),
          KH(g.KH), KW(g.KW), stride(g.stride), dil(g.dil), padT((g.KH - 1) * g.dil - g.pad_top),
          padL((g.KW - 1) * g.dil - g.pad_left), taps(1), dtype(g.dtype), mfma_only(g.up1), ep(kNoEpilogue),
          flops(conv_flops(g)) {}

    int dt() const { return dtype & SPRK_DT_MASK; }
    bool x16() const { return (dtype & SPRK_DT_X16) != 0; }   // x, x2 are 16-bit tensors of the operand type
    bool y16() const { return (dtype & SPRK_DT_Y16) != 0; }   // y is
    bool pin() const { return (dtype & SPRK_DT_PIN) != 0; }   // the choice must not depend on the image count or the plane size
};

}  // namespace sprk
