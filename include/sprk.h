/* sprk.h — C ABI of libsprk.so: the MI355X (gfx950) kernels behind spr_pick's joint
 * denoise+detect hot path.
 *
 * The reference (nextpyp/spr_pick) has no FFI on this path: it calls stock torch.nn /
 * NumPy from Python.  Each entry point below therefore replaces a *torch or NumPy call
 * site* of the reference (cited per function as file:line under /root/reference) and
 * is what a maintainer binds with ctypes from the reference's Python modules — see
 * INTEGRATION.md for the stubs.
 *
 * Conventions
 *   - all tensors are fp32, contiguous NCHW, DEVICE pointers (unless marked host);
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous on it and
 *     re-entrant per stream; nothing is allocated or synchronised inside;
 *   - the caller owns every buffer incl. the workspace `ws` (size from *_ws_bytes);
 *   - return 0 on success, a negative SPRK_E* code otherwise; sprk_last_error() gives
 *     a thread-local message.
 */
#ifndef SPRK_H
#define SPRK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPRK_OK 0
#define SPRK_EINVAL (-1)   /* bad argument / unsupported geometry */
#define SPRK_EWORKSPACE (-2) /* workspace too small */
#define SPRK_ELAUNCH (-3)  /* hip launch error */

#define SPRK_ACT_NONE 0
#define SPRK_ACT_LEAKY 1   /* LeakyReLU(0.1) */
#define SPRK_ACT_RELU 2

/* Geometry of one 2-D convolution  y[N,Cout,Hout,Wout] = conv(in[N,C1+C2,Hin,Win], w).
 * The conv input is the channel concatenation of up to two sources:
 *   src1: x  [N,C1,Hin,Win]           (up1 = 0)
 *         x  [N,C1,Hin/2,Win/2]       (up1 = 1: nearest x2 upsampling fused into the load)
 *   src2: x2 [N,C2,Hin,Win]           (C2 may be 0, x2 NULL)
 * which is torch.cat((Upsample(2)(a), skip), 1) of the reference's U-Nets
 * (models/joint_network_v2.py:212-227) without materialising it.
 * Padding is asymmetric and explicit: rows/cols outside [0,Hin)x[0,Win) read as zero,
 * Hout/Wout are given by the caller.  ShiftConv2d (joint_network_v2.py:565-584) is
 * pad_top = 2*(KH/2), pad_left = KW/2, Hout = Hin, Wout = Win. */
typedef struct sprk_conv_geom {
    int32_t N, C1, C2, Hin, Win, up1;
    int32_t Cout, Hout, Wout;
    int32_t KH, KW, stride, dil, pad_top, pad_left;
    int32_t dtype;   /* SPRK_DT_*: precision of the MFMA OPERANDS (see below); tensors are fp32 either way */
} sprk_conv_geom;

/* Operand precision of the matrix-core convolutions (BASELINE configs[4]: "fp16 MFMA conv").
 * SPRK_DT_F32 (0, the default): v_mfma_f32_16x16x4_f32 — exact fp32 products, what every parity figure of the fp32
 * path refers to.  SPRK_DT_BF16 / SPRK_DT_F16: the two operands of each product (activation or gradient, and
 * weight) are rounded to bf16 / fp16 on their way into v_mfma_f32_16x16x32_{bf16,f16}; products and sums are fp32;
 * inputs, outputs, master weights and weight gradients stay fp32 tensors.  It is a REQUEST: layers the 16-bit
 * kernels do not cover (strided / dilated / tiny detector layers, < 33 output channels, maps below 16x16) run in
 * fp32; sprk_conv16_launch_count() tells which path ran.  Error bound per output: 2u * sum_k |a_k w_k| with
 * u = 2^-8 (bf16) / 2^-11 (fp16). */
#define SPRK_DT_F32 0
#define SPRK_DT_BF16 1
#define SPRK_DT_F16 2
#define SPRK_DT_MASK 0xff
/* or-ed into dtype: take the 16-bit kernel for every layer it covers, also where the library's own choice would be
 * the fp32 Winograd kernel because it is faster there (wide 3x3 layers on planes >= 64x64); used by the parity tests */
#define SPRK_DT_FORCE 0x100
/* or-ed into dtype: run this call on the plain per-output-element kernels (no MFMA, no Winograd): the on-device
 * cross-check the parity tests use.  Per call — the library keeps no mode switch. */
#define SPRK_DT_NAIVE 0x200
/* or-ed into dtype: PIN the algorithm to the layer's structure — the choice between the Winograd and the direct kernel
 * (whose fp32 results differ in the last bits) then depends only on kernel size, channel counts and the divisibility
 * of the plane (H % 8, W % 32 | H % 16, W % 16), never on how many images or workgroups the call has.  Whole-image and
 * halo-tiled inference set it, so that a window of a micrograph is computed by exactly the arithmetic the whole
 * micrograph gets (bit-identical score maps, hence identical picks; tests/test_gpu_pipeline.py). */
#define SPRK_DT_PIN 0x400
/* 16-bit ACTIVATION tensors in HBM (round 4; BASELINE configs[4]).  With SPRK_DT_BF16 / SPRK_DT_F16 alone the tensors of
 * a call are fp32 and only the MFMA operands are rounded on their way in.  SPRK_DT_X16: the activation INPUTS of the call —
 * x and x2 of a forward call, gy of backward-data, x, x2 AND gy of backward-weight — are tensors of the operand type
 * (the `const float *` parameters then point at 2-byte elements).  SPRK_DT_Y16: the activation OUTPUT — y of forward,
 * gin (and mask_y) of backward-data — is such a tensor: the fp32 accumulator is rounded once, at the store.  Weights,
 * biases, weight gradients and all arithmetic stay fp32.  Only the kernels built for it take these calls
 * (sprk_conv2d_storage16 tells which of a layer's three calls exist); any other geometry returns SPRK_EINVAL. */
#define SPRK_DT_X16 0x8000
#define SPRK_DT_Y16 0x10000
/* element types of the tensors of an elementwise call, 4 bits each: SPRK_DT_F32 / _BF16 / _F16 */
#define SPRK_IO2(a, b) ((a) | ((b) << 4))
#define SPRK_IO3(a, b, c) ((a) | ((b) << 4) | ((c) << 8))

/* Optional fused epilogue of sprk_conv2d_fwd, applied in this order:
 *   v = acc (+ res[n,co,oy+res_off,ox+res_off])            res: [N,Cout,res_h,res_w]
 *   v = scale ? v*scale[co] + shift[co] : v + (bias ? bias[co] : 0)
 *   v = act(v)
 * (residual add + eval-mode BatchNorm affine + ReLU of ResidA, feature_extractor.py:384-416).
 * up2 != 0: y is [N,Cout,2*Hout,2*Wout] and every value is stored to its 2x2 block — the
 * nn.Upsample(scale_factor=2, mode="nearest") that follows the conv in the reference's decoder
 * blocks (joint_network_v2.py:69-97), fused into the store. */
typedef struct sprk_conv_epilogue {
    const float *bias, *scale, *shift, *res;
    int32_t res_h, res_w, res_off;
    int32_t act;
    int32_t up2;
} sprk_conv_epilogue;

/* ABI version: bumped whenever a signature or a struct of this header changes incompatibly (100 = round 1; 300: the
 * geometry carries `dtype`, sprk_act_bwd / sprk_bn_* take the stride / group arguments, the head and prepared-weight
 * entry points exist).  A binding must refuse a library whose sprk_version() differs from the header it was
 * written against, and may compare sprk_struct_bytes(0 | 1 | 2) with its own sizeof(sprk_conv_geom |
 * sprk_conv_epilogue | sprk_reduce_item). */
#define SPRK_ABI_VERSION 430   /* 430: sprk_contam_*; sprk_ingest_*, sprk_extract_boxes, sprk_conv2d_fwd_unrot[_eligible] and
                                * sprk_unrot_act_bwd[_eligible], sprk_conv2d_[last_]variant joined it compatibly (no signature or struct changed:
                                * a binding that needs them finds a library without them by the missing symbol); so did the
                                * Winograd and the 16-bit fields of the variant record, in slots that were documented as 0 */
const char *sprk_last_error(void);
int sprk_version(void);
size_t sprk_struct_bytes(int which);
/* number of HIP kernel launches issued by this library since load (diagnostics) */
long sprk_launch_count(void);
/* number of convolutions (forward or backward-data) that took the Winograd F(2x2,3x3) kernel (diagnostics) */
long sprk_wino_launch_count(void);
/* number of masked backward-data calls that took the 1x1 kernel with the mask in its store (diagnostics / tests) */
long sprk_mask1x1_launch_count(void);
/* number of unmasked forward / backward-data calls of wide 1x1 layers that took the streaming GEMM kernel
 * (SPRK_STAGE_GEMM1X1; diagnostics / tests) */
long sprk_gemm1x1_launch_count(void);
/* process-wide host switch of that stage (default on, never read from the environment): off, those calls keep
 * conv_mfma_kernel (SPRK_STAGE_MFMA) and compute the same bits — the A/B of tests and measurements in one process */
void sprk_gemm1x1_enable(int on);
/* number of backward-weight calls of wide 1x1 layers that took the streaming kernel (SPRK_STAGE_WGRAD1X1; diagnostics /
 * tests) */
long sprk_wgrad1x1_launch_count(void);
/* process-wide host switch of that stage (default on, never read from the environment): off, those calls keep
 * conv_wgrad_mfma_kernel (SPRK_STAGE_MFMA) and compute the same bits */
void sprk_wgrad1x1_enable(int on);
/* number of backward-weight calls of 3x3 layers on chunks of 48 input channels that took the streaming kernel
 * (SPRK_STAGE_WGRAD3X3; diagnostics / tests) */
long sprk_wgrad3x3_launch_count(void);
/* process-wide host switch of that stage (default on, never read from the environment): off, those calls keep
 * conv_wgrad_mfma_kernel (SPRK_STAGE_MFMA) and compute the same bits */
void sprk_wgrad3x3_enable(int on);
/* number of Winograd backward-weight calls (SPRK_STAGE_WINOGRAD) whose launches ran on wino_wgrad_stream_kernel
 * (diagnostics / tests) */
long sprk_wino_wgrad_stream_launch_count(void);
/* process-wide host switch of that kernel (default on, never read from the environment): off, those calls keep
 * wino_wgrad_kernel on the same launches and compute the same bits */
void sprk_wino_wgrad_stream_enable(int on);
/* number of convolution launches (forward, backward-data or backward-weight) that ran on the 16-bit-operand
 * kernels (diagnostics / tests) */
long sprk_conv16_launch_count(void);
/* ... of those, the backward-weight launches */
long sprk_wgrad16_launch_count(void);

/* ---- convolution: replaces F.conv2d/F.pad/crop of nn.Conv2d / ShiftConv2d ------------
 * reference: models/joint_network_v2.py:565-584 (ShiftConv2d), :33-153 (all U-Net convs),
 * models/joint_network_v2_shallow.py:33-150, models/feature_extractor.py:285,335-343,
 * models/classifier.py:11.  w is the reference layout [Cout][C1+C2][KH][KW]. */
size_t sprk_conv2d_fwd_ws_bytes(const sprk_conv_geom *g);
int sprk_conv2d_fwd(const float *x, const float *x2, const float *w, float *y,
                    const sprk_conv_geom *g, const sprk_conv_epilogue *ep,
                    void *ws, size_t ws_bytes, void *stream);
/* gin[N,C1+C2,Hin,Win] = d loss / d (concatenated conv input), given gy = d loss / d (pre-activation y) */
size_t sprk_conv2d_bwd_data_ws_bytes(const sprk_conv_geom *g);
int sprk_conv2d_bwd_data(const float *gy, const float *w, float *gin, const sprk_conv_geom *g,
                         void *ws, size_t ws_bytes, void *stream);
/* ---- fused per-pixel head (inference) ------------------------------------------------------------------------------
 * out = W3 . lrelu(W2 . lrelu(W1 . f + b1) + b2) + b3 in ONE launch, LeakyReLU(0.1): the output_block + output_conv of
 * the blind-spot U-Net (K0 = N1 = 384, N3 = 2: models/joint_network_v2.py:123-153, 241-244) and of the sigma net
 * (K0 = N1 = 96, N3 = 1: models/joint_network_v2_shallow.py).  The middle width is 96.  A 128-pixel tile stays in the
 * workgroup from the input features to the outputs: the two hidden tensors (2 x 25.8 GB at 4096^2) never reach HBM.
 * f [B,K0,HW], w1 [N1,K0], w2 [96,N1], w3 [N3,96] (the reference's [Cout,Cin,1,1] layouts), out [B,N3,HW]; HW % 128 == 0.
 * Same channel order in every sum as three sprk_conv2d_fwd calls, another tiling: results agree to fp32 rounding.
 * Training keeps the three calls (the hidden activations are needed by the weight gradients). */
size_t sprk_head1x1_fwd_ws_bytes(int K0, int N1);
int sprk_head1x1_fwd(const float *f, const float *w1, const float *b1, const float *w2, const float *b2,
                     const float *w3, const float *b3, float *out, int B, int K0, int N1, int N3, long HW, void *ws,
                     size_t ws_bytes, void *stream);

/* The blind-spot head reading the rotated stack itself: d [4B,C=96,P,P] (the output of decode_block_1) -> out [B,N3,P,P].
 * Shift2d((1,0)) + chunk(4) + rotate({0,270,180,90}) + cat(dim=1) (joint_network_v2.py:230-239, i.e.
 * sprk_unrot4_shift_concat_fwd) are the address computation of the kernel's input gather: the [B,384,P,P] feature tensor
 * (25.8 GB at 4096^2) is neither written nor read.  Same arithmetic as unrot + sprk_head1x1_fwd: bit-identical. */
int sprk_head1x1_unrot_fwd(const float *d, const float *w1, const float *b1, const float *w2, const float *b2,
                           const float *w3, const float *b3, float *out, int B, int C, int P, int N3, void *ws,
                           size_t ws_bytes, void *stream);

/* The same with the activation backward of the layer that PRODUCED this convolution's input fused in:
 *   gin = (d loss / d conv input) * act'(mask_y),   mask_y = the saved conv input [N,C1+C2,Hin,Win] (post-activation
 * output of that layer), mask_act = its SPRK_ACT_*.  gin is then that layer's pre-activation gradient and its own
 * sprk_act_bwd pass (read gy, read y, write gpre) is not needed; only its bias gradient remains (sprk_act_bwd with
 * SPRK_ACT_NONE: one read).  In conv -> conv chains (joint_network_v2.py:33-97: every block of the U-Nets) this removes
 * two thirds of the activation-backward traffic.  The Winograd kernel applies the mask in its output transform; the
 * other kernels finish with an in-place pass, so the call is valid for every geometry without upsampled input. */
int sprk_conv2d_bwd_data_masked(const float *gy, const float *w, float *gin, const sprk_conv_geom *g,
                                const float *mask_y, int mask_act, void *ws, size_t ws_bytes, void *stream);
/* 1: sprk_conv2d_bwd_data_masked on g applies the mask inside its kernel (the Winograd kernel, or the 1x1 kernel of
 * few reduced channels: 1x1, stride 1, no padding, one full-resolution source, fp32, Hin * Win % 4 == 0, Cout <= 96,
 * a launch of at least 512 workgroups of 128 pixels); 0: the call finishes with the in-place pass.  A caller that may
 * choose (networks.py) fuses a producer's activation backward into this call only where the answer is 1: behind the
 * in-place pass the producer's remaining bias sum is one pass more than the unfused pair.  (16-byte aligned tensors
 * assumed; others take the in-place pass, with the same result.) */
int sprk_conv2d_bwd_data_mask_fused(const sprk_conv_geom *g);
/* bit 0 / 1 / 2: the forward / backward-data / backward-weight call of this layer exists for 16-bit activation tensors
 * (SPRK_DT_X16 / SPRK_DT_Y16; g->dtype carries the operand type, ep the forward epilogue or NULL) */
int sprk_conv2d_storage16(const sprk_conv_geom *g, const sprk_conv_epilogue *ep);
/* gw[Cout][C1+C2][KH][KW] = d loss / d w  (overwritten, not accumulated) */
size_t sprk_conv2d_bwd_weight_ws_bytes(const sprk_conv_geom *g);
int sprk_conv2d_bwd_weight(const float *x, const float *x2, const float *gy, float *gw,
                           const sprk_conv_geom *g, void *ws, size_t ws_bytes, void *stream);
/* ---- which kernel variant a convolution call takes (host only, no launch; tests and diagnostics) -------------------
 * The fp32 MFMA kernels are template families (conv_mfma_kernel<MT, NT, RB, XTAB>: 60 instantiations;
 * conv_wgrad_mfma_kernel<IT, NT, WJ, MODE>: 85) that also branch at run time on flags derived from the geometry and from
 * the tensors' alignment.  sprk_conv2d_variant runs the dispatcher's own routing (the function the dispatcher itself
 * acts on) for call `which` — 0 forward, 1 backward-data (unmasked), 2 backward-weight — of layer g and returns it as
 * SPRK_VARIANT_INTS integers.  x, x2: the layer's inputs (backward-data: x is gin, the tensor written); y_or_gy: y for
 * the forward call, gy otherwise.  The pointers are tested for 16-byte alignment only, never dereferenced.  Without a
 * device the plans are those of a 256-CU device (the MI355X).
 *   out[0] = stage, SPRK_STAGE_*; the other fields are filled by the stages that plan (MASK1X1, MFMA, GEMM1X1, WGRAD1X1, WGRAD3X3: the two lists that
 *   follow), by the Winograd stage (the two lists after them) and by the 16-bit stage (the last two), else 0
 *   which 0 / 1: [1] MT [2] NT [3] RB [4] XTAB [5] chunk_mma_small [6] K stages (1 | 2) [7] ragged last K-chunk
 *                [8] latency-bound re-chunking of K [9] vec1 [10] vec2 [11] vec4 [12] colOff != 0 [13] up1 [14] C2 > 0
 *                [15] taps (1: backward-data weight layout) [16] channels per K-chunk [17] K-chunks
 *                [18] workgroups of the launch (what the planner's 512-workgroup thresholds compare)
 *   which 2:     [1] IT [2] NT [3] WJ [4] MODE [5] xrow [6] xtab [7] g4 [8] vec1 [9] vec2 [10] nChunks > 1
 *                [11] groups > 1 [12] up1 [13] C2 > 0 [14] 64-pixel tiles one workgroup sums over
 *   stage SPRK_STAGE_WINOGRAD, which 0 / 1 (wino_conv_kernel<NT, SQ, UNROT>, csrc/wino.hip):
 *                [1] NT [2] SQ (1: 16 x 16-pixel workgroup tiles, 0: 8 x 32) [3] UNROT (sprk_conv2d_last_variant only: the
 *                query knows no un-rotated store) [4] channel groups of NT * 16 (grid.y) [5] output channels in the last
 *                group [6] 4-channel K chunks of source 1 [7] ... of both sources [8] C1 % 4 [9] C2 % 4 [10] pairs of
 *                unchecked (steady-state) K iterations per tile [11] the issue that moves the cursor to source 2: 0 no
 *                second source, 1 first_loads, 2 iteration 0, 3 a checked iteration, 4 an unchecked one [12] grid.x
 *                [13] tiles [14] fewest and [15] most tiles of a persistent workgroup [16] XCD order in effect (grid.x % 8
 *                == 0) [17] tilesX [18] tilesY [19] padT [20] padL (backward-data: mirrored) [21] reader of the output
 *                transform: 0 plain, 1 mask (sprk_conv2d_last_variant only: the query is the unmasked call), 2 up2,
 *                3 un-rotated store
 *   stage SPRK_STAGE_WINOGRAD, which 2 (wino_wgrad_kernel<MT>):
 *                [1] launches = column ranges of the reduction (1..4) [2 + 3 i] MT of launch i (3: groups of 48 input
 *                channels, 1: a tail of <= 16) [3 + 3 i] its groups (MT 3) or tail channels (MT 1) [4 + 3 i] its parts
 *                (grid.x: the K split) [14] regionsX [15] regionsY (regions of 4 x 16 pixels) [16] bit i: a workgroup of
 *                launch i carries its region cursor over a region row (cx) [17] ... over an image (cy) [18] padT [19] padL
 *                [20] Cout [21] bit i: launch i walks its regions in XCD order [22] bit i: launch i reads source 2
 *   stage SPRK_STAGE_16BIT, which 0 / 1 (csrc/conv16.hip; the plans that launch fill it, backward-data in the terms of its
 *   correlation: C1 = the layer's Cout, pads mirrored): [1] kind: 1 conv16_mfma_kernel<T, MT, NT, RB>, 2 conv16_tile_kernel
 *                <T, NT, X16, Y16>, 3 conv16_head_kernel<T, CQ, CK, X16, Y16> [2] T: 1 bf16, 2 f16 [3] X16 [4] Y16, then
 *     kind 1:    [5] MT [6] NT [7] RB [8] CK [9] K chunks [10] channels and [11] 8-channel groups (c8) of the last chunk
 *                [12] colOff [13] NI (images per tile) [14] tilesX [15] tilesY [16] image groups [17] output-channel blocks
 *                (grid.y) [18] up2 [19] 1 + the chunk that takes channels of both sources (0: none) [20] a chunk comes from
 *                source 2 alone [21] taps (1 | 9) [22] padT [23] padL
 *     kind 2:    [5] NT [6] lgTC [7] lgTR [8] NI [9] tilesX [10] tilesY [11] image groups [12] output-channel blocks
 *                [13] K chunks of 16 [14] c8 of the last chunk (1 | 2) [15] cshift + 16 padL + 256 padT [16] tiles [17] up2
 *                [18] grid.x on 256 CUs [19] fewest and [20] most tiles of a persistent workgroup [21] 1 + the chunk that
 *                straddles the sources (0: none) [22] bit 0: a chunk comes from source 2 alone, bit 1: some workgroup's
 *                next tile lies in the same image group, bit 2: some workgroup's in another one [23] 16-bit output: the
 *                tiles that take the LDS-transposed store: 0 none, 1 some (the others store directly), 2 all
 *     kind 3:    [5] CQ [6] CK [7] K chunks [8] pixel tiles per image [9] pixels of an image's last tile [10] output-channel
 *                quarters of 96 that store anything [11] channels of the last of them
 *   stage SPRK_STAGE_16BIT, which 2 (csrc/wgrad16.hip): [1] kind: 1 wgrad16_kernel<T, MC, LGRW, X16, PL1>, 2 wgrad16_1x1_kernel
 *                <T, .., X16> [2] T [3] X16, then
 *     kind 1:    [4] MC [5] lgRW [6] PL1 [7] regX [8] regY [9] seg (vertical segments of a strip) [10] segLen [11] units
 *                (N * regX * seg) [12] parts (grid.x) [13] input-channel blocks of 48 (grid.y) [14] tail (the 48 k + 1-th
 *                channel rides in block 0) [15] fewest and [16] most units of a workgroup [17] a block holds channels of both
 *                sources [18] the source of the tail channel (0: no tail) [19] padT [20] padL [21] XCD order in effect
 *                [22] 16-channel tiles of the last block that hold channels (1..3)
 *     kind 2:    [4] wide (192 x 192 blocks; 0: 96 x 384) [5] coBlocks [6] ciBlocks [7] parts [8] regions of 64 pixels per part
 *                [9] ... of the last part [10] regions per image [11] output and [12] input channels of the last block
 * sprk_conv2d_last_variant returns the same record for the calling THREAD's last call of that kind as it was routed
 * (stage SPRK_STAGE_NONE before the first one; prepared-weight describe calls are not recorded).  Backward calls made
 * by an autograd engine run on its threads. */
#define SPRK_VARIANT_INTS 24
#define SPRK_STAGE_NONE (-2)     /* sprk_conv2d_last_variant: no call yet */
#define SPRK_STAGE_REFUSED (-1)  /* the call is refused: storage guard, no plan fits LDS, unaligned 1x1 row staging */
#define SPRK_STAGE_DIRECT 0
#define SPRK_STAGE_STEM 1
#define SPRK_STAGE_16BIT 2
#define SPRK_STAGE_WINOGRAD 3
#define SPRK_STAGE_MASK1X1 4
#define SPRK_STAGE_MFMA 5
#define SPRK_STAGE_GEMM1X1 6     /* gemm1x1_kernel (csrc/gemm1x1.hip) on the MFMA stage's plan and slabs: the record is that plan's */
#define SPRK_STAGE_WGRAD1X1 7    /* backward-weight: wgrad1x1_kernel (csrc/wgrad1x1.hip) on the MFMA stage's plan: the record is that plan's */
#define SPRK_STAGE_WGRAD3X3 8    /* backward-weight: wgrad3x3_kernel (csrc/wgrad3x3.hip) on the MFMA stage's plan: the record is that plan's */
int sprk_conv2d_variant(int which, const sprk_conv_geom *g, const sprk_conv_epilogue *ep, const void *x, const void *x2,
                        const void *y_or_gy, int32_t *out);
int sprk_conv2d_last_variant(int which, int32_t *out);

/* ---- prepared weights: one launch per training step instead of one per convolution call ------------------------
 * Every convolution call re-lays its weights out in its workspace before the main kernel (k-chunked slabs, Winograd
 * G g G^T, 16-bit slabs): ~100 small launches per training step, 2-3 % of it.  A caller whose weights change once per
 * step (an optimiser) can hoist them:
 *   1. once per layer and direction, with a workspace that it KEEPS: sprk_conv2d_fwd_wprep / _bwd_data_wprep describe
 *      the transform that call would run (no launch; item->kind == 0: that path has none);
 *   2. after every weight update: sprk_prepare_weights(items, n) — all transforms in one launch per 40 items;
 *   3. the convolution calls pass the same workspace and SPRK_DT_WPREP in dtype: the transform launch is skipped.
 * Same device code either way: results are bit-identical to the plain calls.  The items are opaque.
 * A SPRK_DT_WPREP call may add SPRK_DT_WPREP_KIND(item.kind): the library then checks that the kernel path the call takes
 * reads a transform of that kind and returns SPRK_EINVAL otherwise (instead of reading a slab in another layout). */
#define SPRK_DT_WPREP 0x800
#define SPRK_DT_WPREP_KIND(kind) (((kind) & 7) << 12)
#define SPRK_DT_WPREP_KIND_OF(dtype) (((dtype) >> 12) & 7)
typedef struct sprk_wprep_item {
    const float *w;
    void *dst;
    int32_t kind, blocks;
    int32_t p[12];
} sprk_wprep_item;
int sprk_conv2d_fwd_wprep(const float *w, const sprk_conv_geom *g, const sprk_conv_epilogue *ep, void *ws,
                          size_t ws_bytes, sprk_wprep_item *item);
int sprk_conv2d_bwd_data_wprep(const float *w, const sprk_conv_geom *g, void *ws, size_t ws_bytes, sprk_wprep_item *item);
int sprk_prepare_weights(const sprk_wprep_item *items, int n, void *stream);

/* gpre[N,C,H,W] = gy * act'(y) where y is the saved POST-activation output (gpre may alias gy;
 * with act == NONE and up2 == 0 nothing is written to gpre and it may be NULL); if gbias != NULL
 * also gbias[c] = sum over n,h,w of gpre (conv bias gradient).  up2 != 0: gy and y are the
 * [N,C,2H,2W] tensors of a conv with the fused-upsample epilogue; gy is first summed over each
 * 2x2 block (backward of nn.Upsample).  ws: C*nsplit floats. */
size_t sprk_act_bwd_ws_bytes(int N, int C, int HW);
/* g_image_stride: elements between consecutive images of gy, 0 = dense (C*H*W, or 4*C*H*W with up2).  A larger
 * stride reads gy out of a channel slice of a wider tensor (the two halves of a concat layer's input gradient are
 * handed on as views); y and gpre are always dense. */
/* io = SPRK_IO3(type of gy, type of y, type of gpre): every tensor fp32 or the call's 16-bit type (all bf16 or all fp16);
 * gbias and the arithmetic are fp32.  With act == NONE and different gy / gpre types the call is a change of storage
 * type (+ the bias sum). */
int sprk_act_bwd(const void *gy, const void *y, void *gpre, float *gbias, int act,
                 int N, int C, int H, int W, int up2, long g_image_stride, int io,
                 void *ws, size_t ws_bytes, void *stream);
/* ---- deferred second-stage reductions ------------------------------------------------------
 * Backward-weight and the bias gradient are two-stage sums: the main kernel leaves per-workgroup partial sums in
 * ws and a small second kernel adds them in a fixed order.  A training step runs ~80 of those second kernels
 * (5 us of dispatch each).  The *_partial entry points run only the main kernel and describe the pending sum in
 * *item; sprk_reduce_items then finishes any number of them in one launch per 48 items.  Between the two calls the
 * item's ws must stay untouched (give every call its own ws) and dst is undefined.  item->kind == SPRK_RED_NONE:
 * the call already produced its final result (kernels without a partial stage).  The plain entry points above are
 * the *_partial call followed by sprk_reduce_items on its one item: results are bit-identical either way. */
#define SPRK_RED_NONE 0
#define SPRK_RED_ROWS 1   /* dst[i] = sum_p src[p * n + i],                        i < n          */
#define SPRK_RED_COLS 2   /* dst[i] = sum_p src[i * parts + p],                    i < n          */
#define SPRK_RED_WGRAD 3  /* dst[co * K + k] = sum_p src[(p * K + k) * CoutP + co], co < Cout, k < K */
typedef struct sprk_reduce_item {
    const float *src;
    float *dst;
    int kind, parts, n, K, Cout, CoutP;
} sprk_reduce_item;
int sprk_conv2d_bwd_weight_partial(const float *x, const float *x2, const float *gy, float *gw,
                                   const sprk_conv_geom *g, void *ws, size_t ws_bytes,
                                   sprk_reduce_item *item, void *stream);
int sprk_act_bwd_partial(const void *gy, const void *y, void *gpre, float *gbias, int act,
                         int N, int C, int H, int W, int up2, long g_image_stride, int io,
                         void *ws, size_t ws_bytes, sprk_reduce_item *item, void *stream);
/* every sum: four interleaved chains over p (p mod 4), combined as (s0 + s1) + (s2 + s3) */
int sprk_reduce_items(const sprk_reduce_item *items, int n, void *stream);

/* split the gradient of a fused (upsample2(a) ++ b) conv input: ga[N,C1,H/2,W/2] = 2x2 sums
 * of gin[:, :C1], gb[N,C2,H,W] = gin[:, C1:].  (autograd of nn.Upsample + torch.cat) */
int sprk_concat_up_bwd(const float *gin, float *ga, float *gb, int N, int C1, int C2, int H, int W,
                       int up1, void *stream);

/* ---- U-Net plumbing (HBM-bound) --------------------------------------------------------
 * Shift2d((1,0)) + MaxPool2d(2): models/joint_network_v2.py:27-30, models/utility.py:46-72;
 * shift = 0 gives the plain MaxPool2d(2) of the sigma net (joint_network_v2_shallow.py). */
/* io = SPRK_IO2(type of x, type of y) / SPRK_IO3(type of gy, type of x, type of gx) */
int sprk_shift_maxpool2_fwd(const void *x, void *y, int NC, int H, int W, int shift, int io, void *stream);
/* act != SPRK_ACT_NONE: x is the post-activation output of a convolution consumed by this pool only; gx is multiplied
 * by act'(x) and is then that convolution's PRE-activation gradient (its sprk_act_bwd pass reduces to the bias sum) */
int sprk_shift_maxpool2_bwd(const void *gy, const void *x, void *gx, int NC, int H, int W, int shift, int act,
                            int io, void *stream);
/* rotate(x,{0,90,180,270}) + cat(dim=0): joint_network_v2.py:198-200, utils/data.py:43-68.
 * x [B,C,P,P] -> y [4B,C,P,P]; bwd sums the four inverse rotations into gx. */
int sprk_rot4_stack_fwd(const float *x, float *y, int B, int C, int P, void *stream);
int sprk_rot4_stack_bwd(const float *gy, float *gx, int B, int C, int P, void *stream);
/* Shift2d((1,0)) + chunk(4) + rotate({0,270,180,90}) + cat(dim=1): joint_network_v2.py:230-239.
 * d [4B,C,P,P] -> f [B,4C,P,P] */
/* io = SPRK_IO2(type of the input, type of the output) */
int sprk_unrot4_shift_concat_fwd(const void *d, void *f, int B, int C, int P, int io, void *stream);
int sprk_unrot4_shift_concat_bwd(const void *gf, void *gd, int B, int C, int P, int io, void *stream);
/* Training: sprk_unrot4_shift_concat_bwd followed by sprk_act_bwd of the activated layer that produced d, in one pass
 * (fp32).  gf [B,4C,P,P]: gradient of f; f [B,4C,P,P]: the un-rotated tensor itself, which holds the layer's
 * post-activation output at the very addresses its gradient arrives at, so the stack tensor d need not be kept;
 * gpre [4B,C,P,P]: the layer's pre-activation gradient (row P-1 of every plane is +0); gbias as in sprk_act_bwd, with
 * ws of sprk_act_bwd_ws_bytes(4B, C, P*P) bytes.  item != NULL: the bias sum is left pending (sprk_act_bwd_partial),
 * NULL: finished at once.  Same additions in the same order as the two calls it replaces: bit-identical.
 * sprk_unrot_act_bwd_eligible: 1 where the kernel exists (P == 64, act LEAKY or RELU), else the call is refused. */
int sprk_unrot_act_bwd_eligible(int B, int C, int P, int act);
/* Training: sprk_conv2d_fwd whose kernel stores straight into the un-rotated tensor: x (x2) are the 4B images of a
 * 4-rotation stack, f [B,4*Cout,P,P] = sprk_unrot4_shift_concat_fwd(sprk_conv2d_fwd(...)) bit for bit, the stack tensor
 * [4B,Cout,P,P] is never written (row 0 of every shifted plane, which no output reaches, is written as zeros by the same
 * launch).  Same workspace, same prepared weights (sprk_conv2d_fwd_wprep, SPRK_DT_WPREP) as sprk_conv2d_fwd.
 * sprk_conv2d_fwd_unrot_eligible: 1 where the call runs (the layer takes the fp32 Winograd kernel, P == 64, N % 4 == 0,
 * 49..96 output channels, no fused up-sampling, no residual); elsewhere it is refused (SPRK_EINVAL). */
int sprk_conv2d_fwd_unrot_eligible(const sprk_conv_geom *g, const sprk_conv_epilogue *ep);
int sprk_conv2d_fwd_unrot(const float *x, const float *x2, const float *w, float *f, const sprk_conv_geom *g,
                          const sprk_conv_epilogue *ep, void *ws, size_t ws_bytes, void *stream);
int sprk_unrot_act_bwd(const float *gf, const float *f, float *gpre, float *gbias, int act, int B, int C, int P,
                       void *ws, size_t ws_bytes, sprk_reduce_item *item, void *stream);

/* ---- BatchNorm2d (+ optional ReLU), detector: joint_network_v2.py:547,558;
 * feature_extractor.py:287-288,320-324,338-346,412-414.
 * train: batch statistics (biased var for normalisation, unbiased for the running update,
 * momentum 0.1) saved to save_mean/save_invstd [groups][C]; eval: running statistics.
 * groups: the batch is `groups` independent passes of N / groups images stacked along N (the reference calls the
 * detector once per pass: patches, then their flipped copies): each group is normalised with its own batch
 * statistics, the running averages are updated group after group and the parameter gradients are summed in
 * group order, as if the module had been called once per pass.  groups = 1: plain BatchNorm2d.
 * ws (sprk_bn_ws_bytes): per-slice fp64 partial sums of the two-kernel reduction. */
size_t sprk_bn_ws_bytes(int N, int C, int HW, int groups);
int sprk_bn_train_fwd(const float *x, float *y, const float *gamma, const float *beta,
                      float *running_mean, float *running_var, float *save_mean, float *save_invstd,
                      int N, int C, int HW, int groups, float momentum, float eps, int relu,
                      void *ws, size_t ws_bytes, void *stream);
int sprk_bn_eval_fwd(const float *x, float *y, const float *gamma, const float *beta,
                     const float *running_mean, const float *running_var,
                     int N, int C, int HW, float eps, int relu, void *stream);
/* gy is d loss / d y (post-ReLU if relu); y is the saved output (for the ReLU mask). */
int sprk_bn_train_bwd(const float *gy, const float *x, const float *y, const float *gamma,
                      const float *save_mean, const float *save_invstd,
                      float *gx, float *ggamma, float *gbeta,
                      int N, int C, int HW, int groups, int relu, void *ws, size_t ws_bytes, void *stream);

/* ---- per-pixel maths of the pipeline ---------------------------------------------------
 * reparameterize: z = mu + eps * A^2 on out_stats [B,2,H,W] (joint_network_v2.py:469-475) */
int sprk_reparam_fwd(const float *out_stats, const float *eps, float *z, int B, int HW, void *stream);
/* g_out_stats [B,2,HW] (overwritten): d/dmu = gz, d/dA = gz * eps * 2A */
int sprk_reparam_bwd(const float *gz, const float *out_stats, const float *eps, float *g_out_stats,
                     int B, int HW, void *stream);
/* _sigmoid: clamp(sigmoid(x), 1e-4, 1-1e-4)  (denoiser_v2.py:32-34) */
int sprk_sigmoid_clamp_fwd(const float *x, float *p, long n, void *stream);
int sprk_sigmoid_clamp_bwd(const float *gp, const float *x, float *gx, long n, void *stream);
/* Small fused pieces of the training step's tail (ABI 410).  Each replaces a chain of framework launches by one: a
 * kernel of a replayed step costs ~5 us whatever it does, and these chains were a quarter of the step's launches.
 *
 * ResidA's residual (models/feature_extractor.py:384-416: x = x[:, :, edge:-edge, edge:-edge], optionally
 * x[:, :, ::s, ::s]; y = y + x):   out[nc][i][j] = y[nc][i][j] + x[nc][off + s i][off + s j]   (y == NULL: the crop
 * alone, for the 1x1 projection); NC = N * C planes, y / out [NC][Ho][Wo], x [NC][Hx][Wx].  crop_embed_bwd is the
 * gradient with respect to x: g scattered to those positions, zero elsewhere (the gradient with respect to y is g). */
int sprk_crop_add_fwd(const float *y, const float *x, float *out, long NC, int Ho, int Wo, int Hx, int Wx, int off, int stride,
                      void *stream);
int sprk_crop_embed_bwd(const float *g, float *gx, long NC, int Ho, int Wo, int Hx, int Wx, int off, int stride, void *stream);
/* Noise level of an image from the estimator's map (denoiser_v2.py:392-402; NoiseValue.UNKNOWN_VARIABLE):
 *   z[b] = mean(est[b]) - 4;  noise_std[b] = softplus(z[b]) + 1e-3   (softplus with torch's threshold 20)
 * est [B][HW]; z is kept for the backward pass:  g_est[b][i] = g[b] * sigmoid(z[b]) / HW.  One workgroup per image
 * (meant for patches; the whole-micrograph path keeps the framework's reduction). */
int sprk_noise_std_fwd(const float *est, float *noise_std, float *z, int B, int HW, void *stream);
int sprk_noise_std_bwd(const float *g, const float *z, float *g_est, int B, int HW, void *stream);
/* The training loss of the joint pipeline (denoiser_v2.py:516-519):
 *   consis[0] = mean((p - flip(pf))^2);   final[b] = alpha * loss_out[b] + (1 - alpha) * pred[0] + w_consis * consis[0]
 * p, pf: [B][1][H][W] scores of the batch and of the flipped batch, pf NOT yet flipped back (axis 0: along W, 1: along
 * H); loss_out [B] per-image denoising loss; pred [1] the PU loss.  joint_loss_bwd: g_final [B] ->
 *   g_loss_out[b] = alpha g_final[b];  g_pred[0] = (1 - alpha) S;  gp = w_consis S 2 (p - flip(pf)) / n;  gpf = -flip(gp)
 * with S = sum_b g_final[b], n = B H W.  One workgroup, sums in a fixed order. */
int sprk_joint_loss_fwd(const float *loss_out, const float *pred, const float *p, const float *pf, float *final_loss,
                        float *consis, int B, int H, int W, int axis, float alpha, float w_consis, void *stream);
int sprk_joint_loss_bwd(const float *g_final, const float *p, const float *pf, float *g_loss_out, float *g_pred, float *gp,
                        float *gpf, int B, int H, int W, int axis, float alpha, float w_consis, void *stream);
/* PU detection loss and its gradient in one launch (utils/losses.py:303-349: BCE on the labelled patches + slack *
 * binomial generalised-expectation penalty on the unlabelled ones):
 *   y[i] >= 0: labelled with target y[i];  y[i] == -1: unlabelled;  N = number of unlabelled, n_lab of labelled
 *   cls = sum_lab -(y log p + (1-y) log(1-p)) / max(n_lab, 1)
 *   mu = sum_unl p, var = sum_unl p (1-p);  q = softmax_k(-(mu - k)^2 / (2 (var + 1e-7))), k = 0..N
 *   loss[0] = cls - slack * sum_k log_binom[N][k] q[k];   gp[i] = d loss / d p[i]
 * log_binom: [B+1][B+1] table, row N = binom.logpmf(0..N; N, tau) (the host computes it once per (B, tau)).
 * p in (0, 1) (sigmoid_clamp output).  One workgroup; sums in a fixed order. */
int sprk_pu_loss(const float *p, const float *y, const float *log_binom, int B, float slack,
                 float *loss, float *gp, void *stream);
/* Adam update of many parameter tensors in ONE launch (train.py:128-140: Adam(lr, betas = (0.9, 0.99)), eps 1e-8, no
 * weight decay, no amsgrad; the formulas of torch.optim.Adam):
 *   t = step_in[0] + 1;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2
 *   p -= lr[0] / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps);   step_out[0] = t
 * items / start live in DEVICE memory (built once: the addresses of a training run do not change): item i owns
 * workgroups start[i] .. start[i+1]-1, 1024 elements each.  lr, step_in, step_out: device scalars (step_in != step_out),
 * so the call can sit in a captured graph and the learning-rate ramp needs no host sync. */
typedef struct sprk_adam_item {
    float *p;
    const float *g;
    float *m, *v;
    long n;
} sprk_adam_item;
int sprk_adam_multi(const sprk_adam_item *items, const int *start, int n_items, int n_blocks,
                    const float *lr, const float *step_in, float *step_out,
                    float beta1, float beta2, float eps, void *stream);
/* sprk_adam_multi for a loss-scaled step: skip = the device flag of sprk_unscale_check.  skip[0] != 0: p, m, v are not
 * touched and step_out[0] = step_in[0]; skip[0] == 0: exactly sprk_adam_multi. */
int sprk_adam_multi_skip(const sprk_adam_item *items, const int *start, int n_items, int n_blocks,
                         const float *lr, const float *step_in, float *step_out,
                         float beta1, float beta2, float eps, const int *skip, void *stream);

/* ---- dynamic loss scaling (torch.amp.GradScaler's rule, every value in device memory) ------------------------------
 * sprk_unscale_check: x[0 .. n) *= inv_scale[0] in place (any length, any 4-byte alignment); found_nonfinite[0] is
 * set to 1 (never cleared) when a result is +-inf or NaN.
 * sprk_loss_scale_update: reads found_nonfinite[0] (one thread):
 *   set:   scale *= backoff, growth_tracker = 0, skipped += 1
 *   clear: growth_tracker += 1; when it reaches `interval`: scale *= growth (if finite), growth_tracker = 0
 * then inv_scale = 1 / scale and next_found[0] = 0 (the flag of the next step: the flag is double-buffered, so no
 * launch both reads and clears the same flag; next_found != found_nonfinite). */
int sprk_unscale_check(float *x, long n, const float *inv_scale, int *found_nonfinite, void *stream);
int sprk_loss_scale_update(float *scale, float *inv_scale, int *growth_tracker, int *skipped,
                           const int *found_nonfinite, int *next_found, float growth, float backoff, int interval,
                           void *stream);
/* SSDN likelihood + posterior mean (denoiser_v2.py:405-424 noise model, :449-462 likelihood, :514 mean):
 *   var_x = A^2, var_y = var_x + var_n
 *   style SPRK_NOISE_GAUSSIAN: s = noise_std[b],                       var_n = s^2
 *   style SPRK_NOISE_POISSON : s = sqrt(max(mu, 1e-3) * noise_std[b]), var_n = s^2   (per pixel; Hasinoff 2012)
 *   nll = (x-mu)^2/var_y + log var_y - 0.05 s      -> loss[b] = mean over HW
 *   pme = (x var_x + mu var_n)/var_y ;  model_std = sqrt(var_x)
 * x [B,1,HW], out_stats [B,2,HW], noise_std [B] (the remapped estimate softplus(.-4)+1e-3);
 * pme/model_std [B,HW] (may be null); noise_std_map [B,HW]: s per pixel, written for POISSON only (may be null); loss [B].
 * ws: B*nblk floats of partial sums. */
enum { SPRK_NOISE_GAUSSIAN = 0, SPRK_NOISE_POISSON = 1 };
size_t sprk_ssdn_ws_bytes(int B, int HW);
int sprk_ssdn_fwd(const float *x, const float *out_stats, const float *noise_std,
                  float *loss, float *pme, float *model_std, float *noise_std_map, int style, int B, int HW,
                  void *ws, size_t ws_bytes, void *stream);
/* gloss [B] = d L / d loss[b];  g_out_stats [B,2,HW] (overwritten), g_noise_std [B] (d L / d noise_std[b]) */
int sprk_ssdn_bwd(const float *gloss, const float *x, const float *out_stats, const float *noise_std,
                  float *g_out_stats, float *g_noise_std, int style, int B, int HW,
                  void *ws, size_t ws_bytes, void *stream);

/* ---- training-patch feed ----------------------------------------------------------------
 * replaces MicrographDataset.__getitem__ (train branch) — datasets/micrograph.py:60-122 — plus the
 * DataLoader collation (train.py:1085-1091): PIL crop box (x-P/2, y-P/2, x+P/2, y+P/2) with zero
 * fill outside the image, RandomHorizontalFlip, to_tensor (uint8 -> float32/255; float images
 * unchanged) and the CWH->CHW permute that transposes the patch:
 *   out[b,0,u,v] = mic[image_b][y_b - P/2 + v][x_b - P/2 + (flip_b ? P-1-u : u)]
 * mics: all micrographs packed back to back in one device buffer of `dtype`
 * (SPRK_MIC_U8 | SPRK_MIC_F32); offsets[n_mics] (elements, device int64); dims[n_mics][2] =
 * (rows, cols) device int32; items[B][4] = (image, x, y, flip) device int32; out [B,1,P,P]. */
#define SPRK_MIC_U8 0
#define SPRK_MIC_F32 1
int sprk_gather_patches(const void *mics, int dtype, const long *offsets, const int *dims, const int *items,
                        float *out, int n_mics, int B, int P, void *stream);

/* ---- 2-D greedy non-maximum suppression ------------------------------------------------
 * replaces non_maximum_suppression(x, r, contam=set(), threshold) —
 * utils/algorithms.py:59-103, call site train.py:564.  Exact greedy semantics incl. the
 * reference's clip-to-H/W border behaviour; ties: score desc, then flat index desc.
 * scores [H,W] device; out_scores[max_out], out_xy[max_out][2] (x=col, y=row) device,
 * written in pick order (descending score).
 * out_count: device int32[2]: [0] = number of picks found (if it exceeds max_out the
 * stored list is incomplete: call again with a larger max_out), [1] = pixels still
 * undecided after `rounds` relaxation launches.  The suppression fixed point is reached
 * by repeated launches (no host sync inside): when [1] != 0 call again with resume = 1
 * (state is kept in ws) until it is 0; typical score maps need < 10 rounds. */
size_t sprk_nms2d_ws_bytes(int H, int W, int max_out);
int sprk_nms2d(const float *scores, int H, int W, int r, float threshold,
               float *out_scores, int32_t *out_xy, int32_t *out_count, int max_out,
               int rounds, int resume, void *ws, size_t ws_bytes, void *stream);

/* ---- contamination mask ----------------------------------------------------------------
 * replaces find_contamination(out_img) — utils/algorithms.py:24-57 (the reference never calls it:
 * train.py:583 passes contam = set() to the NMS).  img [H,W] fp32 device: the un-padded denoised
 * micrograph.  The reference's constants are the defaults: crop 3, ksize 5, k_low 1.5, k_high 2.0,
 * radius 15.  Min-max normalisation to uint8, ksize x ksize box blur of img[crop:H-crop, crop:W-crop]
 * (reflect-101 inside the crop), seeds = blurred pixels below mean - k_low*std or above
 * mean + k_high*std of the whole uint8 image, each seed's clipped disk of `radius` added as the flat
 * index clip(i+di,0,Hb)*Wb + clip(j+dj,0,Wb)  (Hb = H-2crop, Wb = W-2crop): the set C.
 *   mask_out [H,W] uint8 device: 1 at (f / Wb + crop, f % Wb + crop) for every f in C — the score
 *       map's frame (the reference would read f in a W-wide frame; this is the deviation);
 *   set_bitmap_out (nullable) uint8[(Hb+1)*Wb + 1] device: 1 at every f in C (the reference's frame);
 *   stats_out double[8] device: min, max (finite pixels; NaN if there is none), mean, std of the
 *       uint8 image, the two thresholds, the number of seeds, the number of mask pixels.
 * Constraints: crop >= 2, H, W >= 2*crop+1, ksize odd <= 15, 0 <= radius <= 31.  Non-finite pixels:
 * NaN -> 0, +-inf -> 255 / 0 after normalisation by the finite range.  Several launches on `stream`,
 * no host synchronisation. */
size_t sprk_contam_ws_bytes(int H, int W);
int sprk_contam_mask(const float *img, int H, int W, int crop, int ksize, double k_low, double k_high, int radius,
                     uint8_t *mask_out, uint8_t *set_bitmap_out, double *stats_out, void *ws, size_t ws_bytes,
                     void *stream);

/* ---- micrograph ingest ------------------------------------------------------------------
 * replaces the README's `newstack -bin N` step plus the host half of the evaluation feed
 * (utils/loader.py:49-59 load_mrc, cv2.normalize, to_tensor, the transpose and the reflect padding of
 * datasets/image_wrapper.py:197-249).  raw: the sample block of ONE 2-D MRC image as it sits in the file
 * ([ny,nx] row-major, mode 0 int8 / 1 int16 / 2 float32 / 6 uint16), in a device buffer that starts 16-byte
 * aligned.  Inputs are taken to be finite.
 * sprk_ingest_bin: binned_out [by,bx] fp32 = the mean of every bin x bin block of the centred area
 *   (by = ny/bin, bx = nx/bin, first sample (ny%bin)/2, (nx%bin)/2); integer modes: exact integer sum, one
 *   correctly rounded fp32 division by float(bin*bin); float32: fp32 adds from 0.0f in row-major order within
 *   the block, then that division; bin = 1: a conversion.  range_out float[2] device: min and max of binned_out.
 * sprk_ingest_finish: q = uint8(trunc((x*scale + shift) * 255.0f)) with scale = 1/(max-min), shift = -min*scale
 *   formed in double (0 when max-min <= DBL_EPSILON) and applied as separate fp32 operations, then
 *   u8_out  (nullable) [by,bx] = q;
 *   net_out (nullable) [S,S] fp32, net[a][b] = q[refl(b,by)][refl(a,bx)] / 255.0f — transposed, reflect-padded
 *       (np.pad "reflect", folding as often as needed) to S, a multiple of 32 with S >= by, bx (unused when
 *       net_out is null).  At least one of the two outputs.
 * A few launches on `stream`, no host synchronisation. */
#define SPRK_MRC_INT8 0
#define SPRK_MRC_INT16 1
#define SPRK_MRC_FLOAT32 2
#define SPRK_MRC_UINT16 6
#define SPRK_INGEST_MAX_BIN 16
size_t sprk_ingest_ws_bytes(int ny, int nx, int bin);
int sprk_ingest_bin(const void *raw, int mode, int ny, int nx, int bin, float *binned_out, float *range_out, void *ws,
                    size_t ws_bytes, void *stream);
int sprk_ingest_finish(const float *binned, int by, int bx, const float *range, uint8_t *u8_out, float *net_out, int S,
                       void *stream);
/* sprk_ingest_clip (optional, between the two): the binned image clamped to two of its own order statistics, so that
 * a hot pixel or a black spot no longer sets the range sprk_ingest_finish normalises by.
 *   binned_in [by,bx] fp32 as sprk_ingest_bin leaves it (finite), n = by*bx < 2^31; range_in float[2] device: its min
 *   and max (sprk_ingest_bin's range_out); ranks 0 <= k_lo <= k_hi <= n-1.
 *   key(x) = the order-preserving uint32 encoding of the fp32 bits (negative: ~bits, else bits | 2^31; it orders -0.0
 *   before +0.0).  lo = the element with the k_lo-th smallest key (counting from 0), hi = the one with the k_hi-th
 *   smallest: exact order statistics, no interpolation — each an element of the image, bit for bit.
 *   binned_out[i] = x < lo ? lo : (x > hi ? hi : x) in float comparisons (signed zeros are left alone; binned_out may
 *   be binned_in); range_out float[2] device = (lo, hi) (may be range_in).  lo and hi survive the clamp, so the min-max
 *   of binned_out is range_out, on the device and for micrograph_io.minmax_uint8 on the host alike.
 *   k_lo = 0, k_hi = n-1 is the identity (same image, same range).
 * Selection: a radix select on d = key(x) - key(min) in three passes of at most 11 bits taken from the highest set bit
 * of key(max) - key(min) downward (found on the device); every pass counts into per-workgroup 2048-bin histograms
 * (one per rank while their prefixes differ) in the workspace, which every workgroup writes in full: nothing to
 * initialise.  Ten launches on `stream`, no host synchronisation. */
size_t sprk_ingest_clip_ws_bytes(int by, int bx);
int sprk_ingest_clip(const float *binned_in, float *binned_out, int by, int bx, long long k_lo, long long k_hi,
                     const float *range_in, float *range_out, void *ws, size_t ws_bytes, void *stream);
/* sprk_ingest_flatten (optional, before sprk_ingest_finish; with sprk_ingest_clip: clip, flatten, clip again): the mean
 * over a (2R+1) x (2R+1) window, clamped at the image's edges, subtracted from every pixel, so that a slow intensity
 * gradient (ice wedge, carbon edge, uneven illumination) no longer takes the levels of the 8-bit range.
 *   binned_in [by,bx] fp32 (finite), n = by*bx < 2^31; range_in float[2] device = (lo, hi) with lo <= x <= hi for every
 *   pixel (sprk_ingest_bin's or sprk_ingest_clip's range_out); radius 1 <= R <= SPRK_INGEST_MAX_FLATTEN binned pixels.
 *   span = double(hi) - double(lo).  span == 0: binned_out = +0.0f everywhere, range_out = (0, 0).  Else e = ilogb(span),
 *   d = double(x) - double(lo)                       (one rounding),
 *   t = (int64) floor(ldexp(d, 30 - e))              (0 <= t < 2^31; the scaling is exact),
 *   window of (r, c): rows max(0, r-R) .. min(by-1, r+R), columns likewise, cnt its size,
 *   S = the sum of t over the window, in integers: exact, whatever the order.  S < 2^31 * 2047^2 < 2^53, so double(S)
 *       is exact too — that is the limit on R,
 *   bg = ldexp(double(S) / double(cnt), e - 30)      (one correctly rounded division; the ldexp exact),
 *   binned_out = float(d - bg)                       (a double subtraction, then one conversion; no fma);
 *   range_out float[2] device = the exact min and max of binned_out.  binned_out may be binned_in, range_out may be
 *   range_in.  Spans below 2^-60 can give fp32 subnormals; they follow the formula.
 * A row pass writes the horizontal window sums of t as uint64 into the workspace (an LDS prefix sum per segment of 1024
 * columns plus the R columns either side), a column pass moves a running integer sum down each column in chunks of
 * rows that prime their own window, forms binned_out and leaves per-workgroup ranges, which the range kernel of
 * sprk_ingest_bin reduces.  Three launches on `stream`, no host synchronisation, no atomics. */
#define SPRK_INGEST_MAX_FLATTEN 1023
size_t sprk_ingest_flatten_ws_bytes(int by, int bx, int R);
int sprk_ingest_flatten(const float *binned_in, float *binned_out, int by, int bx, int R, const float *range_in,
                        float *range_out, void *ws, size_t ws_bytes, void *stream);

/* sprk_ingest_resample (instead of sprk_ingest_bin; `--ftbin F`): the whole micrograph Fourier-cropped to by x bx pixels, any
 * 2 <= by <= ny <= 16384 and 2 <= bx <= nx <= 16384: out [by,bx] fp32 = My D Mx^T (+ the anchor), where My [by, ny] and
 * Mx [bx, nx] are the real matrices IDFT_S . crop . DFT_B of spr_pick_amd.ingest.resample_matrix (the operator of
 * sprk_extract_scale's m, in closed form; every row sums to 1).  Both axes keep their whole extent: output pixel s sits at
 * input position s*B/S, and the image is taken as periodic (the wrap-around of every Fourier crop; not tapered).
 * my, mx: fp32 on the device, 16-byte aligned, row strides ldmy / ldmx floats, multiples of 4, at least roundup(ny, 4) /
 * roundup(nx, 4); rows 0 .. by-1 / 0 .. bx-1 and columns 0 .. roundup(ny, 4)-1 / roundup(nx, 4)-1 are read.  raw as for
 * sprk_ingest_bin.  D: integer modes float(x - x[0,0]) (exact), float32 x; data are taken to be finite.  The sums are fp32
 * fmaf chains in a fixed order, on v_mfma_f32_16x16x4_f32, one accumulator per element and stage, K never split (so every
 * tiling gives the same bits):
 *   U[r, j] = chain over c = 0 .. nx-1 ascending of D[r, c] * Mx[j, c], from 0.0f   (fp32, in the workspace);
 *   Y[i, j] = chain over r = 0 .. ny-1 ascending of My[i, r] * U[r, j], from 0.0f.
 * Every padded K position is a zero formed in registers on both operands: the workspace may hold anything, NaNs included.
 * out = Y + float(x[0,0]) (one fp32 add) for the integer modes, out = Y for float32; range_out float[2] device: the exact
 * min and max of out (per-workgroup pairs in the workspace, reduced as sprk_ingest_bin's).
 * Refused (SPRK_EINVAL, nothing launched): another mode, other sizes, a row stride too small or not a multiple of 4, null
 * or misaligned pointers (out and ws 16-byte aligned as well); a short workspace: SPRK_EWORKSPACE.
 * Three launches on `stream`, no host synchronisation, no atomics. */
size_t sprk_ingest_resample_ws_bytes(int ny, int nx, int by, int bx);
int sprk_ingest_resample(const void *raw, int mode, int ny, int nx, int by, int bx, const float *my, int ldmy,
                         const float *mx, int ldmx, float *out, float *range_out, void *ws, size_t ws_bytes, void *stream);

/* ---- whole-frame motion correction of movies (`joint align`) --------------------------------
 * sprk_align_corr: the periodic cross-correlation window of Z reduced frames a [Z, Sy, Sx] fp32 against their references
 * (frame f's at r + f * r_stride floats; r_stride 0: one shared reference), for the row and column shifts -R .. R:
 *   cc[f, i, j] = fmaf chain, from 0.0f, over y' = 0 .. Sy-1 and then x = 0 .. Sx-1 ascending of
 *                 a[f, (y' - (i-R)) mod Sy, x] * r[f, y', (x + (j-R)) mod Sx],       cc [Z, 2R+1, 2R+1] fp32,
 * one fp32 GEMM per frame on MFMA (M and N the shifts, K the Sy*Sx pixels, never split): the bytes do not depend on the
 * tiling.  A frame displaced by d against its reference (a(p) = r(p - d)) has its peak at shift -d.
 * 1 <= R <= 31, Sx a multiple of 64 (so 2R+1 <= Sx), 1 <= Sy, Sy and Sx at most 16384, 1 <= Z <= 65535 (Sy may be smaller
 * than the window: the rows roll modulo Sy); a 16-byte aligned; r_stride 0 or at least Sy*Sx.  tile: 0 = the library's choice (the largest of 64, 32, 16 that gives every compute unit a workgroup,
 * else 16), or one of them.  Anything else: SPRK_EINVAL, nothing launched.  One launch on `stream`, no workspace, no host
 * synchronisation, no atomics.
 *
 * sprk_align_accumulate: one frame into a running sum, y (+)= My D Mx^T: sprk_ingest_resample's two GEMMs (its arguments,
 * sizes, matrices and their padding) with
 *   D = (float)(x - anchor) for the integer modes (anchor: a sample value, passed by value: no device read), x for float32
 *       (anchor 0);
 *   U[r, j] = fmaf chain over c ascending of D[r, c] * mx[j, c], from 0.0f (U [ny, roundup(bx, 4)] in the workspace);
 *   y[i, j] = fmaf chain over r ascending of my[i, r] * U[r, j], from 0.0f if `first`, else from the y[i, j] already there
 * (y [by, bx] fp32, 16-byte aligned, not read when `first`).  Z calls in frame order give the bits of one chain over
 * (frame, r) ascending.  No anchor is added back and no range is formed: with matrices whose rows sum to 1 the caller adds
 * Z * anchor once.  Refusals as sprk_ingest_resample's, and an anchor that is no sample value of the mode (SPRK_EINVAL); a
 * short workspace: SPRK_EWORKSPACE; nothing launched.  Two launches on `stream`, no host synchronisation, no atomics. */
int sprk_align_corr(const float *a, const float *r, long r_stride, int Z, int Sy, int Sx, int R, int tile, float *cc,
                    void *stream);
size_t sprk_align_accumulate_ws_bytes(int ny, int nx, int by, int bx);
int sprk_align_accumulate(const void *raw, int mode, int ny, int nx, int by, int bx, const float *my, int ldmy,
                          const float *mx, int ldmx, float anchor, float *y, int first, void *ws, size_t ws_bytes,
                          void *stream);

/* Dose-weighted sums (`joint align --dose`): Y = IDFT2[by,bx]( sum over the frames f of G_f . crop(DFT2[ny,nx](D_f)) ), the
 * movie accumulated in Fourier space.  The four real fp32 GEMMs of sprk_extract_filter (its matrix layouts) over a whole
 * rectangular frame, on v_mfma_f32_16x16x4_f32; every sum an fmaf chain over its K ascending from 0.0f, one accumulator per
 * element and stage, K never split (so every tiling gives the same bits).  Ku kept rows and Hs kept columns of the
 * spectrum; which frequencies they are, every weight and every phase is the caller's (spr_pick_amd.dose): the kernels know
 * no trigonometry.  ldv = roundup(Hs, 4).  All matrices fp32 on the device, 16-byte aligned, dense rows whose length is
 * the column count rounded up to a multiple of 4, the padding columns exact zeros.
 *
 * sprk_align_spectrum: one frame into the running spectrum F (stages 1 and 2).  2 <= ny, nx <= 16384, 1 <= Hs <= nx/2 + 1,
 * 1 <= Ku <= ny + 1; raw, mode, D and anchor as sprk_align_accumulate's.  w1 [2Hs, roundup(nx, 4)], w2 [2Ku, roundup(2ny, 4)].
 *   U[r, q]  = chain over c = 0 .. nx-1 of D[r, c] * w1[q, c];   V = [U[:, :Hs] ; U[:, Hs:]]  [2ny, ldv], the workspace;
 *   A[kk, v] = chain over t = 0 .. 2ny-1 of w2[kk, t] * V[t, v];   B[kk, v] the same with row Ku + kk;
 *   Fr[kk, v] = fmaf(A, Gr, fmaf(-B, Gi, Fr_old)),   Fi[kk, v] = fmaf(A, Gi, fmaf(B, Gr, Fi_old)),
 *   F_old = 0.0f when `first`, and F is then not read.
 * F and g: fp32 [2Ku, ldv], 16-byte aligned, the real rows first, then the imaginary rows; columns Hs .. ldv-1 are never
 * read into a stored value and never written.  Every padded K position is a zero formed in registers on both operands: the
 * workspace and, when `first`, F may hold anything, NaNs included.
 *
 * sprk_align_synthesize: the spectrum back to pixels, once per movie (stages 3 and 4).  2 <= by, bx <= 16384,
 * 1 <= Hs <= bx/2 + 1, 1 <= Ku <= by + 1.  w3 [2by, roundup(2Ku, 4)], w4 [bx, roundup(2Hs, 4)].
 *   Zr[i, v] = chain over t = 0 .. 2Ku-1 of w3[i, t] * F[t, v];   Zi the same with row by + i;
 *   Z = [Zr, Zi]  [by, roundup(2Hs, 4)], the workspace;
 *   y[i, j]  = chain over t = 0 .. 2Hs-1 of Z[i, t] * w4[j, t],   y [by, bx] fp32, 16-byte aligned.
 *
 * Refused (SPRK_EINVAL, nothing launched): another mode, other sizes, an anchor that is no sample value of the mode, null
 * or misaligned pointers (ws 16-byte aligned as well); a short workspace: SPRK_EWORKSPACE.  The *_ws_bytes functions return
 * 0 for sizes that are refused.  Two launches each on `stream`, no host synchronisation, no atomics. */
size_t sprk_align_spectrum_ws_bytes(int ny, int nx, int Hs);
int sprk_align_spectrum(const void *raw, int mode, int ny, int nx, int Ku, int Hs, const float *w1, const float *w2,
                        const float *g, float anchor, float *F, int first, void *ws, size_t ws_bytes, void *stream);
size_t sprk_align_synthesize_ws_bytes(int by, int Hs);
int sprk_align_synthesize(const float *F, int Ku, int Hs, int by, int bx, const float *w3, const float *w4, float *y, void *ws,
                          size_t ws_bytes, void *stream);

/* ---- raw detector movies in (`joint align --gain / --dark / --defects / --hot_sigma`) -----------
 * sprk_movie_correct: one frame of a movie (raw: [ny, nx] samples of mode 0 / 1 / 2 / 6) decoded, dark-subtracted,
 * gain-multiplied and repaired where the fix map says so.  Per pixel p = (y, x), d the sample as fp32:
 *   c(p) = d;  with dark: c = d - dark[p], one fp32 subtraction;  with gain: c = c * gain[p], one fp32 multiplication;
 *   nothing is fused;
 *   fix[p] == 0, or no fix map:  out[p] = c(p);
 *   fix[p] == r > 0:  r = min(r, SPRK_FIX_MAX_RADIUS); the window is rows max(0, y-r) .. min(ny-1, y+r) and the same for the
 *     columns, walked in row-major order over the pixels q with fix[q] == 0: S = S + c(q) in fp32 from 0.0f, n their count;
 *     out[p] = S / (float)n, the correctly rounded fp32 quotient, or 0.0f when n == 0;
 *   with sum:  sum[p] = out[p] when `first` (sum is then not read), else sum[p] + out[p]: one fp32 chain per pixel in call
 *     order.
 * The window recomputes c(q) from raw, gain and dark: the frame is finished in one launch, and the sample, gain and dark of
 * a pixel with fix[p] > 0 reach no output, NaN and Inf included.  gain, dark [ny, nx] fp32, fix [ny, nx] bytes, sum [ny, nx]
 * fp32: each may be NULL; out [ny, nx] fp32.  Refused (SPRK_EINVAL, nothing launched): a null raw or out, another mode, ny
 * or nx outside 1 .. 16384, a pointer that is not 16-byte aligned, out equal to raw, gain, dark or sum.  One launch on
 * `stream` (a hipStream_t), no workspace, no atomics, no host synchronisation. */
#define SPRK_FIX_MAX_RADIUS 8
int sprk_movie_correct(const void *raw, int mode, int ny, int nx, const float *gain, const float *dark,
                       const uint8_t *fix, float *out, float *sum, int first, void *stream);

/* ---- TIFF movies in (`joint align` on .tif / .tiff) ----------------------------------------------
 * sprk_tiff_decode: the strips of one frame, as they lie in the file, decoded into the frame's sample block.
 * src: `nbytes` bytes on the device.  strip_off, strip_len, strip_out: int64 [n_strips] on the device.  Strip s reads the
 * bytes [lo, hi) of src: [strip_off[s], strip_off[s] + strip_len[s]) clamped into [0, nbytes) (empty for a length <= 0).
 * It must yield so = strip_out[s] decoded bytes, and writes them at the decoded position base(s) = the sum of strip_out[t]
 * over t < s; every strip_out value is clamped into [0, out_elems], base(s) to out_elems and so to out_elems - base(s) and to
 * 2^31 - 1.  `out` holds out_elems decoded bytes: one byte each, or (widen = 1) one little-endian uint16 each with the byte
 * in its low half.  Decoded positions at or past the sum of all strip_out are not written.  status: int32 [n_strips].
 *
 * Each strip is decoded on its own; its output and status depend on nothing but its own bytes and so.
 * compression 1 (stored): the first min(hi - lo, so) bytes are copied; fewer than so: status 2.
 * compression 5 (LZW, TIFF 6.0): codes of 9..12 bits, the first bit of a code in the most significant free bit of the byte
 * (MSB first).  State: width = 9, next = 258 (the next free code), no previous string; this is also the state a strip
 * starts in, so a strip that does not begin with a Clear is decoded as if it did.  Until so bytes are out:
 *   fewer than `width` bits left in [lo, hi): status 2, stop;   code = the next `width` bits;
 *   code 256 (Clear): back to the starting state;   code 257 (EOI): status 2, stop (so bytes are not out yet);
 *   no previous string: a code above 255: status 1, stop; else the string is the byte `code`;
 *   else code < 256: that byte;  258 <= code < next: the string of that table entry;  code == next: the previous string
 *     plus its own first byte;  code > next: status 1, stop;
 *   a string longer than the so - n bytes still missing: its first so - n bytes are written, status 3, stop;
 *   the string is written;  with a previous string and next < 4096: entry `next` = the previous string plus the first byte
 *     of this one, next = next + 1, and when next is now 511, 1023 or 2047, width = width + 1 (the early change);
 *   the string becomes the previous string.
 * Decoding ends when so bytes are out: an EOI is not asked for, and what follows it is not read.  The first error of a
 * strip is its status (0: none); the bytes before it stay, and the rest of the strip's so bytes are zeros, so the output is
 * a function of the input alone.
 * Bounds: no byte outside [0, nbytes) of src is read and no bit outside [lo, hi) reaches the output; every write lies in
 * the strip's own [base(s), base(s) + so) within out_elems; every table index comes from a code below `next` <= 4096.  No
 * content of src, strip_off, strip_len or strip_out makes the kernel read or write out of bounds.
 * Refused (SPRK_EINVAL, nothing launched): a null pointer, nbytes < 1, n_strips outside 1 .. 2^20, another compression or
 * widen, out_elems < 1, src or out not 16-byte aligned, a table not 8-byte or status not 4-byte aligned, out == src.  One
 * launch on `stream` (one wave per strip), no workspace, no atomics, no host synchronisation. */
int sprk_tiff_decode(const uint8_t *src, long nbytes, const long *strip_off, const long *strip_len, const long *strip_out,
                     int n_strips, int compression, int widen, void *out, long out_elems, int *status, void *stream);

/* ---- local motion correction (`joint align --patch`) ---------------------------------------------
 * sprk_align_warp: one fp32 frame src [ny, nx] resampled through a smooth displacement field into a running sum y [ny, nx]:
 *   out(i, j) = src(i + sy(i, j), j + sx(i, j)) with periodic edges;   y = out when `first` (y is then not read), else
 *   y + out, one fp32 add.
 * cy, cx: 6 coefficients each of sy and sx, HOST pointers read during the call and passed on by value (no device read, no
 * synchronisation).  inv_nx = 1.0f / (float)nx and inv_ny = 1.0f / (float)ny, rounded on the host.  Per pixel and axis, in
 * fp32, every fmaf one rounding and every other product or difference one rounding (nothing else is fused):
 *   u = fmaf((float)j, inv_nx, -0.5f),  v = fmaf((float)i, inv_ny, -0.5f),  uu = u * u,  uv = u * v,  vv = v * v;
 *   s = c[0];  s = fmaf(c[1], u, s);  s = fmaf(c[2], v, s);  s = fmaf(c[3], uu, s);  s = fmaf(c[4], uv, s);
 *   s = fmaf(c[5], vv, s);   s = fminf(fmaxf(s, -16.0f), 16.0f)   (a NaN, which only an overflow can make, becomes -16);
 *   fl = floorf(s),  t = s - fl (exact),  tt = t * t,  the first tap at i0 - 1 with i0 = i + (int)fl (j0 likewise);
 *   w0 = fmaf(fmaf(-0.5f, t, 1.0f), t, -0.5f) * t,    w1 = fmaf(fmaf(1.5f, t, -2.5f), tt, 1.0f),
 *   w2 = fmaf(fmaf(-1.5f, t, 2.0f), t, 0.5f) * t,     w3 = fmaf(0.5f, t, -0.5f) * tt          (Catmull-Rom, Horner form);
 *   r_a = fmaf chain from 0.0f over b = 0 .. 3 ascending of wx_b * src[(i0 - 1 + a) mod ny, (j0 - 1 + b) mod nx];
 *   out = fmaf chain from 0.0f over a = 0 .. 3 ascending of wy_a * r_a.
 * The clamp to +-SPRK_WARP_MAX_SHIFT is part of the contract: it bounds what a workgroup stages, so no coefficient set
 * reads out of bounds.  With all coefficients zero the weights are (-0, 1, 0, 0) and out == src on finite data; a constant
 * integer shift is a roll, value for value.  1 <= ny, nx <= 16384 (the taps wrap as often as it takes).
 * Refused (SPRK_EINVAL, nothing launched): a null pointer, other sizes, a coefficient that is not finite, src or y not
 * 4-byte aligned, y == src.  One launch on `stream`, no workspace, no atomics, no host synchronisation. */
#define SPRK_WARP_MAX_SHIFT 16
int sprk_align_warp(const float *src, int ny, int nx, const float *cy, const float *cx, float *y, int first, void *stream);

/* ---- reference-free 2-D classification (`joint class2d`) ------------------------------------------
 * The rigid transform T(src, ct, st, dy, dx) of an fp32 image src [S, S] (S even, 2..128; c = S / 2), per output pixel
 * (i, j), in fp32, every fmaf one rounding and every other product or difference one rounding (nothing else is fused):
 *   y = (float)(i - c),  x = (float)(j - c);
 *   u = fmaf(ct, y, -(st * x)),  v = fmaf(st, y, ct * x)                (the inner product rounded first);
 *   fu = floorf(u),  tu = u - fu;   fv = floorf(v),  tv = v - fv;   the first tap at (i0, j0) = ((int)fu + c + dy,
 *   (int)fv + c + dx);   s[a][b] = src[i0 + a, j0 + b], or 0.0f where that lies outside [0, S) (formed in registers, never
 *   read: the edges are not periodic);
 *   r_a = fmaf(tv, s[a][1], (1.0f - tv) * s[a][0]),  a = 0, 1;     T = fmaf(tu, r_1, (1.0f - tu) * r_0).
 * With (ct, st) = (1, 0) this is the shifted copy T(i, j) = src[i + dy, j + dx], zero-filled, value for value on finite data.
 * (ct, st) come from cs [A_n, 2] fp32 on the device, row a = (cos, sin) of 2 pi a / A_n formed in float64 and rounded once
 * (spr_pick_amd.class2d.angle_table); 1 <= A_n <= 720.  Every index read from device memory (a source, an angle, a member,
 * a packed pixel, a class offset) is clamped into its array and a shift to +-256 (past +-S every tap is outside): no
 * content of these arrays makes a kernel read or write out of bounds.
 *
 * sprk_class_transform: M output images; output m is T of src[idx[m]] (src [n_src, S, S]) at the angle cs[ang[m]] and the
 * shift (dy, dx) = shift[m] (int32 [M, 2]); idx, ang, shift int32 on the device.  flags:
 *   SPRK_CLASS_MASK: pixels with (i-c)^2 + (j-c)^2 > radius^2 become 0.0f (integer arithmetic; 0 <= radius <= S);
 *   SPRK_CLASS_NORMALIZE (implies the mask): with v the masked image and `count` the pixels inside the mask,
 *     part[t] = fp64 sum, from 0.0, over the linear pixels e = t, t + 256, ... ascending of (double)v[e],  t = 0 .. 255;
 *     sum = the halving tree over part (h = 128, 64, .. 1: part[t] += part[t + h] for t < h);
 *     mean = (float)(sum / (double)count);   w[e] = v[e] - mean inside the mask (one fp32 subtraction), 0.0f outside;
 *     q = the same partial sums and tree over (double)w[e] * (double)w[e];   norm = sqrtf((float)q), correctly rounded;
 *     out[e] = w[e] / norm, the correctly rounded fp32 quotient; all zeros unless count > 0 and norm > 0.
 *   The statistics are formed over the whole image whatever the output form.
 * Output: pix == NULL: out [M, S, S].  Else pix is int32 [D] on the device, linear pixel indices (ascending in the callers'
 * use), 1 <= D <= S*S: out[m * ldo + q] = the value at pixel pix[q] for q < D and 0.0f for q = D .. ldo-1; ldo >= D a
 * multiple of 4.  src and out 16-byte aligned.  One workgroup per output, the source image staged in LDS.
 *
 * sprk_class_score: for Q [N, ldq] and B [Mb, ldb], row-major fp32, 16-byte aligned, ldq and ldb multiples of 4 and at
 * least D, data taken to be finite:
 *   s[n, m] = fmaf chain from 0.0f over d = 0 .. D-1 ascending of Q[n, d] * B[m, d]
 * on v_mfma_f32_16x16x4_f32, one accumulator per score, K never split (the bytes do not depend on the tiling);
 *   best_index[n] = the lowest m with s[n, m] == max over m of s[n, m] (int32 [N]),  best_score[n] = s[n, best_index[n]].
 * Rows and columns of padding take no part: a row whose scores are all negative reports a negative best.  scores: NULL, or
 * fp32 [N, lds] (lds >= Mb) that receives s[n, m] for m < Mb; columns Mb .. lds-1 are not written.
 * 1 <= N; 1 <= Mb <= 65536; 4 <= D <= 16384, a multiple of 4.
 *
 * sprk_class_average: class sums in a fixed order.  members int32 [N]: particle indices grouped by class; offsets int32
 * [K + 1]: class k's members are members[offsets[k] .. offsets[k+1] - 1] (offsets clamped to 0 .. N).  ang int32 [n_src] and
 * shift int32 [n_src, 2]: each PARTICLE's angle index and shift.  Per class k with count = offsets[k+1] - offsets[k] > 0 and
 * per pixel:
 *   sum = 0.0f;  sum = sum + T(src[p], cs[ang[p]], shift[p]) over the members p in list order, one fp32 add each;
 *   out[k] = sum * (1.0f / (float)count)                (the reciprocal rounded, then one multiplication);
 * no mask and no normalisation.  A class with count <= 0 leaves out[k] untouched.  out [K, S, S] fp32, not src;
 * 1 <= K <= 65535.  One workgroup per class and 256 pixels, the particles read straight from memory.
 *
 * All three: refused (SPRK_EINVAL, nothing launched): sizes outside the limits, unknown flags, a stride too small or not a
 * multiple of 4, null or misaligned pointers.  One launch on `stream`, no workspace, no atomics, no host synchronisation. */
#define SPRK_CLASS_MASK 1
#define SPRK_CLASS_NORMALIZE 2
int sprk_class_transform(const float *src, int n_src, int S, const int *idx, const int *ang, const int *shift, int M,
                         const float *cs, int A_n, int radius, int flags, const int *pix, int D, int ldo, float *out,
                         void *stream);
int sprk_class_score(const float *Q, int ldq, int N, const float *B, int ldb, int Mb, int D, float *scores, long lds,
                     float *best_score, int *best_index, void *stream);
int sprk_class_average(const float *src, int n_src, int S, const int *ang, const int *shift, const float *cs, int A_n,
                       const int *members, int N, const int *offsets, int K, float *out, void *stream);

/* ---- Wiener-weighted class averages (`joint class2d --ctf_weight`) -----------------------------------
 * Per class A = IDFT2(sum_i wn_i . DFT2(y_i) / (sum_i wd_i + tau)) in three calls, over the half plane sprk_extract_filter
 * keeps.  side = S even, 16..128; h = S/2, Hs = h + 1, Ku = S + 1, ldv = roundup4(Hs), ldz = roundup4(2Hs).  A spectrum is
 * fp32 [2Ku, ldv]: row kk = k + h holds Re at the row frequency k = -h .. h, row Ku + kk holds Im, column v = 0 .. h the
 * column frequency; columns Hs .. ldv-1 are written by nobody and read by nobody.  w1 [2Hs, roundup4(S)], w2 [2Ku, 2S],
 * w3 [2S, roundup4(2Ku)], w4 [S, ldz] are the four matrices of sprk_extract_filter for box = side = S
 * (spr_pick_amd.extract.filter_matrices(S, S); the weights of the rows +-h, of the columns and 1/S^2 sit inside w3 and w4).
 * Every chain below is an fmaf chain on v_mfma_f32_16x16x4_f32 over its K ascending from 0.0f, one accumulator per element,
 * K never split; data are taken to be finite.
 *
 * sprk_class_spectrum: spec[p] of img[p] for p < n, img fp32 [n, S, S] (stages 1 and 2 of sprk_extract_filter with the image
 * as D, no anchor, no filter):
 *   U[r, q]   = chain over c = 0 .. S-1 of img[r, c] * w1[q, c],  q < 2Hs;     V = [U[:, :Hs] ; U[:, Hs:]]   [2S, Hs]
 *   Re[kk, v] = chain over t = 0 .. 2S-1 of w2[kk, t] * V[t, v];  Im[kk, v] the same with row Ku + kk of w2.
 * Images run in batches of max_batch (0: the library's choice) that share the workspace (V of one batch,
 * sprk_class_spectrum_ws_bytes(n, side, max_batch)); an image's bits depend on nothing but the image.  Two launches per
 * batch.  n == 0 is SPRK_OK with nothing done.
 *
 * sprk_class_wiener: the class sums.  spec [n, 2Ku, ldv]; wn, wd fp32 [G, Ku, ldv] (spr_pick_amd.ctf.weight_tables); group
 * int32 [n]: the table of each IMAGE; members int32 [N]: image indices grouped by class; offsets int32 [K + 1]: class k's
 * members are members[offsets[k] .. offsets[k+1] - 1].  Per class k with offsets[k+1] > offsets[k] and per bin (kk, v < Hs):
 *   nr = ni = d = 0.0f;   over the members m in list order, with g = group[m]:
 *     nr = fmaf(wn[g, kk, v], spec[m, kk, v], nr);   ni = fmaf(wn[g, kk, v], spec[m, Ku + kk, v], ni);
 *     d  = d + wd[g, kk, v]                                       (one fp32 add);
 *   den = d + tau (one fp32 add);   out[k, kk, v] = nr / den,   out[k, Ku + kk, v] = ni / den   (correctly rounded quotients).
 * A member listed twice counts twice.  An empty class leaves out[k] untouched.  Every index read from device memory is
 * clamped into its array (a member to 0 .. n-1, a group to 0 .. G-1, an offset to 0 .. N): no content of these arrays makes
 * the kernel read or write out of bounds.  out fp32 [K, 2Ku, ldv], not spec; 1 <= K <= 65535, G >= 1, tau finite and > 0
 * (1 / SNR per image and bin).  n == 0 or N == 0 is SPRK_OK with nothing done.  One launch, one workgroup per class and 256
 * bins, no workspace.
 *
 * sprk_class_synthesize: out[k] fp32 [S, S] of the spectrum f[k] for k < K, f [K, 2Ku, ldv] (stages 3 and 4 of
 * sprk_extract_filter; no anchor, no normalisation):
 *   Zr[i, v] = chain over t = 0 .. 2Ku-1 of w3[i, t] * f[t, v];  Zi the same with row S + i of w3;   Z = [Zr, Zi]   [S, 2Hs]
 *   out[i, j] = chain over t = 0 .. 2Hs-1 of Z[i, t] * w4[j, t].
 * The workspace is Z of all K spectra (sprk_class_synthesize_ws_bytes(K, side)); 1 <= K <= 65535.  Two launches.
 *
 * All three: refused (SPRK_EINVAL, nothing launched): an odd side or one outside 16..128, negative counts, K < 1, G < 1, a
 * tau that is not finite or not > 0, a negative max_batch, null pointers, fp32 arrays or a workspace that do not start
 * 16-byte aligned (index arrays: 4-byte); SPRK_EWORKSPACE for a missing or short workspace (the message states the bytes
 * needed: the _ws_bytes query of the same arguments returns them, 0 for arguments that would be refused).  On `stream`, no
 * atomics, no host synchronisation. */
size_t sprk_class_spectrum_ws_bytes(int n, int side, int max_batch);
int sprk_class_spectrum(const float *img, int n, int side, const float *w1, const float *w2, int max_batch, float *spec,
                        void *ws, size_t ws_bytes, void *stream);
int sprk_class_wiener(const float *spec, int n, int side, const float *wn, const float *wd, int G, const int *group,
                      const int *members, int N, const int *offsets, int K, float tau, float *out, void *stream);
size_t sprk_class_synthesize_ws_bytes(int K, int side);
int sprk_class_synthesize(const float *f, int K, int side, const float *w3, const float *w4, float *out, void *ws,
                          size_t ws_bytes, void *stream);

/* ---- tiled power spectra (`joint ctf`)-----------------------------------------------------
 * sprk_psd_tiles: the summed half-plane power spectrum of T x T tiles of ONE raw micrograph (raw as for sprk_ingest_bin:
 * [ny,nx] samples of mode 0 / 1 / 2 / 6, 16-byte aligned start; rows may be only itemsize-aligned).  T a multiple of 16 in
 * 16..1024, T <= ny, nx <= 16384, H = T/2 + 1.  Tiles at a step of T/2: ty = (ny - T) / (T/2) + 1 rows of tx = (nx - T) /
 * (T/2) + 1 tiles, tile t = i*tx + j with its origin at (i*T/2, j*T/2); the trailing margin of fewer than T/2 samples on
 * either axis is not covered.  D: integer modes float(x - x[0,0]) with x[0,0] of the micrograph (exact), float32 x, taken
 * to be finite; no taper, no per-tile mean (the DC bin is of no use).
 * w1 [2H, T] fp32: row v cos(2 pi ((v c) mod T) / T), row H+v the sine of the same angle; w2 [2T, 2T] fp32 = [[C, -S], [S,
 * C]], C[u,r] = cos(2 pi ((u r) mod T) / T), S likewise (spr_pick_amd.ctf.dft_matrices: built in float64, the integer
 * product reduced mod T first).  On the device, 16-byte aligned, row strides ldw1 >= T and ldw2 >= 2T floats, multiples
 * of 4; rows 0 .. 2H-1 / 0 .. 2T-1 and columns 0 .. T-1 / 0 .. 2T-1 are read.  The sums are fp32 fmaf chains in a fixed
 * order on v_mfma_f32_16x16x4_f32, one accumulator per element and stage, K never split:
 *   U[r, q]  = chain over c = 0 .. T-1 ascending of D_t[r, c] * w1[q, c], from 0.0f, q < 2H;
 *   V        = [U[:, :H] ; U[:, H:]], [2T, H] (in the workspace);
 *   Re[u, v] = chain over k = 0 .. 2T-1 ascending of w2[u, k] * V[k, v], from 0.0f; Im[u, v] the same with row T+u;
 *   Q_t      = fmaf(Im, Im, Re * Re), the product rounded first;
 *   p_out[u, v] = ((0 + Q_0) + Q_1) + ... in ascending tile order, plain fp32 adds: fp32 [T, H], the un-normalised sum.
 * Nothing uninitialised is read into a stored value: the workspace may hold anything, NaNs included.
 * max_batch: tiles whose V and Q the workspace holds at a time (0 = the library's choice, about 256 MiB); p_out does not
 * depend on it.  Refused (SPRK_EINVAL, nothing launched): another mode, T not a multiple of 16 or out of range, ny or nx
 * below T or above 16384, a negative max_batch, a row stride too small or not a multiple of 4, null or misaligned
 * pointers (p_out and ws 16-byte aligned as well); a short workspace: SPRK_EWORKSPACE.
 * Three launches per batch on `stream`, no host synchronisation, no atomics. */
size_t sprk_psd_tiles_ws_bytes(int ny, int nx, int T, int max_batch);
int sprk_psd_tiles(const void *raw, int mode, int ny, int nx, int T, const float *w1, int ldw1, const float *w2, int ldw2,
                   int max_batch, float *p_out, void *ws, size_t ws_bytes, void *stream);

/* ---- 2-D Thon-ring fit (`joint ctf --astigmatism`) -------------------------------------------
 * sprk_ctf_score: for every candidate (d0, e1, e2) the three sums over n bins of the spectrum from which the host forms a
 * Pearson correlation (spr_pick_amd.ctf.score).  bins fp32 [5, ldb] on the device: rows b, p, q, r, Y of
 * spr_pick_amd.ctf.fit_bins, columns 0 .. n-1 read (what lies past them may be anything, NaNs included); cand fp32
 * [ncand, 3] contiguous.  1 <= n <= 2^20, 1 <= ncand <= 2^24, ldb >= n a multiple of 4.  Per bin i and candidate c:
 *   t = fmaf(r[i], e2, fmaf(q[i], e1, fmaf(p[i], d0, b[i])))   in fp32 (the phase of cos 2 chi in turns);
 *   x = cospif(2 t)                                            in fp32: |x - cos(2 pi t)| <= 2^-22;
 *   S1 += x, S2 += x * x, S3 += Y[i] * x                       in fp64, the products of two converted floats exact.
 * out fp64 [ncand, 3] = (S1, S2, S3).  The bins are cut into slices of consecutive bins, their number a function of n and
 * ncand alone; a slice is summed in ascending bin order from 0.0 (straight into out when there is only one), the slices'
 * sums, held in the workspace, are added in ascending slice order from 0.0.  No atomics: the bits do not depend on
 * scheduling.  Nothing uninitialised is read into a stored value: the workspace may hold anything.
 * Refused (SPRK_EINVAL, nothing launched): sizes outside the limits, ldb below n or not a multiple of 4, null or
 * misaligned pointers (bins, cand, out and ws 16-byte aligned); a short workspace: SPRK_EWORKSPACE (sprk_ctf_score_ws_bytes
 * is 0 where one slice does, and for sizes that are refused).
 * One or two launches on `stream`, no host synchronisation. */
size_t sprk_ctf_score_ws_bytes(int n, int ncand);
int sprk_ctf_score(const float *bins, int ldb, int n, const float *cand, int ncand, double *out, void *ws, size_t ws_bytes,
                   void *stream);

/* ---- particle extraction (`joint extract`) -----------------------------------------------
 * Boxes cut out of ONE raw micrograph (the buffer sprk_ingest_bin takes: [ny,nx] samples of mode 0 / 1 / 2 / 6, 16-byte
 * aligned start), binned, background-normalised and optionally inverted: out [P, b, b] fp32 with b = box / bin, status [P].
 * xy: int32 [P,2] on the device, (x along nx, y along ny) of each centre in raw samples; particle p covers rows
 * y0 .. y0+box-1, columns x0 .. x0+box-1 with x0 = x - box/2, y0 = y - box/2, output pixel (i, j) the bin x bin block at
 * (y0 + i*bin, x0 + j*bin).  2 <= box <= 1024, bin in 1..SPRK_INGEST_MAX_BIN, box % bin == 0, b >= 2, bg_radius >= 0 (in
 * output pixels).
 * Block value v: sprk_ingest_bin's sum (exact integer; float32: fp32 adds from 0.0f, row-major within the block).
 * status 1: the box is not entirely inside the image — all zeros, and none of its samples is read.
 * flags = 0: out = float(v) / float(bin*bin) (sprk_ingest_bin's value for that block, bit for bit), status 0.
 * SPRK_EXTRACT_NORMALIZE: background = {(i,j): (i - b/2)^2 + (j - b/2)^2 > bg_radius^2}, n pixels.
 *   integer modes: d = v - v[0,0]; S1 = sum_bg d, S2 = sum_bg d^2 exact (int64); mean = double(S1)/double(n);
 *     var = double(S2)/double(n) - mean*mean (two roundings); out = float((double(d) - mean) / sqrt(var));
 *   float32: mean = sum_bg v / n and var = sum_bg (v - mean)^2 / n in double (a fixed summation order: the same call
 *     gives the same bytes); out = float((double(v) - mean) / sqrt(var));
 *   status 2 and all zeros when n == 0 or !(var > 0).
 * SPRK_EXTRACT_INVERT: out is negated.
 * P == 0 returns SPRK_OK without a launch.  One launch on `stream`, no workspace, no host synchronisation. */
#define SPRK_EXTRACT_NORMALIZE 1
#define SPRK_EXTRACT_INVERT 2
int sprk_extract_boxes(const void *raw, int mode, int ny, int nx, const int *xy, int P, int box, int bin, int bg_radius,
                       int flags, float *out, int *status, void *stream);

/* sprk_extract_scale: the same boxes Fourier-cropped to side x side pixels, any 2 <= side <= box <= 1024: out [P, side,
 * side] = M D M^T, where M [side, box] is the real matrix IDFT_side . crop . DFT_box (spr_pick_amd.extract.crop_matrix:
 * M[s, b] = (1/box) sum_{k=-h..h} w_k cos(2 pi k (s/side - b/box)), h = side/2, w = 1 except 1/2 at k = +-side/2 for even
 * side; every row sums to 1, so the mean passes through as with `bin`).  m: fp32 on the device, row stride ldm floats, ldm %
 * 4 == 0, ldm >= roundup(box, 4), 16-byte aligned, columns box .. roundup(box, 4)-1 exact zeros; rows 0 .. side-1 are read.
 * Box placement, the inside test (64-bit, status 1, zeros, no sample read) and raw are those of sprk_extract_boxes.
 * D: integer modes float(x - x[0,0]) (exact), float32 x.  The sums are fp32 fmaf chains in a fixed order, on
 * v_mfma_f32_16x16x4_f32 (one accumulator per element and stage; data are taken to be finite):
 *   U[r, j] = chain over c = 0 .. box-1 ascending of D[r, c] * M[j, c], from 0.0f;
 *   Y[i, j] = chain over r = 0 .. box-1 ascending of M[i, r] * U[r, j], from 0.0f.
 * flags = 0: out = Y + float(x[0,0]) (one fp32 add) for the integer modes, out = Y for float32; status 0.
 * SPRK_EXTRACT_NORMALIZE, every mode: background = {(i,j): (i - side/2)^2 + (j - side/2)^2 > bg_radius^2}, n pixels;
 *   mean = sum_bg Y / n and var = sum_bg (Y - mean)^2 / n in double (a fixed summation order: the same call gives the same
 *   bytes); out = float((double(Y) - mean) / sqrt(var)); status 2 and all zeros when n == 0 or !(var > 0).
 * SPRK_EXTRACT_INVERT: out is negated.
 * P == 0 returns SPRK_OK without a launch.  One launch on `stream`, no workspace, no host synchronisation. */
int sprk_extract_scale(const void *raw, int mode, int ny, int nx, const int *xy, int P, int box, int side, const float *m,
                       int ldm, int bg_radius, int flags, float *out, int *status, void *stream);

/* sprk_extract_filter: the same boxes CTF-corrected and Fourier-cropped (`joint extract --ctf_correct`): out [P, side,
 * side] = IDFT2(phi . crop(DFT2(D))), box and side even, 16 <= side <= box <= 1024.  h = side/2, Hs = h + 1, Ku = side + 1.
 * Kept frequencies: columns v = 0 .. h, rows k = -h .. h (index kk = k + h), also for side == box, where k = +-h are one
 * frequency of the box and share it half and half.  phi: fp32 [Ku, Hs] contiguous on the device, the real and even filter
 * of the micrograph (spr_pick_amd.ctf.correction_filter); with phi = 1 the result is sprk_extract_scale's M D M^T.
 * Box placement, the inside test (64-bit, status 1, zeros, no sample read), raw and D are those of sprk_extract_scale.
 * The matrices (spr_pick_amd.extract.filter_matrices: float64 with the integer phase reduced mod box or side before the
 * division, rounded once) are fp32 on the device, 16-byte aligned, dense rows whose length is the column count rounded up
 * to a multiple of 4; the added columns are never used:
 *   w1 [2Hs, box]:   row v cos(2 pi v c / box), row Hs+v the sine;
 *   w2 [2Ku, 2 box]: row kk [cos t | -sin t], row Ku+kk [-sin t | -cos t], t = 2 pi k r / box;
 *   w3 [2 side, 2Ku]: row i [a cos f | -a sin f], row side+i [a sin f | a cos f], f = 2 pi k i / side, a = 1/2 at k = +-h, else 1;
 *   w4 [side, 2Hs]:  row j [w cos(2 pi v j / side) | -w sin(2 pi v j / side)] / box^2, w = 1 at v = 0 and v = h, else 2.
 * The sums are fp32 fmaf chains on v_mfma_f32_16x16x4_f32, each over its K ascending from 0.0f, one accumulator per
 * element and stage, K never split; K positions padded to a multiple of 4 are zeros in registers on both operands:
 *   U[r, q]   = chain over c = 0 .. box-1 of D[r, c] * w1[q, c];            V = [U[:, :Hs] ; U[:, Hs:]]    [2 box, Hs]
 *   Re[kk, v] = chain over t = 0 .. 2 box-1 of w2[kk, t] * V[t, v], Im with row Ku+kk;
 *   F = [Re * phi ; Im * phi], one fp32 multiply each                                                       [2Ku, Hs]
 *   Zr[i, v]  = chain over t = 0 .. 2Ku-1 of w3[i, t] * F[t, v], Zi with row side+i;   Z = [Zr, Zi]        [side, 2Hs]
 *   Y[i, j]   = chain over t = 0 .. 2Hs-1 of Z[i, t] * w4[j, t].
 * flags = 0: out = fmaf(phi[h, 0], float(x[0,0]), Y) for the integer modes (phi at k = 0, v = 0), out = Y for float32.
 * SPRK_EXTRACT_NORMALIZE and SPRK_EXTRACT_INVERT: as for sprk_extract_scale, on this Y.
 * V, F and Z live in the workspace, max_batch particles at a time (0 = the library's choice, about 256 MiB); out does not
 * depend on it.  Nothing uninitialised is read into a stored value: the workspace may hold anything, NaNs included.
 * Refused (SPRK_EINVAL, nothing launched): another mode, odd or out-of-range sizes, unknown flags, a negative max_batch or
 * bg_radius, null or misaligned pointers (out and ws 16-byte aligned as well); a short workspace: SPRK_EWORKSPACE.
 * P == 0 returns SPRK_OK without a launch.  Four launches per batch on `stream`, five with SPRK_EXTRACT_NORMALIZE; no host
 * synchronisation, no atomics. */
size_t sprk_extract_filter_ws_bytes(int P, int box, int side, int max_batch);
int sprk_extract_filter(const void *raw, int mode, int ny, int nx, const int *xy, int P, int box, int side, const float *w1,
                        const float *w2, const float *w3, const float *w4, const float *phi, int bg_radius, int flags,
                        int max_batch, float *out, int *status, void *ws, size_t ws_bytes, void *stream);

/* ---- in-library kernel timing (bench.py's roofline leg) --------------------------------
 * sprk_prof_enable(mask): bit k set = every launch of kernel class k is bracketed by HIP events
 * on its own stream (an event pair costs the GPU front end a few microseconds, so the timed
 * region of bench.py enables the dominant class only); sprk_prof_collect synchronises those
 * events and returns, per kernel class (0 = conv_mfma_kernel<4, 6, *>, the widest direct
 * forward / backward-data tile shape; 1 = conv_wgrad_mfma_kernel (all instantiations); 2 = the
 * other conv_mfma_kernel instantiations and wino_conv_kernel<3>; 3 = wino_conv_kernel<6>, the
 * Winograd kernel of the 96-channel 3x3 layers, the largest single kernel of a training step;
 * 4 = wino_wgrad_kernel, the Winograd backward-weight kernel of the largest layers),
 * the launch count, the summed duration in ms and the summed algorithmic (direct-convolution)
 * FLOPs. */
void sprk_prof_enable(int mask);
int sprk_prof_collect(int kclass, long *launches, double *ms, double *flops);
/* the same plus the summed ALGORITHMIC HBM bytes of the launches (every tensor read and written once, fp32): classes
 * 5 (16-bit-operand forward / backward-data kernels) and 6 (16-bit-operand backward-weight kernels) are HBM-bound
 * and are priced in GB/s; 0 for the other classes */
int sprk_prof_collect_bytes(int kclass, long *launches, double *ms, double *flops, double *bytes);

#ifdef __cplusplus
}
#endif
#endif /* SPRK_H */
