"""Which variants of the Winograd convolution kernels the suite runs ("Variant coverage of the Winograd
kernels"): the code shared by tests/test_wino_variants_cpu.py and tests/test_gpu_wino_variants.py, and the tool that
writes their case list, tests/golden/wino_variants.json.

wino_conv_kernel<NT, SQ, UNROT> and wino_wgrad_kernel<MT> (csrc/wino.hip) are few instantiations with many loop
shapes: how many K chunks a tile has and which of them are ragged, where the cursor moves to the second source, how
many tiles a persistent workgroup walks, which border masks a region takes.  One host function per kernel describes a
call in those terms (wino_variant / wino_wgrad_variant); sprk_conv2d_variant returns its answer without a device, with
the plans of a 256-CU device.  Everything here asks it; nothing re-states the planner.

    python tests/wino_variant_cases.py --search    walk the grid below, rewrite the fixture (--out PATH: write there)
    python tests/wino_variant_cases.py --margin    fp32 CPU convolution against fp64 for the backward-weight cases
    python tests/wino_variant_cases.py --report    what WINO_CASES reach, what the fixture reaches
"""
import ctypes
import itertools
import json
import os
import re
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(HERE, "golden", "wino_variants.json")

WINO = 3          # SPRK_STAGE_WINOGRAD (include/sprk.h)
# sprk_conv2d_variant's record for the Winograd stage (include/sprk.h): forward / backward-data, and backward-weight
FWD_FIELDS = ("stage", "NT", "SQ", "UNROT", "groups", "lastCh", "nc1", "nch", "r1", "r2", "pairs", "sw", "gridX", "ntiles",
              "tpwMin", "tpwMax", "xcd", "tilesX", "tilesY", "padT", "padL", "mode")
WG_FIELDS = ("stage", "launches", "MT0", "ch0", "parts0", "MT1", "ch1", "parts1", "MT2", "ch2", "parts2", "MT3", "ch3",
             "parts3", "regionsX", "regionsY", "cx", "cy", "padT", "padL", "Cout", "xcdMask", "srcMask")

# The instantiation tables, written out from the launch switches of wino_conv / wino_wgrad (csrc/wino.hip):
#   wino_conv_kernel<NT, SQ, UNROT>: NT 3 | 6, SQ 0 | 1; UNROT 1 with NT 6 only
#   wino_wgrad_kernel<MT>: MT 3 (groups of 48 input channels) | 1 (a tail of <= 16)
INST_TABLE = [(3, 0, 0), (3, 1, 0), (6, 0, 0), (6, 1, 0), (6, 0, 1), (6, 1, 1)]
WG_TABLE = [3, 1]
# The K loop of a tile (wino_conv_kernel): chunks 0 and 1 by first_loads, iteration c issues chunk c + 2; iterations 0 and
# 1, then pairs of unchecked ("steady") iterations while c + 4 < nch and source 1 is not ragged, then checked ones.
K_SHAPES = ("nch1", "nch2", "tail_odd", "tail_even",            # nch 1, 2; 3..6 odd / even: the checked tail loop only
            "steady1_odd", "steady1_even", "steady_many",       # the unchecked pair once (nch 7 / 8), more than once
            "steady_rag2_1", "steady_rag2_2", "steady_rag2_3",  # the unchecked loop stops in front of a ragged last chunk
            "rag1_1", "rag1_2", "rag1_3", "rag2_1", "rag2_2", "rag2_3", "rag_both",     # C % 4 of each source
            "sw_first_loads", "sw_iter0", "sw_checked", "sw_steady")                      # which issue moves to source 2
# The tiles of a persistent workgroup (tile, tile + grid.x, ...)
P_SHAPES = ("one", "two", "three+", "uneven", "xcd_off", "next_other_image", "next_same_image", "tilesX1", "one_tile_row")
PADS = tuple(range(5))          # wino_eligible: 0 <= padL <= 4
BATCHES = (4, 16, 32)           # images per GPU: the README's workflow, bench.py's two sizes

A0 = 0x10000000                 # a 16-byte aligned address that is never dereferenced
MAX_CASE_MACS, MAX_TOTAL_MACS = 4e9, 1.5e11
DT_PIN = 0x400


def _lib():
    from spr_pick_amd import _lib as m
    return m


def case_geom(c, dtype=None):
    """-> ConvGeom of the 3x3 stride-1 layer of case c (Hout = Hin: the bottom / right pads follow from the top / left)"""
    pt, pb, pl, pr = c["pad"]
    assert pt + pb == 2 and pl + pr == 2
    return _lib().ConvGeom(c["N"], c["C1"], c["C2"], c["H"], c["W"], 0, c["Cout"], c["H"], c["W"], 3, 3, 1, 1, pt, pl,
                           c["dtype"] if dtype is None else dtype)


def macs(c):
    """multiply-adds of the fp64 reference's forward (as many again for each gradient it computes)"""
    return c["N"] * c["H"] * c["W"] * c["Cout"] * (c["C1"] + c["C2"]) * 9


def query(which, g, ep=None):
    out = (ctypes.c_int32 * 24)()
    rc = _lib().lib().sprk_conv2d_variant(which, ctypes.byref(g), ep, A0, A0 if g.C2 else None, A0, out)
    assert rc == 0, _lib().lib().sprk_last_error()
    return list(out)


def as_dict(which, rec):
    """The record as {field: value}: the Winograd fields behind stage 3, the bare stage otherwise (the other stages'
    variants are the business of tests/conv_variant_cases.py)"""
    if rec[0] != WINO:
        return {"stage": rec[0]}
    return dict(zip(WG_FIELDS if which == 2 else FWD_FIELDS, rec))


def planned(c):
    """The variant each direction of case c takes, as sprk_conv2d_variant plans it -> {"fwd", "bwd", "wg"}; a case of
    kind "wgrad" calls the backward-weight entry alone, one of kind "fwd" the forward entry alone"""
    g = case_geom(c)
    if c["kind"] == "wgrad":
        return {"wg": as_dict(2, query(2, g))}
    if c["kind"] == "fwd":
        return {"fwd": as_dict(0, query(0, g))}
    ep = _lib().ConvEpilogue(None, None, None, None, 0, 0, 0, 0, 1) if c.get("up_out") else None
    return {"fwd": as_dict(0, query(0, g, ctypes.byref(ep) if ep else None)), "bwd": as_dict(1, query(1, g)),
            "wg": as_dict(2, query(2, g))}


def inst(v):
    return (v["NT"], v["SQ"], v["UNROT"])


def k_shapes(v):
    """the names of K_SHAPES that a forward / backward-data record shows"""
    nch, pairs, r1, r2 = v["nch"], v["pairs"], v["r1"], v["r2"]
    got = set()
    if nch <= 2:
        got.add("nch%d" % nch)
    elif pairs == 0 and nch <= 6:
        got.add("tail_odd" if nch % 2 else "tail_even")
    if pairs == 1:
        got.add("steady1_odd" if nch % 2 else "steady1_even")
    if pairs > 1:
        got.add("steady_many")
    if pairs and r2:
        got.add("steady_rag2_%d" % r2)
    if r1:
        got.add("rag1_%d" % r1)
    if r2:
        got.add("rag2_%d" % r2)
    if r1 and r2:
        got.add("rag_both")
    if v["sw"]:
        got.add(("sw_first_loads", "sw_iter0", "sw_checked", "sw_steady")[v["sw"] - 1])
    return got


def p_shapes(v):
    """the names of P_SHAPES that a forward / backward-data record shows"""
    got = {"one" if v["tpwMax"] == 1 else "two" if v["tpwMax"] == 2 else "three+"}
    if v["tpwMin"] != v["tpwMax"]:
        got.add("uneven")
    if not v["xcd"] and v["tpwMax"] > 1:        # (with one tile per workgroup xcd_slot changes nothing that shows)
        got.add("xcd_off")
    per_image, step = v["tilesX"] * v["tilesY"], v["gridX"]
    if v["tpwMax"] > 1:
        # tile t and its successor t + grid.x: in the same image for some t, in another one for some t
        n_pairs = v["ntiles"] - step
        same = any((t // per_image) == ((t + step) // per_image) for t in range(min(n_pairs, per_image)))
        other = step >= per_image or any((t // per_image) != ((t + step) // per_image) for t in range(min(n_pairs, per_image)))
        if same:
            got.add("next_same_image")
        if other:
            got.add("next_other_image")
    if v["tilesX"] == 1:
        got.add("tilesX1")
    if v["tilesY"] == 1:
        got.add("one_tile_row")
    return got


def p_class(v):
    """the persistence shape a workload call is matched by"""
    return ("one" if v["tpwMax"] == 1 else "two" if v["tpwMax"] == 2 else "three+", int(v["tpwMin"] != v["tpwMax"]), v["xcd"])


def wg_launches(v):
    return [(v["MT%d" % i], v["ch%d" % i], v["parts%d" % i], (v["srcMask"] >> i) & 1, (v["cx"] >> i) & 1, (v["cy"] >> i) & 1,
             (v["xcdMask"] >> i) & 1) for i in range(v["launches"])]


def _few(n):
    return "1" if n == 1 else "2" if n == 2 else "3+"


def wg_items(v):
    got = set()
    ls = wg_launches(v)
    for (mt, ch, parts, src, cx, cy, xcd) in ls:
        got.add(("wg", "MT", mt))
        if mt == 3:
            got.add(("wg", "g48", ch))
        else:
            got.add(("wg", "tail", "1" if ch == 1 else "16" if ch == 16 else "2..15"))
            if not any(m == 3 and s == src for (m, _, _, s, _, _, _) in ls):
                got.add(("wg", "tail_only_source"))
        if cx:
            got.add(("wg", "carry_cx", mt))
        if cy:
            got.add(("wg", "carry_cy", mt))
        got.add(("wg", "xcd", xcd))
    got.add(("wg", "ranges", v["launches"]))
    if v["launches"] == 4 and len({l[2] for l in ls}) > 1:
        got.add(("wg", "ranges4_parts_differ"))
    got.add(("wg", "Cout", "81" if v["Cout"] == 81 else "96" if v["Cout"] == 96 else "82..95"))
    got.add(("wg", "region_rows", _few(v["regionsY"])))
    got.add(("wg", "region_cols", _few(v["regionsX"])))
    got.add(("wg", "padT", v["padT"]))
    got.add(("wg", "padL", v["padL"]))
    return got


def items(plan):
    """Everything a case with this plan covers"""
    got = set()
    for d in ("fwd", "bwd"):
        v = plan.get(d)
        if v and v["stage"] == WINO:
            got.add(("inst",) + inst(v))
            got.update(("k", v["NT"], s) for s in k_shapes(v))
            if v["tpwMax"] > 1:         # ... and entered again for a workgroup's next tile, its first loads issued early
                got.update(("km", v["NT"], s) for s in k_shapes(v))
            got.update(("p", v["SQ"], s) for s in p_shapes(v))
            got.add(("padL", d, v["padL"]))
            got.add(("padT", d, min(v["padT"], 3)))
            got.add(("groups", min(v["groups"], 3)))
            if v["tpwMax"] > 1:         # every blockIdx.y walks on to a second tile
                got.add(("groups_more", min(v["groups"], 3)))
            if v["padT"] >= (16 if v["SQ"] else 8) + 2 and v["tilesY"] > 1:
                got.add(("padT_block", v["SQ"]))        # the whole raw row block of the first tile row lies above the image
            if v["lastCh"] % 8:
                got.add(("cut", v["NT"]))       # the last group ends inside a wave's 8-channel stride
            if v["groups"] == 1:
                got.add(("cout1", v["NT"], v["lastCh"]))
            got.add(("wk",) + inst(v) + (tuple(sorted(k_shapes(v))),))
            got.add(("wp",) + inst(v) + (p_class(v),))
    v = plan.get("wg")
    if v and v["stage"] == WINO:
        got |= wg_items(v)
    return got


def min_cout():
    """the smallest Cout each NT admits (one channel group), asked of the library on a pinned 8 x 32 plane"""
    out = {}
    for cout in range(1, 97):
        v = as_dict(0, query(0, _lib().ConvGeom(1, 4, 0, 8, 32, 0, cout, 8, 32, 3, 3, 1, 1, 1, 1, DT_PIN)))
        if v["stage"] == WINO:
            out.setdefault(v["NT"], cout)
    return out


def all_items(work=None):
    """The item table: the instantiations, each K-loop shape per NT, each persistence shape per SQ, the geometry and
    channel items, the backward-weight items, and what the workload reaches (workload_items())"""
    want = {("inst",) + k for k in INST_TABLE}
    want.update((k, nt, s) for k in ("k", "km") for nt in (3, 6) for s in K_SHAPES)
    want.update(("p", sq, s) for sq in (0, 1) for s in P_SHAPES)
    want.update(("padL", d, p) for d in ("fwd", "bwd") for p in PADS)
    want.update(("padT", d, p) for d in ("fwd", "bwd") for p in (0, 1, 2, 3))
    want.update((k, n) for k in ("groups", "groups_more") for n in (1, 2, 3))
    want.update(("padT_block", sq) for sq in (0, 1))
    want.update(("cut", nt) for nt in (3, 6))
    want.update(("cout1", nt, c) for nt, c in min_cout().items())
    want.update(("wg", "MT", mt) for mt in WG_TABLE)
    want.update(("wg", "g48", n) for n in (1, 2, 3))
    want.update(("wg", "tail", t) for t in ("1", "2..15", "16"))
    want.add(("wg", "tail_only_source"))
    want.update(("wg", c, mt) for c in ("carry_cx", "carry_cy") for mt in WG_TABLE)
    want.update(("wg", "xcd", x) for x in (0, 1))
    want.update(("wg", "ranges", n) for n in (1, 2, 3, 4))
    want.add(("wg", "ranges4_parts_differ"))
    want.update(("wg", "Cout", c) for c in ("81", "82..95", "96"))
    want.update(("wg", "region_rows", n) for n in ("1", "2", "3+"))
    want.update(("wg", "region_cols", n) for n in ("1", "2", "3+"))
    want.update(("wg", "padT", p) for p in PADS)
    want.update(("wg", "padL", p) for p in PADS)
    want.update(workload_items() if work is None else work)
    return want


# Items the code rules out, each with its rule (csrc/wino.hip, csrc/corr.h).  Pinned here: the search fails on any other
# item it cannot reach, so nothing lands in the fixture's list because the grid was too small.
UNROT_SQ = ("wino_variant: the un-rotated store takes SQ from wino_square(64, 64) = 0; SQ 1 needs SPRK_WINO_UNROT_SQ, which "
            "only a DIAG build reads")
MIRROR = "Corr(g): backward-data mirrors the pad to 2 - pad, and a pad of the layer is >= 0: at most 2"
RULED_OUT = {
    ("inst", 6, 1, 1): UNROT_SQ,
    ("padL", "bwd", 3): MIRROR, ("padL", "bwd", 4): MIRROR, ("padT", "bwd", 3): MIRROR,
}


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def seed_of(name):
    return zlib.crc32(name.encode()) % 10000


def guarded(t, device):
    """A copy of ``t`` on the device as the inner slice along N of a buffer whose first and last image are NaN: a read
    that strays into a neighbouring image shows in the result"""
    import torch
    buf = torch.full((t.shape[0] + 2,) + tuple(t.shape[1:]), float("nan"), device=device)
    buf[1:-1].copy_(t)
    v = buf[1:-1]
    assert v.is_contiguous() and v.data_ptr() % 16 == 0
    return v


def tensors(c):
    """CPU fp32 tensors of case c from the seed of its name -> x, x2 | None, w, b | None, gy"""
    import numpy as np
    import torch
    g = torch.Generator().manual_seed(seed_of(c["name"]))
    x = torch.randn(c["N"], c["C1"], c["H"], c["W"], generator=g)
    x2 = torch.randn(c["N"], c["C2"], c["H"], c["W"], generator=g) if c["C2"] else None
    cin = c["C1"] + c["C2"]
    w = torch.randn(c["Cout"], cin, 3, 3, generator=g) / np.sqrt(cin * 9)
    b = torch.randn(c["Cout"], generator=g) * 0.1 if c.get("bias") else None
    gy = torch.randn(c["N"], c["Cout"], c["H"], c["W"], generator=g)
    return x, x2, w, b, gy


# ---- the explicit lists: epilogue forms and the un-rotated store -----------------------------------------------------
def epilogue_cases():
    """Every (reader mode x act x bias | affine | none x mact) the host accepts, on one NT = 3 and one NT = 6 geometry
    with a partly filled last channel group.  plain and up2: the forward call (up2 = up_out); mask: the backward-data
    call of a conv -> conv chain with the fused activation backward (no epilogue of its own: act 0, neither)."""
    out = []
    for nt, (N, C1, C2, H, W, Cout) in ((3, (3, 7, 0, 16, 64, 41)), (6, (2, 9, 2, 32, 32, 75))):
        base = dict(N=N, C1=C1, C2=C2, H=H, W=W, Cout=Cout, pad=[2, 0, 1, 1], dtype=DT_PIN)
        for mode in ("plain", "up2"):
            for act in (0, 1, 2):
                for ep in ("bias", "affine", "none"):
                    out.append(dict(base, name="ep NT%d %s act%d %s" % (nt, mode, act, ep), mode=mode, act=act, ep=ep, mact=0))
        for mact in (1, 2):
            # the chain's second layer Cout -> Cout: its backward-data has Cout output channels, the same partly filled group
            out.append(dict(base, name="ep NT%d mask mact%d" % (nt, mact), mode="mask", act=0, ep="none", mact=mact))
    return out


def epilogue_plan(e):
    """the record of the call an epilogue case is about, as the query plans it; the mask form is the backward-data call
    of the layer Cout -> C1 + C2 + 3, which the query knows unmasked: reader mode set to 1"""
    L = _lib()
    pt, _, pl, _ = e["pad"]
    if e["mode"] == "mask":
        g = L.ConvGeom(e["N"], e["Cout"], 0, e["H"], e["W"], 0, e["C1"] + e["C2"] + 3, e["H"], e["W"], 3, 3, 1, 1, pt, pl, e["dtype"])
        return dict(as_dict(1, query(1, g)), mode=1)
    ep = L.ConvEpilogue(None, None, None, None, 0, 0, 0, e["act"], 1 if e["mode"] == "up2" else 0)
    return as_dict(0, query(0, case_geom(e), ctypes.byref(ep)))


UNROT_PAD = (2, 0, 1, 1)        # the blind-spot shift convolution in front of the un-rotation


def ref_unrot_layer(x, w, b):
    """fp64: ShiftConv2d, then (on the activated result) Shift2d + chunk + rotate + concat (oracle/networks.py) ->
    pre-activation, the un-rotation as a function"""
    import torch
    import torch.nn.functional as F
    from oracle.networks import rot90cw, shift_down
    pt, pb, pl, pr = UNROT_PAD
    pre = F.conv2d(F.pad(x, (pl, pr, pt, pb)), w, b)
    return pre, lambda y: torch.cat([rot90cw(q, a) for q, a in zip(torch.chunk(shift_down(y), 4, dim=0), (0, 270, 180, 90))], dim=1)


def zero_lines(f):
    """Row 0 of the shifted plane is zero: row 0 for the first rotation, and its images under the other three"""
    C, P = f.shape[1] // 4, f.shape[2]
    return (bool((f[:, 0:C, 0, :] == 0).all()) and bool((f[:, C:2 * C, :, P - 1] == 0).all())
            and bool((f[:, 2 * C:3 * C, P - 1, :] == 0).all()) and bool((f[:, 3 * C:, :, 0] == 0).all()))


def unrot_cases():
    """The un-rotated store at the smallest Cout it is eligible from and at the workload's, with one and two sources;
    B = 5: a workgroup's second tile lies in another image, for some in another rotation; B = 12: three tiles per workgroup,
    as the workload has them at batch 16 and 32"""
    return [dict(name="unrot %d%s->%d B%d" % (C1, "+%d" % C2 if C2 else "", Cout, B), B=B, C1=C1, C2=C2, Cout=Cout)
            for (B, C1, C2, Cout) in ((2, 96, 0, 96), (5, 6, 0, 68), (2, 9, 3, 68), (5, 8, 5, 96), (12, 4, 0, 96))]


def unrot_plan(u):
    """the forward record of an un-rotated case: the query's, which knows no un-rotated store, with UNROT and the reader
    mode set (tests/test_gpu_wino_variants.py compares it with what ran)"""
    g = _lib().ConvGeom(4 * u["B"], u["C1"], u["C2"], 64, 64, 0, u["Cout"], 64, 64, 3, 3, 1, 1, 2, 1, 0)
    v = as_dict(0, query(0, g))
    return dict(v, UNROT=1, mode=3)


# ---- the workload ----------------------------------------------------------------------------------------------------
def suite_table():
    """WINO_CASES of tests/test_gpu_ops.py as cases"""
    import test_gpu_ops
    return [dict(name=r[0], kind="conv", N=r[1], C1=r[2], C2=r[3], H=r[4], W=r[5], Cout=r[6], pad=list(r[7]), act=r[8],
                 bias=bool(r[9]), dtype=0) for r in test_gpu_ops.WINO_CASES]


def workload_calls():
    """Every Winograd-stage call of the workload at per-GPU batch 4, 16 and 32: the f32 configurations of
    tests/golden/unet_trace.json (each call's own geometry, its image count re-scaled from the configuration's batch)
    and WS_GEOMS of tests/test_abi.py -> [(which, record, unrot, note, geometry fields)]"""
    L = _lib()
    out, seen = [], set()

    def visit(which, fields, unrot, note):
        key = (which, tuple(fields), unrot)
        if key in seen:
            return
        seen.add(key)
        v = as_dict(which, query(which, L.ConvGeom(*fields)))
        if v["stage"] == WINO:
            if unrot:
                v = dict(v, UNROT=1, mode=3)
            out.append((which, v, unrot, note, list(fields)))

    trace = json.load(open(os.path.join(HERE, "golden", "unet_trace.json")))
    for cfg, rec in trace.items():
        m = re.fullmatch(r"(?:nograd-)?[a-z]+-f32-(\d+)x\d+(-.*)?", cfg)
        if not m:
            continue
        base = int(m.group(1))
        for call in rec["calls"]:
            which = {"conv2d_fwd": 0, "conv2d_fwd_unrot": 0, "conv2d_bwd_data": 1, "conv2d_bwd_weight": 2}.get(call[0])
            if which is None:
                continue
            geom = next(a for a in call[1] if isinstance(a, list) and len(a) == 16)
            if geom[15] & 0xff:
                continue
            for batch in BATCHES:
                f = list(geom)
                f[0] = geom[0] * batch // base
                if f[0] > 0:
                    visit(which, f, call[0] == "conv2d_fwd_unrot", "%s %s at batch %d" % (cfg, call[0], batch))
    import test_abi
    for (N, C1, C2, H, W, up1, Cout, K, stride, dil, (pt, pb, pl, pr)) in test_abi.WS_GEOMS:
        Ho = (H + pt + pb - dil * (K - 1) - 1) // stride + 1
        Wo = (W + pl + pr - dil * (K - 1) - 1) // stride + 1
        for n in sorted({N} | ({N // 4 * b for b in BATCHES} if N % 4 == 0 else set())):
            for which in (0, 1, 2):
                visit(which, [n, C1, C2, H, W, up1, Cout, Ho, Wo, K, K, stride, dil, pt, pl, 0], False, "WS_GEOMS at N = %d" % n)
    return out


_WORK = None


def workload_items():
    """{item: a call that reaches it}: per forward / backward-data call its instantiation with its K-loop shape ("wk")
    and with its persistence shape ("wp"); per backward-weight call its items as wg_items() names them"""
    global _WORK
    if _WORK is None:
        _WORK = {}
        for which, v, unrot, note, fields in workload_calls():
            if which == 2:
                for it in wg_items(v):
                    _WORK.setdefault(it, (note, fields))
            else:
                _WORK.setdefault(("inst",) + inst(v), (note, fields))
                _WORK.setdefault(("wk",) + inst(v) + (tuple(sorted(k_shapes(v))),), (note, fields))
                _WORK.setdefault(("wp",) + inst(v) + (p_class(v),), (note, fields))
    return _WORK


def explicit_items():
    """what the un-rotated cases cover (they are listed, not searched)"""
    got = set()
    for u in unrot_cases():
        v = unrot_plan(u)
        got.add(("inst",) + inst(v))
        got.add(("wk",) + inst(v) + (tuple(sorted(k_shapes(v))),))
        got.add(("wp",) + inst(v) + (p_class(v),))
    return got


# ---- the search -----------------------------------------------------------------------------------------------------
# A bounded grid, walked unit by unit: the K loop depends on the channel counts alone, the persistence shape on the
# tile count and the channel groups, the border handling on the pads, so each unit crosses its own axes in full with a
# few values of the others.  Pinned geometries (SPRK_DT_PIN: the choice ignores the image count) take the Winograd
# kernel below its 128-workgroup floor; the backward-weight floors (2048 regions, 8192 with a tail) have no such switch.
GRID = {
    "C1": [1, 200], "C2": [0, 60], "Cout": [33, 300],
    # (H, W): multiples of 8 x 32 and of 16 x 16, down to one tile row and one tile column
    "HW_tiles": [[8, 32], [8, 64], [16, 32], [24, 32], [8, 96], [32, 64], [64, 64], [128, 512], [16, 16], [32, 16], [16, 48],
                 [48, 48], [64, 16], [256, 272]],
    "N": [1, 2, 3, 4, 5, 6, 8, 12, 16, 24, 32, 43, 48, 64, 85, 86, 96, 128, 129, 170, 171, 192, 255, 256, 257, 300, 384, 512,
          513, 600, 768, 769, 1024],
    "Cout_groups": [34, 41, 48, 68, 75, 96, 140, 192, 202, 250, 288],
    "K_Cout": [34, 41, 68, 75], "K_HW": [[8, 32], [16, 16]], "K_N": [[3, DT_PIN], [300, 0]],
    "pad_layers": [[5, 0, 41], [41, 0, 75], [41, 3, 96]],            # C1, C2, Cout
    "pad_HW": [[8, 32], [32, 64], [16, 16], [32, 48]], "pad_tall": [10, 18],
    # backward-weight (the entry called directly): regions of 4 x 16 pixels
    "wg_HW": [[4, 16], [4, 32], [8, 16], [8, 32], [12, 48], [16, 64], [64, 64]],
    "wg_regions": [2048, 2049, 2100, 4096, 8192, 8193, 8200],
    "wg_C1": [1, 2, 7, 15, 16, 48, 49, 50, 63, 64, 96, 97, 112, 144, 145, 160],
    "wg_C2": [0, 1, 2, 9, 16, 48, 49, 57, 64],
    "wg_Cout": [81, 82, 88, 95, 96],
    "max_case_macs": MAX_CASE_MACS, "max_total_macs": MAX_TOTAL_MACS,
}


def _conv(N, C1, C2, H, W, Cout, pad=(2, 0, 1, 1), dtype=DT_PIN):
    return dict(kind="conv", N=N, C1=C1, C2=C2, H=H, W=W, Cout=Cout, pad=list(pad), dtype=dtype,
                act=(N + C1 + Cout) % 3, bias=bool((C1 + Cout) % 3))


def grid_units():
    G = GRID
    return ([("k", cout, hw) for cout in G["K_Cout"] for hw in G["K_HW"]] + [("cout",)] +
            [("p", hw) for hw in G["HW_tiles"]] + [("pad",)] + [("wg", hw) for hw in G["wg_HW"]])


def grid_cases(unit):
    G = GRID
    if unit[0] == "k":          # every channel pair of the grid on a few tiles
        _, cout, (H, W) = unit
        for N, dtype in G["K_N"]:       # a few tiles, pinned; and more tiles than workgroups
            for C1 in range(G["C1"][0], G["C1"][1] + 1):
                for C2 in range(G["C2"][0], G["C2"][1] + 1):
                    yield _conv(N, C1, C2, H, W, cout, dtype=dtype)
            # and as the backward-data call sees them: the layer's Cout is its K
            for Cout in range(G["Cout"][0], G["Cout"][1] + 1):
                yield _conv(N, cout, 0, H, W, Cout, dtype=dtype)
    elif unit[0] == "cout":     # every Cout of the grid
        for Cout in range(G["Cout"][0], G["Cout"][1] + 1):
            for (H, W) in G["K_HW"]:
                yield _conv(2, 5, 0, H, W, Cout)
    elif unit[0] == "p":        # tile counts x channel groups, pinned and not
        _, (H, W) = unit
        for N, Cout, dtype, C1 in itertools.product(G["N"], G["Cout_groups"], (DT_PIN, 0), (5, 41)):
            yield _conv(N, C1, 0, H, W, Cout, dtype=dtype)
    elif unit[0] == "pad":
        for (C1, C2, Cout), (H, W), pt, pl, N in itertools.product(G["pad_layers"], G["pad_HW"], PADS, PADS, (2, 5)):
            yield _conv(N, C1, C2, H, W, Cout, pad=(pt, 2 - pt, pl, 2 - pl))
        # pads taller than a workgroup's raw row block (wino_eligible bounds padT from below only); the forward entry
        # alone: the backward calls of such a layer leave the Winograd stage (the mirrored pad is negative, padT > 4)
        for (C1, C2, Cout), (H, W), pt in itertools.product(G["pad_layers"], G["pad_HW"], G["pad_tall"]):
            yield dict(_conv(3, C1, C2, H, W, Cout, pad=(pt, 2 - pt, 1, 1)), kind="fwd")
    else:
        _, (H, W) = unit
        per_image = (H // 4) * (W // 16)
        for regions, C1, C2, Cout in itertools.product(G["wg_regions"], G["wg_C1"], G["wg_C2"], G["wg_Cout"]):
            N = -(-regions // per_image)
            pads = itertools.product(PADS, PADS) if (C1 <= 16 and C2 in (0, 9) and Cout in (81, 88)) else ((2, 1), (1, 1))
            for pt, pl in pads:
                yield dict(kind="wgrad", N=N, C1=C1, C2=C2, H=H, W=W, Cout=Cout, pad=[pt, 2 - pt, pl, 2 - pl], dtype=0)


def describe(c):
    src = "%d" % c["C1"] + ("+%d" % c["C2"] if c["C2"] else "")
    return "%s%s->%d @%dx%d N%d pad%s%s" % ({"wgrad": "wgrad ", "fwd": "fwd "}.get(c["kind"], ""), src, c["Cout"], c["H"], c["W"], c["N"],
                                          tuple(c["pad"]), " pin" if c["dtype"] & DT_PIN else "")


def _rank(cost, c):
    return (cost, json.dumps(c, sort_keys=True))      # ties broken the same way whatever the order of the scan


def scan(cases):
    """-> (geometries seen, {item: (rank, case, plan)}: the cheapest case per coverage item)"""
    best, n = {}, 0
    for c in cases:
        n += 1
        plan = planned(c)
        if any(v["stage"] == -1 for v in plan.values()):
            continue
        cost, rank = macs(c), None
        for it in items(plan):
            if it not in best or cost <= best[it][0][0]:
                rank = rank or _rank(cost, c)
                if it not in best or rank < best[it][0]:
                    best[it] = (rank, c, plan)
    return n, best


def search(out=FIXTURE, verbose=True):
    best, n = {}, 0
    for cases in [suite_table()] + [grid_cases(u) for u in grid_units()]:
        k, part = scan(cases)
        n += k
        for it, rec in part.items():
            if it not in best or rec[0] < best[it][0]:
                best[it] = rec
    want = all_items()
    explicit = explicit_items()
    best = {it: (rank[0], c, plan) for it, (rank, c, plan) in best.items() if it in want}
    if verbose:
        print("grid: %d geometries, %d coverage items reached of %d" % (n, len(best), len(want)), file=sys.stderr)
    # the dearest first (a dear case usually brings cheap items along)
    chosen, covered = [], set(explicit)
    for it in sorted(best, key=lambda it: (-best[it][0], str(it))):
        if it in covered:
            continue
        cost, c, plan = best[it]
        chosen.append(dict(c, name=describe(c), macs=cost, plan=plan))
        covered |= items(plan)
    # drop what the later choices made redundant, the dearest first: every case left is the only one for some item
    for c in sorted(chosen, key=lambda c: -c["macs"]):
        rest = set(explicit).union(*(items(o["plan"]) for o in chosen if o is not c))
        if items(c["plan"]) & want <= rest:
            chosen.remove(c)
    chosen.sort(key=lambda c: (c["macs"], c["name"]))
    total = sum(c["macs"] for c in chosen)
    missing = sorted(want - covered, key=str)
    rules = RULED_OUT
    unruled = [i for i in missing if i not in rules]
    assert not unruled, "items the grid does not reach and no rule excludes: %s" % unruled
    over = [c["name"] for c in chosen if c["macs"] > MAX_CASE_MACS]
    fx = {
        "comment": "written by tests/wino_variant_cases.py --search; do not edit by hand",
        "grid": GRID,
        "total_macs": total,
        "min_cout": {str(k): v for k, v in min_cout().items()},
        "cases": chosen,
        # cases whose eligibility floor (2048 regions, 8192 with a tail) forces more than max_case_macs: the cheapest
        # eligible geometry of their item
        "above_case_bound": over,
        "epilogue_cases": [dict(e, plan=epilogue_plan(e)) for e in epilogue_cases()],
        "unrot_cases": [dict(u, plan=unrot_plan(u)) for u in unrot_cases()],
        "unreached": [dict(item=list(i), why=rules[i]) for i in missing],
        "coverage": coverage(chosen),
    }
    old = load() if os.path.exists(FIXTURE) else {}
    if "fp32_margin" in old:
        fx["fp32_margin"] = {k: v for k, v in old["fp32_margin"].items() if k in {c["name"] for c in chosen}}
    assert total <= MAX_TOTAL_MACS, total
    with open(out, "w") as f:
        json.dump(fx, f, indent=1, sort_keys=True)
        f.write("\n")
    if verbose:
        print("%d cases, %.3g multiply-adds in all (dearest %.3g, %d above the per-case bound); %d items ruled out" % (
            len(chosen), total, max(c["macs"] for c in chosen), len(over), len(missing)), file=sys.stderr)
    return fx


# ---- fp32 CPU convolution against fp64: is the budget wide enough for a correct fp32 result? --------------------------
def ref_wgrad(x, x2, gy, pad):
    """d loss / d w of the 3x3 stride-1 layer, in the precision of its arguments (CPU)"""
    import torch
    import torch.nn.functional as F
    xin = x if x2 is None else torch.cat((x, x2), 1)
    pt, pb, pl, pr = pad
    xin = F.pad(xin, (pl, pr, pt, pb))
    return torch.nn.grad.conv2d_weight(xin, (gy.shape[1], xin.shape[1], 3, 3), gy)


def margin(path=FIXTURE):
    """Per backward-weight case: max |fp32 CPU - fp64 CPU| of gw over max |gw|; written into the fixture"""
    fx = load()
    out = {}
    for c in fx["cases"]:
        if c["plan"].get("wg", {}).get("stage") != WINO:
            continue
        x, x2, w, b, gy = tensors(c)
        want = ref_wgrad(x.double(), None if x2 is None else x2.double(), gy.double(), c["pad"])
        got = ref_wgrad(x, x2, gy, c["pad"])
        out[c["name"]] = float((got.double() - want).abs().max() / want.abs().max())
        print("%-60s %.3e" % (c["name"], out[c["name"]]), file=sys.stderr)
    fx["fp32_margin"] = out
    with open(path, "w") as f:
        json.dump(fx, f, indent=1, sort_keys=True)
        f.write("\n")


KINDS = (("inst", "instantiations"), ("k", "K-loop shapes per NT"), ("km", "... entered for a second tile"),
         ("p", "persistence shapes per SQ"), ("padL", "padL per direction"), ("padT", "padT per direction"),
         ("padT_block", "padT beyond a raw row block per SQ"), ("groups", "channel groups"),
         ("groups_more", "... walking on to a second tile"), ("cut", "cut last group per NT"), ("cout1", "smallest Cout per NT"),
         ("wk", "workload K-loop shapes"), ("wp", "workload persistence shapes"), ("wg", "backward-weight items"))


def coverage(cases):
    """{kind: [items, reached by WINO_CASES alone, reached by the cases (and the explicit lists), ruled out]}, and the totals under the key all"""
    want = all_items()
    before = set()
    for c in suite_table():
        before |= items(planned(c))
    after = explicit_items()
    for c in cases:
        after |= items(c["plan"])
    out = {k: [sum(i[0] == k for i in want), sum(i[0] == k for i in before & want), sum(i[0] == k for i in after & want),
               sum(i[0] == k for i in RULED_OUT)] for k, _ in KINDS}
    out["all"] = [len(want), len(before & want), len(after & want), len(RULED_OUT)]
    return out


def report():
    cov = coverage(load()["cases"])
    return "\n".join("%-36s %3d items: WINO_CASES reach %3d, the fixture %3d, ruled out %d" % ((name,) + tuple(cov[k]))
                     for k, name in KINDS + (("all", "all"),))


if __name__ == "__main__":
    if "--search" in sys.argv:      # --search [--out PATH]
        search(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE)
    if "--margin" in sys.argv:
        margin()
    if "--report" in sys.argv:
        print(report())
