"""Which loop shapes of the 16-bit convolution kernels the suite runs ("Variant coverage of the 16-bit
kernels"): the code shared by tests/test_conv16_variants_cpu.py and tests/test_gpu_conv16_variants.py, and the tool that
writes their case list, tests/golden/conv16_variants.json.

conv16_mfma_kernel, conv16_tile_kernel, conv16_head_kernel (csrc/conv16.hip), wgrad16_kernel and wgrad16_1x1_kernel
(csrc/wgrad16.hip) are 126 instantiations with many loop shapes: how many K chunks a tile has and how the last one is
cut, where the sources meet, how many tiles a persistent workgroup walks, which store a tile takes.  One host function
beside each planner describes a call in those terms; sprk_conv2d_variant returns its answer without a device, with the
plans of a 256-CU device (include/sprk.h lists the fields).  Everything here asks it; nothing re-states a planner.

    python tests/conv16_variant_cases.py --search    walk the grid below, rewrite the fixture (--out PATH: write there)
    python tests/conv16_variant_cases.py --margin    the exact model in fp32 on the CPU against fp64, per case and budget
    python tests/conv16_variant_cases.py --report    what CONV16_CASES + STORE16_CASES reach, what the fixture reaches
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
FIXTURE = os.path.join(HERE, "golden", "conv16_variants.json")

S16 = 2           # SPRK_STAGE_16BIT (include/sprk.h)
# sprk_conv2d_variant's record for stage 2 (include/sprk.h): the common head, then the fields of each kernel kind
HEAD = ("stage", "kind", "T", "X16", "Y16")
KIND_FIELDS = {
    1: ("MT", "NT", "RB", "CK", "nchunks", "ckeLast", "c8Last", "colOff", "NI", "tilesX", "tilesY", "imgGroups", "nblkN", "up2",
        "straddle", "whole2", "taps", "padT", "padL"),
    2: ("NT", "lgTC", "lgTR", "NI", "tilesX", "tilesY", "imgGroups", "nblkN", "nchunks", "c8Last", "pads", "ntiles", "up2", "gridX",
        "tpwMin", "tpwMax", "straddle", "walk", "store"),
    3: ("CQ", "CK", "nchunks", "tilesPerImage", "lastPixels", "quarters", "lastQuarterCh"),
}
WG_HEAD = ("stage", "kind", "T", "X16")
WG_FIELDS = {
    1: ("MC", "lgRW", "PL1", "regX", "regY", "seg", "segLen", "nUnits", "parts", "nBlocks", "tail", "upwMin", "upwMax", "straddle",
        "tailSrc", "padT", "padL", "xcd", "lastTiles"),
    2: ("wide", "coBlocks", "ciBlocks", "parts", "perPart", "lastPart", "regPerImg", "lastCo", "lastCi"),
}
KIND_NAME = {1: "mfma", 2: "tile", 3: "head"}

# The instantiation tables, written out from the launch switches (launch16 / launch16_nt, launch_tile / launch_tile_io,
# run_head / launch_head of csrc/conv16.hip; wgrad16_run, wgrad16_run_1x1 of csrc/wgrad16.hip), per operand type T:
#   conv16_mfma_kernel<T, MT, NT, RB>: MT 4 with RB 1 | 2 | 4, MT 2 with RB 1 | 2; NT 3 | 4 | 6
#   conv16_tile_kernel<T, NT, X16, Y16>: NT 3 | 6
#   conv16_head_kernel<T, CQ, CK, X16, Y16>: (CQ, CK) (4, 64) | (4, 32) | (1, 32)
#   wgrad16_kernel<T, MC, LGRW, X16, PL1>: MC 3 | 6, LGRW 4 | 5 | 6
#   wgrad16_1x1_kernel<T, 4 | 2, 3, 6, X16>: wide 1 | 0
TYPES, BITS = (1, 2), (0, 1)
MFMA_TABLE = [(t, mt, nt, rb) for t in TYPES for (mt, rbs) in ((4, (1, 2, 4)), (2, (1, 2))) for nt in (3, 4, 6) for rb in rbs]
TILE_TABLE = [(t, nt, x, y) for t in TYPES for nt in (3, 6) for x in BITS for y in BITS]
HEAD_SHAPES = ((4, 64), (4, 32), (1, 32))
HEAD_TABLE = [(t, cq, ck, x, y) for t in TYPES for (cq, ck) in HEAD_SHAPES for x in BITS for y in BITS]
WG_TABLE = [(t, mc, lg, x, p) for t in TYPES for mc in (3, 6) for lg in (4, 5, 6) for x in BITS for p in BITS]
WG1_TABLE = [(t, w, x) for t in TYPES for w in BITS for x in BITS]
assert (len(MFMA_TABLE), len(TILE_TABLE), len(HEAD_TABLE), len(WG_TABLE), len(WG1_TABLE)) == (30, 16, 24, 48, 8)

SW_SHAPES = ("none", "boundary", "first", "middle", "last", "C2=1", "whole2", "one_chunk")
P_SHAPES = ("one", "two", "three+", "uneven", "mod8_zero", "mod8_nonzero", "next_same_group", "next_other_group", "nblk1", "nblk2",
            "nblk3+")
HEAD_COUTS = (33, 96, 97, 192, 193, 384)
PADS = tuple(range(5))
BATCHES = (4, 16, 32)           # images per GPU: the README's workflow, bench.py's two sizes
WORK_CONFIGS = ("bs-bf16-2x64", "bs-f16-2x64", "shallow-bf16operands-2x32")

A0 = 0x10000000                 # a 16-byte aligned address that is never dereferenced
MAX_CASE_MACS, MAX_TOTAL_MACS = 4e9, 1e11
DT_CODE = {"bf16": 1, "f16": 2}
T_NAME = {1: "bf16", 2: "f16"}


def _lib():
    from spr_pick_amd import _lib as m
    return m


def unit_roundoff(dt):
    return 2.0 ** -8 if dt == "bf16" else 2.0 ** -11


def base_dtype(c):
    return DT_CODE[c["dt"]] | _lib().DT_FORCE


def case_geom(c, dtype):
    pt, pb, pl, pr = c["pad"]
    K = c["K"]
    assert pt + pb == K - 1 and pl + pr == K - 1        # Hout = Hin: the kernels' own condition
    return _lib().ConvGeom(c["N"], c["C1"], c["C2"], c["H"], c["W"], 0, c["Cout"], c["H"], c["W"], K, K, 1, 1, pt, pl, dtype)


def macs(c):
    """multiply-adds of the fp64 reference's forward (as many again for each gradient it computes)"""
    return c["N"] * c["H"] * c["W"] * c["Cout"] * (c["C1"] + c["C2"]) * c["K"] ** 2


def query(which, g, ep=None):
    out = (ctypes.c_int32 * 24)()
    rc = _lib().lib().sprk_conv2d_variant(which, ctypes.byref(g), ep, A0, A0 if g.C2 else None, A0, out)
    assert rc == 0, _lib().lib().sprk_last_error()
    return list(out)


def as_dict(which, rec):
    """The record as {field: value}: the 16-bit stage's fields, the bare stage otherwise (the other stages' variants
    are the business of tests/conv_variant_cases.py and tests/wino_variant_cases.py)"""
    if rec[0] != S16:
        return {"stage": rec[0]}
    head, fields = (WG_HEAD, WG_FIELDS) if which == 2 else (HEAD, KIND_FIELDS)
    names = head + fields[rec[1]]
    assert not any(rec[len(names):]), rec
    return dict(zip(names, rec))


def call_dtypes(c):
    """The geometry dtype of each call ops.conv2d makes for case c (spr_pick_amd/ops.py: the storage bits follow the
    tensors' types where sprk_conv2d_storage16 says the call has a kernel for them) -> {"fwd", "bwd", "wg"}, or None
    where a call of the case would have to convert its tensors first: such a geometry is no case"""
    L = _lib()
    base = base_dtype(c)
    ep = L.ConvEpilogue(None, None, None, None, 0, 0, 0, 0, 1 if c.get("up_out") else 0)
    caps = int(L.lib().sprk_conv2d_storage16(ctypes.byref(case_geom(c, base)), ctypes.byref(ep)))
    x16, y16 = c["x16"], c["y16"]
    if c["kind"] == "wgrad":
        return None if (x16 and not caps & 4) else {"wg": base | (L.DT_X16 if x16 else 0)}
    if (x16 or y16) and not caps & 1:
        return None
    out = {"fwd": base | (L.DT_X16 if x16 else 0) | (L.DT_Y16 if y16 else 0)}
    if c["kind"] == "conv":
        if (x16 or y16) and not caps & 2:
            return None
        # backward-data reads the gradient in y's type and writes it in x's; backward-weight reads 16-bit tensors as
        # soon as one of x, gy is
        out["bwd"] = base | (L.DT_X16 if y16 else 0) | (L.DT_Y16 if x16 else 0)
        out["wg"] = base | (L.DT_X16 if ((x16 or y16) and caps & 4) else 0)
    return out


def planned(c):
    """The record of each call of case c, as sprk_conv2d_variant plans it -> {"fwd", "bwd", "wg"} (kind "fwd": the
    forward call alone; kind "wgrad": the backward-weight entry alone), or None (call_dtypes)"""
    L = _lib()
    dts = call_dtypes(c)
    if dts is None:
        return None
    out = {}
    if "fwd" in dts:
        ep = L.ConvEpilogue(None, None, None, None, 0, 0, 0, c.get("act", 0), 1 if c.get("up_out") else 0)
        out["fwd"] = as_dict(0, query(0, case_geom(c, dts["fwd"]), ctypes.byref(ep)))
    if "bwd" in dts:
        out["bwd"] = as_dict(1, query(1, case_geom(c, dts["bwd"])))
    if "wg" in dts:
        out["wg"] = as_dict(2, query(2, case_geom(c, dts["wg"])))
    return out


def valid(c, plan):
    """A case runs the 16-bit kernels in every call it makes but (kind conv) the backward-weight one, which the small
    layers leave to the fp32 kernels"""
    if plan is None:
        return False
    need = {"conv": ("fwd", "bwd"), "fwd": ("fwd",), "wgrad": ("wg",)}[c["kind"]]
    return all(plan[d]["stage"] == S16 for d in need)


# ---- what a record covers ---------------------------------------------------------------------------------------------
def _few(n):
    return "1" if n == 1 else "2" if n == 2 else "3+"


def inst(v):
    k = v["kind"]
    if k == 1:
        return ("mfma", v["T"], v["MT"], v["NT"], v["RB"])
    if k == 2:
        return ("tile", v["T"], v["NT"], v["X16"], v["Y16"])
    return ("head", v["T"], v["CQ"], v["CK"], v["X16"], v["Y16"])


def wg_inst(v):
    if v["kind"] == 1:
        return ("wg", v["T"], v["MC"], v["lgRW"], v["X16"], v["PL1"])
    return ("wg1x1", v["T"], v["wide"], v["X16"])


def unpack_pads(v):
    """-> (cshift, padL, padT) of a tile-kernel record"""
    return v["pads"] & 15, (v["pads"] >> 4) & 15, v["pads"] >> 8


def k_shape(v):
    """the K loop of a forward / backward-data record: (1 | 2 | 3+ chunks, the form of the last one)"""
    k = v["kind"]
    if k == 2:
        form = "c8_%d" % v["c8Last"]            # the last chunk's own group table: 9 or 18 groups
    elif k == 1:
        last = v["ckeLast"]
        form = "full" if last == v["CK"] else "one" if last % 8 == 1 else "short"   # 8 m + 1: a one-channel group
    else:
        form = "full"                            # Cin is a multiple of CK
    return (_few(v["nchunks"]), form)


def sw_shapes(v, C2):
    """where the K loop meets the second source (tile and mfma kernels); C2: the call's own second-source width"""
    n, s = v["nchunks"], v["straddle"]
    got = set()
    whole2 = v["whole2"] if v["kind"] == 1 else v["walk"] & 1
    if C2 == 0:
        got.add("none")
    else:
        if n == 1:
            got.add("one_chunk")
        if s == 0:
            got.add("boundary")
        elif n > 1:
            got.add("first" if s == 1 else "last" if s == n else "middle")
        if C2 == 1:
            got.add("C2=1")
        if whole2:
            got.add("whole2")
    return got


def p_shapes(v):
    """the tiles of a persistent workgroup of the tile kernel"""
    got = {"one" if v["tpwMax"] == 1 else "two" if v["tpwMax"] == 2 else "three+"}
    if v["tpwMin"] != v["tpwMax"]:
        got.add("uneven")
    if v["tpwMax"] > 1:     # a launch that walks a second tile
        got.add("mod8_zero" if v["ntiles"] % 8 == 0 else "mod8_nonzero")
        if v["walk"] & 2:
            got.add("next_same_group")
        if v["walk"] & 4:
            got.add("next_other_group")
        got.add("nblk" + _few(v["nblkN"]))
    return got


def p_class(v):
    return (_few(v["tpwMax"]), int(v["tpwMin"] != v["tpwMax"]), int(v["ntiles"] % 8 == 0))


def fwd_items(d, v, c):
    """what the forward (d = "fwd") or backward-data ("bwd") record v of case / call c covers"""
    got = {("inst",) + inst(v)}
    name = KIND_NAME[v["kind"]]
    C2 = c["C2"] if d == "fwd" else 0           # backward-data reads one tensor, gy
    if v["kind"] == 3:
        shape = (v["CQ"], v["CK"])
        got.add(("k", name, shape, k_shape(v)[0]))
        if d == "fwd":
            if c["Cout"] in HEAD_COUTS:
                got.add(("head", "Cout", c["Cout"]))
            if c["Cout"] % 16:
                got.add(("head", "cut_tile", v["CQ"]))
        if v["lastPixels"] != 64 * (8 // v["CQ"]):
            got.add(("head", "ragged_pixels", v["CQ"]))
        got.add(("head", "quarters", v["CQ"], v["quarters"], "full" if v["lastQuarterCh"] == 96 else "cut"))
        return got
    got.add(("k", name) + k_shape(v))
    got.update(("sw", name, s) for s in sw_shapes(v, C2))
    if v["kind"] == 1:
        got.add(("mfma", "taps", v["taps"]))
        got.add(("mfma", "up2", v["up2"]))
        return got
    x16 = v["X16"]
    got.update(("p", x16, s) for s in p_shapes(v))
    got.add(("shape", v["lgTC"], v["lgTR"], v["NI"]))
    TC, TR = 1 << v["lgTC"], 1 << v["lgTR"]
    if c["W"] % TC:
        got.add(("edge", "right"))
    if c["H"] % TR:
        got.add(("edge", "bottom"))
    if c["N"] % v["NI"]:
        got.add(("edge", "image_group"))
    cshift, padL, padT = unpack_pads(v)
    assert cshift == (padL & 1 if x16 else 0)
    got.add(("padL", x16, padL))
    got.add(("padT", d, min(padT, 3)))
    if v["Y16"]:
        got.add(("store", ("none", "mixed", "all")[v["store"]], v["up2"]))
    return got


def wg_items(v, c):
    got = {("inst",) + wg_inst(v)}
    if v["kind"] == 2:
        if v["lastPart"] < v["perPart"]:
            got.add(("wg1", "short_last_part"))
        wide = v["wide"]
        CO, CI = (192, 192) if wide else (96, 384)
        got.add(("wg1", "coBlocks", "1" if v["coBlocks"] == 1 else "2+"))
        got.add(("wg1", "ciBlocks", "1" if v["ciBlocks"] == 1 else "2+"))
        if v["lastCo"] < CO and v["coBlocks"] > 1:
            got.add(("wg1", "ragged_co"))
        if v["lastCi"] < CI and v["ciBlocks"] > 1:
            got.add(("wg1", "ragged_ci"))
        return got
    got.add(("wg", "seg", "1" if v["seg"] == 1 else "2+"))
    got.add(("wg", "units", _few(v["upwMax"])))
    if v["upwMin"] != v["upwMax"]:
        got.add(("wg", "units", "uneven"))
    got.add(("wg", "nBlocks", _few(v["nBlocks"])))
    if v["straddle"]:
        got.add(("wg", "straddle"))
    if v["tail"]:
        cin = c["C1"] + c["C2"]
        got.add(("wg", "tail", v["tailSrc"], "49" if cin == 49 else "97" if cin == 97 else "145+"))
        if v["tailSrc"] == 2 and c["C2"] > 48:
            got.add(("wg", "tail_behind_wide_C2"))
    got.add(("wg", "regX", "1" if v["regX"] == 1 else "2+"))
    got.add(("wg", "padT", v["padT"]))
    got.add(("wg", "padL", v["padL"]))
    return got


def work_fwd(d, v):
    """a workload call's kernel (its template arguments but the operand type: a loop shape needs one type only) with its
    K-loop shape, and (tile kernel) with its persistence class"""
    kern = inst(v)[:1] + inst(v)[2:]
    got = {("wk", d) + kern + (k_shape(v), v.get("straddle", 0) and min(v["straddle"], 2))}
    if v["kind"] == 2:
        got.add(("wp",) + kern + (p_class(v), v["store"], v["up2"]))
    return got


def work_wg(v):
    """... a backward-weight call's kernel with its channel-block shape, and with its units per workgroup"""
    kern = wg_inst(v)[:1] + wg_inst(v)[2:]
    if v["kind"] == 2:
        return {("ww",) + kern + (v["coBlocks"] > 1, v["ciBlocks"] > 1, v["lastPart"] < v["perPart"])}
    return {("ww",) + kern + (_few(v["nBlocks"]), v["tailSrc"], v["straddle"]), ("wu",) + kern[:4] + (v["seg"] > 1, _few(v["upwMax"]))}


def items(plan, c):
    """Everything a case c with this plan covers"""
    got = set()
    for d in ("fwd", "bwd"):
        v = plan.get(d)
        if v and v["stage"] == S16:
            got |= fwd_items(d, v, c) | work_fwd(d, v)
    v = plan.get("wg")
    if v and v["stage"] == S16:
        got |= wg_items(v, c) | work_wg(v)
    return got


def tile_shapes():
    """every (lgTC, lgTR, NI) plan_tile gives, asked of the library on a grid of planes up to 128 x 128"""
    L = _lib()
    out = set()
    for H in range(1, 130):
        for W in range(4, 133, 4):
            n = max(1, -(-131072 // (H * W)))
            v = as_dict(0, query(0, L.ConvGeom(n, 3, 0, H, W, 0, 33, H, W, 3, 3, 1, 1, 1, 1, 1 | L.DT_FORCE)))
            if v["stage"] == S16 and v["kind"] == 2:
                out.add((v["lgTC"], v["lgTR"], v["NI"]))
    return sorted(out)


_SHAPES = None


def all_items(work=None):
    """The item table"""
    global _SHAPES
    if _SHAPES is None:
        _SHAPES = tile_shapes()
    want = {("inst", "mfma") + k for k in MFMA_TABLE} | {("inst", "tile") + k for k in TILE_TABLE}
    want |= {("inst", "head") + k for k in HEAD_TABLE} | {("inst", "wg") + k for k in WG_TABLE}
    want |= {("inst", "wg1x1") + k for k in WG1_TABLE}
    want.update(("k", "tile", n, f) for n in ("1", "2", "3+") for f in ("c8_1", "c8_2"))
    want.update(("k", "mfma", n, f) for n in ("1", "2", "3+") for f in ("full", "short", "one"))
    want.update(("k", "head", s, n) for s in HEAD_SHAPES for n in ("1", "2", "3+"))
    want.update(("sw", k, s) for k in ("tile", "mfma") for s in SW_SHAPES)
    want.update(("mfma", "taps", t) for t in (1, 9))
    want.update(("mfma", "up2", u) for u in (0, 1))
    want.update(("p", x, s) for x in BITS for s in P_SHAPES)
    want.update(("shape",) + s for s in _SHAPES)
    want.update(("edge", e) for e in ("right", "bottom", "image_group"))
    want.update(("padL", x, p) for x in BITS for p in PADS)
    want.update(("padT", d, p) for d in ("fwd", "bwd") for p in (0, 1, 2, 3))
    want.update(("store", s, u) for s in ("none", "mixed", "all") for u in (0, 1))
    want.update(("head", "Cout", n) for n in HEAD_COUTS)
    want.update(("head", w, cq) for w in ("cut_tile", "ragged_pixels") for cq in (1, 4))
    # Cout 97..192 leaves quarters 2 and 3 empty, 193..288 quarter 3; the last one that stores is full or cut
    want.update(("head", "quarters", 4, q, f) for q in (2, 3, 4) for f in ("full", "cut"))
    want.update(("head", "quarters", 1, 1, f) for f in ("full", "cut"))
    want.update(("wg", "seg", s) for s in ("1", "2+"))
    want.update(("wg", "units", s) for s in ("1", "2", "3+", "uneven"))
    want.update(("wg", "nBlocks", s) for s in ("1", "2", "3+"))
    want.add(("wg", "straddle"))
    want.update(("wg", "tail", src, n) for src in (1, 2) for n in ("49", "97", "145+"))
    want.add(("wg", "tail_behind_wide_C2"))
    want.update(("wg", "regX", s) for s in ("1", "2+"))
    want.update(("wg", p, n) for p in ("padT", "padL") for n in PADS)
    want.add(("wg1", "short_last_part"))
    want.update(("wg1", b, n) for b in ("coBlocks", "ciBlocks") for n in ("1", "2+"))
    want.update(("wg1", r) for r in ("ragged_co", "ragged_ci"))
    want.update(workload_items() if work is None else work)
    return want


# Items the code rules out, each with its rule (csrc/conv16.hip, csrc/wgrad16.hip, csrc/corr.h).  Pinned here: the search
# fails on any other item it cannot reach, so nothing lands in the fixture's list because the grid was too small.
MIRROR = "Corr(g): backward-data mirrors the pad to K - 1 - pad, and a pad of the layer is >= 0: at most 2"
HEAD_64 = "head_shape: CQ 4 takes CK 64 as soon as C1 % 64 == 0, so two chunks of 32 (C1 = 64) run as one of 64"
ONE_CHUNK = "plan16: a single chunk is CK = roundup(Ck, 8) channels wide: all of it, or all but the one odd channel of Ck = 8 m + 1"
RULED_OUT = {
    ("padT", "bwd", 3): MIRROR,
    ("k", "mfma", "1", "short"): ONE_CHUNK,
    ("k", "head", (4, 32), "2"): HEAD_64,
}


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def seed_of(name):
    return zlib.crc32(name.encode()) % 10000


def guard_images(t):
    """leading guard images that keep the inner slice of ``t`` 16-byte aligned: the fewest (at least one) whose
    elements are a multiple of 16 bytes"""
    per = t[0].numel() * t.element_size()
    n = 1
    while (n * per) % 16:
        n += 1
    return n


def guarded(t, device):
    """A copy of ``t`` (any storage type) on the device as the inner slice along N of a buffer whose outer images are
    NaN: a read that strays into a neighbouring image shows in the result"""
    import torch
    lead = guard_images(t)
    buf = torch.full((t.shape[0] + lead + 1,) + tuple(t.shape[1:]), float("nan"), dtype=t.dtype, device=device)
    buf[lead:-1].copy_(t)
    v = buf[lead:-1]
    assert v.is_contiguous() and v.data_ptr() % 16 == 0
    return v


def tensors(c):
    """CPU fp32 tensors of case c from the seed of its name -> x, x2 | None, w, b | None, gy (of y's shape)"""
    import numpy as np
    import torch
    g = torch.Generator().manual_seed(seed_of(c.get("seed", c["name"])))
    x = torch.randn(c["N"], c["C1"], c["H"], c["W"], generator=g)
    x2 = torch.randn(c["N"], c["C2"], c["H"], c["W"], generator=g) if c["C2"] else None
    cin = c["C1"] + c["C2"]
    w = torch.randn(c["Cout"], cin, c["K"], c["K"], generator=g) / np.sqrt(cin * c["K"] ** 2)
    b = torch.randn(c["Cout"], generator=g) * 0.1 if c.get("bias") else None
    m = 2 if c.get("up_out") else 1
    gy = torch.randn(c["N"], c["Cout"], c["H"] * m, c["W"] * m, generator=g)
    return x, x2, w, b, gy


# ---- the exact model (tests/test_gpu_ops.py: test_conv2d_16bit_operands / test_conv2d_16bit_storage) ------------------
def torch_type(dt):
    import torch
    return torch.bfloat16 if dt == "bf16" else torch.float16


def act_fn(act):
    import torch.nn.functional as F
    return (lambda t: F.leaky_relu(t, 0.1)) if act == 1 else F.relu if act == 2 else (lambda t: t)


def ref_conv(x, x2, w, b, pad, K):
    import torch
    import torch.nn.functional as F
    xin = x if x2 is None else torch.cat((x, x2), 1)
    pt, pb, pl, pr = pad
    return F.conv2d(F.pad(xin, (pl, pr, pt, pb)), w, b)


def model_forward(c, x, x2, w, b, prec):
    """y of the exact model in precision ``prec``: act(conv(round16(x), round16(w)) + b), before the store's rounding"""
    t = torch_type(c["dt"])
    r = lambda v: None if v is None else v.to(t).to(prec)
    return act_fn(c["act"])(ref_conv(r(x), r(x2), r(w), None if b is None else b.to(prec), c["pad"], c["K"]))


def model_gpre(c, y_dev, gy):
    """The pre-activation gradient as act_bwd leaves it (fp32 product with the mask of the DEVICE's own y, 2 x 2 sums of
    an up-sampled gradient first), and as backward-data / backward-weight then read it: rounded to the operand type
    -> (gpre in fp64 before the rounding, gpre as read in fp64)"""
    import torch
    t = torch_type(c["dt"])
    g = gy.to(t).double() if c["y16"] else gy.double()      # the gradient arrives in y's storage type
    if c.get("up_out"):
        g = (g[:, :, 0::2, 0::2] + g[:, :, 0::2, 1::2]) + (g[:, :, 1::2, 0::2] + g[:, :, 1::2, 1::2])
    if c["act"]:
        g = torch.where(y_dev.double() > 0, g, g * (0.1 if c["act"] == 1 else 0.0))
    return g, g.float().to(t).double()


def model_gin(c, w, gpre16, prec):
    import torch.nn.functional as F
    t = torch_type(c["dt"])
    pt, pb, pl, pr = c["pad"]
    full = F.conv_transpose2d(gpre16.to(prec), w.to(t).to(prec))
    # (a pad beyond K - 1 crops the input: the cropped rows and columns receive no gradient)
    return full[:, :, pt:pt + c["H"], pl:pl + c["W"]]


def model_gw(c, x, x2, gpre16, prec):
    import torch
    import torch.nn.functional as F
    t = torch_type(c["dt"])
    r = lambda v: v.to(t).to(prec)
    xin = r(x) if x2 is None else torch.cat((r(x), r(x2)), 1)
    pt, pb, pl, pr = c["pad"]
    xp = F.pad(xin, (pl, pr, pt, pb))
    return torch.nn.grad.conv2d_weight(xp, (c["Cout"], xin.shape[1], c["K"], c["K"]), gpre16.to(prec))


# The budgets of those two tests, per quantity: |got - ref| <= rel_ref * |ref| + rel_max * max |ref|
def budget(c, what, plan):
    u = unit_roundoff(c["dt"])
    if what == "y":
        return (u * 1.001 if c["y16"] else 0.0), 2e-5
    if what == "gin":
        if c.get("up_out"):
            return (8 * u * 1.001 if c["x16"] else 0.0), 8 * u
        return (u * 1.001 if c["x16"] else 0.0), 5e-5
    if what == "gw":
        return 0.0, (1e-4 if plan["wg"]["stage"] == S16 else 8 * u)
    return 0.0, 5e-5        # gb


def ratio(got, ref, bud):
    """worst |got - ref| over its budget, every element compared"""
    rel_ref, rel_max = bud
    err = (got.double() - ref.double()).abs()
    return float((err / (rel_ref * ref.double().abs() + rel_max * ref.double().abs().max())).max())


# ---- the explicit list: epilogue forms -------------------------------------------------------------------------------
def epilogue_cases():
    """act 0 / 1 / 2 x bias | scale + shift | neither x up2 where the kind has it, fp32 and 16-bit output where the kind
    has it, on two geometries per kernel kind: forward calls"""
    geoms = {
        # (a partial right tile column; a partial last image group: with 16-bit output both stores run in one launch)
        "tile": ((dict(N=66, C1=5, C2=0, H=8, W=72, Cout=41, K=3, pad=[2, 0, 1, 1], dt="bf16"),
                  dict(N=259, C1=7, C2=3, H=16, W=16, Cout=75, K=3, pad=[1, 1, 1, 1], dt="f16")), (0, 1), (0, 1)),
        "head": ((dict(N=130, C1=32, C2=0, H=20, W=16, Cout=41, K=1, pad=[0, 0, 0, 0], dt="f16"),
                  dict(N=43, C1=64, C2=0, H=20, W=16, Cout=200, K=1, pad=[0, 0, 0, 0], dt="bf16")), (0,), (0, 1)),
        "mfma": ((dict(N=3, C1=9, C2=0, H=16, W=16, Cout=41, K=3, pad=[2, 0, 1, 1], dt="bf16"),
                  dict(N=5, C1=16, C2=8, H=16, W=32, Cout=75, K=1, pad=[0, 0, 0, 0], dt="f16")), (0, 1), (0,)),
    }
    out = []
    for kind, (gs, ups, y16s) in geoms.items():
        for i, base in enumerate(gs):
            for up, y16, act, ep in itertools.product(ups, y16s, (0, 1, 2), ("bias", "affine", "none")):
                name = "ep %s%d %s%s act%d %s" % (kind, i, "y16" if y16 else "y32", " up2" if up else "", act, ep)
                # (seed: the forms of a geometry share their tensors, so the test computes the fp64 convolution once)
                out.append(dict(base, name=name, seed="ep %s%d" % (kind, i), kind="fwd", want=kind, x16=y16, y16=y16, up_out=bool(up),
                                act=act, ep=ep, bias=False))
    return out


def epilogue_plan(e):
    return planned(e)["fwd"]


# ---- the workload ----------------------------------------------------------------------------------------------------
def suite_table():
    """CONV16_CASES and STORE16_CASES of tests/test_gpu_ops.py as cases, both operand types"""
    import test_gpu_ops
    out = []
    for dt in ("bf16", "f16"):
        for r in test_gpu_ops.CONV16_CASES:
            out.append(dict(name=r[0] + " " + dt, kind="conv", N=r[1], C1=r[2], C2=r[3], H=r[4], W=r[5], Cout=r[6], K=r[7], pad=list(r[8]),
                            act=r[9], bias=bool(r[10]), up_out=bool(r[11]), dt=dt, x16=0, y16=0))
        for r in test_gpu_ops.STORE16_CASES:
            out.append(dict(name=r[0] + " " + dt, kind="conv", N=r[1], C1=r[2], C2=r[3], H=r[4], W=r[5], Cout=r[6], K=r[7], pad=list(r[8]),
                            act=r[9], bias=bool(r[10]), up_out=bool(r[11]), dt=dt, x16=int(r[12] == "16"), y16=int("fp32 out" not in r[0])))
    return out


def suite_items():
    """what those two tables reach through the query: per direction whatever record its call gets (a table case whose
    backward calls leave the 16-bit stage still counts with its forward call)"""
    got = set()
    for c in suite_table():
        plan = planned(c) or planned(dict(c, kind="fwd")) or {}
        got |= items(plan, c)
    return got


def workload_calls():
    """Every 16-bit-stage call of the 16-bit configurations of tests/golden/unet_trace.json at per-GPU batch 4, 16 and
    32 (each call's own geometry and dtype bits, its image count re-scaled from the configuration's batch), and of
    WS_GEOMS of tests/test_abi.py under both operand types -> [(which, record, note, geometry fields)]"""
    L = _lib()
    out, seen = [], set()

    def visit(which, fields, up2, note):
        key = (which, tuple(fields), up2)
        if key in seen:
            return
        seen.add(key)
        ep = L.ConvEpilogue(None, None, None, None, 0, 0, 0, 0, up2)
        v = as_dict(which, query(which, L.ConvGeom(*fields), ctypes.byref(ep) if which == 0 else None))
        if v["stage"] == S16:
            out.append((which, v, note, list(fields)))

    trace = json.load(open(os.path.join(HERE, "golden", "unet_trace.json")))
    for cfg in WORK_CONFIGS:
        base = int(re.fullmatch(r".*-(\d+)x\d+", cfg).group(1))
        for call in trace[cfg]["calls"]:
            which = {"conv2d_fwd": 0, "conv2d_bwd_data": 1, "conv2d_bwd_weight": 2}.get(call[0])
            if which is None:
                continue
            geom = next(a for a in call[1] if isinstance(a, list) and len(a) == 16)
            rest = [a for a in call[1] if not isinstance(a, list)]
            up2 = int(rest[-2]) if which == 0 else 0
            for batch in BATCHES:
                f = list(geom)
                f[0] = geom[0] * batch // base
                if f[0] > 0:
                    visit(which, f, up2, "%s %s at batch %d" % (cfg, call[0], batch))
    import test_abi
    for (N, C1, C2, H, W, up1, Cout, K, stride, dil, (pt, pb, pl, pr)) in test_abi.WS_GEOMS:
        Ho = (H + pt + pb - dil * (K - 1) - 1) // stride + 1
        Wo = (W + pl + pr - dil * (K - 1) - 1) // stride + 1
        for n in sorted({N} | ({N // 4 * b for b in BATCHES} if N % 4 == 0 else set())):
            for which, dt in itertools.product((0, 1, 2), (1, 2)):
                visit(which, [n, C1, C2, H, W, up1, Cout, Ho, Wo, K, K, stride, dil, pt, pl, dt], 0, "WS_GEOMS at N = %d" % n)
    return out


_WORK = None


def workload_items():
    """{item: a call that reaches it}"""
    global _WORK
    if _WORK is None:
        _WORK = {}
        for which, v, note, fields in workload_calls():
            for it in (work_wg(v) if which == 2 else work_fwd("bwd" if which else "fwd", v)):
                _WORK.setdefault(it, (note, fields))
    return _WORK


# ---- the search -----------------------------------------------------------------------------------------------------
# A bounded grid, walked unit by unit: the K loop depends on the channel counts alone, the persistence shape on the
# tile count and the channel blocks, the borders on the pads and the plane, so each unit crosses its own axes in full
# with a few values of the others.  The floors are small (128 workgroups of 512 pixels; 512 regions of 128 pixels; 1024
# of 64), so with 33..48 outputs and <= 16 inputs a case is a few 1e8 multiply-adds.
GRID = {
    "k_C1": [1, 50], "k_C2": [0, 20], "k_plane": [256, 16, 16],                # N, H, W: 128 tiles of two images
    "k_bwd_Cout": [33, 100], "k_bwd_C": [[33, 0], [33, 5], [40, 9]],
    "p_planes": [[16, 16], [16, 32], [8, 64], [32, 32], [64, 64], [256, 256], [256, 512], [512, 512]],
    "p_tiles": [128, 129, 136, 255, 256, 257, 260, 264, 384, 385, 392, 512, 513, 520, 600, 768, 769, 776, 800, 1024, 1025, 1032],
    "p_Cout": [33, 97, 193, 200],
    "shape_H": [4, 5, 8, 12, 16, 20, 32, 40, 64, 68, 128], "shape_W": [4, 8, 12, 16, 20, 32, 36, 64, 68, 128, 132],
    "pad_layers": [[3, 0, 33], [34, 2, 40]], "pad_planes": [[16, 16], [32, 64]],
    "head_C1": [32, 64, 96, 128, 160, 192, 384], "head_Cout": [33, 40, 96, 97, 100, 192, 193, 200, 288, 300, 384],
    "head_planes": [[16, 16], [20, 16], [16, 32]], "head_N": [32, 33, 64, 65, 128, 129, 256],
    "mfma_C": [[8, 0], [9, 0], [16, 0], [17, 0], [24, 0], [33, 0], [40, 0], [48, 0], [8, 1], [8, 8], [9, 8], [16, 1], [16, 8], [12, 4],
               [20, 4], [16, 16], [16, 17], [32, 1], [40, 8], [1, 8], [1, 0], [32, 0], [64, 0], [128, 0]],
    "mfma_Cout": [33, 48, 49, 64, 65, 96, 97, 130, 200],
    "mfma_planes": [[16, 16], [16, 32], [32, 32], [16, 64], [64, 64], [8, 32], [4, 64], [128, 64], [20, 16]],
    "mfma_N": [1, 2, 3, 4, 16, 17, 65, 128, 256, 513],
    "wg_planes": [[8, 16], [16, 16], [4, 32], [8, 32], [32, 32], [2, 64], [4, 64], [64, 64], [256, 64], [64, 128], [2, 128]],
    "wg_regions": [512, 513, 520, 768, 770, 1024, 1030, 1536, 1540],
    "wg_C1": [1, 16, 33, 47, 48, 49, 50, 96, 97, 98, 144, 145], "wg_C2": [0, 1, 2, 48, 49, 60, 96, 97],
    "wg_Cout": [33, 48, 49, 96],
    "wg1_C1": [97, 104, 192, 193, 200, 384, 385, 400, 768, 770], "wg1_Cout": [33, 40, 96, 97, 130, 192, 193, 200, 384, 400],
    "wg1_planes": [[8, 8], [16, 16], [24, 48]], "wg1_regions": [1024, 1025, 1030, 1100, 1280, 1290, 2048],
    "max_case_macs": MAX_CASE_MACS, "max_total_macs": MAX_TOTAL_MACS,
}
STORAGE = ((0, 0), (1, 1), (1, 0), (0, 1))


def _case(kind, N, C1, C2, H, W, Cout, K=3, pad=None, dt="bf16", x16=0, y16=0, up_out=False):
    pad = list(pad) if pad is not None else ([2, 0, 1, 1] if K == 3 else [0, 0, 0, 0])
    return dict(kind=kind, N=N, C1=C1, C2=C2, H=H, W=W, Cout=Cout, K=K, pad=pad, dt=dt, x16=x16, y16=y16, up_out=bool(up_out),
                act=(N + C1 + Cout) % 3, bias=bool((C1 + Cout) % 3))


def _alternate(*key):
    """operand type and storage of a geometry of a unit: each loop-shape item needs one of them only, so they alternate
    (by a checksum of the geometry, so that neither is tied to an axis of the grid)"""
    i = zlib.crc32(repr(key).encode())
    return ("bf16", "f16")[i % 2], STORAGE[(i // 2) % 4]


def grid_units():
    return ["k", "p", "shape", "pad", "store", "head", "mfma", "wg", "wg1x1", "inst"]


def grid_cases(unit):
    G = GRID
    if unit == "k":             # every channel pair of the grid on 128 tiles; the forward call alone where C1 + C2 < 33
        N, H, W = G["k_plane"]
        for C1 in range(G["k_C1"][0], G["k_C1"][1] + 1):
            for C2 in range(G["k_C2"][0], G["k_C2"][1] + 1):
                dt, (x16, y16) = _alternate(C1, C2)
                yield _case("conv" if C1 + C2 >= 33 else "fwd", N, C1, C2, H, W, 33, dt=dt, x16=x16, y16=y16)
        # ... and as the backward-data call sees them: the layer's Cout is its K
        for (C1, C2), Cout in itertools.product(G["k_bwd_C"], range(G["k_bwd_Cout"][0], G["k_bwd_Cout"][1] + 1)):
            dt, (x16, y16) = _alternate(C1, C2, Cout)
            yield _case("conv", N, C1, C2, H, W, Cout, dt=dt, x16=x16, y16=y16)
    elif unit == "p":           # tile counts x channel blocks: the forward call of a 2-channel layer
        for (H, W), tiles, Cout in itertools.product(G["p_planes"], G["p_tiles"], G["p_Cout"]):
            per = max(1, (H * W) // 512)
            ni = max(1, 512 // (H * W))
            for N in sorted({max(1, tiles // per) * ni, -(-tiles // per) * ni, max(1, tiles // per) * ni - (ni > 1)}):
                dt, (x16, y16) = _alternate(H, W, N, Cout)
                yield _case("fwd", N, 2, 0, H, W, Cout, dt=dt, x16=x16, y16=y16)
    elif unit == "shape":       # every plane of the grid at its floor, and one image more
        for H, W in itertools.product(G["shape_H"], G["shape_W"]):
            if H * W < 256:
                continue
            n = -(-65536 // (H * W))
            for N, (x16, y16) in itertools.product((n, n + 1, 2 * n + 1), STORAGE):   # (16-bit input has wider halo rows: PX)
                dt, _ = _alternate(H, W, N, x16, y16)
                yield _case("fwd", N, 3, 0, H, W, 33, dt=dt, x16=x16, y16=y16)
    elif unit == "pad":
        for (C1, C2, Cout), (H, W), pt, pl, dt, (x16, y16) in itertools.product(G["pad_layers"], G["pad_planes"], PADS, PADS, ("bf16", "f16"),
                                                                               ((0, 0), (1, 1))):
            N = -(-65536 // (H * W)) + 1
            yield _case("conv" if C1 + C2 >= 33 else "fwd", N, C1, C2, H, W, Cout, pad=(pt, 2 - pt, pl, 2 - pl), dt=dt, x16=x16, y16=y16)
    elif unit == "store":       # the two stores of 16-bit output x up2
        for (H, W), extra, up, (x16, y16), dt, Cout in itertools.product(
                ((16, 16), (32, 32), (20, 32), (32, 36), (16, 12), (16, 20), (64, 64)), (0, 1), (0, 1), STORAGE, ("bf16", "f16"), (33, 49)):
            N = -(-65536 // (H * W)) + extra
            yield _case("fwd", N, 3, 0, H, W, Cout, dt=dt, x16=x16, y16=y16, up_out=up)
            yield _case("conv", N, 33, 0, H, W, Cout, dt=dt, x16=x16, y16=y16, up_out=up)
    elif unit == "head":
        for C1, Cout, (H, W), N in itertools.product(G["head_C1"], G["head_Cout"], G["head_planes"], G["head_N"]):
            dt, (x16, y16) = _alternate(C1, Cout, H, W, N)
            yield _case("conv", N, C1, 0, H, W, Cout, K=1, dt=dt, x16=x16, y16=y16)
            yield _case("fwd", N, C1, 0, H, W, Cout, K=1, dt=dt, x16=x16, y16=y16)
    elif unit == "mfma":        # what the other two refuse: fp32 tensors only
        for K, (C1, C2), Cout, (H, W), N, up in itertools.product((1, 3), G["mfma_C"], G["mfma_Cout"], G["mfma_planes"], G["mfma_N"], (0, 1)):
            if up and (Cout != 33 or N > 4):
                continue
            dt, _ = _alternate(K, C1, C2, Cout, H, W, N)
            yield _case("conv" if C1 + C2 >= 33 else "fwd", N, C1, C2, H, W, Cout, K=K, dt=dt, up_out=up)
    elif unit == "wg":
        for (H, W), regions, C1, C2, Cout in itertools.product(G["wg_planes"], G["wg_regions"], G["wg_C1"], G["wg_C2"], G["wg_Cout"]):
            N = -(-regions * 128 // (H * W))
            dt, (x16, _) = _alternate(H, W, N, C1, C2, Cout)
            pads = itertools.product(PADS, PADS) if (C1 in (1, 33) and C2 in (0, 2) and Cout in (33, 49) and regions == 512) else ((2, 1), (1, 2))
            for pt, pl in pads:
                yield _case("wgrad", N, C1, C2, H, W, Cout, pad=(pt, 2 - pt, pl, 2 - pl), dt=dt, x16=x16)
    elif unit == "wg1x1":
        for (H, W), regions, C1, Cout in itertools.product(G["wg1_planes"], G["wg1_regions"], G["wg1_C1"], G["wg1_Cout"]):
            N = -(-regions * 64 // (H * W))
            dt, (x16, _) = _alternate(H, W, N, C1, Cout)
            yield _case("wgrad", N, C1, 0, H, W, Cout, K=1, dt=dt, x16=x16)
    else:                       # every storage combination and both operand types on a few geometries of each family
        for dt, (x16, y16) in itertools.product(("bf16", "f16"), STORAGE):
            for Cout in (33, 49):
                yield _case("fwd", 256, 3, 0, 16, 16, Cout, dt=dt, x16=x16, y16=y16)
            for C1, Cout in ((64, 100), (32, 100), (32, 40)):
                yield _case("fwd", 64, C1, 0, 20, 16, Cout, K=1, dt=dt, x16=x16, y16=y16)
            for (H, W), Cout, pl in itertools.product(((8, 16), (4, 32), (2, 64)), (33, 49), (1, 2)):
                yield _case("wgrad", 512, 1, 0, H, W, Cout, pad=(2, 0, pl, 2 - pl), dt=dt, x16=x16)
            for Cout in (33, 97):
                yield _case("wgrad", 1024, 97, 0, 8, 8, Cout, K=1, dt=dt, x16=x16)


def describe(c):
    src = "%d" % c["C1"] + ("+%d" % c["C2"] if c["C2"] else "")
    return "%s%s %s->%d %dx%d @%dx%d N%d pad%s x%d y%d%s" % (
        {"wgrad": "wgrad ", "fwd": "fwd "}.get(c["kind"], ""), c["dt"], src, c["Cout"], c["K"], c["K"], c["H"], c["W"], c["N"],
        tuple(c["pad"]), 16 if c["x16"] else 32, 16 if c["y16"] else 32, " up_out" if c.get("up_out") else "")


def _rank(cost, c):
    return (cost, json.dumps(c, sort_keys=True))      # ties broken the same way whatever the order of the scan


def scan(cases):
    """-> (geometries seen, {item: (rank, case, plan)}: the cheapest case per coverage item)"""
    best, n = {}, 0
    for c in cases:
        n += 1
        plan = planned(c)
        if not valid(c, plan):
            continue
        cost, rank = macs(c), None
        for it in items(plan, c):
            if it not in best or cost <= best[it][0][0]:
                rank = rank or _rank(cost, c)
                if it not in best or rank < best[it][0]:
                    best[it] = (rank, c, plan)
    return n, best


def search(out=FIXTURE, verbose=True):
    best, n = {}, 0
    for cases in [grid_cases(u) for u in grid_units()]:
        k, part = scan(cases)
        n += k
        for it, rec in part.items():
            if it not in best or rec[0] < best[it][0]:
                best[it] = rec
    want = all_items()
    best = {it: (rank[0], c, plan) for it, (rank, c, plan) in best.items() if it in want}
    if verbose:
        print("grid: %d geometries, %d coverage items reached of %d" % (n, len(best), len(want)), file=sys.stderr)
    # the dearest first (a dear case usually brings cheap items along)
    chosen, covered = [], set()
    for it in sorted(best, key=lambda it: (-best[it][0], str(it))):
        if it in covered:
            continue
        cost, c, plan = best[it]
        chosen.append(dict(c, name=describe(c), macs=cost, plan=plan))
        covered |= items(plan, c)
    # drop what the later choices made redundant, the dearest first: every case left is the only one for some item
    for c in sorted(chosen, key=lambda c: -c["macs"]):
        rest = set().union(*(items(o["plan"], o) for o in chosen if o is not c))
        if items(c["plan"], c) & want <= rest:
            chosen.remove(c)
    chosen.sort(key=lambda c: (c["macs"], c["name"]))
    total = sum(c["macs"] for c in chosen)
    missing = sorted(want - covered, key=str)
    unruled = [i for i in missing if i not in RULED_OUT]
    assert not unruled, "items the grid does not reach and no rule excludes:\n%s" % "\n".join(
        "%s %s" % (i, workload_items().get(i, "")) for i in unruled)
    stale = [i for i in RULED_OUT if i in covered]
    assert not stale, "ruled out, yet a case reaches it: %s" % stale
    over = {c["name"]: c["macs"] for c in chosen if c["macs"] > MAX_CASE_MACS}
    fx = {
        "comment": "written by tests/conv16_variant_cases.py --search; do not edit by hand",
        "grid": GRID,
        "total_macs": total,
        "tile_shapes": [list(s) for s in _SHAPES],
        "cases": chosen,
        # cases whose item's eligibility floor forces more than max_case_macs: the cheapest eligible geometry, with its cost
        "above_case_bound": over,
        "epilogue_cases": [dict(e, plan=epilogue_plan(e)) for e in epilogue_cases()],
        "unreached": [dict(item=list(i), why=RULED_OUT[i]) for i in missing],
        "coverage": coverage(chosen),
    }
    old = load() if os.path.exists(FIXTURE) else {}
    if "margin" in old:
        names = {c["name"] for c in chosen}
        fx["margin"] = {k: v for k, v in old["margin"].items() if k in names}
    assert total <= MAX_TOTAL_MACS, total
    with open(out, "w") as f:
        json.dump(fx, f, indent=1, sort_keys=True)
        f.write("\n")
    if verbose:
        print("%d cases, %.3g multiply-adds in all (dearest %.3g, %d above the per-case bound); %d items ruled out" % (
            len(chosen), total, max(c["macs"] for c in chosen), len(over), len(missing)), file=sys.stderr)
    return fx


# ---- the exact model in fp32 on the CPU against fp64: are the budgets wide enough for a correct result? ---------------
def margin_of(c):
    """{quantity: worst |fp32 model - fp64 model| over its budget} of case c; the activation mask is the fp64 model's
    own y (rounded as the store rounds it) for both.  A 16-bit store's own rounding is no part of this: a correct
    round-to-nearest uses all of the u |ref| the budget grants it, so the un-rounded fp32 result is held to the rest of
    the budget alone, the share of max |ref|."""
    summing = lambda bud: (0.0, bud[1])
    import torch
    t = torch_type(c["dt"])
    x, x2, w, b, gy = tensors(c)
    plan = c["plan"]
    out = {}
    if c["kind"] == "wgrad":
        g16 = gy.to(t).double()
        out["gw"] = ratio(model_gw(c, x, x2, g16, torch.float32), model_gw(c, x, x2, g16, torch.float64), (0.0, 1e-4))
        return out
    y64 = model_forward(c, x, x2, w, b, torch.float64)
    y32 = model_forward(c, x, x2, w, b, torch.float32)
    out["y"] = ratio(y32, y64, summing(budget(c, "y", plan)))
    if c["kind"] == "conv":
        y_dev = y64.to(t) if c["y16"] else y64.float()
        gpre, g16 = model_gpre(c, y_dev, gy)
        gin32 = model_gin(c, w, g16, torch.float32)
        out["gin"] = ratio(gin32, model_gin(c, w, g16, torch.float64), summing(budget(c, "gin", plan)))
        if plan["wg"]["stage"] == S16:
            out["gw"] = ratio(model_gw(c, x, x2, g16, torch.float32), model_gw(c, x, x2, g16, torch.float64), budget(c, "gw", plan))
        if b is not None:
            out["gb"] = ratio(gpre.float().sum((0, 2, 3)), gpre.sum((0, 2, 3)), budget(c, "gb", plan))
    return out


def margin(path=FIXTURE):
    import time
    fx = load()
    out, slow, t0 = {}, (0, ""), time.time()
    for c in fx["cases"]:
        t1 = time.time()
        out[c["name"]] = margin_of(c)
        slow = max(slow, (time.time() - t1, c["name"]))
        print("%-70s %s" % (c["name"], " ".join("%s %.3f" % kv for kv in out[c["name"]].items())), file=sys.stderr)
    print("all references (fp32 and fp64): %.1f s, the slowest %.1f s (%s)" % (time.time() - t0, slow[0], slow[1]), file=sys.stderr)
    fx["margin"] = out
    with open(path, "w") as f:
        json.dump(fx, f, indent=1, sort_keys=True)
        f.write("\n")


KINDS = (("inst", "instantiations"), ("k", "K-loop shapes"), ("sw", "source switch (tile, mfma)"), ("mfma", "mfma taps, up2"),
         ("p", "persistence shapes per X16"), ("shape", "tile shapes"), ("edge", "partial edges"), ("padL", "padL per X16"),
         ("padT", "padT per direction"), ("store", "store paths x up2"), ("head", "head kernel forms"), ("wg", "wgrad16 items"),
         ("wg1", "wgrad16 1x1 items"), ("wk", "workload K-loop shapes"), ("wp", "workload persistence shapes"),
         ("ww", "workload backward-weight channel shapes"), ("wu", "workload backward-weight units per workgroup"))


def coverage(cases):
    """{kind: [items, reached by CONV16_CASES + STORE16_CASES, reached by the cases, ruled out]}, the totals under all"""
    want = all_items()
    before = suite_items()
    after = set()
    for c in cases:
        after |= items(c["plan"], c)
    out = {k: [sum(i[0] == k for i in want), sum(i[0] == k for i in before & want), sum(i[0] == k for i in after & want),
               sum(i[0] == k for i in RULED_OUT)] for k, _ in KINDS}
    out["all"] = [len(want), len(before & want), len(after & want), len(RULED_OUT)]
    return out


def report():
    cov = coverage(load()["cases"])
    return "\n".join("%-36s %3d items: the two tables reach %3d, the fixture %3d, ruled out %d" % ((name,) + tuple(cov[k]))
                     for k, name in KINDS + (("all", "all"),))


if __name__ == "__main__":
    if "--search" in sys.argv:      # --search [--out PATH]
        search(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE)
    if "--margin" in sys.argv:
        margin()
    if "--report" in sys.argv:
        print(report())
