"""Which variants of the fp32 MFMA convolution kernels the suite runs ("Variant coverage of the MFMA
convolution kernels"): the code shared by tests/test_conv_variants_cpu.py and tests/test_gpu_conv_variants.py, and
the tool that writes their case list, tests/golden/conv_variants.json.

The library routes every convolution call through one host function per family (fwd_route / wg_route of
csrc/conv.hip); sprk_conv2d_variant returns that function's answer without a device, with the plans of a 256-CU
device.  Everything here asks it; nothing re-states the planner.

    python tests/conv_variant_cases.py --search    walk the grid below, rewrite the fixture (--out PATH: write there)
    python tests/conv_variant_cases.py --report    what CONV_CASES + WINO_CASES reach, what the fixture reaches
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
FIXTURE = os.path.join(HERE, "golden", "conv_variants.json")

MFMA = 5          # SPRK_STAGE_MFMA (include/sprk.h; -1 refused, 0 direct, 1 stem, 2 16-bit, 3 Winograd, 4 mask1x1)
# sprk_conv2d_variant's record (include/sprk.h), forward / backward-data and backward-weight
FWD_FIELDS = ("stage", "MT", "NT", "RB", "XTAB", "small", "stages", "ragged_k", "latency", "vec1", "vec2", "vec4",
              "colOff", "up1", "c2", "taps", "CK", "nChunks", "blocks")
WG_FIELDS = ("stage", "IT", "NT", "WJ", "MODE", "xrow", "xtab", "g4", "vec1", "vec2", "chunks", "groups", "up1", "c2",
             "tiles")
# the run-time flags whose two values a covered family shows on each side of its split
FWD_FLAGS = ("small", "stages", "ragged_k", "latency", "vec1", "vec2", "vec4", "colOff", "up1", "c2")
WG_FLAGS = ("xrow", "xtab", "g4", "vec1", "vec2", "chunks", "groups", "up1", "c2")
FLAG_VALUES = {"stages": (1, 2)}          # every other flag: (0, 1)
# The K loop an instantiation runs with, beside its name: (K stages, ragged last chunk).  One chunk (1, 0) is the
# degenerate loop; the two-stage shapes count only with at least MIN_CHUNKS chunks, so that the double buffer turns over
# and a full chunk is followed by another full one before the last.  Backward-weight: a workgroup that sums over at
# least MIN_TILES 64-pixel tiles (its double-buffered tile loop turns over).
K_SHAPES = ((1, 0), (2, 0), (2, 1))
MIN_CHUNKS, MIN_TILES = 3, 3
# plan_fwd halves MT while the launch has fewer than 512 workgroups: a case that ends at MT = 1 or 2 with 896..1023
# workgroups had 448..511 at the MT it left (a tile of twice the pixels), just below the threshold; the cheapest MT >= 2
# cases sit just above it, at 512
NEAR_THRESHOLD = (896, 1023)

# The instantiation tables, written out from the switches of launch_fwd* / launch_wg* (csrc/conv.hip):
#   conv_mfma_kernel<MT, NT, RB, XTAB>:  MT 1 | 2 | 4, NT 1 | 2 | 3 | 4 | 6, RB 1 | 2 | 4 and <= MT, XTAB 0 | 1
#   conv_wgrad_mfma_kernel<IT, NT, WJ, MODE>:  MODE 0 | 2 with IT 1..7, MODE 1 with IT 1..3; WJ = 2 for even NT, else 1
NTS = (1, 2, 3, 4, 6)
FWD_TABLE = [(mt, nt, rb, xt) for mt in (1, 2, 4) for nt in NTS for rb in (1, 2, 4) if rb <= mt for xt in (0, 1)]
WG_TABLE = [(it, nt, 2 if nt % 2 == 0 else 1, mode) for mode in (0, 1, 2) for it in range(1, 8 if mode != 1 else 4)
            for nt in NTS]
assert len(FWD_TABLE) == 60 and len(WG_TABLE) == 85

A0 = 0x10000000          # a 16-byte aligned address that is never dereferenced
MAX_CASE_MACS, MAX_TOTAL_MACS = 4e9, 1e11


def _lib():
    from spr_pick_amd import _lib as m
    return m


def out_size(n, k, stride, dil, lo, hi):
    return (n + lo + hi - dil * (k - 1) - 1) // stride + 1


def case_geom(c):
    """-> ConvGeom of the layer of case c (fp32 operands and tensors)"""
    pt, pb, pl, pr = c["pad"]
    Ho = out_size(c["H"], c["K"], c["stride"], c["dil"], pt, pb)
    Wo = out_size(c["W"], c["K"], c["stride"], c["dil"], pl, pr)
    return _lib().ConvGeom(c["N"], c["C1"], c["C2"], c["H"], c["W"], c["up1"], c["Cout"], Ho, Wo, c["K"], c["K"],
                           c["stride"], c["dil"], pt, pl, 0)


def macs(c):
    """multiply-adds of the fp64 reference's forward"""
    g = case_geom(c)
    return g.N * g.Hout * g.Wout * g.Cout * (g.C1 + g.C2) * g.KH * g.KW


def _query(which, g, x, x2, y_or_gy):
    out = (ctypes.c_int32 * 24)()
    rc = _lib().lib().sprk_conv2d_variant(which, ctypes.byref(g), None, x, x2, y_or_gy, out)
    assert rc == 0, _lib().lib().sprk_last_error()
    return list(out)


def as_dict(which, rec):
    return dict(zip(WG_FIELDS if which == 2 else FWD_FIELDS, rec))


def gy_offset(c):
    """The gradient the backward kernels read is the test's own tensor only behind a linear layer: an activation's
    backward writes a fresh (aligned) one."""
    return c["off"]["gy"] if c["act"] == 0 else 0


def planned(c):
    """The variant each direction of ops.conv2d takes for case c, as sprk_conv2d_variant plans it for tensors with the
    case's alignment offsets (in floats) -> {"fwd": {...}, "bwd": {...}, "wg": {...}}"""
    from spr_pick_amd import ops
    g = case_geom(c)
    x, x2 = A0 + 4 * c["off"]["x"], (A0 + 4 * c["off"]["x2"]) if c["C2"] else None
    gy = A0 + 4 * gy_offset(c)
    gs = ops.stuffed_bwd_data_geom(g)       # strided layers: backward-data of a zero-stuffed (fresh) gradient
    return {"fwd": as_dict(0, _query(0, g, x, x2, A0)),
            "bwd": as_dict(1, _query(1, gs, A0, None, A0) if gs is not None else _query(1, g, A0, None, gy)),
            "wg": as_dict(2, _query(2, g, x, x2, gy))}


def fwd_key(v):
    return (v["MT"], v["NT"], v["RB"], v["XTAB"]) if v["stage"] == MFMA else None


def wg_key(v):
    return (v["IT"], v["NT"], v["WJ"], v["MODE"]) if v["stage"] == MFMA else None


def items(plan):
    """Everything a case with this plan covers: ("f", MT, NT, RB, XTAB), ("w", IT, NT, WJ, MODE), and the flag values
    ("ff", side, flag, value) with side = "MT1" | "MT2+", ("wf", MODE, flag, value); the K-loop shapes
    ("fs", MT, NT, RB, XTAB, stages, ragged_k), ("wd", IT, NT, WJ, MODE) and the threshold neighbours ("fb", MT)."""
    got = set()
    for d in ("fwd", "bwd"):
        v = plan[d]
        if v["stage"] == MFMA:
            got.add(("f",) + fwd_key(v))
            side = "MT1" if v["MT"] == 1 else "MT2+"
            got.update(("ff", side, f, v[f]) for f in FWD_FLAGS)
            if v["stages"] == 1 or v["nChunks"] >= MIN_CHUNKS:
                got.add(("fs",) + fwd_key(v) + (v["stages"], v["ragged_k"]))
            if v["MT"] < 4 and NEAR_THRESHOLD[0] <= v["blocks"] <= NEAR_THRESHOLD[1]:
                got.add(("fb", v["MT"]))
    v = plan["wg"]
    if v["stage"] == MFMA:
        got.add(("w",) + wg_key(v))
        got.update(("wf", v["MODE"], f, v[f]) for f in WG_FLAGS)
        if v["tiles"] >= MIN_TILES:
            got.add(("wd",) + wg_key(v))
    return got


def all_items():
    want = {("f",) + k for k in FWD_TABLE} | {("w",) + k for k in WG_TABLE}
    for side in ("MT1", "MT2+"):
        want.update(("ff", side, f, val) for f in FWD_FLAGS for val in FLAG_VALUES.get(f, (0, 1)))
    for mode in (0, 1, 2):
        want.update(("wf", mode, f, val) for f in WG_FLAGS for val in (0, 1))
    want.update(("fs",) + k + sh for k in FWD_TABLE for sh in K_SHAPES)
    want.update(("wd",) + k for k in WG_TABLE)
    want.update({("fb", 1), ("fb", 2)})
    return want


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def seed_of(name):
    return zlib.crc32(name.encode()) % 10000


def float_offset(t, off, device):
    """A copy of ``t`` on the device that starts ``off`` floats into its (16-byte aligned) buffer."""
    import torch
    buf = torch.empty(t.numel() + 4, device=device)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off
    return v


def tensors(c):
    """CPU fp32 tensors of case c from the seed of its name -> x, x2 | None, w, b | None, gy"""
    import numpy as np
    import torch
    g = torch.Generator().manual_seed(seed_of(c["name"]))
    geom = case_geom(c)
    h1, w1 = (c["H"] // 2, c["W"] // 2) if c["up1"] else (c["H"], c["W"])
    x = torch.randn(c["N"], c["C1"], h1, w1, generator=g)
    x2 = torch.randn(c["N"], c["C2"], c["H"], c["W"], generator=g) if c["C2"] else None
    cin = c["C1"] + c["C2"]
    w = torch.randn(c["Cout"], cin, c["K"], c["K"], generator=g) / np.sqrt(cin * c["K"] * c["K"])
    b = torch.randn(c["Cout"], generator=g) * 0.1 if c["bias"] else None
    gy = torch.randn(c["N"], c["Cout"], geom.Hout, geom.Wout, generator=g)
    return x, x2, w, b, gy


# ---- the workload ---------------------------------------------------------------------------------------------------
def suite_tables():
    """CONV_CASES and WINO_CASES of tests/test_gpu_ops.py as cases (aligned tensors)"""
    import test_gpu_ops
    cases = []
    for (name, N, C1, C2, H, W, up1, Cout, K, stride, dil, pad, act, bias) in test_gpu_ops.CONV_CASES:
        cases.append(dict(name=name, N=N, C1=C1, C2=C2, H=H, W=W, up1=up1, Cout=Cout, K=K, stride=stride, dil=dil,
                          pad=list(pad), act=act, bias=bool(bias), off=dict(x=0, x2=0, gy=0)))
    for row in test_gpu_ops.WINO_CASES:
        name, N, C1, C2, H, W, Cout, pad, act, bias = row[:10]
        cases.append(dict(name=name, N=N, C1=C1, C2=C2, H=H, W=W, up1=0, Cout=Cout, K=3, stride=1, dil=1,
                          pad=list(pad), act=act, bias=bool(bias), off=dict(x=0, x2=0, gy=0)))
    return cases


BATCHES = (4, 16, 32)     # images per GPU: the README's workflow, bench.py's two sizes


def workload_variants():
    """Every (direction, instantiation) the workload's layers reach on the MFMA stages at per-GPU batch 4, 16 and 32:
    the f32 configurations of tests/golden/unet_trace.json (each call's own geometry, its image count re-scaled
    from the configuration's batch) and WS_GEOMS of tests/test_abi.py (an N that is a multiple of 4 is a multiple of
    the batch; other rows keep their N).  -> {item: a geometry that reaches it} with items ("f" | "w", ...) and, for the
    forward family, ("fs", ..., stages, ragged_k): the K loop the workload runs that instantiation with"""
    L = _lib()
    reached = {}

    def visit(which, fields, note):
        g = L.ConvGeom(*fields)
        if which == 1:
            from spr_pick_amd import ops
            g = ops.stuffed_bwd_data_geom(g) or g
        v = as_dict(which, _query(which, g, A0, A0 if g.C2 else None, A0))
        key = wg_key(v) if which == 2 else fwd_key(v)
        if key is not None:
            reached.setdefault(("w" if which == 2 else "f",) + key, (note, list(fields)))
            if which != 2:
                reached.setdefault(("fs",) + key + (v["stages"], v["ragged_k"]), (note, list(fields)))

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
            if geom[15] != 0:
                continue
            for batch in BATCHES:
                f = list(geom)
                f[0] = geom[0] * batch // base
                if f[0] > 0:
                    visit(which, f, "%s %s at batch %d" % (cfg, call[0], batch))
    import test_abi
    for (N, C1, C2, H, W, up1, Cout, K, stride, dil, (pt, pb, pl, pr)) in test_abi.WS_GEOMS:
        Ho, Wo = out_size(H, K, stride, dil, pt, pb), out_size(W, K, stride, dil, pl, pr)
        for n in sorted({N} | ({N // 4 * b for b in BATCHES} if N % 4 == 0 else set())):
            for which in (0, 1, 2):
                visit(which, [n, C1, C2, H, W, up1, Cout, Ho, Wo, K, K, stride, dil, pt, pl, 0], "WS_GEOMS at N = %d" % n)
    return reached


def instantiations(cases):
    got = set()
    for c in cases:
        got |= {i for i in items(c["plan"] if "plan" in c else planned(c)) if i[0] in "fw" and len(i[0]) == 1}
    return got


def report():
    before = instantiations(suite_tables())
    fx = load()
    after = instantiations(fx["cases"])
    work = set(workload_variants())
    lines = []
    for fam, table, name in (("f", FWD_TABLE, "conv_mfma_kernel"), ("w", WG_TABLE, "conv_wgrad_mfma_kernel")):
        n = len(table)
        lines.append("%s: CONV_CASES + WINO_CASES reach %d of %d instantiations, the fixture %d, the grid leaves %d "
                     "unreached; the workload at batch 4 / 16 / 32 reaches %d, of which %d were outside the two tables" % (
                         name, sum(i[0] == fam for i in before), n, sum(i[0] == fam for i in after),
                         sum(u["family"] == fam for u in fx["unreached"]), sum(i[0] == fam for i in work),
                         sum(i[0] == fam and i not in before for i in work)))
    return "\n".join(lines)


# ---- the search -----------------------------------------------------------------------------------------------------
GRID = {
    "N": (1, 2, 3, 4, 8, 16, 32, 64, 128, 256, 512, 1024),
    "HW": ((1, 1), (2, 2), (3, 3), (4, 4), (5, 7), (8, 8), (13, 9), (16, 16), (17, 17), (21, 21), (16, 32), (29, 29),
           (32, 32), (8, 96), (33, 47), (60, 44), (64, 64), (64, 16), (66, 70), (96, 128), (128, 128)),
    "C": (1, 2, 5, 8, 16, 17, 24, 32, 48, 64, 80, 96, 112, 128, 192, 384),
    "Cout": (1, 7, 16, 24, 32, 40, 48, 64, 80, 96, 384),
    "C2": (0, 1, 16),
    # the pads and the alignment offsets are crossed with these only (they change flags, not the tile plan's size)
    "N_few": (1, 4, 32, 256), "C_few": (1, 8, 17, 48, 96), "Cout_few": (1, 16, 48, 96),
    "K_stride_dil": ((1, 1, 1), (1, 2, 1), (3, 1, 1), (3, 2, 1), (3, 1, 2), (3, 2, 2), (3, 1, 4), (3, 1, 8), (7, 1, 1),
                     (7, 2, 1), (7, 1, 2)),
    # per kernel: valid; "same"; the blind-spot shift (2 * (K // 2) rows on top, none below); asymmetric ones
    "pads": ("valid", "same", "shift", (1, 2, 0, 1), (0, 2, 2, 0), (1, 1, 2, 0), (2, 1, 3, 0)),
    "offsets": ((0, 0, 0), (1, 0, 0), (0, 0, 1), (0, 1, 0), (1, 1, 1)),     # floats off 16 bytes: x, x2, gy
    "max_case_macs": MAX_CASE_MACS, "max_total_macs": MAX_TOTAL_MACS,
}


def _pad(p, K, dil):
    h = (K // 2) * dil
    return {"valid": (0, 0, 0, 0), "same": (h, h, h, h), "shift": (2 * h, 0, h, h)}.get(p, p)


def grid_units():
    return list(itertools.product(GRID["K_stride_dil"], GRID["HW"]))


def grid_cases(unit):
    G = GRID
    for (K, stride, dil), (H, W), up1, C2 in itertools.product((unit[0],), (unit[1],), (0, 1), G["C2"]):
        if up1 and (H % 2 or W % 2):
            continue
        for p in G["pads"]:
            if K == 1 and p not in ("valid", (1, 2, 0, 1)):
                continue
            pad = _pad(p, K, dil)
            Ho, Wo = out_size(H, K, stride, dil, pad[0], pad[1]), out_size(W, K, stride, dil, pad[2], pad[3])
            if Ho <= 0 or Wo <= 0:
                continue
            main = p in ("valid", "shift")
            for N, C1, Cout in (itertools.product(G["N"], G["C"], G["Cout"]) if main else
                                itertools.product(G["N_few"], G["C_few"], G["Cout_few"])):
                cost = N * Ho * Wo * Cout * (C1 + C2) * K * K
                if cost > MAX_CASE_MACS:
                    continue
                few = N in G["N_few"] and C1 in G["C_few"] and Cout in G["Cout_few"]
                for off in (G["offsets"] if few else (G["offsets"][0], G["offsets"][-1])):
                    if off[1] and not C2:
                        continue
                    # act and bias are the epilogue's business, not the variant's; a linear layer lets an offset
                    # gradient reach the backward kernels
                    act = 0 if off[2] else 1 + (N + H + C1) % 2
                    yield dict(N=N, C1=C1, C2=C2, H=H, W=W, up1=up1, Cout=Cout, K=K, stride=stride, dil=dil,
                               pad=list(pad), act=act, bias=bool((C1 + Cout) % 3), off=dict(x=off[0], x2=off[1], gy=off[2]))


def describe(c):
    src = ("up(%d)" % c["C1"] if c["up1"] else "%d" % c["C1"]) + ("+%d" % c["C2"] if c["C2"] else "")
    s = "%s->%d %dx%d s%d d%d @%dx%d N%d pad%s" % (src, c["Cout"], c["K"], c["K"], c["stride"], c["dil"], c["H"], c["W"],
                                                 c["N"], tuple(c["pad"]))
    off = "".join(k for k in ("x", "x2", "gy") if c["off"][k])
    return s + (" off:" + "+".join(k for k in ("x", "x2", "gy") if c["off"][k]) if off else "")


# why the grid cannot reach an instantiation: the planner rule (csrc/conv.hip) to look at
def why_unreached(item):
    if item[0] == "f":
        return ("no geometry of the grid gives this (MT, NT, RB, XTAB): plan_fwd keeps MT >= 2 and NT > 1 only with >= 512 "
                "workgroups, fwd_variant takes RB from the tile width (MT * 16 >> lgTC, or MT when strided) and XTAB from "
                "the staged plane's size and the sources' alignment")
    if item[4] == 1:
        return ("no geometry of the grid gives this IT in the 1x1 row form: plan_wgrad's cost loop stops at the first "
                "split into chunks of <= 64 channels (IT = 1) and prefers it whenever the tiles allow")
    return ("no geometry of the grid gives this (IT, NT): plan_wgrad's cost loop (tiles per workgroup * (4 * IT + 1)) never "
            "settles on this IT for it")


def why_shape(item):
    if item[0] == "fs":
        stages, ragged = item[5:]
        if stages == 1:
            return ("no geometry of the grid runs this instantiation with all of K in one chunk: plan_fwd's lds(CK) "
                    "limits cap CK below every channel count of the grid that reaches it")
        return ("no geometry of the grid under %.0e multiply-adds runs this instantiation with two K stages, >= %d "
                "chunks%s: plan_fwd's CK (16 channels for 1x1, 36 / KHW otherwise, doubled while the stages stay small) "
                "against the grid's channel counts" % (MAX_CASE_MACS, MIN_CHUNKS, " and a ragged last one" if ragged else ""))
    if item[0] == "wd":
        return ("no geometry of the grid under %.0e multiply-adds gives a workgroup of this instantiation >= %d tiles: "
                "plan_wgrad spreads the tiles over num_cus() / (nChunks * nblkN) groups" % (MAX_CASE_MACS, MIN_TILES))
    return "no geometry of the grid ends at this MT with %d..%d workgroups" % NEAR_THRESHOLD


def known_cases():
    """The geometries the suite and the workload already have, as candidates beside the grid's (aligned tensors)"""
    out = [dict(c) for c in suite_tables()]
    for key, (note, f) in sorted(workload_variants().items()):
        N, C1, C2, H, W, up1, Cout, Ho, Wo, KH, KW, stride, dil, pt, pl = f[:15]
        pb = (Ho - 1) * stride + dil * (KH - 1) + 1 - H - pt
        pr = (Wo - 1) * stride + dil * (KW - 1) + 1 - W - pl
        if KH == KW and pb >= 0 and pr >= 0:
            out.append(dict(N=N, C1=C1, C2=C2, H=H, W=W, up1=up1, Cout=Cout, K=KH, stride=stride, dil=dil,
                            pad=[pt, pb, pl, pr], act=1, bias=True, off=dict(x=0, x2=0, gy=0)))
    return [c for c in out if macs(c) <= MAX_CASE_MACS]


def _rank(cost, c):
    return (cost, json.dumps(c, sort_keys=True))      # ties broken the same way whatever the order of the scan


def scan(unit):
    """-> (geometries seen, {item: (rank, case, plan)}: the cheapest case per coverage item) over one unit of the grid,
    or over the known cases (unit None)"""
    best, n = {}, 0
    for c in (known_cases() if unit is None else grid_cases(unit)):
        n += 1
        plan = planned(c)
        if any(v["stage"] == -1 for v in plan.values()):
            continue            # a refused call (the 1x1 row staging of backward-weight on unaligned tensors)
        cost, rank = macs(c), None
        for it in items(plan):
            if it not in best or cost <= best[it][0][0]:
                rank = rank or _rank(cost, c)
                if it not in best or rank < best[it][0]:
                    best[it] = (rank, c, plan)
    return n, best


def search(out=FIXTURE, verbose=True):
    best, n = {}, 0
    for unit in [None] + grid_units():         # (about six minutes on one CPU)
        k, part = scan(unit)
        n += k
        for it, rec in part.items():
            if it not in best or rec[0] < best[it][0]:
                best[it] = rec
    best = {it: (rank[0], c, plan) for it, (rank, c, plan) in best.items()}
    if verbose:
        print("grid: %d geometries, %d coverage items reached of %d" % (n, len(best), len(all_items())), file=sys.stderr)
    # instantiations first, the dearest first (a dear case usually brings cheap items along), then the flag values
    chosen, covered = [], set()
    order = sorted(best, key=lambda it: (len(it[0]) > 1, -best[it][0], it))
    for it in order:
        if it in covered:
            continue
        cost, c, plan = best[it]
        c = dict(c, name=describe(c), macs=cost, plan=plan)
        chosen.append(c)
        covered |= items(plan)
    # drop what the later choices made redundant, the dearest first: every case left is the only one for some item
    for c in sorted(chosen, key=lambda c: -c["macs"]):
        rest = set().union(*(items(o["plan"]) for o in chosen if o is not c))
        if items(c["plan"]) <= rest:
            chosen.remove(c)
    chosen.sort(key=lambda c: (c["macs"], c["name"]))
    total = sum(c["macs"] for c in chosen)
    assert total <= MAX_TOTAL_MACS, total
    missing = sorted(all_items() - covered, key=str)
    fx = {
        "comment": "written by tests/conv_variant_cases.py --search; do not edit by hand",
        "grid": {k: v for k, v in GRID.items()},
        "total_macs": total,
        "cases": chosen,
        "unreached": [dict(family=i[0], variant=list(i[1:]), why=why_unreached(i)) for i in missing if len(i[0]) == 1],
        "unreached_shapes": [dict(item=list(i), why=why_shape(i)) for i in missing if i[0] in ("fs", "wd", "fb")],
        "unreached_flag_values": [list(i) for i in missing if i[0] in ("ff", "wf")],
    }
    with open(out, "w") as f:
        json.dump(fx, f, indent=1, sort_keys=True)
        f.write("\n")
    if verbose:
        print("%d cases, %.3g multiply-adds in all (dearest %.3g); %d instantiations, %d K-loop shapes and %d flag values "
              "unreached" % (len(chosen), total, max(c["macs"] for c in chosen), len(fx["unreached"]),
                             len(fx["unreached_shapes"]), len(fx["unreached_flag_values"])),
            file=sys.stderr)
    return fx


if __name__ == "__main__":
    if "--search" in sys.argv:      # --search [--out PATH]
        search(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE)
    if "--report" in sys.argv:
        print(report())
