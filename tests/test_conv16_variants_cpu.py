"""CPU: the case list of tests/test_gpu_conv16_variants.py (tests/golden/conv16_variants.json) reaches every loop shape of
the 16-bit convolution kernels that the item table of tests/conv16_variant_cases.py names, and every variant the
16-bit configurations of the workload take.

sprk_conv2d_variant answers on the host with the plans of a 256-CU device, so all of this runs without a GPU.  When a
threshold of csrc/conv16.hip or csrc/wgrad16.hip is re-tuned a case may move to another variant: the first test names
what lost its case, and `python tests/conv16_variant_cases.py --search --margin` writes the list again."""
import conv16_variant_cases as cv

FX = cv.load()
CASES = FX["cases"]


def covered(cases=CASES):
    got = set()
    for c in cases:
        got |= cv.items(c["plan"], c)
    return got


def _tuple(x):
    return tuple(_tuple(e) for e in x) if isinstance(x, list) else x


def test_every_case_still_takes_its_recorded_variant():
    lost = []
    for c in CASES:
        now = cv.planned(c)
        if now != c["plan"]:
            gone = sorted(cv.items(c["plan"], c) - (cv.items(now, c) if now else set()), key=str)
            lost.append("%s: (recorded) %s (now) %s; no longer covers %s" % (c["name"], c["plan"], now, gone))
        elif not cv.valid(c, now):
            lost.append("%s: a call of the case left the 16-bit stage" % c["name"])
    for e in FX["epilogue_cases"]:
        if cv.epilogue_plan(e) != e["plan"]:
            lost.append("%s: (recorded) %s (now) %s" % (e["name"], e["plan"], cv.epilogue_plan(e)))
    assert not lost, "%d cases moved to another variant (python tests/conv16_variant_cases.py --search --margin rewrites " \
                     "the fixture):\n%s" % (len(lost), "\n".join(lost))


def test_cases_and_unreached_list_make_up_the_item_table():
    got = covered()
    want = cv.all_items()
    unreached = {_tuple(u["item"]) for u in FX["unreached"]}
    # the tables are what the launch switches give, written out (conv16_variant_cases.py): 126 instantiations
    inst = {i[1:] for i in want if i[0] == "inst"}
    assert inst == ({("mfma",) + k for k in cv.MFMA_TABLE} | {("tile",) + k for k in cv.TILE_TABLE} | {("head",) + k for k in cv.HEAD_TABLE}
                    | {("wg",) + k for k in cv.WG_TABLE} | {("wg1x1",) + k for k in cv.WG1_TABLE}) and len(inst) == 126
    assert sum(i[0] == "sw" for i in want) == 2 * len(cv.SW_SHAPES) and sum(i[0] == "p" for i in want) == 2 * len(cv.P_SHAPES)
    assert [list(s) for s in cv.tile_shapes()] == FX["tile_shapes"]
    assert unreached == set(cv.RULED_OUT), "the unreached list and the rules differ: %s" % sorted(unreached ^ set(cv.RULED_OUT), key=str)
    assert all(u["why"] == cv.RULED_OUT[_tuple(u["item"])] for u in FX["unreached"])
    assert not (got & unreached), "listed as unreached but a case records it: %s" % sorted(got & unreached, key=str)
    assert want <= got | unreached, "neither covered by a case nor ruled out: %s" % sorted(want - got - unreached, key=str)
    # every instantiation of the five families runs, for both operand types
    assert inst <= {i[1:] for i in got if i[0] == "inst"}


def test_every_case_is_needed_and_within_the_cost_bounds():
    """Dropping any case leaves an item of the table without one; no case's fp64 reference exceeds 4e9 multiply-adds but
    those whose floor forces more (listed by name with their cost), all together stay under 1e11."""
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names) and all(c["name"] == cv.describe(c) for c in CASES)
    assert all(cv.macs(c) == c["macs"] for c in CASES)
    over = {c["name"]: c["macs"] for c in CASES if c["macs"] > cv.MAX_CASE_MACS}
    assert over == FX["above_case_bound"]
    assert sum(c["macs"] for c in CASES) == FX["total_macs"] <= cv.MAX_TOTAL_MACS
    want = cv.all_items()
    per = [cv.items(c["plan"], c) & want for c in CASES]
    for i, c in enumerate(CASES):
        others = set().union(*(p for j, p in enumerate(per) if j != i))
        assert per[i] - others, "%s covers nothing of its own" % c["name"]


def test_the_epilogue_product_is_complete():
    eps = FX["epilogue_cases"]
    assert [{k: v for k, v in e.items() if k != "plan"} for e in eps] == cv.epilogue_cases()
    for kind, code, ups, y16s in (("tile", 2, (0, 1), (0, 1)), ("head", 3, (0,), (0, 1)), ("mfma", 1, (0, 1), (0,))):
        for i in (0, 1):
            mine = [e for e in eps if e["name"].startswith("ep %s%d " % (kind, i))]
            forms = {(int(e["up_out"]), e["y16"], e["act"], e["ep"]) for e in mine}
            want = {(u, y, a, p) for u in ups for y in y16s for a in (0, 1, 2) for p in ("bias", "affine", "none")}
            assert forms == want and len(mine) == len(want)
            for e in mine:      # the recorded call: that kernel, with a cut last channel tile
                v = e["plan"]
                assert v["stage"] == cv.S16 and v["kind"] == code and e["Cout"] % 16 and v["Y16"] == e["y16"], (e["name"], v)
                assert v.get("up2", 0) == int(e["up_out"])
    # 16-bit output of the tile kernel: both stores in one launch
    assert all(e["plan"]["store"] == 1 for e in eps if e["want"] == "tile" and e["y16"])


def test_the_workload_takes_covered_variants_only():
    """Every 16-bit-stage convolution of the traced 16-bit U-Net configurations and of test_abi's WS_GEOMS, re-batched
    to per-GPU batch 4, 16 and 32, runs a kernel that some case runs with the workload's K-loop shape and that some case
    runs with the workload's persistence shape; its backward-weight calls likewise."""
    got = covered()
    work = cv.workload_items()
    assert sum(k[0] == "wk" for k in work) >= 10 and sum(k[0] == "wp" for k in work) >= 4 and any(k[0] == "ww" for k in work), work
    assert {k[2] for k in work if k[0] == "wk"} == {"mfma", "tile", "head"}
    bare = {k: v for k, v in work.items() if k not in got}
    assert not bare, "the workload reaches variants without a case (python tests/conv16_variant_cases.py --search; widen " \
                     "its grid if they stay unreached):\n%s" % "\n".join("%s: %s %s" % (k, *v) for k, v in sorted(bare.items(), key=str))


def test_margin_is_recorded_for_every_case_and_under_one_half():
    """The exact model evaluated in fp32 on the CPU misses its fp64 evaluation by less than half of each budget's
    summation share (python tests/conv16_variant_cases.py --margin records the worst ratio per case and quantity)."""
    margin = FX["margin"]
    assert set(margin) == {c["name"] for c in CASES}
    for c in CASES:
        m = margin[c["name"]]
        wg16 = c["plan"].get("wg", {}).get("stage") == cv.S16
        want = {"wgrad": {"gw"}, "fwd": {"y"}}.get(c["kind"]) or ({"y", "gin"} | ({"gw"} if wg16 else set()) | ({"gb"} if c["bias"] else set()))
        assert set(m) == want, (c["name"], m)
        assert max(m.values()) < 0.5, (c["name"], m)


def test_report_before_and_after():
    """The measured coverage that DESIGN quotes: per kind of item what CONV16_CASES + STORE16_CASES of
    tests/test_gpu_ops.py reach by themselves, what the fixture reaches and what is ruled out, equal to what the search
    recorded; nothing the table cases reach is lost."""
    cov = cv.coverage(CASES)
    print(cv.report())
    assert cov == FX["coverage"], (cov, FX["coverage"])
    for kind, (n, before, after, ruled) in cov.items():
        assert before <= after and after + ruled == n, (kind, n, before, after, ruled)
    # items the issue names as never run before have no table case: they are the fixture's alone
    want, before = cv.all_items(), cv.suite_items()
    for it in (("sw", "tile", "first"), ("sw", "tile", "one_chunk"), ("p", 0, "mod8_nonzero"), ("p", 1, "mod8_nonzero"), ("padL", 1, 0),
               ("padL", 1, 3), ("padL", 0, 4), ("padT", "fwd", 0), ("padT", "fwd", 3), ("store", "mixed", 0), ("store", "mixed", 1),
               ("wg", "tail", 1, "49"), ("wg", "tail", 1, "97"), ("wg", "tail", 1, "145+"), ("wg", "tail_behind_wide_C2")):
        assert it in want and it not in before and it in covered(), it
