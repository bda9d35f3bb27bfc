"""CPU: the case list of tests/test_gpu_conv_variants.py (tests/golden/conv_variants.json) reaches every instantiation of
the fp32 MFMA convolution kernels that a bounded grid of geometries can reach, and every variant the workload takes.

sprk_conv2d_variant answers on the host with the plans of a 256-CU device, so all of this runs without a GPU.  When the
planner is re-tuned a case may move to another variant: the first test names what lost its case, and
`python tests/conv_variant_cases.py --search` writes the list again."""
import conv_variant_cases as cv

FX = cv.load()
CASES = FX["cases"]

# The flag values no geometry can show, each with the rule of csrc/conv.hip that excludes it.  Pinned here, so that a
# planner change which makes another value unreachable fails this test instead of moving into the fixture's list.
MT1_ONLY = "plan_fwd: chunk_mma_small and the latency-bound re-chunking are rules for MT == 1"
XROW = "wg_variant: xrow is MODE 1 (or the call is refused), and MODE 1 is xrow"
XROW_SRC = "plan_wgrad: xrow needs one full-resolution source (no up1, C2 == 0)"
XROW_ALIGN = "wgrad_dispatch refuses the 1x1 row form on tensors that are not 16-byte aligned"
MODE2 = "plan_wgrad / wg_variant: MODE 2 needs a full-resolution source 1 and g4, xtab and vec1; without them MODE 0 runs"
NO_FLAG_VALUE = {
    ("ff", "MT2+", "small", 1): MT1_ONLY, ("ff", "MT2+", "latency", 1): MT1_ONLY,
    ("wf", 0, "xrow", 1): XROW, ("wf", 1, "xrow", 0): XROW, ("wf", 2, "xrow", 1): XROW,
    ("wf", 1, "up1", 1): XROW_SRC, ("wf", 1, "c2", 1): XROW_SRC, ("wf", 1, "vec2", 1): XROW_SRC,
    ("wf", 1, "g4", 0): XROW_ALIGN, ("wf", 1, "vec1", 0): XROW_ALIGN, ("wf", 1, "xtab", 0): XROW_ALIGN,
    ("wf", 2, "up1", 1): MODE2, ("wf", 2, "g4", 0): MODE2, ("wf", 2, "vec1", 0): MODE2, ("wf", 2, "xtab", 0): MODE2,
}


def covered():
    got = set()
    for c in CASES:
        got |= cv.items(c["plan"])
    return got


def test_every_case_still_takes_its_recorded_variant():
    lost = []
    for c in CASES:
        now = cv.planned(c)
        if now != c["plan"]:
            gone = sorted(i for i in cv.items(c["plan"]) - cv.items(now) if len(i[0]) == 1)      # (instantiations only)
            diff = {d: {k: (c["plan"][d][k], now[d][k]) for k in now[d] if now[d][k] != c["plan"][d][k]} for d in now}
            lost.append("%s: (recorded, now) %s; no longer covers %s" % (c["name"], {d: v for d, v in diff.items() if v}, gone))
    assert not lost, "%d of %d cases moved to another variant (python tests/conv_variant_cases.py --search rewrites " \
                     "the fixture):\n%s" % (len(lost), len(CASES), "\n".join(lost))


def test_cases_and_unreached_list_make_up_the_instantiation_tables():
    got = covered()
    unreached = {(u["family"],) + tuple(u["variant"]) for u in FX["unreached"]}
    tables = {("f",) + k for k in cv.FWD_TABLE} | {("w",) + k for k in cv.WG_TABLE}
    assert len(tables) == 60 + 85
    reached = {i for i in got if i[0] in ("f", "w")}
    assert reached <= tables, sorted(reached - tables)
    assert not (reached & unreached), "listed as unreached but a case records it: %s" % sorted(reached & unreached)
    assert reached | unreached == tables, "neither covered by a case nor listed as unreached: %s" % sorted(tables - reached - unreached)
    assert all(u["why"] for u in FX["unreached"])
    # both values of every run-time flag on each side of the split: MT == 1 / MT >= 2, each MODE
    flags = {i for i in cv.all_items() if i[0] in ("ff", "wf")}
    missing = {tuple(i) for i in FX["unreached_flag_values"]}
    have = {i for i in got if i[0] in ("ff", "wf")}
    assert missing == set(NO_FLAG_VALUE), "flag values without a case and without a rule that excludes them: %s; excluded " \
                                          "by rule but listed as reached: %s" % (sorted(missing - set(NO_FLAG_VALUE), key=str),
                                                                                 sorted(set(NO_FLAG_VALUE) - missing, key=str))
    assert not (have & missing), sorted(have & missing, key=str)
    assert have | missing == flags, "flag values without a case: %s" % sorted(flags - have - missing, key=str)


def test_every_instantiation_runs_a_real_k_loop():
    """The name of an instantiation is not enough: each one runs with all of K in one chunk, with two K stages over at
    least cv.MIN_CHUNKS full chunks, and with a ragged last chunk behind them (forward / backward-data); each
    backward-weight instantiation in a workgroup that sums over at least cv.MIN_TILES tiles; and plan_fwd's 512-workgroup
    threshold has a case just below it for each MT it can leave.  What the grid cannot give is listed with its reason."""
    got = covered()
    want = {i for i in cv.all_items() if i[0] in ("fs", "wd", "fb")}
    assert len(want) == 3 * 60 + 85 + 2
    have = {i for i in got if i[0] in ("fs", "wd", "fb")}
    missing = {tuple(u["item"]) for u in FX["unreached_shapes"]}
    assert all(u["why"] for u in FX["unreached_shapes"])
    assert not (have & missing), sorted(have & missing, key=str)
    assert have | missing == want, "K-loop shapes without a case: %s" % sorted(want - have - missing, key=str)
    # the deep shapes are what the degenerate ones cannot stand in for: most of them must be reached, family by family
    for kind, n in (("fs", 120), ("wd", 85)):
        deep = sum(1 for i in have if i[0] == kind and (kind == "wd" or i[5] == 2))
        assert deep >= n // 2, (kind, deep, n)


def test_every_case_is_needed_and_cheap():
    """No case's fp64 reference exceeds 4e9 multiply-adds, all together stay under 1e11; and every case is the only one
    for some item, so that dropping it from the fixture fails the test above."""
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    assert all(cv.macs(c) == c["macs"] <= cv.MAX_CASE_MACS for c in CASES), max(c["macs"] for c in CASES)
    assert sum(c["macs"] for c in CASES) <= cv.MAX_TOTAL_MACS
    per = [cv.items(c["plan"]) for c in CASES]
    for i, c in enumerate(CASES):
        others = set().union(*(p for j, p in enumerate(per) if j != i))
        assert per[i] - others, "%s covers nothing of its own" % c["name"]


def test_the_workload_takes_covered_variants_only():
    """Every convolution of the traced U-Net configurations and of test_abi's WS_GEOMS, re-batched to per-GPU batch 4, 16
    and 32, that lands on an MFMA stage lands on an instantiation some case runs, and (forward / backward-data) some
    case runs that instantiation with the workload's K loop: the same number of stages and raggedness, over at least
    cv.MIN_CHUNKS chunks when there are two stages."""
    got = covered()
    work = cv.workload_variants()
    assert sum(k[0] == "f" for k in work) >= 8 and sum(k[0] == "fs" for k in work) >= 8, work
    bare = {k: v for k, v in work.items() if k not in got}
    assert not bare, "the workload reaches variants without a case (python tests/conv_variant_cases.py --search; " \
                     "widen its grid if they stay unreached):\n%s" % "\n".join("%s: %s %s" % (k, *v) for k, v in sorted(bare.items()))


def test_report_before_and_after():
    """The measured coverage: what CONV_CASES + WINO_CASES of tests/test_gpu_ops.py reach by themselves ("before") and
    what the fixture reaches.  The fixture never reaches less than the two tables, family by family."""
    before = cv.instantiations(cv.suite_tables())
    after = cv.instantiations(CASES)
    text = cv.report()
    print(text)
    assert before <= after | {(u["family"],) + tuple(u["variant"]) for u in FX["unreached"]}, text
    assert before <= after, "%s\nreached by the two tables only: %s" % (text, sorted(before - after))
    for fam, n in (("f", 60), ("w", 85)):
        assert sum(i[0] == fam for i in after) + sum(u["family"] == fam for u in FX["unreached"]) == n, text
