"""CPU: the case list of tests/test_gpu_wino_variants.py (tests/golden/wino_variants.json) reaches every loop shape of the
Winograd kernels that the item table of tests/wino_variant_cases.py names, and every variant the workload takes.

sprk_conv2d_variant answers on the host with the plans of a 256-CU device, so all of this runs without a GPU.  When a
threshold of csrc/wino.hip is re-tuned a case may move to another variant: the first test names what lost its case,
and `python tests/wino_variant_cases.py --search` writes the list again."""
import wino_variant_cases as wv

FX = wv.load()
CASES = FX["cases"]


def covered(cases=CASES):
    got = wv.explicit_items()
    for c in cases:
        got |= wv.items(c["plan"])
    return got


def test_every_case_still_takes_its_recorded_variant():
    lost = []
    for c in CASES:
        now = wv.planned(c)
        if now != c["plan"]:
            gone = sorted(wv.items(c["plan"]) - wv.items(now), key=str)
            diff = {d: {k: (c["plan"][d].get(k), now[d].get(k)) for k in set(now[d]) | set(c["plan"][d])
                        if now[d].get(k) != c["plan"][d].get(k)} for d in now}
            lost.append("%s: (recorded, now) %s; no longer covers %s" % (c["name"], {d: v for d, v in diff.items() if v}, gone))
    for u in FX["unrot_cases"]:
        if wv.unrot_plan(u) != u["plan"]:
            lost.append("%s: (recorded) %s (now) %s" % (u["name"], u["plan"], wv.unrot_plan(u)))
    for e in FX["epilogue_cases"]:
        if wv.epilogue_plan(e) != e["plan"]:
            lost.append("%s: (recorded) %s (now) %s" % (e["name"], e["plan"], wv.epilogue_plan(e)))
    assert not lost, "%d cases moved to another variant (python tests/wino_variant_cases.py --search rewrites the " \
                     "fixture):\n%s" % (len(lost), "\n".join(lost))


def test_cases_and_unreached_list_make_up_the_item_table():
    got = covered()
    want = wv.all_items()
    unreached = {tuple(tuple(x) if isinstance(x, list) else x for x in u["item"]) for u in FX["unreached"]}
    # the table is what the launch switches and the kernels' loops give, written out (wino_variant_cases.py)
    assert {i[1:] for i in want if i[0] == "inst"} == set(wv.INST_TABLE) and len(wv.INST_TABLE) == 6
    assert {i[2] for i in want if i[:2] == ("wg", "MT")} == set(wv.WG_TABLE)
    assert sum(i[0] in ("k", "km") for i in want) == 2 * 2 * len(wv.K_SHAPES)
    assert sum(i[0] == "p" for i in want) == 2 * len(wv.P_SHAPES)
    assert unreached == set(wv.RULED_OUT), "the unreached list and the rules differ: %s" % sorted(unreached ^ set(wv.RULED_OUT), key=str)
    assert all(u["why"] for u in FX["unreached"])
    assert not (got & unreached), "listed as unreached but a case records it: %s" % sorted(got & unreached, key=str)
    assert want <= got | unreached, "neither covered by a case nor ruled out: %s" % sorted(want - got - unreached, key=str)
    # the five reachable instantiations of wino_conv_kernel, both of wino_wgrad_kernel
    assert {i[1:] for i in got if i[0] == "inst"} == set(wv.INST_TABLE) - {(6, 1, 1)}
    assert {("wg", "MT", 3), ("wg", "MT", 1)} <= got


def test_the_smallest_cout_of_each_nt_is_the_librarys():
    now = wv.min_cout()
    assert {str(k): v for k, v in now.items()} == FX["min_cout"]
    got = covered()
    for nt, c in now.items():
        assert ("cout1", nt, c) in got


def test_every_case_is_needed_and_within_the_cost_bounds():
    """Dropping any case leaves an item of the table without one; no case's fp64 reference exceeds 4e9 multiply-adds but
    the backward-weight ones whose eligibility floor forces more (listed by name), all together stay under 1.5e11."""
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    assert all(wv.macs(c) == c["macs"] for c in CASES)
    over = [c for c in CASES if c["macs"] > wv.MAX_CASE_MACS]
    assert sorted(c["name"] for c in over) == sorted(FX["above_case_bound"])
    assert all(c["kind"] == "wgrad" for c in over), "only a backward-weight floor may force a case above the bound"
    assert sum(c["macs"] for c in CASES) == FX["total_macs"] <= wv.MAX_TOTAL_MACS
    want = wv.all_items()
    per = [wv.items(c["plan"]) & want for c in CASES]
    explicit = wv.explicit_items()
    for i, c in enumerate(CASES):
        others = explicit.union(*(p for j, p in enumerate(per) if j != i))
        assert per[i] - others, "%s covers nothing of its own" % c["name"]


def test_the_epilogue_product_and_the_unrot_list_are_complete():
    eps = FX["epilogue_cases"]
    assert [{k: v for k, v in e.items() if k != "plan"} for e in eps] == wv.epilogue_cases()
    for nt in (3, 6):
        mine = [e for e in eps if e["name"].startswith("ep NT%d " % nt)]
        forms = {(e["mode"], e["act"], e["ep"], e["mact"]) for e in mine}
        want = {(m, a, e, 0) for m in ("plain", "up2") for a in (0, 1, 2) for e in ("bias", "affine", "none")}
        want |= {("mask", 0, "none", m) for m in (1, 2)}       # backward-data has no epilogue of its own
        assert forms == want and len(mine) == len(want)
        for e in mine:      # the recorded call: the Winograd kernel of that NT, its reader mode, a partly filled last group
            v = e["plan"]
            assert v["stage"] == wv.WINO and v["NT"] == nt and v["lastCh"] % 16, (e["name"], v)
            assert v["mode"] == {"plain": 0, "mask": 1, "up2": 2}[e["mode"]], (e["name"], v)
    us = FX["unrot_cases"]
    assert {(u["Cout"], bool(u["C2"])) for u in us} == {(68, False), (68, True), (96, False), (96, True)}
    assert all(u["plan"]["stage"] == wv.WINO and u["plan"]["NT"] == 6 for u in us)


def test_the_workload_takes_covered_variants_only():
    """Every Winograd-stage convolution of the traced U-Net configurations and of test_abi's WS_GEOMS, re-batched to
    per-GPU batch 4, 16 and 32, runs an instantiation that some case runs with the workload's K-loop shape and that
    some case runs with the workload's persistence shape; its backward-weight calls show only items that a case shows."""
    got = covered()
    work = wv.workload_items()
    assert sum(k[0] == "wk" for k in work) >= 6 and sum(k[0] == "wp" for k in work) >= 6 and any(k[0] == "wg" for k in work), work
    bare = {k: v for k, v in work.items() if k not in got}
    assert not bare, "the workload reaches variants without a case (python tests/wino_variant_cases.py --search; widen " \
                     "its grid if they stay unreached):\n%s" % "\n".join("%s: %s %s" % (k, *v) for k, v in sorted(bare.items(), key=str))


def test_fp32_reference_margin_is_recorded_for_every_backward_weight_case():
    """The budget of the backward-weight comparison (5e-5 of max |gw|) is at least twice what a correct fp32 CPU
    convolution of the same tensors misses fp64 by (python tests/wino_variant_cases.py --margin records it)."""
    margin = FX["fp32_margin"]
    names = {c["name"] for c in CASES if c["plan"].get("wg", {}).get("stage") == wv.WINO}
    assert set(margin) == names
    assert max(margin.values()) <= 2.5e-5, max(margin.items(), key=lambda kv: kv[1])


def test_report_before_and_after():
    """The measured coverage that DESIGN quotes: per kind of item what WINO_CASES of tests/test_gpu_ops.py reach by
    themselves, what the fixture reaches and what is ruled out, equal to what the search recorded; nothing the table
    cases reach is lost, and the fixture reaches every item that no rule excludes."""
    cov = wv.coverage(CASES)
    print(wv.report())
    assert cov == FX["coverage"], (cov, FX["coverage"])
    for kind, (n, before, after, ruled) in cov.items():
        assert before <= after and after + ruled == n, (kind, n, before, after, ruled)
    assert cov["all"][1] < cov["all"][2] // 2
    # the items the issue names as never run before have no table case: they are the fixture's alone
    want = wv.all_items()
    before = set()
    for c in wv.suite_table():
        before |= wv.items(wv.planned(c))
    for it in (("k", 6, "nch1"), ("k", 3, "nch2"), ("k", 6, "rag_both"), ("k", 6, "sw_first_loads"), ("p", 0, "xcd_off"),
               ("p", 1, "xcd_off"), ("groups_more", 3), ("padT_block", 0), ("padT_block", 1), ("wg", "g48", 3)):
        assert it in want and it not in before and it in covered(), it
