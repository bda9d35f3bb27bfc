"""Whole-tensor parity of HIP results against the fp64 oracle (oracle/pipeline.py), with the fp32 oracle as yardstick.

The golden train-step test (tests/test_gpu_pipeline.py::test_joint_train_step_matches_reference) checks sampled gradient
probes at the random initial weights.  These helpers apply its rule to EVERY element of every tensor:

  * base rule, per tensor:  max |got - fp64| <= 3e-3 * max|fp64| + 1e-4
    and over all tensors at most 0.1 % of the elements beyond 1e-3 * max|fp64| + 1e-6 of their tensor;
    (the 1e-6 in the count is an absolute floor for tensors whose true gradient is zero, such as detector.m: a BatchNorm
    feeding a BatchNorm; the golden probe test counts the same way).  A tensor with max|fp64| <= 1e-4 is checked by the
    absolute term alone, so `summary` reports how many there are;
  * yardstick rule, for a tensor that misses the base rule: one forward / backward pass is a local statement, so how far
    the fp32 oracle lands from the fp64 one ON THE SAME parameters and inputs measures how ill-conditioned that tensor
    is (e.g. behind a BatchNorm with a tiny running variance).  Such a tensor passes only if the fp32 oracle misses the
    base rule on it too, the tensor's worst error is within K = 4 times the fp32 oracle's worst deviation, its count of
    elements beyond 1e-3 * max|fp64| + 1e-6 within K times the fp32 oracle's count, and its worst error within CAP of
    max|fp64| whatever the oracle does.  Callers assert how many tensors took this branch.

The fp32 oracle may be given as a callable: it is evaluated only when some tensor misses the base rule.
`grad_report` / `check_grads` for gradients (dict name -> tensor or None), `output_report` for single outputs."""
import numpy as np
import torch

K = 4.0           # multiples of the fp32 oracle's own deviation from fp64 (the issue's ceiling)
CAP = 3e-2        # the yardstick never admits more than this fraction of max|fp64|
TENSOR_REL, TENSOR_ABS = 3e-3, 1e-4
LOOSE_REL, LOOSE_ABS = 1e-3, 1e-6
LOOSE_FRACTION = 1e-3


def _np(t):
    if torch.is_tensor(t):
        t = t.detach().cpu().double().numpy()
    return np.asarray(t, dtype=np.float64)


def _tensor_row(got, ref):
    got, ref = _np(got), _np(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    err = np.abs(got - ref)
    row = {"numel": int(ref.size), "absmax": scale, "err": float(err.max()) if err.size else 0.0,
           "loose": int((err > LOOSE_REL * scale + LOOSE_ABS).sum()), "err32": None, "loose32": None}
    row["base_ok"] = row["err"] <= TENSOR_REL * scale + TENSOR_ABS
    return row


def _add_fp32(row, ref32, ref):
    e32 = np.abs(_np(ref32) - _np(ref))
    row["err32"] = float(e32.max()) if e32.size else 0.0
    row["loose32"] = int((e32 > LOOSE_REL * row["absmax"] + LOOSE_ABS).sum())


def grad_report(got, ref, ref32=None):
    """got / ref / ref32: {name: gradient tensor or None}; ref32 may be a callable returning that dict, called only when a
    tensor misses the base rule.  -> dict(rows, failures, yardstick, loose, numel, ref32: the fp32 dict if evaluated)."""
    have = {n for n, g in got.items() if g is not None}
    want = {n for n, g in ref.items() if g is not None}
    failures = []
    if have != want:
        failures.append("parameters with a gradient differ from the oracle's: extra %s, missing %s"
                        % (sorted(have - want), sorted(want - have)))
    rows = {n: _tensor_row(got[n], ref[n]) for n in sorted(have & want)}
    missed = [n for n, r in rows.items() if not r["base_ok"]]
    if missed and callable(ref32):
        ref32 = ref32()
    yardstick = []
    for n in missed:
        r, scale = rows[n], rows[n]["absmax"]
        if ref32 is not None:
            _add_fp32(r, ref32[n], ref[n])
            fp32_misses = r["err32"] > TENSOR_REL * scale + TENSOR_ABS
            if fp32_misses and r["err"] <= min(K * r["err32"], CAP * scale) and r["loose"] <= K * r["loose32"]:
                yardstick.append(n)
                continue
        failures.append("%s: max err %.3e vs max|g| %.3e (rel %.2e); fp32 oracle %s; %d of %d beyond 1e-3" % (
            n, r["err"], scale, r["err"] / (scale + 1e-30),
            "n/a" if r["err32"] is None else "%.3e" % r["err32"], r["loose"], r["numel"]))
    base = [r for r in rows.values() if r["base_ok"]]
    loose, numel = sum(r["loose"] for r in base), sum(r["numel"] for r in base)
    if loose > LOOSE_FRACTION * numel:
        failures.append("%d of %d gradient elements beyond 1e-3 of their tensor's max|g| (more than 0.1 %%)" % (loose, numel))
    return {"rows": rows, "failures": failures, "yardstick": yardstick, "loose": loose, "numel": numel,
            "ref32": None if callable(ref32) else ref32}


def check_grads(got, ref, ref32=None, max_yardstick=0, what="gradients"):
    """Assert the rule; at most ``max_yardstick`` tensors may take the yardstick branch.  Returns the report."""
    rep = grad_report(got, ref, ref32)
    assert not rep["failures"], "%s: %s" % (what, "; ".join(rep["failures"]))
    assert len(rep["yardstick"]) <= max_yardstick, "%s: %d tensors need the fp32 yardstick (allowed %d): %s" % (
        what, len(rep["yardstick"]), max_yardstick, rep["yardstick"])
    return rep


def summary(rep, n=4):
    """One line: the tensors closest to their budget (max err / (3e-3 * max|g| + 1e-4), and max err / max|g|), how many
    tensors sit under the 1e-4 absolute floor, and the yardstick ratios."""
    used = lambda r: r["err"] / (TENSOR_REL * r["absmax"] + TENSOR_ABS)
    worst = sorted(rep["rows"].items(), key=lambda kv: -used(kv[1]))[:n]
    parts = ["%s %.2f of budget (%.1e of max|g|)" % (k.split("denoiser_model.")[-1], used(r), r["err"] / (r["absmax"] + 1e-30))
             for k, r in worst]
    floor = sum(r["absmax"] <= TENSOR_ABS for r in rep["rows"].values())
    ys = ["%s %.2fx fp32 (fp32 oracle %.1e of max|g|)" % (k.split("denoiser_model.")[-1], rep["rows"][k]["err"] / rep["rows"][k]["err32"],
                                                          rep["rows"][k]["err32"] / rep["rows"][k]["absmax"])
          for k in rep["yardstick"]]
    return "%d tensors (%d with max|g| <= 1e-4), %d of %d elements beyond 1e-3; worst %s; yardstick %s" % (
        len(rep["rows"]), floor, rep["loose"], rep["numel"], parts, ys or "none")


def output_report(got, ref, ref32=None, rel=1e-4):
    """A pipeline output against the fp64 oracle: max error within ``rel`` of max|fp64|, else the yardstick rule (the
    fp32 oracle misses ``rel`` too, and the error is within K x its max deviation, never beyond CAP of max|fp64|).
    ref32 may be a callable, called only when the base rule fails.  -> dict(err, err32, ok, yardstick)."""
    got, ref = _np(got).reshape(_np(ref).shape), _np(ref)
    scale = float(np.abs(ref).max()) + 1e-30
    err = float(np.abs(got - ref).max())
    ok = err <= rel * scale
    err32 = None
    if not ok and ref32 is not None:
        ref32 = ref32() if callable(ref32) else ref32
        err32 = float(np.abs(_np(ref32).reshape(ref.shape) - ref).max())
    yard = (not ok) and err32 is not None and err32 > rel * scale and err <= min(K * err32, CAP * scale)
    return {"err": err / scale, "err32": None if err32 is None else err32 / scale, "ok": ok or yard, "yardstick": yard}
