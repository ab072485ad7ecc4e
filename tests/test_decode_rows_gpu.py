"""The persistent decode kernel (csrc/decode_mega2.hip) across its memory-length range, 2 <= Ti <= 256, with inputs that LOOK at the rows.

The kernel's row ownership changes with Ti: R = ceil(Ti / 32) energy rows per workgroup (r0 = wg * R, w = i / R), rows lane + 64 q
(q < 4) in the softmax, the recursion and the teacher rows, rows 127 - rl and 255 - rl of a row lane in the context tables (LDS form
up to Ti = 112 at B = 1, "one row per thread" up to 128), cnt = min(64, n - beg) per wave in gather_vec.  The other decode suites launch
Ti = 33, 57, 100, 113 and 140 only, and their inputs barely weight a row above 32: forward attention starts at row 0 and moves one row
per step, flat teacher rows give every context the memory's mean.  Here:

  * forced alignments from decode_common.focus_rows - 0.6 of every row's mass on one focus row per mechanism, the focus rows visiting
    both ends and both sides of 32, 64, 96, 112, 128, 192, 224;
  * free-running location-sensitive attention (softmax rows, no recursion) at every R from 1 to 8 and all four q;
  * free-running forward attention under decode_common.seeded_start - the forward variable starts one-hot at a high row, so that 16
    steps carry the mass across 127 / 128, 191 / 192 and towards row 255;
  * groups of B = 5 (padded) and B = 16 (all eight XCDs) at Ti = 256.

TIGHT TIER: the persistent kernel against the hipGraph of launch-per-layer steps (csrc/decode.hip), decode_common.BAR = 2e-5 relative to
the largest element on mel, stop and both alignments; bf16, production widths, parameters as initialised (the softmax rows are flat:
an error in a single entry shows at BAR), 16 steps with MEGA_STEPS = 8 (the baseline model from 226 rows on: 24, its one mechanism has
18 rows to visit).  Every case asserts the instantiation decode_common.expected_variant names.
ANCHOR: both paths against frozen float64 vectors at Ti = 256, 257 and 2 (tests/golden/decode_rows_*.npz, made by
tests/golden/make_decode_rows_golden.py); the launch-per-layer path is the reference of the tight tier and the only path above 256 rows.
Bars: 3 x what the MI355X measured (profiles/decode_rows_golden.txt), none above decode_common.GOLDEN_BARS, the f32 mel bar of a
forced case below sens / 4 of its fixture."""
import contextlib
import os

import numpy as np
import pytest
import torch

from decode_common import (BAR, BASELINE, GOLDEN_BARS, ROWS_STEPS, Engines, expected_variant, focus_rows, focus_steps, golden_engine,
                           history_is_as_given, host_outputs, infer_kwargs, inputs, keys_of, last_session, same, seeded_start, switches,
                           traced_infer)
from golden.make_decode_rows_golden import CASES, case_rows

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = 8                                          # steps per launch: a launch boundary inside every run
LS = dict(attention="location_sensitive", cumulative_weights=True)
MODELS = {"dual": dict(), "baseline": BASELINE, "location-sensitive": LS, "agent": dict(transition_agent=True)}


def pair(Ti):
    return (Ti, Ti // 2 + 1)


# (model, mode, B, Ti, lengths, seeded rows) of the matrix; tests/test_decode_rows_cpu.py reads FORCED for the focus_rows properties
FORCED = [("dual", 1, Ti, (Ti,)) for Ti in (2, 31, 32, 33, 64, 65, 96, 97, 112, 113, 128, 129, 160, 161, 192, 193, 224, 225, 255, 256)] + \
         [("dual", 2, Ti, pair(Ti)) for Ti in (64, 65, 128, 129, 192, 193, 255, 256)] + \
         [("baseline", B, Ti, (Ti,) if B == 1 else pair(Ti)) for B in (1, 2) for Ti in (112, 113, 128, 129, 255, 256)]
LOCATION = [(B, Ti, (Ti,) if B == 1 else pair(Ti)) for B in (1, 2) for Ti in (32, 33, 64, 65, 128, 129, 192, 193, 224, 225, 255, 256)]
# the seeds: 16 steps at initial weights move the argmax about 8 rows up (236 -> 244 on the float64 oracle): across 127 / 128 (Ti = 129,
# and sample 1 of Ti = 256), across 191 / 192 (Ti = 193), towards the last rows (Ti = 256); the short sample of a pair across 63 / 64, 95 / 96
SEEDS = {129: (124, 60), 193: (188, 92), 256: (236, 124)}
SEEDED = [(m, B, Ti, (Ti,) if B == 1 else pair(Ti), SEEDS[Ti][:B]) for m in ("dual", "baseline") for B in (1, 2) for Ti in (129, 193, 256)] + \
         [("agent", 1, 256, (256,), (236,))]
FIVE = (256, 193, 129, 65, 2)                  # an odd batch: the last group is padded
SIXTEEN = (256, 241, 225, 224, 193, 192, 161, 129, 128, 113, 112, 97, 65, 64, 33, 2)          # all eight XCDs at the largest LDS footprint
GROUPS_FORCED = [(5, FIVE), (16, SIXTEEN)]

engine = Engines(MODELS, agent={None: (3.0, 1.5)})          # Wa x 3: u far from 0.5, different per step (tests/test_attn_general_gpu.py)


def run(model, B, Ti, lens, mega, forced=False, seeds=None, mode="free"):
    """one utterance; returns (outputs on the host, the session, the variants the persistent kernel was launched with, the teacher rows)"""
    eng, cfg = engine(model, stop=(mode == "stop"))
    steps = focus_steps(lens, cfg.dual) if forced else ROWS_STEPS
    src, sl, mel = inputs(cfg, B, Ti, steps, lens)
    ta = focus_rows(B, steps, Ti, lens, cfg.dual) if forced else None
    kw = infer_kwargs(mode, steps, mel)
    if ta is not None:
        kw["teacher_alignments"] = ta
    with (seeded_start(seeds) if seeds is not None else contextlib.nullcontext()):
        out, ses, launches = traced_infer(eng, src, sl, dict(MEGA=mega, MEGA_STEPS=K, MEGA_GROUPS_STEPS=K), **kw)
    return host_outputs(out), ses, launches, ta


def compare(model, B, Ti, lens, forced=False, seeds=None, mode="free", want_steps=None):
    """the persistent kernel against the launch-per-layer path: the instantiation, then mel, stop and the model's alignments at BAR"""
    cfg = engine.config(model)
    new, ses, launches, ta = run(model, B, Ti, lens, True, forced, seeds, mode)
    grouped = B > 2
    want = expected_variant(cfg, B, Ti, forced=forced, groups=grouped)
    name = "dec_mega" + ("_groups" if grouped else "") + ("_forced" if forced else ("_opt" if cfg.transition_agent and not grouped else ""))
    assert want >= 0 and launches and {l.variant for l in launches} == {want}, (launches, want)
    assert {l.name for l in launches} == {name}, launches
    assert {l.groups for l in launches} == {(B + 1) // 2 if grouped else 0} and max(l.nsteps for l in launches) == K
    assert (ses.mega_groups is not None) == grouped and (ses.mega is not None) == (not grouped) and ses.graph is None and ses.Ti == Ti
    old, ses_old, none, _ = run(model, B, Ti, lens, False, forced, seeds, mode)
    assert ses_old.mega is None and ses_old.mega_groups is None and ses_old.graph is not None and not none
    steps = focus_steps(lens, cfg.dual) if forced else ROWS_STEPS
    assert new["steps"] == (steps if want_steps is None else want_steps)
    same(new, old, "%s B=%d Ti=%d%s%s %s" % (model, B, Ti, " forced" if forced else "", " seeded" if seeds else "", mode), keys_of(cfg))
    for k in keys_of(cfg):
        assert new[k].shape == old[k].shape and new[k].shape[0] == B
    if forced:
        history_is_as_given(new, ta)
        history_is_as_given(old, ta)
    return new, old


# ---- 1: forced alignments that look at the rows
@pytest.mark.parametrize("model,B,Ti,lens", FORCED, ids=lambda v: str(v).replace(" ", ""))
def test_forced_focus_rows_at_every_table_form(model, B, Ti, lens):
    compare(model, B, Ti, lens, forced=True)


# ---- 2: the softmax phase at every R and q
@pytest.mark.parametrize("B,Ti,lens", LOCATION, ids=lambda v: str(v).replace(" ", ""))
def test_location_sensitive_softmax_at_every_rows_per_workgroup(B, Ti, lens):
    """R = ceil(Ti / 32) = 1 .. 8 and q = 0 .. 3; cumulative weights: the location features read the running sum of all rows"""
    new, _ = compare("location-sensitive", B, Ti, lens)
    assert np.allclose(new["alignment1"].sum(-1).numpy(), 1.0, atol=1e-4)


# ---- 3: the forward recursion on the high rows
@pytest.mark.parametrize("model,B,Ti,lens,seeds", SEEDED, ids=lambda v: str(v).replace(" ", ""))
def test_forward_recursion_from_a_seeded_start(model, B, Ti, lens, seeds):
    """both paths start from the same seeded alpha_state: the first row's mass sits on the seed row and its successor, and the
    run stays at and above the seed - the seed took effect, the recursion runs on the rows it is meant to"""
    new, old = compare(model, B, Ti, lens, seeds=seeds)
    for res in (new, old):
        a = res["alignment1"]
        for b, s in enumerate(seeds):
            top = min(s + 2, lens[b])
            assert float(a[b, 0, s:top].sum()) > 0.99, (b, s, float(a[b, 0, s:top].sum()))
            path = a[b].argmax(-1)          # (the recursion's + 1e-7 under a flat softmax grows to a few per cent below the seed in 16 steps)
            assert int(path.min()) >= s and int(path[-1]) > s and float(a[b, :, s:].sum(-1).min()) > 0.9, (b, s, path.tolist())


# ---- 4: groups at the largest memory
def test_groups_location_sensitive_at_256_rows():
    compare("location-sensitive", 5, 256, FIVE)


@pytest.mark.parametrize("B,lens", GROUPS_FORCED, ids=["B=5", "B=16"])
def test_groups_forced_focus_rows_at_256_rows(B, lens):
    compare("dual", B, 256, lens, forced=True)


# ---- 5: teacher feeding and the stop rule at (2, 256)
@pytest.mark.parametrize("mode", ["teacher", "stop"])
def test_teacher_feeding_and_the_stop_rule_at_256_rows(mode):
    """teacher= feeding (no folded feedback), and the stop rule firing inside the first launch (min_steps = 5, the stop logit always
    large: 7 steps), both from the seeded start of the (2, 256) case"""
    compare("dual", 2, 256, pair(256), seeds=SEEDS[256], mode=mode, want_steps=7 if mode == "stop" else None)


# ---- 6: the float64 anchor
# per case and (path, precision): (mel abs, stop abs, alignment rows abs, per-step mean |mel| abs, argmax path agreement) - the metrics of
# tests/test_decode_golden_gpu.py.  MEASURED holds what the MI355X measured (profiles/decode_rows_golden.txt, with the fixtures' bf16w_*
# floors beside it); a bar is 3 x measured and at most the entry of decode_common.GOLDEN_BARS (ls_sharp_256, alignment rows and paths:
# judged against the fixture's own bf16-weight floor, as BARS_SHARP of tests/test_decode_golden_gpu.py - a near one-hot row moves by a
# whole position where two energies are close); path agreement: 1 - 3 x (1 - measured)
PATHS = [("layer", "f32"), ("layer", "bf16"), ("persistent", "bf16")]
MEASURED = {
    ("forced_dual_256", "layer", "f32"): dict(mel=2.370e-07, stop=1.565e-07, align=0.000e+00, drift=2.857e-08, path=1.0000),
    ("forced_dual_256", "layer", "bf16"): dict(mel=3.246e-04, stop=9.701e-05, align=0.000e+00, drift=6.815e-06, path=1.0000),
    ("forced_dual_256", "persistent", "bf16"): dict(mel=3.246e-04, stop=9.703e-05, align=0.000e+00, drift=6.813e-06, path=1.0000),
    ("forced_single_256", "layer", "f32"): dict(mel=1.863e-07, stop=8.568e-08, align=0.000e+00, drift=2.981e-08, path=1.0000),
    ("forced_single_256", "layer", "bf16"): dict(mel=3.667e-04, stop=1.297e-04, align=0.000e+00, drift=1.753e-05, path=1.0000),
    ("forced_single_256", "persistent", "bf16"): dict(mel=3.666e-04, stop=1.297e-04, align=0.000e+00, drift=1.753e-05, path=1.0000),
    ("ls_sharp_256", "layer", "f32"): dict(mel=2.384e-07, stop=1.714e-07, align=6.080e-06, drift=3.009e-08, path=1.0000),
    ("ls_sharp_256", "layer", "bf16"): dict(mel=4.629e-04, stop=7.557e-05, align=1.169e-02, drift=1.521e-05, path=1.0000),
    ("ls_sharp_256", "persistent", "bf16"): dict(mel=4.629e-04, stop=7.562e-05, align=1.169e-02, drift=1.521e-05, path=1.0000),
    ("seeded_256", "layer", "f32"): dict(mel=2.636e-07, stop=1.490e-07, align=1.192e-07, drift=3.144e-08, path=1.0000),
    ("seeded_256", "layer", "bf16"): dict(mel=3.657e-04, stop=8.891e-05, align=1.222e-04, drift=8.208e-06, path=1.0000),
    ("seeded_256", "persistent", "bf16"): dict(mel=3.657e-04, stop=8.887e-05, align=1.222e-04, drift=8.207e-06, path=1.0000),
    ("forced_257", "layer", "f32"): dict(mel=2.887e-07, stop=1.304e-07, align=0.000e+00, drift=3.510e-08, path=1.0000),
    ("forced_257", "layer", "bf16"): dict(mel=3.250e-04, stop=5.864e-05, align=0.000e+00, drift=8.120e-06, path=1.0000),
    ("forced_257", "persistent", "bf16"): dict(mel=3.250e-04, stop=5.864e-05, align=0.000e+00, drift=8.120e-06, path=1.0000),
    ("seeded_257", "layer", "f32"): dict(mel=2.774e-07, stop=1.490e-07, align=7.451e-08, drift=2.925e-08, path=1.0000),
    ("seeded_257", "layer", "bf16"): dict(mel=3.932e-04, stop=6.016e-05, align=1.473e-04, drift=4.967e-06, path=1.0000),
    ("seeded_257", "persistent", "bf16"): dict(mel=3.932e-04, stop=6.016e-05, align=1.473e-04, drift=4.967e-06, path=1.0000),
    ("forced_2", "layer", "f32"): dict(mel=2.356e-07, stop=1.015e-07, align=0.000e+00, drift=1.811e-08, path=1.0000),
    ("forced_2", "layer", "bf16"): dict(mel=1.497e-04, stop=3.172e-05, align=0.000e+00, drift=1.205e-05, path=1.0000),
    ("forced_2", "persistent", "bf16"): dict(mel=1.497e-04, stop=3.169e-05, align=0.000e+00, drift=1.205e-05, path=1.0000),
}


def bars_of(case, path, prec):
    cap = GOLDEN_BARS[prec]
    m = MEASURED[(case, path, prec)]
    sharp = case.startswith("ls_sharp")
    bar = {k: (3 * m[k] if sharp and k == "align" else min(3 * m[k], cap[k])) for k in ("mel", "stop", "align", "drift")}
    bar["path"] = 1 - 3 * (1 - m["path"]) if sharp else max(1 - 3 * (1 - m["path"]), cap["path"])
    return bar


@pytest.mark.parametrize("path,prec", PATHS, ids=["layer-f32", "layer-bf16", "persistent-bf16"])
@pytest.mark.parametrize("case", list(CASES))
def test_rows_decode_vs_frozen_float64_oracle(case, path, prec):
    """the f32 and the bf16 launch-per-layer path and the bf16 persistent kernel; at Ti = 257 the persistent kernel must decline, and
    what the session runs instead is judged"""
    from satt_amd import ops
    from satt_amd.inference import infer
    c = CASES[case]
    z = np.load(os.path.join(GOLD, "decode_rows_%s.npz" % case))
    steps, B = int(z["steps"]), c["B"]
    kw = {}
    if c["mode"] == "forced":
        ta = case_rows(c, float(z["weight"]))
        kw["teacher_alignments"] = ta
    try:
        with switches(MEGA=path == "persistent", MEGA_STEPS=K), (seeded_start(c["alpha0"]) if "alpha0" in c else contextlib.nullcontext()):
            cfg, eng = golden_engine(z, prec, cfg_kw=c["kw"], sharpen=c.get("sharpen"))
            out = infer(eng, z["source"], z["source_length"], max_steps=steps, min_steps=10 ** 6, **kw)
            torch.cuda.synchronize()
            ses = last_session(eng)          # (a new engine: the session is new)
            assert (ses.mega is not None) == (path == "persistent" and c["mega"]), "Ti = %d: taken %s" % (c["Ti"], ses.mega is not None)
            if ses.mega is not None:
                want = expected_variant(cfg, B, c["Ti"], forced=c["mode"] == "forced")
                got = ops.dec_mega_forced_variant(ses.mega, ses.mega_opt, ses.mega_forced) if ses.mega_forced is not None else ops.dec_mega_variant(ses.mega)
                assert got == want, (got, want)
    finally:
        ops.set_precision("bf16")
    assert out["steps"] == steps
    mel = out["mel"].float().cpu().numpy().astype(np.float64)
    stop = out["stop"].float().cpu().numpy()[..., 0].astype(np.float64)
    al1 = out["alignment1"].float().cpu().numpy()
    al2 = out["alignment2"].float().cpu().numpy() if cfg.dual else np.zeros_like(al1)
    assert np.isfinite(mel).all() and np.allclose(al1.sum(-1), 1.0, atol=1e-4) and (not cfg.dual or np.allclose(al2.sum(-1), 1.0, atol=1e-4))
    sm = mel.reshape(B, steps, -1)
    rb, rt = z["rows_b"], z["rows_t"]
    e = dict(mel=np.abs(sm[rb, rt] - z["mel_rows"]).max(), stop=np.abs(stop - z["stop"]).max(),
             align=max(np.abs(al1[rb, rt] - z["align1_rows"]).max(), np.abs(al2[rb, rt] - z["align2_rows"]).max()),
             drift=np.abs(np.abs(sm).mean(-1) - z["step_abs_mel"]).max(),
             path=min((al1.argmax(-1) == z["path1"]).mean(), (al2.argmax(-1) == z["path2"]).mean() if cfg.dual else 1.0))
    if "mel" in z.files:                       # B = 1: every frame
        e["mel"] = max(e["mel"], np.abs(mel - z["mel"]).max())
    bar = bars_of(case, path, prec)
    sens = float(z["sens"]) if "sens" in z.files else float("nan")
    print("ROWS %s %s %s: mel %.3e stop %.3e align %.3e drift %.3e path %.4f | bars mel %.3e stop %.3e align %.3e drift %.3e path %.4f | "
          "floor (float64 oracle, bf16-rounded weights) mel %.2e stop %.2e align %.2e drift %.2e path %.4f | |mel| max %.3f sens %.3e"
          % (case, path, prec, e["mel"], e["stop"], e["align"], e["drift"], e["path"], bar["mel"], bar["stop"], bar["align"], bar["drift"],
             bar["path"], float(z["bf16w_mel_abs_err"].max()), float(z["bf16w_stop_abs_err"].max()), float(z["bf16w_align_abs_err"]),
             float(z["bf16w_drift"]), float(z["bf16w_path1_agree"]), float(z["mel_abs_max"]), sens))
    if c["mode"] == "forced" and prec == "f32":
        assert bar["mel"] <= sens / 4, (bar["mel"], sens)
    for k in ("mel", "stop", "align", "drift"):
        assert e[k] <= bar[k], (k, e[k], bar[k])
    assert e["path"] >= bar["path"], e["path"]
