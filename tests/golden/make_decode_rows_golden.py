"""Freezes the float64 oracle's decode (oracle/torch_ref.py:infer) at the memory lengths no other fixture reaches: Ti = 256 (the longest
memory the persistent decode kernel takes), 257 (the first one it declines) and 2, with inputs that LOOK at the high rows.

  * forced_*: forced alignments from decode_common.focus_rows - every step weights one focus row per mechanism with `weight`, the focus
    rows visit both ends and both sides of every row-ownership boundary of the kernel (decode_common.focus_visits);
  * ls_sharp_256: free-running location-sensitive attention with cumulative weights, sharpened (make_bench_golden.sharpen_params) so
    that the softmax peaks - in rows 128 .. 191 at some steps and at rows >= 192 at others (the source seed is searched for that);
  * seeded_*: free-running forward attention whose forward variable starts one-hot at a high row (infer(alpha0=...); on the GPU
    decode_common.seeded_start), so that the steps carry most of the mass on rows >= 192.

Kept per case (make_decode_golden.py's fields): every stop logit, the argmax paths, the per-step mean |mel|, NROW sampled (sample, step)
rows of mel and both alignments, the full mel at B = 1, and the `bf16w_*` floor - the same oracle with every weight matrix rounded to
bf16.  The conditions on the INPUTS are asserted here and again by tests/test_decode_rows_cpu.py on the committed files: the coverage
above, and for the forced cases `sens` - the smallest, over (sample, step, mechanism), change of that step's frame (max |.|) when the
step's focus is moved 64 rows away modulo the length (length 2: to the other row); the f32 mel bar of the GPU test stays below sens / 4.
The baseline model's one mechanism has 18 rows to visit at 256 rows: its fixture holds 24 steps (decode_common.focus_steps), the others 16.
CPU only, about a minute:
    python tests/golden/make_decode_rows_golden.py [--weight=0.8 --out=DIR] [case ...]
"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NROW = 24
PARAM_SEED = 0
WEIGHT = 0.6
BASELINE = dict(sa_units=0, att2_units=0, dec_sa_units=0, att1_units=256)          # decode_common.BASELINE
LS = dict(attention="location_sensitive", cumulative_weights=True)
# kw: ModelConfig / oracle Cfg keywords; mode: forced | free; alpha0: the seeded start; mega: the persistent kernel takes the case
CASES = {
    "forced_dual_256": dict(kw={}, B=2, Ti=256, lens=(256, 129), mode="forced", mega=True),
    "forced_single_256": dict(kw=BASELINE, B=2, Ti=256, lens=(256, 129), mode="forced", mega=True),
    "ls_sharp_256": dict(kw=LS, B=1, Ti=256, lens=(256,), mode="free", sharpen=dict(keep=0, sv=60.0, sq=8.0, sk=8.0), mega=True),
    "seeded_256": dict(kw={}, B=2, Ti=256, lens=(256, 129), mode="free", alpha0=(236, 120), mega=True),
    "forced_257": dict(kw={}, B=1, Ti=257, lens=(257,), mode="forced", mega=False),
    "seeded_257": dict(kw={}, B=1, Ti=257, lens=(257,), mode="free", alpha0=(240,), mega=False),
    "forced_2": dict(kw={}, B=1, Ti=2, lens=(2,), mode="forced", mega=True),
}


def rows_inputs(B, Ti, lens, seed=1234):
    """sources in the style of make_decode_golden.decode_inputs (symbols 1 .. 67, 0 at both ends and behind the length), the lengths given"""
    g = np.random.default_rng(seed)
    src = g.integers(1, 68, (B, Ti))
    sl = np.array(lens, dtype=np.int64)
    for b in range(B):
        src[b, 0] = 0
        src[b, sl[b] - 1] = 0
        src[b, sl[b]:] = 0
    return src.astype(np.int64), sl


def moved(f, length):
    """the focus row 64 rows away modulo the length (length 2: the other row)"""
    n = (f + 64) % length
    return n if n != f else (f + 1) % length


def is_dual(case):
    return case["kw"].get("sa_units", 32) > 0


def case_params(case):
    """common.make_params: the recurrent weight slices, which the engine consumes as bf16 in BOTH precisions, are
    bf16-representable, so the f32 path's distance is that of its arithmetic, not of an encoder LSTM run 256 steps on rounded weights"""
    from common import make_params
    cfg, P = make_params(case["kw"], seed=PARAM_SEED, bias_noise=0.0)
    if case.get("sharpen"):
        from golden.make_bench_golden import sharpen_params
        P = sharpen_params(P, **case["sharpen"])
    return cfg, P


def case_steps(case):
    from decode_common import ROWS_STEPS, focus_steps
    return focus_steps(case["lens"], is_dual(case)) if case["mode"] == "forced" else ROWS_STEPS


def case_rows(case, weight):
    """the teacher rows of a forced case (float32, as the engine is given them), else None"""
    from decode_common import focus_rows
    if case["mode"] != "forced":
        return None
    return focus_rows(case["B"], case_steps(case), case["Ti"], case["lens"], is_dual(case), weight=weight)


def coverage(name, case, al1, plan=None):
    """the conditions on the inputs that make the case look at the rows it is about"""
    from decode_common import focus_visits
    if case["mode"] == "forced":
        for b, n in enumerate(case["lens"]):
            seen = set(plan[:, b].reshape(-1).tolist())
            assert seen == set(focus_visits(n)), (name, b, sorted(set(focus_visits(n)) - seen))
        assert (plan[0] != plan[-1]).all() or plan.shape[0] == 1, name
    elif "alpha0" in case:
        high = al1[0, :, 192:].sum(-1)
        assert (high > 0.5).all(), (name, high)
    else:
        path = al1[0].argmax(-1)
        mid = (path >= 128) & (path < 192)          # (peaks in the third AND the fourth quarter, most steps in the upper half)
        assert mid.any() and (path >= 192).any() and 2 * (path >= 128).sum() >= len(path), (name, path)


def sensitivity(case, P, ocfg, src, sl, mv, ta, plan, base_mel, weight):
    """`sens`: every (sample, step, mechanism) with its focus moved is one more row of ONE oracle batch (the samples of a decode do
    not see each other); returns the smallest change of the moved step's own frame"""
    from oracle import torch_ref
    B, T = plan.shape[1:]
    M = plan.shape[0]
    idx = [(b, t, m) for b in range(B) for t in range(T) for m in range(M)]
    rows = [[a[b].clone().double() for (b, t, m) in idx] if a is not None else None for a in ta]
    for i, (b, t, m) in enumerate(idx):
        f = int(plan[m, b, t])
        rows[m][i][t, f] -= weight
        rows[m][i][t, moved(f, int(sl[b]))] += weight
    bs = np.array([b for b, _, _ in idx])
    tas = [torch.stack(r) if r is not None else None for r in rows]
    if tas[1] is None:
        tas[1] = torch.zeros_like(tas[0])
    out = torch_ref.infer(torch_ref.to_torch(P), torch.as_tensor(src[bs]), torch.as_tensor(sl[bs]), ocfg, T, mv, min_steps=10 ** 6,
                          teacher_alignments=tas)
    mel = out["mel"].numpy().reshape(len(idx), T, -1)
    d = np.array([np.abs(mel[i, t] - base_mel[b, t]).max() for i, (b, t, m) in enumerate(idx)])
    return float(d.min()), idx[int(d.argmin())]


def run(name, weight=WEIGHT, out=HERE):
    import satt_amd  # noqa: F401
    from decode_common import focus_plan
    from golden.make_decode_golden import moving_stats
    from oracle import torch_ref
    case = CASES[name]
    B, Ti, steps = case["B"], case["Ti"], case_steps(case)
    cfg, P = case_params(case)
    ocfg = torch_ref.Cfg(**case["kw"])
    mvn = moving_stats(cfg)
    mv = {k: (torch.as_tensor(m, dtype=torch.float64), torch.as_tensor(v, dtype=torch.float64)) for k, (m, v) in mvn.items()}
    ta = case_rows(case, weight)
    plan = focus_plan(B, steps, case["lens"], cfg.dual) if ta is not None else None
    kw = {}
    if ta is not None:
        kw["teacher_alignments"] = [ta[0].double(), ta[1].double() if ta[1] is not None else torch.zeros_like(ta[0]).double()]
    if "alpha0" in case:
        kw["alpha0"] = list(case["alpha0"])
    t0 = time.time()
    for seed in range(1234, 1234 + 64):          # (ls_sharp_256: the first source whose peaks reach the high rows within the steps)
        src, sl = rows_inputs(B, Ti, case["lens"], seed)
        ref = torch_ref.infer(torch_ref.to_torch(P), torch.as_tensor(src), torch.as_tensor(sl), ocfg, steps, mv, min_steps=10 ** 6, **kw)
        al1, al2 = ref["alignment1"].numpy(), ref["alignment2"].numpy()
        try:
            coverage(name, case, al1, plan)
            break
        except AssertionError:
            if case["mode"] == "forced" or "alpha0" in case:
                raise
    else:
        raise RuntimeError("%s: no source seed gives the coverage" % name)
    Pb = {k: (torch.as_tensor(np.asarray(v, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()
              if (np.asarray(v).ndim >= 2) else v) for k, v in P.items()}
    rb = torch_ref.infer(torch_ref.to_torch(Pb), torch.as_tensor(src), torch.as_tensor(sl), ocfg, steps, mv, min_steps=10 ** 6, **kw)
    mel, melb = ref["mel"].numpy(), rb["mel"].numpy()
    stop = ref["stop"].numpy()[..., 0]
    step_mel = mel.reshape(B, steps, -1)
    g = np.random.default_rng(77)
    rb_, rt_ = g.integers(0, B, NROW).astype(np.int32), g.integers(0, steps, NROW).astype(np.int32)
    rt_[:4] = 0; rt_[4:8] = steps - 1; rt_[8:12] = 8          # the first and last step, the first step of the second launch
    keep = dict(source=src, source_length=sl, source_seed=np.int64(seed), stop=stop.astype(np.float32),
                path1=al1.argmax(-1).astype(np.int16), path2=al2.argmax(-1).astype(np.int16),
                step_abs_mel=np.abs(step_mel).mean(-1).astype(np.float32),
                rows_b=rb_, rows_t=rt_, mel_rows=step_mel[rb_, rt_].astype(np.float32),
                align1_rows=al1[rb_, rt_].astype(np.float32), align2_rows=al2[rb_, rt_].astype(np.float32),
                high_mass=al1[:, :, min(192, Ti - 1):].sum(-1).astype(np.float32),
                bf16w_mel_abs_err=np.abs(melb - mel).reshape(B, steps, -1).max(-1).astype(np.float32),
                bf16w_stop_abs_err=np.abs(rb["stop"].numpy()[..., 0] - stop).astype(np.float32),
                bf16w_align_abs_err=np.float64(max(np.abs(rb["alignment1"].numpy() - al1).max(), np.abs(rb["alignment2"].numpy() - al2).max())),
                bf16w_drift=np.float64(np.abs(np.abs(melb.reshape(B, steps, -1)).mean(-1) - np.abs(step_mel).mean(-1)).max()),
                bf16w_path1_agree=np.float64((rb["alignment1"].numpy().argmax(-1) == al1.argmax(-1)).mean()),
                mel_abs_max=np.float64(np.abs(mel).max()))
    if plan is not None:
        sens, where = sensitivity(case, P, ocfg, src, sl, mv, ta, plan, step_mel, weight)
        keep.update(plan=plan.astype(np.int16), weight=np.float64(weight), sens=np.float64(sens))
        print("%s: weight %.1f: sens = %.3e (sample, step, mechanism = %s), |mel| max %.3f" % (name, weight, sens, where, keep["mel_abs_max"]), flush=True)
    if B == 1:
        keep["mel"] = mel.astype(np.float32)
    for k, (m, v) in mvn.items():
        keep["bn_mean." + k] = m
        keep["bn_var." + k] = v
    path = os.path.join(out, "decode_rows_%s.npz" % name)
    np.savez_compressed(path, steps=np.int64(steps), param_seed=np.int64(PARAM_SEED), **keep)
    print("%s: %d steps in %.0f s, wrote %s (%.0f KB); source seed %d; alignment-1 argmax of sample 0: %s; mass on rows >= 192: %.2f .. %.2f; "
          "bf16-weight oracle vs float64: mel %.3e, stop %.3e, alignment %.3e, drift %.3e, path1 agreement %.4f"
          % (name, steps, time.time() - t0, path, os.path.getsize(path) / 1024, seed, al1[0].argmax(-1).tolist(), keep["high_mass"][0].min(),
             keep["high_mass"][0].max(), keep["bf16w_mel_abs_err"].max(), keep["bf16w_stop_abs_err"].max(), keep["bf16w_align_abs_err"],
             keep["bf16w_drift"], keep["bf16w_path1_agree"]), flush=True)


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("SATT_ORACLE_THREADS", "6")))
    opts = dict(a[2:].split("=") for a in sys.argv[1:] if a.startswith("--"))          # --weight=0.8 --out=DIR: a trial, not the committed files
    for n in ([a for a in sys.argv[1:] if not a.startswith("--")] or list(CASES)):
        run(n, float(opts.get("weight", WEIGHT)), opts.get("out", HERE))
