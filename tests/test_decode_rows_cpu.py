"""CPU checks of the inputs of tests/test_decode_rows_gpu.py: decode_common.focus_rows visits the rows it promises for every shape of
that suite's matrix and never focuses both mechanisms on one row, decode_common.seeded_start moves the one-hot start and puts the
reset back, oracle infer(alpha0=None) is the run from row 0, and the committed tests/golden/decode_rows_*.npz satisfy the conditions
their generator (tests/golden/make_decode_rows_golden.py) asserts - coverage of the high rows and the recorded sensitivity - and are
what a short live run of the oracle gives."""
import os
import types

import numpy as np
import pytest
import torch

from decode_common import (FOCUS_BOUNDARIES, ROWS_STEPS, focus_plan, focus_rows, focus_steps, focus_visits, seeded_start, teacher_rows)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def forced_shapes():
    """(dual, B, Ti, lens) of every forced case of the GPU suite's matrix, the groups included"""
    import test_decode_rows_gpu as m
    shapes = [(model != "baseline", B, Ti, lens) for model, B, Ti, lens in m.FORCED] + [(True, B, 256, lens) for B, lens in m.GROUPS_FORCED]
    return [pytest.param(*s, id="%s B=%d Ti=%d" % ("dual" if s[0] else "baseline", s[1], s[2])) for s in shapes]


def test_the_visit_list():
    assert focus_visits(2) == [0, 1] and focus_visits(33) == [0, 1, 31, 32]
    assert focus_visits(32) == [0, 1, 30, 31]          # a boundary AT the length lies beyond the sample
    assert focus_visits(129) == [0, 1, 31, 32, 63, 64, 95, 96, 111, 112, 127, 128]
    assert focus_visits(256) == sorted({0, 1, 254, 255} | {r for b in FOCUS_BOUNDARIES for r in (b - 1, b)}) and len(focus_visits(256)) == 18
    assert focus_steps((256, 129), True) == ROWS_STEPS == 16 and focus_steps((225,), False) == 16 and focus_steps((226,), False) == 24


@pytest.mark.parametrize("dual,B,Ti,lens", forced_shapes())
def test_focus_rows_visit_every_boundary_row_and_keep_the_mechanisms_apart(dual, B, Ti, lens):
    steps = focus_steps(lens, dual)
    ta = focus_rows(B, steps, Ti, lens, dual)
    like = teacher_rows(B, steps, Ti, lens, dual)
    assert (ta[1] is None) == (not dual) == (like[1] is None)
    rows = [a for a in ta if a is not None]
    plan = focus_plan(B, steps, lens, dual)
    for m, a in enumerate(rows):
        assert a.shape == like[0].shape == (B, steps, Ti) and a.dtype == like[0].dtype == torch.float32
        assert torch.allclose(a.sum(-1), torch.ones(B, steps), atol=1e-5) and float(a.min()) >= 0.0
        assert np.array_equal(a.argmax(-1).numpy(), plan[m])          # the focus row carries the row's largest entry ...
        top = a.gather(2, torch.as_tensor(plan[m])[:, :, None])[..., 0]
        assert 0.6 <= float(top.min()) and float(top.max()) <= 1.0 + 1e-6          # ... weight + its share of the background
        for b, n in enumerate(lens):
            assert float(a[b, :, n:].abs().sum()) == 0.0          # masked
            if n > 2:
                assert float((a[b, :, :n] > 0).float().mean()) > 0.99          # a background on every row of the sample
    for b, n in enumerate(lens):
        assert set(plan[:, b].reshape(-1).tolist()) == set(focus_visits(n)), (b, n)
    if dual:
        assert (plan[0] != plan[1]).all()
    again = focus_rows(B, steps, Ti, lens, dual)
    assert all(torch.equal(x, y) for x, y in zip(rows, [a for a in again if a is not None]))


def fake_session(B, Ti, groups):
    """the attributes DecodeSession.reset touches, on the CPU"""
    Ba = 2 * ((B + 1) // 2)
    Z = torch.zeros
    s = types.SimpleNamespace(B=B, Ba=Ba, Ti=Ti, steps2=Z(2), flag=Z(1), mega=None, mega_groups=[object()] * (Ba // 2) if groups else None,
                              states=[Z(2, B, 4)], ctx=Z(2, B, 4), a_state=Z(2, B, Ti), alpha_state=Z(2, B, Ti), yout=Z(Ba, 3, 5)[:B],
                              _mega_part=Z(8), _gsteps=Z(Ba // 2, 2), _gstates=[Z(Ba // 2, 2, 2, 4)], _ga_state=Z(Ba // 2, 2, 2, Ti),
                              _gctx=Z(Ba // 2, 2, 2, 4), _galpha_state=Z(Ba // 2, 2, 2, Ti), _t0=5)
    return s


@pytest.mark.parametrize("B,groups", [(1, False), (2, False), (5, True)])
def test_seeded_start_moves_the_one_hot_and_puts_the_reset_back(B, groups, satt):
    from satt_amd.inference import DecodeSession
    real, Ti = DecodeSession.reset, 9
    rows = [7, 3, 8, 0, 5][:B]
    s = fake_session(B, Ti, groups)
    with seeded_start(rows):
        assert DecodeSession.reset is not real
        DecodeSession.reset(s)
        want = torch.zeros(B, Ti)
        want[torch.arange(B), torch.as_tensor(rows)] = 1.0
        assert torch.equal(s.alpha_state[0], want) and float(s.alpha_state[1].abs().sum()) == 0.0
        if groups:
            g = s._galpha_state[:, 0].reshape(-1, Ti)          # [Ba][Ti]: group g holds samples 2 g, 2 g + 1
            assert torch.equal(g[:B], want) and torch.equal(g[B], want[B - 1]) and float(s._galpha_state[:, 1].abs().sum()) == 0.0
        with pytest.raises(AssertionError):
            with seeded_start([Ti] * B):          # a row beyond the memory is refused, not written
                DecodeSession.reset(s)
    assert DecodeSession.reset is real
    DecodeSession.reset(s)
    assert float(s.alpha_state[0, :, 0].sum()) == B and float(s.alpha_state.sum()) == B
    with pytest.raises(KeyError):
        with seeded_start(rows):
            raise KeyError("the body raises")
    assert DecodeSession.reset is real


def oracle_inputs(case):
    from golden.make_decode_rows_golden import case_params
    from oracle import torch_ref
    return case_params(case), torch_ref.Cfg(**case["kw"])


def test_alpha0_none_is_the_start_from_row_0(satt):
    from common import SMALL, make_params, small_batch
    from oracle import torch_ref
    cfg, P = make_params(SMALL, seed=1)
    batch = small_batch(cfg, 2, 9, 12, seed=3)
    mv = {n: (torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64))
          for n, c in (("bank", cfg.max_filter_width * cfg.conv_channels), ("proj1", cfg.proj1), ("proj2", cfg.proj2))}
    run = lambda **kw: torch_ref.infer(torch_ref.to_torch(P), torch.as_tensor(batch["source"]), torch.as_tensor(batch["source_length"]),
                                       torch_ref.Cfg(**SMALL), 5, mv, min_steps=10 ** 6, **kw)
    none, zero, moved = run(), run(alpha0=[0, 0]), run(alpha0=[3, 0])
    for k in ("mel", "stop", "alignment1", "alignment2"):
        assert torch.equal(none[k], zero[k]), k
    assert torch.equal(none["alignment1"][1], moved["alignment1"][1]) and torch.equal(none["mel"][1], moved["mel"][1])          # per sample
    a = moved["alignment1"][0]
    assert float(a[0, 3:5].sum()) > 0.999 and float(none["alignment1"][0, 0, :2].sum()) > 0.999
    assert float((moved["mel"][0] - none["mel"][0]).abs().max()) > 1e-6


def cases():
    from golden.make_decode_rows_golden import CASES
    return list(CASES)


@pytest.mark.parametrize("case", ["forced_dual_256", "forced_single_256", "ls_sharp_256", "seeded_256", "forced_257", "seeded_257", "forced_2"])
def test_rows_fixture_meets_its_conditions_and_is_reproducible(case, satt):
    from golden.make_decode_golden import moving_stats
    from golden.make_decode_rows_golden import CASES, WEIGHT, case_rows, case_steps, coverage, moved, rows_inputs
    from oracle import torch_ref
    assert case in cases() and len(cases()) == 7
    c = CASES[case]
    z = np.load(os.path.join(GOLD, "decode_rows_%s.npz" % case))
    assert os.path.getsize(os.path.join(GOLD, "decode_rows_%s.npz" % case)) < 100 * 1024
    (cfg, P), ocfg = oracle_inputs(c)
    B, Ti, steps = c["B"], c["Ti"], int(z["steps"])
    assert steps == case_steps(c) and steps in (16, 24) and (steps == 24) == (case == "forced_single_256")
    src, sl = rows_inputs(B, Ti, c["lens"], int(z["source_seed"]))
    assert np.array_equal(src, z["source"]) and np.array_equal(sl, z["source_length"]) and tuple(sl) == tuple(c["lens"])
    for k, (m, v) in moving_stats(cfg).items():
        assert np.array_equal(m, z["bn_mean." + k]) and np.array_equal(v, z["bn_var." + k])
    assert z["stop"].shape == z["path1"].shape == z["step_abs_mel"].shape == (B, steps)
    assert ("mel" in z.files) == (B == 1)          # sampled rows only above B = 1
    for b in range(B):
        assert z["path1"][b].max() < sl[b] and z["path2"][b].max() < sl[b]
    a = z["align1_rows"]
    assert (a >= 0).all() and np.allclose(a.sum(-1), 1.0, atol=1e-5) and all(np.all(a[i, sl[b]:] == 0) for i, b in enumerate(z["rows_b"]))
    assert np.array_equal(a.argmax(-1), z["path1"][z["rows_b"], z["rows_t"]])
    # ---- the conditions on the inputs
    kw = {}
    if c["mode"] == "forced":
        weight = float(z["weight"])
        assert weight in (0.6, 0.8, 0.9) and weight >= WEIGHT
        plan = z["plan"].astype(np.int64)
        coverage(case, c, None, plan)
        ta = case_rows(c, weight)
        assert np.array_equal(ta[0].argmax(-1).numpy(), plan[0]) and np.array_equal(z["path1"], plan[0])
        assert np.array_equal(ta[0].numpy()[z["rows_b"], z["rows_t"]], z["align1_rows"])          # the rows given ARE the alignments
        if cfg.dual:
            assert np.array_equal(ta[1].numpy()[z["rows_b"], z["rows_t"]], z["align2_rows"]) and np.array_equal(z["path2"], plan[1])
        # the least a frame moves when its focus goes 64 rows away (tests/test_decode_rows_gpu.py asserts f32 mel bar <= sens / 4)
        assert 1e-4 < float(z["sens"]) < float(z["mel_abs_max"])
        assert all(moved(f, n) != f and 0 <= moved(f, n) < n for n in c["lens"] for f in range(n))
        kw["teacher_alignments"] = [ta[0].double(), ta[1].double() if cfg.dual else torch.zeros_like(ta[0]).double()]
    elif "alpha0" in c:
        assert (z["high_mass"][0] > 0.5).all(), z["high_mass"][0]          # more than half of sample 0's mass on rows >= 192 at every step
        assert z["path1"][0, 0] in (c["alpha0"][0], c["alpha0"][0] + 1) and z["path1"][0, -1] > z["path1"][0, 0]
        kw["alpha0"] = list(c["alpha0"])
    else:
        path = z["path1"][0]
        assert ((path >= 128) & (path < 192)).any() and (path >= 192).any() and 2 * (path >= 128).sum() >= steps, path
    # ---- live oracle, the first 3 steps
    mv = {k: (torch.as_tensor(z["bn_mean." + k], dtype=torch.float64), torch.as_tensor(z["bn_var." + k], dtype=torch.float64))
          for k in ("bank", "proj1", "proj2")}
    if "teacher_alignments" in kw:
        kw["teacher_alignments"] = [t[:, :3] for t in kw["teacher_alignments"]]
    ref = torch_ref.infer(torch_ref.to_torch(P), torch.as_tensor(src), torch.as_tensor(sl), ocfg, 3, mv, min_steps=10 ** 6, **kw)
    assert np.abs(ref["stop"].numpy()[..., 0] - z["stop"][:, :3]).max() < 1e-6
    assert np.array_equal(ref["alignment1"].numpy().argmax(-1), z["path1"][:, :3])
    assert np.abs(np.abs(ref["mel"].numpy().reshape(B, 3, -1)).mean(-1) - z["step_abs_mel"][:, :3]).max() < 1e-6
