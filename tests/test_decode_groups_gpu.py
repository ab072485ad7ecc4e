"""Batches of 3 .. 16 on the persistent decode kernel in GROUP mode (csrc/decode_mega2.hip: template flag GRP; include/satt_hip.h:
satt_dec_mega_group) - one pair of samples per XCD, ceil(B / 2) independent B = 2 problems in one launch, the batch's stop rule
scanned behind every launch (satt_dec_stop_scan) - against the hipGraph of launch-per-layer steps such batches ran on before, against
the B = 2 launch of the same kernel, and against the frozen float64 oracle.

EVERY COMPARISON TEST FIRST ASSERTS THAT THE GROUPED PATH WAS TAKEN (`ses.mega_groups is not None`, `ses.mega is None`, the launched
variant carries MEGA_VAR_GROUPS), so each of them fails on the parent; the stop-scan tests fail there because the symbol is missing.
Bar: 2e-5 relative to the largest element - the bar test_persistent_decode_kernel_equals_the_launch_per_layer_path (tests/
test_inference_gpu.py) sets for exactly this comparison: same bf16 weights, fp32 sums in another order, fed back through the steps.
Production widths (A = D = 256, which the kernel requires), short memories, at most 40 steps."""
import os

import numpy as np
import pytest
import torch

from common import rel_err, small_batch
from decode_common import (BAR, BASELINE, GOLDEN_BARS, Engines, expected_variant, golden_engine, infer_kwargs, keys_of, last_session, switches,
                           traced_infer)

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SPK = dict(num_speakers=7, speaker_dim=16, speaker_offset=225)
MODELS = {
    "plain": dict(),
    "speakers": dict(SPK),
    "agent": dict(transition_agent=True),
    "dropout": dict(apply_dropout_on_inference=True),
    "baseline": BASELINE,
    "baseline+speakers": dict(BASELINE, **SPK),
    # the remaining instantiations: one fed frame = the widths the compile-time specialisation (LJ) is keyed on
    "one fed frame": dict(n_feed_frame=1),
    "speakers, one fed frame": dict(SPK, n_feed_frame=1),
    "agent, one fed frame": dict(transition_agent=True, n_feed_frame=1),
    "dropout+speakers": dict(SPK, apply_dropout_on_inference=True),
    "dropout+speakers, one fed frame": dict(SPK, apply_dropout_on_inference=True, n_feed_frame=1),
}
SIX = (225, 230, 226, 229, 227, 228)          # six DIFFERENT speakers in the six rows

engine = Engines(MODELS, agent={None: (3.0, 1.5)})          # u far from 0.5, different per step and sample (tests/test_decode_options_gpu.py)


def run(eng, cfg, B, Ti, steps, mode, grouped, gsteps=8, poison=None, source=None):
    """one utterance; returns (outputs, session, the (variant, groups, nsteps) of the group launches).  grouped=False:
    DecodeSession.MEGA = False, the hipGraph of launch-per-layer steps."""
    batch = small_batch(cfg, B, Ti, steps * cfg.r, seed=6) if source is None else source
    kw = infer_kwargs(mode, steps, batch.get("mel"), [SIX[b % 6] for b in range(B)] if cfg.num_speakers else None,
                      1234 if cfg.apply_dropout_on_inference else None)          # the same masks on both paths
    out, ses, launches = traced_infer(eng, batch["source"], batch["source_length"],
                                      dict(MEGA=grouped, MEGA_STEPS=gsteps, MEGA_GROUPS_STEPS=gsteps), poison, **kw)
    return out, ses, [l[1:] for l in launches if l.name == "dec_mega_groups"]


def took_groups(ses, launched, B, cfg):
    """the session holds the group blocks and every launch carried MEGA_VAR_GROUPS with the bits of the model's B = 2 form"""
    from satt_amd import ops
    assert ses.mega_groups is not None and ses.mega is None and ses.kernel_launches == 1          # FAILS ON THE PARENT
    assert len(ses.mega_groups) == (B + 1) // 2 and ses.graph is None
    var = ops.dec_mega_groups_variant(ses.mega_groups)
    want = expected_variant(cfg, B, ses.Ti, groups=True)
    assert var == want, (var, want)
    assert launched and {v for v, _, _ in launched} == {want} and {n for _, n, _ in launched} == {(B + 1) // 2}, launched
    return var


def compare(model, B, Ti, steps, mode="free", gsteps=8, want_steps=None):
    eng, cfg = engine(model, stop=(mode == "stop"))
    new, ses, launched = run(eng, cfg, B, Ti, steps, mode, True, gsteps)
    took_groups(ses, launched, B, cfg)
    again, ses2, _ = run(eng, cfg, B, Ti, steps, mode, True, gsteps)          # the cached session, reset
    assert ses2 is ses
    old, ses_old, none = run(eng, cfg, B, Ti, steps, mode, False, gsteps)
    assert ses_old.mega is None and ses_old.mega_groups is None and ses_old.graph is not None and not none
    assert new["steps"] == old["steps"] == again["steps"] == (steps if want_steps is None else want_steps)
    for k in keys_of(cfg):
        assert new[k].shape[0] == B and new[k].shape == old[k].shape
        e = rel_err(new[k].cpu().numpy(), old[k].cpu().numpy())
        print(model, B, Ti, mode, k, e)
        assert e < BAR, (k, e)
        assert torch.equal(new[k], again[k]), k
    assert torch.isfinite(new["mel"]).all()
    return new, launched


# ---- 1: equal to the launch-per-layer path
@pytest.mark.parametrize("B,Ti,steps,mode", [(3, 57, 19, "free"),         # an odd batch: the last group is padded
                                             (4, 7, 12, "free"),          # a memory shorter than the workgroup count
                                             (16, 57, 19, "free"),        # all eight XCDs
                                             (5, 140, 33, "teacher"),     # several launches and a ragged last one, no scan
                                             (16, 33, 40, "stop")])       # the scan fires inside the first launch
def test_grouped_decode_equals_the_launch_per_layer_path(B, Ti, steps, mode):
    _, launched = compare("plain", B, Ti, steps, mode, want_steps=7 if mode == "stop" else None)
    if mode == "teacher":          # (the ragged launch has blocks of its own: nsteps is part of a block; in front: the warm-up launch)
        assert [n for _, _, n in launched] == [8] + [8, 8, 8, 8, 1]


@pytest.mark.parametrize("model", ["speakers", "agent", "dropout", "baseline", "baseline+speakers"])
def test_grouped_decode_of_the_other_models(model):
    """B = 6, Ti = 57, 19 steps: six different speakers (the speaker term reaches its own row in every group), the transition agent
    (u_state and the agent table per group), dropout on inference (the mask row is b0 + b: a wrong row gives O(1) errors) and the
    single-source form"""
    new, _ = compare(model, 6, 57, 19)
    if "speakers" in model:
        m = new["mel"]
        assert min(float((m[a] - m[b]).abs().max()) for a in range(6) for b in range(a)) > 1e-3
    if model == "dropout":          # the rows of one group, and the same row of different groups, draw different masks
        m = new["mel"]
        assert float((m[0] - m[2]).abs().max()) > 1e-3 and float((m[0] - m[1]).abs().max()) > 1e-3


@pytest.mark.parametrize("model", ["one fed frame", "speakers, one fed frame", "agent, one fed frame", "dropout+speakers",
                                   "dropout+speakers, one fed frame"])
def test_grouped_instantiations_no_other_test_launches(model):
    compare(model, 4, 33, 9)


# ---- 2: a group is a B = 2 launch
def test_a_group_computes_what_the_two_sample_launch_computes():
    """B = 8, Ti = 57, 24 steps, 8 steps per launch on both sides (launch boundaries and unfolded steps coincide).  The B = 2 session of
    the existing kernel gets the memories, keys and context tables of samples 2 g, 2 g + 1 of the grouped session (copied: the
    comparison is about the kernel, not about how a GEMM tiles 8 x 57 rows against 2 x 57) and runs three launches: its frames,
    stop logits and both alignment histories are BIT-IDENTICAL to rows 2 g, 2 g + 1 of the grouped run - the group mode adds no
    arithmetic."""
    from satt_amd import ops
    eng, cfg = engine("plain")
    B, Ti, steps, K = 8, 57, 24, 8
    batch = small_batch(cfg, B, Ti, steps * cfg.r, seed=6)
    big, ses8, launched = run(eng, cfg, B, Ti, steps, "free", True, K, source=batch)
    took_groups(ses8, launched, B, cfg)
    pair = {k: batch[k][:2] for k in ("source", "source_length")}
    _, ses2, none = run(eng, cfg, 2, Ti, steps, "free", True, K, source=pair)
    assert ses2.mega is not None and ses2.mega_groups is None and not none and ses2.K == K and ses8.K == K
    assert ops.dec_mega_variant(ses2.mega) | ops.MEGA_VAR_GROUPS == ops.dec_mega_groups_variant(ses8.mega_groups)
    NO = ses8.yout.shape[-1]
    for g in range(B // 2):
        rows = slice(2 * g, 2 * g + 2)
        ses2.lengths.copy_(ses8.lengths[rows])
        for name in ("values1", "keys1", "values2", "keys2", "ctab"):
            dst, src = getattr(ses2, name), getattr(ses8, name)
            dst.copy_(src.view(-1, Ti, src.shape[-1])[rows].reshape(dst.shape))
        ses2.reset()
        for _ in range(steps // K):
            ses2.replay()
        torch.cuda.synchronize()
        ses2.check()
        for name, a, b in (("frames", ses2.yout[:, 1:steps + 1], ses8.yout[rows, 1:steps + 1]),
                           ("alignment1", ses2.al1[:, :steps], ses8.al1[rows, :steps]), ("alignment2", ses2.al2[:, :steps], ses8.al2[rows, :steps])):
            print("group", g, name, float((a - b).abs().max()))
            assert torch.equal(a, b), (g, name)
        assert torch.equal(ses8.yout[rows, 1:steps + 1, :NO - 1].reshape(2, steps * cfg.r, -1), big["mel"][rows])
        assert torch.equal(ses8.yout[rows, 1:steps + 1, NO - 1:], big["stop"][rows])


# ---- 3: the stop scan alone
def numpy_scan(yout, t0, n, min_steps, thr, flag=0):
    """StopTokenBasedInferenceHelper over steps t0 .. t0 + n - 1 (row t + 1 of yout is step t's): the first step t > min_steps at which
    every sample's sigmoid(stop logit) > thr -> t + 1"""
    if flag:
        return flag
    for t in range(t0, t0 + n):
        x = yout[:, t + 1, -1].astype(np.float32)
        if t > min_steps and bool((np.float32(1) / (np.float32(1) + np.exp(-x)) > np.float32(thr)).all()):
            return t + 1
    return 0


def crafted(joint, B=5, rows=40, NO=161, seed=3):
    """stop logits of +-4 (far from the threshold): every sample is above it on its own pattern of steps, ALL of them only at `joint`"""
    g = np.random.default_rng(seed)
    y = g.normal(0, 1, (B, rows, NO)).astype(np.float32)
    up = g.random((B, rows)) < 0.6
    for t in range(rows - 1):
        if up[:, t + 1].all():
            up[g.integers(B), t + 1] = False
    for t in joint:
        up[:, t + 1] = True
    y[:, :, -1] = np.where(up, 4.0, -4.0)
    return y


@pytest.mark.parametrize("joint,want", [((23,), 24), ((9, 30), 31), ((), 0), ((11, 12), 12), ((10, 31), 32), ((32,), 0)])
def test_stop_scan(joint, want):
    from satt_amd import ops
    y = crafted(joint)
    assert numpy_scan(y, 0, 32, 10, 0.5) == want
    yd = torch.as_tensor(y).cuda()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.dec_stop_scan(yd, 5, 40, 161, 0, 32, 10, 0.5, flag)
    assert int(flag.item()) == want
    # the same over four launches of 8 steps: a flag that is set stays
    flag.zero_()
    f = 0
    for t0 in range(0, 32, 8):
        ops.dec_stop_scan(yd, 5, 40, 161, t0, 8, 10, 0.5, flag)
        f = numpy_scan(y, t0, 8, 10, 0.5, f)
        assert int(flag.item()) == f
    assert f == want
    # the padding sample of an odd batch takes no part: with B = 4 the fifth row is not looked at
    y4 = y.copy(); y4[4, :, -1] = -4.0
    flag.zero_()
    ops.dec_stop_scan(torch.as_tensor(y4).cuda(), 4, 40, 161, 0, 32, 10, 0.5, flag)
    assert int(flag.item()) == numpy_scan(y4[:4], 0, 32, 10, 0.5)


def test_stop_scan_refuses_rows_beyond_the_buffer():
    from satt_amd import ops
    from satt_amd._lib import SattError
    yd = torch.zeros(2, 9, 161, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.dec_stop_scan(yd, 2, 9, 161, 0, 8, 0, 0.5, flag)          # rows 1 .. 8
    for t0, n in ((0, 9), (1, 8), (-1, 4), (0, 0)):
        with pytest.raises(SattError):
            ops.dec_stop_scan(yd, 2, 9, 161, t0, n, 0, 0.5, flag)


# ---- 4: the frozen float64 oracle
def test_grouped_decode_vs_frozen_float64_oracle():
    """tests/golden/decode_ljspeech_b8.npz (production dimensions, B = 8 with ragged lengths, 200 free-running steps) through the
    grouped path, with the bars tests/test_decode_golden_gpu.py applies to b8 in bf16"""
    from satt_amd import ops
    from satt_amd.inference import infer
    z = np.load(os.path.join(GOLD, "decode_ljspeech_b8.npz"))
    steps = int(z["steps"])
    try:
        cfg, eng = golden_engine(z, "bf16", case="b8")
        out = infer(eng, z["source"], z["source_length"], max_steps=steps, min_steps=10 ** 6, use_graph=True)
        torch.cuda.synchronize()
        ses = last_session(eng)
    finally:
        ops.set_precision("bf16")
    assert ses.mega_groups is not None and ses.mega is None          # FAILS ON THE PARENT
    # (the fixture's model is ModelConfig(): two fed frames, so the run-time-width instantiation - LJ is keyed on one fed frame)
    assert ops.dec_mega_groups_variant(ses.mega_groups) == ops.MEGA_VAR_GROUPS | ops.MEGA_VAR_TWO_SAMPLES | \
        (ops.MEGA_VAR_LJ if cfg.n_feed_frame == 1 else 0)
    assert len(ses.mega_groups) == 4
    assert out["steps"] == steps
    B = z["source"].shape[0]
    mel = out["mel"].float().cpu().numpy().astype(np.float64)
    stop = out["stop"].float().cpu().numpy()[..., 0].astype(np.float64)
    al1 = out["alignment1"].float().cpu().numpy(); al2 = out["alignment2"].float().cpu().numpy()
    assert np.isfinite(mel).all() and np.allclose(al1.sum(-1), 1.0, atol=1e-4) and np.allclose(al2.sum(-1), 1.0, atol=1e-4)
    sm = mel.reshape(B, steps, -1)
    rb, rt = z["rows_b"], z["rows_t"]
    e = dict(mel=np.abs(sm[rb, rt] - z["mel_rows"]).max(), stop=np.abs(stop - z["stop"]).max(),
             align=max(np.abs(al1[rb, rt] - z["align1_rows"]).max(), np.abs(al2[rb, rt] - z["align2_rows"]).max()),
             drift=np.abs(np.abs(sm).mean(-1) - z["step_abs_mel"]).max(),
             path=min((al1.argmax(-1) == z["path1"]).mean(), (al2.argmax(-1) == z["path2"]).mean()))
    print("grouped decode b8 bf16 vs frozen float64: mel %.3e, stop %.3e, alignment rows %.3e, per-step mean|mel| %.3e, argmax path "
          "agreement %.4f" % (e["mel"], e["stop"], e["align"], e["drift"], e["path"]))
    bar = GOLDEN_BARS["bf16"]
    for k in ("mel", "stop", "align", "drift"):
        assert e[k] <= bar[k], (k, e[k], bar[k])
    assert e["path"] >= bar["path"], e["path"]


# ---- 5: LDS contents
def test_grouped_decode_does_not_depend_on_what_the_lds_held_before_the_launch():
    """quiet NaN in every LDS word of every CU in front of every group launch (satt_debug_poison_lds): the clean run within the bar,
    and finite - the start-of-launch zeroing runs in every group"""
    eng, cfg = engine("plain")
    clean, ses, launched = run(eng, cfg, 4, 57, 12, "free", True)
    took_groups(ses, launched, 4, cfg)
    dirty, _, again = run(eng, cfg, 4, 57, 12, "free", True, poison=0x7fc00000)
    assert len(again) == 2 and dirty["steps"] == clean["steps"] == 12          # (two launches, each behind the pattern)
    for k in keys_of(cfg):
        e = rel_err(dirty[k].cpu().numpy(), clean[k].cpu().numpy())
        print(k, e, "bit-identical" if torch.equal(dirty[k], clean[k]) else "")
        assert e < BAR, (k, e)
        assert torch.isfinite(dirty[k]).all(), k


# ---- 6: the switches
def test_the_switches_fall_back_to_the_launch_per_layer_path():
    from satt_amd.inference import infer, DecodeSession
    eng, cfg = engine("plain")
    batch = small_batch(cfg, 4, 33, 9 * cfg.r, seed=6)
    kw = dict(max_steps=9, min_steps=10 ** 6)
    with switches("MEGA_GROUPS", "MEGA_GROUPS_MAX_B"):
        on = infer(eng, batch["source"], batch["source_length"], **kw)
        assert last_session(eng).mega_groups is not None
        DecodeSession.MEGA_GROUPS = False
        off = infer(eng, batch["source"], batch["source_length"], **kw)
        assert last_session(eng).mega_groups is None and last_session(eng).graph is not None
        DecodeSession.MEGA_GROUPS, DecodeSession.MEGA_GROUPS_MAX_B = True, 3
        infer(eng, batch["source"], batch["source_length"], **kw)
        assert last_session(eng).mega_groups is None and last_session(eng).graph is not None
    assert rel_err(on["mel"].cpu().numpy(), off["mel"].cpu().numpy()) < BAR
