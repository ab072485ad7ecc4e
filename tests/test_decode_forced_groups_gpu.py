"""Forced-alignment batches of 3 .. 16 (infer(..., teacher_alignments=...), B > 2) on the persistent decode kernel in GROUP mode with
the FORCED instantiations (csrc/decode_mega2.hip: template flags GRP and FRC together; satt_dec_mega_groups_forced) against the
hipGraph of launch-per-layer steps such batches ran on before, against the forced B = 2 launch of the same kernel, and against the
float64 oracle.

What can go wrong here is which teacher rows a group reads: the forced block is ONE for the batch ([Ba][Td][Ti]), group g reads
batch rows 2 g and 2 g + 1, the padding sample of an odd batch has rows of its own.  The cases are shaped for that (odd batches,
rows rotated across groups, all eight XCDs) and otherwise follow tests/test_decode_forced_gpu.py and tests/test_decode_groups_gpu.py.

EVERY COMPARISON TEST FIRST ASSERTS THAT THE NEW PATH WAS TAKEN (the session holds `mega_groups` AND `mega_forced`, every recorded
launch carries MEGA_VAR_FORCED | MEGA_VAR_GROUPS with exactly the model's other bits, no launch went through ops.dec_mega* or
ops.dec_mega_groups), so each of them fails on the parent, where such a session runs the hipGraph path.
Bar: 2e-5 relative to the largest element, the bar of both neighbours for exactly this comparison (same bf16 weights, same buffers,
fp32 sums in another order, fed back through the steps); "live" means a difference above 100 bars.
Production widths (A = D = 256, which the kernel requires), short memories, at most 40 steps, 8 steps per launch."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from common import rel_err
from decode_common import (BAR, BASELINE, Engines, expected_variant, history_is_as_given, host_outputs, infer_kwargs, inputs, keys_of,
                           recording, same, sessions_used, switches, teacher_rows, traced_infer)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 8                                          # steps per launch
SPK = dict(num_speakers=7, speaker_dim=16, speaker_offset=225)
MODELS = {
    "dual": dict(),
    "speakers": dict(SPK),
    "dropout": dict(apply_dropout_on_inference=True),
    "spk decoder": dict(SPK, speaker_to_decoder=True),
    "agent": dict(transition_agent=True),
    "baseline": BASELINE,
    "baseline+speakers": dict(BASELINE, **SPK),
    "baseline agent": dict(BASELINE, transition_agent=True),
}
SIX = (225, 230, 226, 229, 227, 228)          # six DIFFERENT speakers in the six rows

engine = Engines(MODELS, stats=True)
_runs = {}


def run(model, B, Ti, steps, mega=True, mode="free", lens=None, ta=None, tag="masked", poison=None, fresh=False, switches=None):
    """one forced utterance; returns (outputs on the host, the session, the recorded forced group launches (variant, groups, nsteps)).
    mega=False: DecodeSession.MEGA = False, the hipGraph of launch-per-layer steps.  Results are computed once per key and shared."""
    key = (model, B, Ti, steps, mega, mode, None if lens is None else tuple(lens), tag, poison, None if switches is None else tuple(sorted(switches.items())))
    if key in _runs and not fresh:
        return _runs[key]
    eng, cfg, _, _ = engine(model, stop=(mode == "stop"))
    src, sl, mel = inputs(cfg, B, Ti, steps, lens)
    if ta is None:
        ta = teacher_rows(B, steps, Ti, sl, cfg.dual)
    kw = infer_kwargs(mode, steps, mel, [SIX[b % 6] for b in range(B)] if cfg.num_speakers else None,
                      1234 if cfg.apply_dropout_on_inference else None)          # the same masks on both paths
    out, ses, launches = traced_infer(eng, src, sl, dict(MEGA=mega, MEGA_STEPS=K, MEGA_GROUPS_STEPS=K, **(switches or {})), poison,
                                      teacher_alignments=ta, **kw)
    others = [l.name for l in launches if l.name != "dec_mega_groups_forced"]
    assert B <= 2 or not others, others          # a forced group session launches through ops.dec_mega_groups_forced only
    _runs[key] = (host_outputs(out), ses, [l[1:] for l in launches if l.name == "dec_mega_groups_forced"])
    return _runs[key]


def took_forced_groups(ses, launched, model, B):
    """the session holds the group blocks AND the forced block; every launch carried both bits with exactly the model's other bits"""
    from satt_amd import ops
    cfg = engine(model)[1]
    assert ses.mega_groups is not None and ses.mega_forced is not None, "the forced batch did not take the group mode"      # FAILS ON THE PARENT
    assert ses.mega is None and ses.graph is None and ses.kernel_launches == 1 and ses.K == K
    assert len(ses.mega_groups) == (B + 1) // 2 and ses.Ba == 2 * ((B + 1) // 2)
    assert ses.agent_tab is None and ses.u_state is None          # the agent is dead under forced alignments
    assert ses.teach1._base.shape[0] == ses.Ba and ses.teach1.shape[0] == B
    want = expected_variant(cfg, B, ses.Ti, forced=True, groups=True)
    assert ops.dec_mega_groups_forced_variant(ses.mega_groups, ses.mega_forced) == want
    assert launched and {v for v, _, _ in launched} == {want} and {n for _, n, _ in launched} == {(B + 1) // 2}, (launched, want)


def compare(model, B, Ti, steps, mode="free", lens=None, want_steps=None):
    cfg = engine(model)[1]
    new, ses, launched = run(model, B, Ti, steps, True, mode, lens)
    took_forced_groups(ses, launched, model, B)
    again, ses2, _ = run(model, B, Ti, steps, True, mode, lens, fresh=True)          # the cached session, reset
    assert ses2 is ses
    old, ses_old, none = run(model, B, Ti, steps, False, mode, lens)
    assert ses_old.mega is None and ses_old.mega_groups is None and ses_old.mega_forced is None and ses_old.graph is not None and not none
    assert new["steps"] == (steps if want_steps is None else want_steps)
    same(new, old, "%s B=%d Ti=%d %s" % (model, B, Ti, mode), keys_of(cfg))
    for k in keys_of(cfg):
        assert new[k].shape[0] == B and new[k].shape == old[k].shape
        assert torch.equal(new[k], again[k]), k
    sl = inputs(cfg, B, Ti, steps, lens)[1]
    ta = teacher_rows(B, steps, Ti, sl, cfg.dual)
    history_is_as_given(new, ta)
    history_is_as_given(old, ta)
    return new, launched


# ---- 1: equal to the launch-per-layer path
@pytest.mark.parametrize("B,Ti,steps,mode,lens", [(3, 57, 19, "free", (57, 41, 33)),   # an odd batch: the last group padded, a ragged last launch of 3
                                                  (4, 7, 12, "free", None),            # a memory shorter than the workgroup count
                                                  (16, 57, 19, "free", None),          # all eight XCDs
                                                  (5, 140, 33, "teacher", None),       # teacher-fed: several launches, no scan
                                                  (4, 33, 40, "stop", None)])          # the scan ends it at 7
def test_forced_groups_equal_the_launch_per_layer_path(B, Ti, steps, mode, lens):
    _, launched = compare("dual", B, Ti, steps, mode, lens, want_steps=7 if mode == "stop" else None)
    if mode == "teacher":          # (in front: the warm-up launch of the new session; the ragged launch has blocks of its own)
        assert [n for _, _, n in launched] == [8] + [8, 8, 8, 8, 1]
    if B == 3:
        assert [n for _, _, n in launched][-3:] == [8, 8, 3]


# ---- 2: the other models
@pytest.mark.parametrize("model", ["speakers", "dropout", "spk decoder", "agent", "baseline", "baseline+speakers", "baseline agent"])
def test_forced_groups_of_the_other_models(model):
    """B = 6, Ti = 57, 19 steps: six different speakers, dropout on inference (the mask row is b0 + b), the wide memories of
    speaker_embedd_to_decoder, the transition-agent models without any option block, and the single-source form"""
    new, _ = compare(model, 6, 57, 19)
    ses = run(model, 6, 57, 19)[1]
    m = new["mel"]
    if "speakers" in model or model == "spk decoder":
        assert min(float((m[a] - m[b]).abs().max()) for a in range(6) for b in range(a)) > 1e-3
    if model == "dropout":          # the rows of one group, and the same row of different groups, draw different masks
        assert float((m[0] - m[2]).abs().max()) > 1e-3 and float((m[0] - m[1]).abs().max()) > 1e-3
    if "agent" in model:
        assert all(not g.has_opt for g in ses.mega_groups) and ses.agent_tab is None


# ---- 3: masking
@pytest.mark.parametrize("model", ["dual", "baseline"])
def test_rows_are_masked_in_the_products_and_not_in_the_history(model):
    """lengths (57, 41, 33, 57) and teacher rows with mass BEYOND the lengths: the contexts ignore that mass (equal to the
    launch-per-layer path: r < length ? a[r] : 0), the histories show the rows as given"""
    lens = (57, 41, 33, 57)
    ta = teacher_rows(4, 19, 57, lens, engine(model)[1].dual, masked=False)
    assert float(ta[0][1, :, 41:].sum()) > 1.0 and float(ta[0][2, :, 33:].sum()) > 1.0
    new, ses, launched = run(model, 4, 57, 19, True, lens=lens, ta=ta, tag="unmasked")
    took_forced_groups(ses, launched, model, 4)
    old, _, _ = run(model, 4, 57, 19, False, lens=lens, ta=ta, tag="unmasked")
    same(new, old, model + " unmasked rows")
    history_is_as_given(new, ta)
    assert float(new["alignment1"][2, :, 33:].sum()) > 1.0


# ---- 4: the rows belong to their batch row, across groups
def test_teacher_rows_belong_to_their_batch_row_across_groups():
    """B = 6 on the cached session: the teacher rows rotated by one sample, so every row moves to the other slot of its pair or into
    the next group.  The result equals the launch-per-layer result for the rotated rows, differs from the first run by more than
    100 bars in every sample, and the first input again gives the first run's bits."""
    B, Ti, steps = 6, 57, 19
    lens = (57, 41, 33, 57, 49, 37)
    ta = teacher_rows(B, steps, Ti, lens, True, sharp=4)
    rot = (ta[0].roll(1, 0).contiguous(), ta[1].roll(1, 0).contiguous())
    first, ses, launched = run("dual", B, Ti, steps, True, lens=lens, ta=ta, tag="sharp", fresh=True)
    took_forced_groups(ses, launched, "dual", B)
    rotated, ses2, _ = run("dual", B, Ti, steps, True, lens=lens, ta=rot, tag="rotated")
    again, ses3, _ = run("dual", B, Ti, steps, True, lens=lens, ta=ta, tag="sharp", fresh=True)
    assert ses2 is ses and ses3 is ses
    old, _, _ = run("dual", B, Ti, steps, False, lens=lens, ta=rot, tag="rotated")
    same(rotated, old, "rotated rows", ("mel", "stop", "alignment1", "alignment2"))
    history_is_as_given(rotated, rot)
    for row in range(B):
        d = rel_err(rotated["mel"][row].numpy(), first["mel"][row].numpy())
        print("row %d: its neighbour's rows: mel differs by %.3e (must exceed %.0e)" % (row, d, 100 * BAR))
        assert d > 100 * BAR, (row, d)
    for k in ("mel", "stop", "alignment1", "alignment2"):
        assert torch.equal(again[k], first[k]), k


# ---- 5: a group is the forced B = 2 launch
def test_a_forced_group_computes_what_the_forced_two_sample_launch_computes():
    """B = 4, Ti = 57, 24 steps, 8 steps per launch on both sides.  The forced B = 2 session of the existing kernel gets the memories,
    keys, context tables and teacher rows of samples 2 g, 2 g + 1 of the grouped session (copied: the comparison is about the kernel)
    and runs three launches: frames, stop logits and both histories are torch.equal to rows 2 g, 2 g + 1 of the grouped run."""
    from satt_amd import ops
    B, Ti, steps = 4, 57, 24
    big, ses4, launched = run("dual", B, Ti, steps, True, fresh=True)
    took_forced_groups(ses4, launched, "dual", B)
    _, ses2, none = run("dual", 2, Ti, steps, True, fresh=True)
    assert ses2.mega is not None and ses2.mega_forced is not None and ses2.mega_groups is None and not none and ses2.K == K
    assert ops.dec_mega_forced_variant(ses2.mega, ses2.mega_opt, ses2.mega_forced) | ops.MEGA_VAR_GROUPS == \
        ops.dec_mega_groups_forced_variant(ses4.mega_groups, ses4.mega_forced)
    NO = ses4.yout.shape[-1]
    cfg = engine("dual")[1]
    for g in range(B // 2):
        rows = slice(2 * g, 2 * g + 2)
        ses2.lengths.copy_(ses4.lengths[rows])
        for name in ("values1", "keys1", "values2", "keys2", "ctab"):
            dst, src = getattr(ses2, name), getattr(ses4, name)
            dst.copy_(src.view(-1, Ti, src.shape[-1])[rows].reshape(dst.shape))
        ses2.teach1.copy_(ses4.teach1[rows]); ses2.teach2.copy_(ses4.teach2[rows])
        ses2.reset()
        for _ in range(steps // K):
            ses2.replay()
        torch.cuda.synchronize()
        ses2.check()
        for name, a, b in (("frames", ses2.yout[:, 1:steps + 1], ses4.yout[rows, 1:steps + 1]),
                           ("alignment1", ses2.al1[:, :steps], ses4.al1[rows, :steps]), ("alignment2", ses2.al2[:, :steps], ses4.al2[rows, :steps])):
            print("group", g, name, float((a - b).abs().max()))
            assert torch.equal(a, b), (g, name)
        assert torch.equal(ses4.yout[rows, 1:steps + 1, :NO - 1].reshape(2, steps * cfg.r, -1).cpu(), big["mel"][rows])
        assert torch.equal(ses4.yout[rows, 1:steps + 1, NO - 1:].cpu(), big["stop"][rows])


# ---- 6: self-consistency
@pytest.mark.parametrize("model", ["dual", "baseline"])
def test_a_free_run_fed_its_own_alignments_reproduces_itself(model):
    from satt_amd.inference import infer
    B, Ti, steps = 6, 57, 19
    eng, cfg, _, _ = engine(model)
    src, sl, _ = inputs(cfg, B, Ti, steps)
    with switches(MEGA_GROUPS_STEPS=K):
        free = infer(eng, src, sl, max_steps=steps, min_steps=10 ** 6)
    ta = (free["alignment1"].cpu(), free["alignment2"].cpu() if cfg.dual else None)
    again, ses, launched = run(model, B, Ti, steps, True, ta=ta, tag="own", fresh=True)
    took_forced_groups(ses, launched, model, B)
    same(again, {"mel": free["mel"].cpu(), "stop": free["stop"].cpu(), "steps": free["steps"]}, model + " own alignments")


# ---- 7: float64 oracle
def test_forced_groups_are_as_close_to_the_float64_oracle_as_the_launch_per_layer_path():
    """B = 4, 19 steps.  Both paths multiply with the same bf16 weights, so their distance from the float64 oracle (fp32 parameters)
    is the rounding of the weights; the launch-per-layer path's distance, measured in the same test, is the yardstick and the new
    path may be at most twice as far (tests/test_decode_forced_gpu.py test_forced_persistent_path_is_as_close_...)."""
    from oracle import torch_ref
    B, Ti, steps = 4, 57, 19
    eng, cfg, P, mv = engine("dual")
    src, sl, _ = inputs(cfg, B, Ti, steps)
    ta = teacher_rows(B, steps, Ti, sl, True)
    ref = torch_ref.infer(torch_ref.to_torch(P), src, sl, torch_ref.Cfg(), steps, mv, min_steps=10 ** 6,
                          teacher_alignments=[a.double() for a in ta])
    new, ses, launched = run("dual", B, Ti, steps, True)
    took_forced_groups(ses, launched, "dual", B)
    old, _, _ = run("dual", B, Ti, steps, False)
    assert ref["steps"] == new["steps"] == old["steps"] == steps
    bad = {}
    for k in ("mel", "stop", "alignment1", "alignment2"):
        dn, do = rel_err(new[k].numpy(), ref[k].numpy()), rel_err(old[k].numpy(), ref[k].numpy())
        print("oracle distance %-10s forced groups %.3e launch-per-layer %.3e" % (k, dn, do))
        if not dn <= 2 * do:
            bad[k] = (dn, do)
    assert not bad, bad


# ---- 8: LDS poison
@pytest.mark.parametrize("model", ["dual", "baseline"])
def test_forced_groups_do_not_depend_on_what_the_lds_held_before_the_launch(model):
    """quiet NaN in every LDS word of every CU in front of every launch (satt_debug_poison_lds, in process): the bits of the clean run"""
    clean, ses, launched = run(model, 4, 57, 19, True)
    took_forced_groups(ses, launched, model, 4)
    dirty, _, again = run(model, 4, 57, 19, True, poison=0x7fc00000)
    assert len(again) == 3 and dirty["steps"] == clean["steps"] == 19          # (three launches, each behind the pattern)
    for k in keys_of(engine(model)[1]):
        assert torch.equal(dirty[k], clean[k]), k


# ---- 9: the switches
@pytest.mark.parametrize("switch", [dict(MEGA_FORCED=False), dict(MEGA_GROUPS=False), dict(MEGA_GROUPS_MAX_B=3)])
def test_the_switches_return_a_forced_batch_to_the_launch_per_layer_path(switch):
    on, ses, launched = run("dual", 4, 33, 9, True)
    took_forced_groups(ses, launched, "dual", 4)
    off, ses_off, none = run("dual", 4, 33, 9, True, switches=switch)
    assert ses_off.mega_groups is None and ses_off.mega_forced is None and ses_off.mega is None and ses_off.graph is not None and not none
    same(off, on, "switch %s" % switch, ("mel", "stop", "alignment1", "alignment2"))


def test_a_free_running_batch_still_launches_through_the_group_entry_point():
    from satt_amd.inference import infer
    eng, cfg, _, _ = engine("dual")
    src, sl, _ = inputs(cfg, 4, 33, 9)
    with recording() as launches, sessions_used() as used:
        out = infer(eng, src, sl, max_steps=9, min_steps=10 ** 6)
    ses, = used
    assert ses.mega_groups is not None and ses.mega_forced is None and out["steps"] == 9
    calls = [l.name for l in launches]
    assert calls and set(calls) == {"dec_mega_groups"}


# ---- 10: the driver
def write_corpus(root, lengths):
    """a corpus of len(lengths) utterances with (source symbols, raw target frames) as given, the way tests/test_drivers_gpu.py
    builds its corpus; returns the keys"""
    from satt_amd.utils import tfrecord
    g = np.random.default_rng(0)
    keys = ["LJ%03d" % i for i in range(len(lengths))]
    for i, (k, (L, T)) in enumerate(zip(keys, lengths)):
        s = np.concatenate([[0], g.integers(1, 60, L - 2), [0]]).astype("<i8")
        tfrecord.write_records(os.path.join(root, k + ".source.tfrecord"), [tfrecord.make_example(
            {"id": i, "key": k.encode(), "source": s.tobytes(), "source_length": L, "text": b"abc"})])
        mel = g.normal(-40, 10, (T, 80)).astype("<f4")
        tfrecord.write_records(os.path.join(root, k + ".target.tfrecord"), [tfrecord.make_example(
            {"id": i, "key": k.encode(), "mel": mel.tobytes(), "mel_width": 80, "target_length": T})])
    return keys


LENGTHS = [(9, 21), (14, 30), (11, 17), (8, 26), (12, 23)]          # five utterances of different lengths (symbols, raw frames)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """corpus, lists, the LJSpeech example's hparams file and one checkpoint of a freshly initialised model; the global hparams
    object predict_mel.main parses into is restored behind the module's tests"""
    sys.path.insert(0, ROOT)
    import satt_amd  # noqa: F401
    from satt_amd.hparams import hparams
    from satt_amd.models.models import tacotron_model_factory
    import copy
    saved = copy.deepcopy(hparams.values())
    tmp = tmp_path_factory.mktemp("forced_groups_driver")
    data, lists, ckpt = tmp / "data", tmp / "lists", tmp / "ckpt"
    for d in (data, lists, ckpt):
        d.mkdir()
    keys = write_corpus(str(data), LENGTHS)
    (lists / "test.csv").write_text("\n".join(keys) + "\n")
    d = json.load(open(os.path.join(ROOT, "examples", "ljspeech", "self-attention-tacotron.json")))
    d.pop("_comment", None)
    d.update(average_mel_level_db=[-40.0], stddev_mel_level_db=[10.0])
    cfg = str(tmp / "hparams.json")
    json.dump(d, open(cfg, "w"))
    hp = hparams.copy()
    hp.parse_json(open(cfg).read())
    try:
        model = tacotron_model_factory(hp, str(ckpt), device="cuda")
        model.save()
        del model
        common = ["--source-data-root", str(data), "--target-data-root", str(data), "--checkpoint-dir", str(ckpt),
                  "--selected-list-dir", str(lists), "--hparam-json-file", cfg]
        yield tmp, keys, common
    finally:
        hparams._v.clear(); hparams._v.update(saved)
        from satt_amd import ops
        ops.set_precision("bf16")


def predict(corpus, name, forced, extra=(), mega=True):
    """predict_mel.main in process; returns (output directory, the recorded forced group launches)"""
    import predict_mel
    tmp, keys, common = corpus
    out = tmp / name
    out.mkdir()
    with switches(MEGA=mega), recording() as launches:
        predict_mel.main(["--output-dir", str(out), "--hparams", "use_forced_alignment_mode=%s" % forced] + common + list(extra))
    return out, [(l.variant, l.groups) for l in launches if l.name == "dec_mega_groups_forced"]


def prepared(T, r=2):
    return T + 2 * r + (-(T + 2 * r)) % r          # + 2r silence frames, tail-padded to a multiple of r


def test_predict_mel_batch_size_decodes_forced_batches_in_group_mode(corpus):
    from satt_amd import ops
    tmp, keys, _ = corpus
    new, launched = predict(corpus, "bs4", True, ("--batch-size", "4"))
    old, none = predict(corpus, "bs4_graph", True, ("--batch-size", "4"), mega=False)
    # the first batch of four ran both passes in group mode - the second pass through the forced group launch; the fifth utterance is a batch of one
    want = ops.MEGA_VAR_FORCED | ops.MEGA_VAR_GROUPS | ops.MEGA_VAR_TWO_SAMPLES
    assert launched and {v for v, _ in launched} == {want} and {n for _, n in launched} == {2}, launched          # FAILS ON THE PARENT
    assert not none
    files = sorted(os.listdir(new))
    assert files == sorted(k + e for k in keys for e in (".mfbsp", ".alignment.npz", ".png", ".tfrecord")) == sorted(os.listdir(old))
    for k, (L, T) in zip(keys, LENGTHS):
        n = prepared(T)
        a, b = (np.fromfile(d / (k + ".mfbsp"), dtype="<f4").reshape(-1, 80) for d in (new, old))
        assert a.shape == b.shape == (n, 80) and np.isfinite(a).all(), (k, a.shape, n)          # each utterance's own ceil(target_length / r) * r
        e = rel_err(a, b)
        print("%s mel rel_err=%.3e (bar %.0e)" % (k, e, BAR))
        assert e < BAR, (k, e)
        za, zb = np.load(new / (k + ".alignment.npz")), np.load(old / (k + ".alignment.npz"))
        for name in ("alignment", "alignment2"):
            assert za[name].shape == zb[name].shape == (L, n // 2), (k, name, za[name].shape)          # [T_memory, T_query], cut to the utterance
            e = rel_err(za[name], zb[name])
            print("%s %s rel_err=%.3e" % (k, name, e))
            assert e < BAR, (k, name, e)
            assert np.allclose(za[name].sum(0), 1.0, atol=1e-4)


def test_predict_mel_batch_size_needs_forced_mode(corpus):
    with pytest.raises(SystemExit) as e:
        predict(corpus, "refused", False, ("--batch-size", "4"))
    assert "use_forced_alignment_mode" in str(e.value)
    assert not os.listdir(corpus[0] / "refused")
    for n in ("0", "17"):
        with pytest.raises(SystemExit):
            predict(corpus, "refused" + n, True, ("--batch-size", n))


def test_predict_mel_batch_size_one_is_the_run_without_the_option(corpus):
    tmp, keys, _ = corpus
    one, _ = predict(corpus, "bs1", True, ("--batch-size", "1"))
    plain, _ = predict(corpus, "plain", True)
    assert sorted(os.listdir(one)) == sorted(os.listdir(plain))
    for f in sorted(os.listdir(plain)):
        assert open(one / f, "rb").read() == open(plain / f, "rb").read(), f
    for k, (L, T) in zip(keys, LENGTHS):          # ... and the cut of the batched run gives each file these shapes
        assert np.fromfile(plain / (k + ".mfbsp"), dtype="<f4").size == prepared(T) * 80
        assert np.load(plain / (k + ".alignment.npz"))["alignment"].shape == (L, prepared(T) // 2)
