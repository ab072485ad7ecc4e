"""Forced-alignment synthesis (infer(..., teacher_alignments=...): use_forced_alignment_mode, reference
modules/teacher_forcing_attention.py:29-35) on the forced instantiations of the persistent decode kernel (csrc/decode_mega2.hip,
template flag FRC; satt_dec_mega_forced) against the hipGraph of launch-per-layer steps every forced session ran on before
(csrc/decode.hip) and against the float64 oracle.

The step under forced alignments has no query layer, no energies, no softmax, no recursion and no agent: row t of the teacher
histories IS the alignment.  What can go wrong is where the rows go: the histories and the hand-over take them AS GIVEN, the table
products and the handed-over contexts take them masked by the length, each sample has its own rows, the row of step t + 1 is
requested during step t (and across launch boundaries), and the transition-agent models run without any option block.  The cases
are shaped for that: B = 1 with the context tables in LDS (Ti = 33) and in global memory (Ti = 113), B = 2 with lengths (57, 41);
19 steps with MEGA_STEPS = 8 (launch boundaries at 8 and 16, a ragged last launch, folded and unfolded pre-net 0), the fold off, and
one long launch.

TEST 1 FAILS ON THE PARENT (a forced session never takes the kernel there: `ses.mega is None`), and with it every test that asserts
the path through run().
Bar: 2e-5 relative to the largest element, the bar of tests/test_decode_speaker_gpu.py for exactly this comparison (same bf16
weights, same buffers, fp32 sums in another order, fed back through the steps)."""
import pytest
import torch

from common import rel_err
from decode_common import (BAR, BASELINE, Engines, expected_variant, history_is_as_given, host_outputs, infer_kwargs, inputs, same, switches,
                           teacher_rows, traced_infer)

pytestmark = pytest.mark.gpu

STEPS = 19
SPK = dict(num_speakers=4, speaker_dim=16, speaker_offset=225)
MODELS = {
    "dual": dict(),
    "baseline": BASELINE,
    "speakers": SPK,
    "dropout": dict(apply_dropout_on_inference=True),
    "agent": dict(transition_agent=True),
    "baseline agent": dict(BASELINE, transition_agent=True),
}
SHAPES = {"B=1 Ti=33": (1, 33, (33,)), "B=1 Ti=113": (1, 113, (113,)), "B=2 Ti=57": (2, 57, (57, 41))}
FORMS = {"tables": (8, True), "nofold": (8, False), "long": (32, True)}          # -> (MEGA_STEPS, MEGA_FOLD_FEEDBACK)
IDS = {1: (226,), 2: (225, 227)}
B2 = "B=2 Ti=57"

engine = Engines(MODELS, stats=True)
_runs = {}


def inputs_of(cfg, shape):
    """source, lengths (the shape's own: B = 2 has (57, 41)) and the target frames of `shape`"""
    B, Ti, lens = SHAPES[shape]
    return inputs(cfg, B, Ti, STEPS, lens)


def rows_of(shape, dual, **kw):
    """the teacher rows of `shape` (masked=False: mass beyond the lengths)"""
    B, Ti, lens = SHAPES[shape]
    return teacher_rows(B, STEPS, Ti, lens, dual, **kw)


def run(model, shape, mega, form="tables", mode="free", ta=None, tag="masked", poison=None, fresh=False, forced_switch=True):
    """one forced utterance; returns (outputs on the host, the session, the set of variants the persistent kernel was launched with).
    Results are computed once per key and shared (fresh=True: computed again).  The launch-per-layer result does not depend on the form."""
    key = (model, shape, mega, form if mega else None, mode, tag, poison, forced_switch)
    if key in _runs and not fresh:
        return _runs[key]
    eng, cfg, _, _ = engine(model, stop=(mode == "stop"))
    B = SHAPES[shape][0]
    src, sl, mel = inputs_of(cfg, shape)
    if ta is None:
        ta = rows_of(shape, cfg.dual)
    kw = infer_kwargs(mode, STEPS, mel, IDS[B] if cfg.num_speakers else None,
                      1234 if cfg.apply_dropout_on_inference else None)          # the same masks on both paths
    K, fold = FORMS[form]
    out, ses, launches = traced_infer(eng, src, sl, dict(MEGA=mega, MEGA_FORCED=forced_switch, MEGA_STEPS=K, MEGA_FOLD_FEEDBACK=fold),
                                      poison, teacher_alignments=ta, **kw)
    others = [l.name for l in launches if l.name != "dec_mega_forced"]
    assert not others, others          # a forced session launches through ops.dec_mega_forced only
    _runs[key] = (host_outputs(out), ses, {l.variant for l in launches})
    return _runs[key]


def took_the_forced_kernel(ses, launched, model, shape, form="tables", mode="free"):
    from satt_amd import ops
    cfg = engine(model)[1]
    B, Ti, _ = SHAPES[shape]
    assert ses.mega is not None and ses.mega_forced is not None, "the forced session did not take the persistent kernel"      # FAILS ON THE PARENT
    assert ses.graph is None and ses.kernel_launches == 1 and ses.K == FORMS[form][0]
    assert ses.agent_tab is None and ses.u_state is None          # the agent is dead under forced alignments
    drop = cfg.apply_dropout_on_inference and cfg.dual
    assert (ses.mega_opt is not None) == bool(drop)
    assert (ses._fb is not None) == (FORMS[form][1] and mode != "teacher")
    want = expected_variant(cfg, B, Ti, forced=True)
    assert launched == {want}, (launched, want)          # every launch carried MEGA_VAR_FORCED, none MEGA_VAR_LJ (no such sibling)
    assert ops.dec_mega_forced_variant(ses.mega, ses.mega_opt, ses.mega_forced) == want


# ---- 1: the path taken
def test_forced_sessions_take_the_persistent_kernel():
    new, ses, launched = run("dual", B2, True)
    took_the_forced_kernel(ses, launched, "dual", B2)          # FAILS ON THE PARENT
    assert ses.mega.Td == ses.Tdp and ses.teach1.shape == (2, ses.Tdp, 57) and ses.teach2.shape == ses.teach1.shape
    old, ses_old, none = run("dual", B2, False)
    assert ses_old.mega is None and ses_old.mega_forced is None and ses_old.graph is not None and not none
    # the switch: MEGA_FORCED = False returns a forced session to the hipGraph path (free-running sessions are not concerned)
    off, ses_off, none = run("dual", B2, True, forced_switch=False)
    assert ses_off.mega is None and ses_off.graph is not None and not none
    same(off, old, "MEGA_FORCED = False", keys=("mel", "stop", "alignment1", "alignment2"))


# ---- 2: equal to the launch-per-layer path
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("model", list(MODELS))
def test_forced_persistent_equals_the_launch_per_layer_path(model, form, shape):
    new, ses, launched = run(model, shape, True, form)
    took_the_forced_kernel(ses, launched, model, shape, form)
    old, ses_old, none = run(model, shape, False)
    assert ses_old.mega is None and not none
    assert new["steps"] == STEPS
    same(new, old, "%s %s %s" % (model, form, shape))
    ta = rows_of(shape, engine(model)[1].dual)
    history_is_as_given(new, ta)
    history_is_as_given(old, ta)


@pytest.mark.parametrize("mode", ["teacher", "stop"])
@pytest.mark.parametrize("model", ["dual", "baseline"])
def test_teacher_feeding_and_the_stop_rule_under_forced_alignments(model, mode):
    """teacher= feeding (no folded feedback, no stop rule) and the stop rule firing inside a launch (min_steps = 5, the stop logit
    always large: 7 steps)"""
    new, ses, launched = run(model, B2, True, "tables", mode)
    took_the_forced_kernel(ses, launched, model, B2, "tables", mode)
    old, ses_old, none = run(model, B2, False, mode=mode)
    assert ses_old.mega is None and not none
    assert new["steps"] == (7 if mode == "stop" else STEPS)
    same(new, old, "%s %s" % (model, mode))
    history_is_as_given(new, rows_of(B2, engine(model)[1].dual))


# ---- 3: masking
@pytest.mark.parametrize("model", ["dual", "baseline"])
def test_rows_are_masked_in_the_products_and_not_in_the_history(model):
    """lengths (57, 41) and teacher rows with mass BEYOND row 41 of sample 1: the contexts weight row r with r < length ? a[r] : 0
    (csrc/decode.hip dec_attn_context_k), the histories show the rows as given"""
    ta = rows_of(B2, engine(model)[1].dual, masked=False)
    assert float(ta[0][1, :, 41:].sum()) > 1.0
    new, ses, launched = run(model, B2, True, "tables", ta=ta, tag="unmasked")
    took_the_forced_kernel(ses, launched, model, B2)
    old, _, _ = run(model, B2, False, ta=ta, tag="unmasked")
    same(new, old, model + " unmasked rows")
    history_is_as_given(new, ta)
    assert float(new["alignment1"][1, :, 41:].sum()) > 1.0


# ---- 4: the rows are live and belong to their sample
@pytest.mark.parametrize("form", ["tables", "nofold"])
def test_teacher_rows_are_live_and_belong_to_their_sample(form):
    """the two samples' teacher rows swapped ON THE CACHED SESSION (the rows are rewritten in place, no pointer changes): the result
    equals the launch-per-layer result for the swapped rows and differs from the first run by more than 100 bars; the first input
    again gives the first run's bits"""
    ta = rows_of(B2, True)
    sw = (ta[0].flip(0).contiguous(), ta[1].flip(0).contiguous())
    first, ses, launched = run("dual", B2, True, form, fresh=True)
    took_the_forced_kernel(ses, launched, "dual", B2, form)
    swapped, ses2, _ = run("dual", B2, True, form, ta=sw, tag="swapped")
    again, ses3, _ = run("dual", B2, True, form, fresh=True)
    assert ses2 is ses and ses3 is ses
    old, _, _ = run("dual", B2, False, ta=sw, tag="swapped")
    same(swapped, old, form + " swapped rows")
    history_is_as_given(swapped, sw)
    for row in (0, 1):
        d = rel_err(swapped["mel"][row].numpy(), first["mel"][row].numpy())
        print("row %d: the other sample's rows: mel differs by %.3e (must exceed %.0e)" % (row, d, 100 * BAR))
        assert d > 100 * BAR, (row, d)
    for k in ("mel", "stop", "alignment1", "alignment2"):
        assert torch.equal(again[k], first[k]), k


# ---- 5: self-consistency
@pytest.mark.parametrize("model", ["dual", "baseline"])
def test_a_free_run_fed_its_own_alignments_reproduces_itself(model):
    from satt_amd.inference import infer
    eng, cfg, _, _ = engine(model)
    src, sl, _ = inputs_of(cfg, B2)
    with switches(MEGA_STEPS=8):
        free = infer(eng, src, sl, max_steps=STEPS, min_steps=10 ** 6)
    ta = (free["alignment1"].cpu(), free["alignment2"].cpu() if cfg.dual else None)
    again, ses, launched = run(model, B2, True, "tables", ta=ta, tag="own", fresh=True)
    took_the_forced_kernel(ses, launched, model, B2)
    same(again, {"mel": free["mel"].cpu(), "stop": free["stop"].cpu(), "steps": free["steps"]}, model + " own alignments")


# ---- 6: hand-over
@pytest.mark.parametrize("model", ["dual", "baseline"])
def test_forced_kernel_hands_over_to_the_launch_per_layer_path(model):
    """the first 8 steps on the kernel, the other 11 on the launch-per-layer entry points (the pattern of
    tests/test_inference_gpu.py test_persistent_decode_kernel_hands_over_to_the_launch_per_layer_path_and_back): recurrent state,
    contexts (masked rows), a_state = alpha_state = the given row of mechanism 1, step counters, K|V|Q rows and histories cross"""
    new, ses, launched = run(model, B2, True, "tables", fresh=True)      # (the session's memories, tables and teacher rows are this utterance's)
    took_the_forced_kernel(ses, launched, model, B2)
    old, _, _ = run(model, B2, False)
    ses.reset()
    ses.replay()
    for _ in range(STEPS - ses.K):
        ses.run_step()
    torch.cuda.synchronize()
    ses.check()
    NO = ses.yout.shape[-1]
    y = ses.yout[:, 1:STEPS + 1].cpu()
    mixed = {"mel": y[:, :, :NO - 1].reshape(old["mel"].shape), "stop": y[:, :, NO - 1:], "steps": STEPS,
             "alignment1": ses.al1[:, :STEPS].cpu(), "alignment2": ses.al2[:, :STEPS].cpu() if ses.al2 is not None else None}
    same(mixed, old, model + " 8 steps persistent + 11 launch per layer")
    history_is_as_given(mixed, rows_of(B2, engine(model)[1].dual))


# ---- 7: float64 oracle
def test_forced_persistent_path_is_as_close_to_the_float64_oracle_as_the_launch_per_layer_path():
    """B = 2, 19 steps.  Both paths multiply with the same bf16 weights, so their distance from the float64 oracle (fp32 parameters)
    is the rounding of the weights; the launch-per-layer path's distance, measured in the same test, is the yardstick and the
    persistent path may be at most twice as far (tests/test_decode_speaker_gpu.py)."""
    from oracle import torch_ref
    eng, cfg, P, mv = engine("dual")
    src, sl, _ = inputs_of(cfg, B2)
    ta = rows_of(B2, True)
    ref = torch_ref.infer(torch_ref.to_torch(P), src, sl, torch_ref.Cfg(), STEPS, mv, min_steps=10 ** 6,
                          teacher_alignments=[a.double() for a in ta])
    new, ses, launched = run("dual", B2, True)
    took_the_forced_kernel(ses, launched, "dual", B2)
    old, _, _ = run("dual", B2, False)
    assert ref["steps"] == new["steps"] == old["steps"] == STEPS
    bad = {}
    for k in ("mel", "stop", "alignment1", "alignment2"):
        dn, do = rel_err(new[k].numpy(), ref[k].numpy()), rel_err(old[k].numpy(), ref[k].numpy())
        print("oracle distance %-10s persistent %.3e launch-per-layer %.3e" % (k, dn, do))
        if not dn <= 2 * do:
            bad[k] = (dn, do)
    assert not bad, bad


# ---- 8: LDS poison
@pytest.mark.parametrize("model,shape", [("dual", B2), ("dual", "B=1 Ti=33"), ("baseline", B2)])
def test_forced_kernel_does_not_depend_on_what_the_lds_held_before_the_launch(model, shape):
    """quiet NaN in every LDS word of every CU in front of every launch (satt_debug_poison_lds, in process): the bits of the clean
    run.  The forced kernel skips the prologue fills of the mechanisms' tables: nothing it reads may be left unwritten by that."""
    clean, ses, launched = run(model, shape, True)
    took_the_forced_kernel(ses, launched, model, shape)
    dirty, _, _ = run(model, shape, True, poison=0x7fc00000)
    assert dirty["steps"] == clean["steps"]
    for k in ("mel", "stop", "alignment1"):
        assert torch.equal(dirty[k], clean[k]), k
