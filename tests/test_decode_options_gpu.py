"""The transition agent, pre-net dropout that stays on and the wide speaker memories on the persistent decode kernel
(csrc/decode_mega2.hip: template flag OPT, include/satt_hip.h: satt_dec_mega_opt_params) against the launch-per-layer path they
ran on before (csrc/decode.hip) and against the float64 oracle.

  * agent: u_{t+1} = sigmoid([context1_t | processed_query1_t] Wa + ba) replaces the 0.5 factors of the forward recursion; the
    kernel takes the context part from a per-utterance table (DecodeSession.agent_tab) and carries u across launches in u_state;
  * dropout (apply_dropout_on_inference): the launch-per-layer masks, element ((b * Td + step) * N + column), behind the ReLU of
    both forms of pre-net 0 and of pre-net 1 - a wrong index gives O(1) errors, not rounding;
  * speaker_to_decoder: memories [encoder output | speaker vector], contexts V + S wide - host work, the kernel is generic.
The forms (MEGA_STEPS, MEGA_FOLD_FEEDBACK): 8 steps per launch = several launches and a ragged last one within 19 steps, so u_state
and the masks' step index cross launch boundaries; the fold off; one long launch.

EVERY TEST HERE FAILS ON THE PARENT: there these models never take the kernel (`ses.mega is None`).
Bars: those of tests/test_decode_speaker_gpu.py (2e-5 relative to the largest element: same bf16 weights, fp32 sums in another
order, fed back through the steps; "live" means a difference of more than 100 bars)."""
import numpy as np
import pytest
import torch

from common import make_params, rel_err, small_batch
from decode_common import (BAR, KEYS, Engines, example_config, expected_variant, host_outputs, infer_kwargs, last_session, same, switches,
                           traced_infer)

pytestmark = pytest.mark.gpu

SPK = dict(num_speakers=4, speaker_dim=16, speaker_offset=225)
WIDE = dict(SPK, speaker_to_decoder=True)
MODELS = {
    "plain": dict(),
    "agent": dict(transition_agent=True),
    "agent0": dict(transition_agent=True),                       # Wa = 0, ba = 0: u = 0.5 at every step
    "agent+cumulative": dict(transition_agent=True, cumulative_weights=True),
    "dropout": dict(apply_dropout_on_inference=True),
    "dropout+speakers": dict(SPK, apply_dropout_on_inference=True),
    "agent+dropout": dict(transition_agent=True, apply_dropout_on_inference=True),
    # one fed-back frame per step (examples/ljspeech): the widths the kernel's compile-time specialisation is keyed on
    "agent, one fed frame": dict(transition_agent=True, n_feed_frame=1),
    "dropout, one fed frame": dict(apply_dropout_on_inference=True, n_feed_frame=1),
    "plain, one fed frame": dict(n_feed_frame=1),
    "dropout+speakers, one fed frame": dict(SPK, apply_dropout_on_inference=True, n_feed_frame=1),
    "wide": WIDE,
    "wide+resize": dict(WIDE, speaker_proj_dim=24),
}
SHAPES = {(1, 33): 9, (1, 140): 10, (2, 57): 19}            # (B, Ti) -> steps; Ti = 140: context tables in global memory
TI = {1: 33, 2: 57}
IDS = {1: (226,), 2: (225, 227)}                            # two DIFFERENT speakers in the two rows
FORMS = {"tables": (8, True), "nofold": (8, False), "tables32": (32, True)}          # -> (MEGA_STEPS, MEGA_FOLD_FEEDBACK)

# u far from 0.5, different per step and sample (tests/test_inference_gpu.py scales Wa the same way); "agent0": u = 0.5 at every step
engine = Engines(MODELS, stats=True, agent={None: (3.0, 1.5), "agent0": (0.0, 0.0)})
_runs = {}


def run(model, B, mode, mega, form="tables", Ti=None, ids=None, poison=None, fresh=False, seed=None):
    """one utterance; returns (outputs on the host, the instantiation of the persistent kernel that was LAUNCHED for it - None if
    none was).  Results are computed once and shared between the tests (fresh=True: computed again)."""
    Ti = TI[B] if Ti is None else Ti
    ids = IDS[B] if ids is None else ids
    key = (model, B, Ti, mode, mega, form, ids, poison, seed)
    if key in _runs and not fresh:
        return _runs[key]
    eng, cfg, _, _ = engine(model, stop=(mode == "stop"))
    steps = SHAPES[(B, Ti)]
    batch = small_batch(cfg, B, Ti, steps * cfg.r, seed=6)
    kw = infer_kwargs(mode, steps, batch["mel"], ids if cfg.num_speakers else None, seed)
    K, fold = FORMS[form]
    out, _, launches = traced_infer(eng, batch["source"], batch["source_length"], dict(MEGA=mega, MEGA_STEPS=K, MEGA_FOLD_FEEDBACK=fold),
                                    poison, **kw)
    launched = {l.variant for l in launches}          # (without options through ops.dec_mega, with them through ops.dec_mega_opt)
    assert len(launched) <= 1
    _runs[key] = (host_outputs(out), launched.pop() if launched else None)
    return _runs[key]


def took(var, B, bits, Ti=None, lj=False):
    """the launched instantiation: the form of the shape, the generic widths (the default model feeds two frames back) or the
    LJ-keyed ones, exactly the option / speaker bits `bits`"""
    from satt_amd import ops
    assert var is not None, "the model did not take the persistent kernel"          # FAILS ON THE PARENT
    form = expected_variant(engine.config("plain"), B, Ti or TI[B])          # (the plain model's instantiation is the form of the shape)
    assert var == form | (ops.MEGA_VAR_LJ if lj else 0) | bits, (var, form, bits)


def against_launch_per_layer(model, B, mode, form, bits, Ti=None, lj=False, **kw):
    new, var = run(model, B, mode, True, form, Ti=Ti, **kw)
    took(var, B, bits, Ti, lj)
    old, none = run(model, B, mode, False, Ti=Ti, **kw)
    assert none is None
    assert new["steps"] == (7 if mode == "stop" else SHAPES[(B, Ti or TI[B])])
    same(new, old, "%s %s %s B=%d" % (model, form, mode, B), KEYS)
    return new


CASES = [("tables", m, B) for B in (1, 2) for m in ("free", "teacher", "stop")] + [("nofold", "free", 2), ("tables32", "free", 2)]


# ---- 1: the agent, persistent against launch per layer
@pytest.mark.parametrize("form,mode,B", CASES)
def test_transition_agent_on_the_persistent_kernel_equals_the_launch_per_layer_path(form, mode, B):
    from satt_amd import ops
    against_launch_per_layer("agent", B, mode, form, ops.MEGA_VAR_AGENT)


@pytest.mark.parametrize("B,Ti", list(SHAPES))
def test_transition_agent_at_the_ljspeech_widths(B, Ti):
    """the specialised instantiations, in their three forms (B = 1 with LDS tables, B = 1 with global tables, B = 2)"""
    from satt_amd import ops
    against_launch_per_layer("agent, one fed frame", B, "free", "tables", ops.MEGA_VAR_AGENT, Ti=Ti, lj=True)


def test_transition_agent_with_global_tables():
    from satt_amd import ops
    against_launch_per_layer("agent", 1, "free", "tables", ops.MEGA_VAR_AGENT, Ti=140)


def test_transition_agent_with_cumulative_weights():
    from satt_amd import ops
    against_launch_per_layer("agent+cumulative", 2, "free", "tables", ops.MEGA_VAR_AGENT)


# ---- 2: the agent is live, and per row
def test_the_agent_is_live_in_each_row():
    """the same model with Wa = 0, ba = 0 has u = 0.5 at every step - the plain recursion, through the same instantiation.  Its
    alignments must differ from the agent's (Wa x 3, ba = 1.5) by more than 100 bars IN EACH ROW of the B = 2 case: an agent that
    is dropped, or whose u reaches row 0 only, fails this.  On the float64 oracle (CPU) these inputs separate the two by
    rel_err(alignment1) = 2.8e-1 (row 0) and 2.6e-1 (row 1): profiles/decode_options_bench_and_kernel_times.txt."""
    from satt_amd import ops
    live, var = run("agent", 2, "free", True, "tables")
    took(var, 2, ops.MEGA_VAR_AGENT)
    flat, var0 = run("agent0", 2, "free", True, "tables")
    took(var0, 2, ops.MEGA_VAR_AGENT)
    old, _ = run("agent0", 2, "free", False)
    same(flat, old, "u = 0.5", KEYS)
    for row in (0, 1):
        d = rel_err(live["alignment1"][row].numpy(), flat["alignment1"][row].numpy())
        print("row %d: alignment1 with the agent against u = 0.5 differs by %.3e (must exceed %.0e)" % (row, d, 100 * BAR))
        assert d > 100 * BAR, (row, d)


# ---- 3: the agent against the float64 oracle
def test_agent_on_the_persistent_path_is_as_close_to_the_float64_oracle_as_the_launch_per_layer_path():
    """B = 2, 19 teacher-fed steps.  Both paths multiply with the same bf16 weights, so their distance from the float64 oracle (fp32
    parameters) is the rounding of the weights; the launch-per-layer path's distance, measured in the same run, is the yardstick
    and the persistent path may be at most twice as far.  Measured (MI355X): profiles/decode_options_bench_and_kernel_times.txt."""
    from oracle import torch_ref
    from satt_amd import ops
    eng, cfg, P, mv = engine("agent")
    steps = SHAPES[(2, 57)]
    batch = small_batch(cfg, 2, 57, steps * cfg.r, seed=6)
    bt = torch_ref.batch_to_torch(batch)
    ref = torch_ref.infer(torch_ref.to_torch(P), bt["source"], bt["source_length"], torch_ref.Cfg(transition_agent=True), None, mv,
                          teacher=bt["mel"])
    new, var = run("agent", 2, "teacher", True, "tables")
    took(var, 2, ops.MEGA_VAR_AGENT)
    old, _ = run("agent", 2, "teacher", False)
    assert ref["steps"] == new["steps"] == old["steps"] == steps
    bad = {}
    for k in KEYS:
        dn, do = rel_err(new[k].numpy(), ref[k].numpy()), rel_err(old[k].numpy(), ref[k].numpy())
        print("oracle distance %-10s persistent %.3e launch-per-layer %.3e ratio %.3f" % (k, dn, do, dn / do))
        if not dn <= 2 * do:
            bad[k] = (dn, do)
    assert not bad, bad


# ---- 4: dropout
@pytest.mark.parametrize("form,mode,B", [(f, m, B) for f in ("tables", "nofold") for m in ("free", "teacher") for B in (1, 2)])
def test_dropout_on_the_persistent_kernel_draws_the_launch_per_layer_masks(form, mode, B):
    from satt_amd import ops
    against_launch_per_layer("dropout", B, mode, form, ops.MEGA_VAR_DROPOUT, seed=7)


@pytest.mark.parametrize("B,Ti", list(SHAPES))
def test_dropout_at_the_ljspeech_widths(B, Ti):
    from satt_amd import ops
    against_launch_per_layer("dropout, one fed frame", B, "free", "tables", ops.MEGA_VAR_DROPOUT, Ti=Ti, lj=True, seed=7)


def test_dropout_with_global_tables():
    from satt_amd import ops
    against_launch_per_layer("dropout", 1, "teacher", "tables", ops.MEGA_VAR_DROPOUT, Ti=140, seed=7)


@pytest.mark.parametrize("mode", ["free", "teacher"])
def test_dropout_in_a_speaker_model_masks_pre_net_1_only(mode):
    """MultiSpeakerPreNet (pre-net 0 of a speaker model) has no dropout, pre-net 1 has"""
    from satt_amd import ops
    new = against_launch_per_layer("dropout+speakers", 2, mode, "tables", ops.MEGA_VAR_DROPOUT | ops.MEGA_VAR_SPEAKER, seed=7)
    eng0, cfg0, P0, _ = engine("dropout+speakers")
    if mode == "free":          # ... and it is applied: the same parameters without the flag
        from satt_amd.engine import Engine
        from satt_amd.inference import infer
        from satt_amd.params import ModelConfig
        eng = Engine(ModelConfig(**SPK), "cuda", params=P0, rng_seed=7)
        for name, (m, v) in eng0.bn.items():
            eng.bn[name][0].copy_(m); eng.bn[name][1].copy_(v)
        batch = small_batch(cfg0, 2, 57, 19 * cfg0.r, seed=6)
        off = infer(eng, batch["source"], batch["source_length"], max_steps=19, min_steps=10 ** 6, speaker_id=torch.as_tensor(np.array(IDS[2], np.int64)))
        assert rel_err(new["mel"].numpy(), off["mel"].cpu().numpy()) > 100 * BAR


def test_dropout_masks_follow_the_seed():
    """without a pinned seed two calls differ; a pinned call repeats bit for bit; both differ from the dropout-free engine (the same
    parameters: the flag adds none)"""
    from satt_amd import ops
    pinned, var = run("dropout", 2, "free", True, "tables", seed=7)
    took(var, 2, ops.MEGA_VAR_DROPOUT)
    again, _ = run("dropout", 2, "free", True, "tables", seed=7, fresh=True)
    for k in KEYS:
        assert torch.equal(again[k], pinned[k]), k
    a, va = run("dropout", 2, "free", True, "tables", fresh=True)
    b, vb = run("dropout", 2, "free", True, "tables", fresh=True)
    took(va, 2, ops.MEGA_VAR_DROPOUT); took(vb, 2, ops.MEGA_VAR_DROPOUT)
    plain, vp = run("plain", 2, "free", True, "tables")
    took(vp, 2, 0)
    for what, x, y in (("two unpinned calls", a, b), ("pinned against dropout-free", pinned, plain), ("unpinned against dropout-free", a, plain)):
        d = rel_err(x["mel"].numpy(), y["mel"].numpy())
        print("%s: mel differs by %.3e (must exceed %.0e)" % (what, d, 100 * BAR))
        assert d > 100 * BAR, (what, d)


# ---- 5: both options
def test_agent_and_dropout_together():
    from satt_amd import ops
    against_launch_per_layer("agent+dropout", 2, "free", "tables", ops.MEGA_VAR_AGENT | ops.MEGA_VAR_DROPOUT, seed=7)


# ---- 6: wide memories (speaker_to_decoder)
@pytest.mark.parametrize("model", ["wide", "wide+resize"])
@pytest.mark.parametrize("mode", ["free", "teacher", "stop"])
@pytest.mark.parametrize("B,Ti", list(SHAPES))
def test_wide_speaker_memories_on_the_persistent_kernel_equal_the_launch_per_layer_path(B, Ti, mode, model):
    """V1 = 256 + S, V2 = 32 + S (S = 16, or 24 behind the resize layer): the generic instantiation with the speaker bit"""
    from satt_amd import ops
    against_launch_per_layer(model, B, mode, "tables", ops.MEGA_VAR_SPEAKER, Ti=Ti)


def test_the_speaker_columns_are_live_and_belong_to_their_row():
    """the two ids swapped ON THE CACHED SESSION: the launch-per-layer result for the swapped ids, and row 0 - the same text with the
    other speaker - moves by more than 100 bars"""
    from satt_amd import ops
    a, b = IDS[2]
    first, var = run("wide", 2, "free", True, "tables")
    took(var, 2, ops.MEGA_VAR_SPEAKER)
    swapped, _ = run("wide", 2, "free", True, "tables", ids=(b, a))
    old, _ = run("wide", 2, "free", False, ids=(b, a))
    same(swapped, old, "swapped ids", KEYS)
    d = rel_err(swapped["mel"][0].numpy(), first["mel"][0].numpy())
    print("row 0: other speaker, same text: mel differs by %.3e (must exceed %.0e)" % (d, 100 * BAR))
    assert d > 100 * BAR, d


def test_step_zero_reads_no_speaker_column():
    """the zero initial attention of step 0 covers the speaker columns: perturbing ONLY the speaker rows of dec.att_lstm.W leaves
    step 0's alignment1 as it was, to the bit, and changes step 1's (the context tables carry the wide rows)"""
    eng, cfg, _, _ = engine("wide")
    base, _ = run("wide", 2, "free", True, "tables")
    V1, V2, S, pn = cfg.cbhg_out_units, cfg.sa_units, cfg.mem_speaker, cfg.dec_prenet[-1]
    rows = [slice(pn + V1, pn + V1 + S), slice(pn + V1 + S + V2, pn + V1 + V2 + 2 * S)]
    W = eng.P["dec.att_lstm.W"]
    keep = W.clone()
    try:
        for sl in rows:
            W[sl] += 0.5
        moved, var = run("wide", 2, "free", True, "tables", fresh=True)
    finally:
        W.copy_(keep)
        _runs.pop(("wide", 2, 57, "free", True, "tables", IDS[2], None, None), None)
    assert var is not None
    assert torch.equal(moved["alignment1"][:, 0], base["alignment1"][:, 0])
    assert not torch.equal(moved["alignment1"][:, 1], base["alignment1"][:, 1])


def test_the_spk_decoder_example_widths():
    """examples/vctk/self-attention-tacotron-spk-decoder.json itself: 152 speakers, two fed-back frames per step (feed = 160)"""
    from satt_amd import ops
    from satt_amd.engine import Engine
    from satt_amd.inference import infer, DecodeSession
    want = example_config("self-attention-tacotron-spk-decoder", "vctk")
    cfg, P = make_params(dict(num_speakers=152, speaker_dim=16, speaker_offset=225, n_feed_frame=2, speaker_to_decoder=True), seed=4)
    for f in ("n_feed_frame", "num_speakers", "speaker_dim", "speaker_offset", "dec_prenet", "att_rnn_units", "att1_units", "att2_units", "dec_units",
              "dec_sa_units", "dec_sa_heads", "cbhg_out_units", "sa_units", "num_mels", "r", "att_kernel", "att_filters", "mem_speaker", "speaker_to_decoder"):
        assert getattr(cfg, f) == getattr(want, f), f
    ops.set_precision("bf16")
    eng = Engine(cfg, "cuda", params=P, rng_seed=7)
    batch = small_batch(cfg, 1, 33, 9 * cfg.r, seed=6)
    call = lambda: infer(eng, batch["source"], batch["source_length"], max_steps=9, min_steps=10 ** 6, speaker_id=torch.as_tensor([225 + 151]))
    with switches(MEGA=True, MEGA_STEPS=8):
        new = call()
        ses = last_session(eng)          # (a new engine: the session is new)
        assert ses.mega is not None          # FAILS ON THE PARENT
        assert ops.dec_mega_variant(ses.mega) == ops.MEGA_VAR_TABLES_LDS | ops.MEGA_VAR_SPEAKER and ses.mega_opt is None
        DecodeSession.MEGA = False
        old = call()
        assert last_session(eng).mega is None
    same(host_outputs(new), host_outputs(old), "spk-decoder example", KEYS)


# ---- 7: LDS poison
@pytest.mark.parametrize("model,bits", [("agent", "AGENT"), ("dropout", "DROPOUT")])
def test_option_kernels_do_not_depend_on_what_the_lds_held_before_the_launch(model, bits):
    """quiet NaN in every LDS word of every CU in front of every launch of the kernel (satt_debug_poison_lds, in process): the bits of
    the clean run.  The agent table and the agent's weights are LDS words behind the tables the plain kernel has: the
    start-of-launch zeroing covers them (rows beyond Ti and weights beyond U1 are multiplied, by zero) before they are filled."""
    from satt_amd import ops
    seed = 7 if model == "dropout" else None
    clean, var = run(model, 2, "free", True, "tables", seed=seed)
    took(var, 2, getattr(ops, "MEGA_VAR_" + bits))
    dirty, _ = run(model, 2, "free", True, "tables", poison=0x7fc00000, seed=seed)
    assert dirty["steps"] == clean["steps"]
    for k in KEYS:
        assert torch.equal(dirty[k], clean[k]), k


# ---- 8: every instantiation of the kernel is launched by a test
@pytest.mark.parametrize("model,B,Ti,bits,lj", [
    ("plain, one fed frame", 1, 140, "", True),                                        # dec_mega2_k<1, false, LJ, -, ->
    ("dropout+speakers", 1, 33, "DROPOUT SPEAKER", False),                             # <1, true, -, SPK, OPT>
    ("dropout+speakers", 1, 140, "DROPOUT SPEAKER", False),                            # <1, false, -, SPK, OPT>
    ("dropout+speakers, one fed frame", 1, 33, "DROPOUT SPEAKER", True),               # <1, true, LJ, SPK, OPT>
    ("dropout+speakers, one fed frame", 1, 140, "DROPOUT SPEAKER", True),              # <1, false, LJ, SPK, OPT>
    ("dropout+speakers, one fed frame", 2, 57, "DROPOUT SPEAKER", True)])              # <2, false, LJ, SPK, OPT>
def test_instantiations_no_other_test_launches(model, B, Ti, bits, lj):
    """the instantiations of dec_mega2_k that neither the tests above nor tests/test_inference_gpu.py, test_decode_golden_gpu.py and
    test_decode_speaker_gpu.py launch (profiles/decode_shared_phases_kernel_regs.txt lists the test of each of the 30): 9 / 10 / 19
    steps with 8 steps per launch against the launch-per-layer path, this file's bar"""
    from satt_amd import ops
    mask = 0
    for b in bits.split():
        mask |= getattr(ops, "MEGA_VAR_" + b)
    kw = dict(seed=7) if "DROPOUT" in bits else {}
    against_launch_per_layer(model, B, "free", "tables", mask, Ti=Ti, lj=lj, **kw)
