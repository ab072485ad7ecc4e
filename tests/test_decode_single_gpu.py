"""The baseline model (ExtendedTacotronV1Model: one attention source, no decoder self-attention) on the single-source form of the
persistent decode kernel (csrc/decode_mega2.hip dec_mega2_single_k) against the hipGraph of launch-per-layer steps it ran on before
(csrc/decode.hip): same engine, same bf16 weight shadows, same buffers - fp32 sums in a different order and nothing else.

EVERY TEST HERE FAILS ON THE PARENT: there the baseline model never takes the kernel (`ses.mega is None`).
Bar: 2e-5 relative to the largest element, the bar test_persistent_decode_kernel_equals_the_launch_per_layer_path (tests/
test_inference_gpu.py) sets for exactly this comparison of the dual form.  Production widths (A = D = 256), short memories, few
steps; MEGA_STEPS = 8 gives several launches, a ragged last one, and an unfolded step every eighth."""
import numpy as np
import pytest
import torch

from common import rel_err, small_batch
from decode_common import BAR, BASELINE, Engines, example_config, expected_variant, infer_kwargs, last_session, switches, traced_infer

pytestmark = pytest.mark.gpu

KEYS = ("mel", "stop", "alignment1")
SPK = dict(num_speakers=7, speaker_dim=16, speaker_offset=225)
MODELS = {
    "plain": BASELINE,
    "location_sensitive": dict(BASELINE, attention="location_sensitive"),
    "cumulative": dict(BASELINE, cumulative_weights=True),
    "narrow attention": dict(BASELINE, att1_units=12),          # U1 % 8 == 4: the query layer's row stride is no multiple of 16 bytes
    "speakers": dict(BASELINE, **SPK),
    "speakers, two fed frames": dict(BASELINE, n_feed_frame=2, **SPK),
    "speakers, one fed frame": dict(BASELINE, n_feed_frame=1, **SPK),
    "agent": dict(BASELINE, transition_agent=True),
    "dropout": dict(BASELINE, apply_dropout_on_inference=True),
}
IDS = {1: (226,), 2: (225, 230)}                            # two DIFFERENT speakers in the two rows

engine = Engines(MODELS)


def run(eng, cfg, B, Ti, steps, mode, mega, mega_steps=8, fold=True, poison=None):
    """one utterance; returns (outputs, session, the variants of the persistent kernel that were launched)"""
    assert not cfg.dual and cfg.dec_sa_units == 0
    batch = small_batch(cfg, B, Ti, steps * cfg.r, seed=6)
    kw = infer_kwargs(mode, steps, batch["mel"], IDS[B] if cfg.num_speakers else None)
    out, ses, launches = traced_infer(eng, batch["source"], batch["source_length"],
                                      dict(MEGA=mega, MEGA_STEPS=mega_steps, MEGA_FOLD_FEEDBACK=fold), poison, **kw)
    return out, ses, {l.variant for l in launches}


def took_single(ses, launched, B, Ti, speaker=False):
    """the session holds the kernel's block and the instantiation that was launched is the single form's for the shape"""
    from satt_amd import ops
    assert ses.mega is not None and ses.mega_opt is None and ses.kernel_launches == 1
    want = expected_variant(ses.eng.cfg, B, Ti)
    assert want & ops.MEGA_VAR_SINGLE and bool(want & ops.MEGA_VAR_SPEAKER) == speaker
    assert ops.dec_mega_variant(ses.mega) == want
    assert launched == {want}, launched


def compare(eng, cfg, B, Ti, steps, mode="free", mega_steps=8, fold=True, want_steps=None, speaker=False):
    new, ses, launched = run(eng, cfg, B, Ti, steps, mode, True, mega_steps, fold)
    took_single(ses, launched, B, Ti, speaker)
    assert (ses._fb is not None) == (fold and mode != "teacher")
    again, ses2, _ = run(eng, cfg, B, Ti, steps, mode, True, mega_steps, fold)          # the cached session, reset
    assert ses2 is ses
    old, ses_old, none = run(eng, cfg, B, Ti, steps, mode, False, mega_steps, fold)
    assert ses_old.mega is None and not none
    assert new["steps"] == old["steps"] == again["steps"] == (steps if want_steps is None else want_steps)
    assert new["alignment2"] is None and new["sa_out"] is None
    for k in KEYS:
        e = rel_err(new[k].cpu().numpy(), old[k].cpu().numpy())
        print(mode, k, e)
        assert e < BAR, (k, e)
        assert torch.equal(new[k], again[k]), k
    assert torch.isfinite(new["mel"]).all()
    return new


# ---- 1: the persistent kernel equals the launch-per-layer path
@pytest.mark.parametrize("form,mode,B,Ti,steps",
                         [("fold", "free", 1, 100, 40), ("nofold", "free", 1, 100, 40), ("fold", "stop", 2, 57, 19),
                          ("fold", "teacher", 1, 140, 33),          # tables in global memory
                          ("fold", "free", 1, 256, 12),             # the longest memory
                          ("fold", "free", 2, 7, 12),               # a memory shorter than the workgroup count
                          ("fold32", "free", 1, 100, 40)])
def test_single_source_kernel_equals_the_launch_per_layer_path(form, mode, B, Ti, steps):
    eng, cfg = engine("plain", stop=(mode == "stop"))
    compare(eng, cfg, B, Ti, steps, mode, mega_steps=32 if form == "fold32" else 8, fold=form != "nofold",
            want_steps=7 if mode == "stop" else None)


@pytest.mark.parametrize("model", ["location_sensitive", "cumulative"])
def test_single_source_kernel_attention_variants(model):
    eng, cfg = engine(model)
    assert (cfg.attention == "location_sensitive") == (model == "location_sensitive") and cfg.cumulative_weights == (model == "cumulative")
    compare(eng, cfg, 1, 57, 12)


def test_single_source_kernel_with_an_attention_width_that_is_no_multiple_of_eight():
    eng, cfg = engine("narrow attention")
    assert cfg.att1_units == 12
    compare(eng, cfg, 2, 57, 12)


@pytest.mark.parametrize("model,B,Ti", [("speakers", 1, 33), ("speakers", 2, 57), ("speakers, two fed frames", 2, 57),
                                        ("speakers, one fed frame", 1, 33),
                                        ("speakers", 1, 140)])          # (tables in global memory with the speaker term)
def test_single_source_kernel_with_the_multi_speaker_prenet(model, B, Ti):
    eng, cfg = engine(model)
    new = compare(eng, cfg, B, Ti, 12, speaker=True)
    if B == 2:          # the two rows carry different speakers: the speaker term reaches its own row
        assert float((new["mel"][0] - new["mel"][1]).abs().max()) > 1e-3


# ---- 2: hand-over
@pytest.mark.parametrize("B,Ti", [(1, 100), (2, 57)])
def test_single_source_kernel_hands_over_to_the_launch_per_layer_path_and_back(B, Ti):
    """8 steps persistent, 8 steps launch per layer (run_step), 8 steps persistent == 24 steps persistent: recurrent state, context
    (V1 columns, written at the last step of a launch only), location-conv input, forward variable, step counters and histories
    cross the boundary in both directions"""
    eng, cfg = engine("plain")
    K, steps = 8, 24
    ref, ses, launched = run(eng, cfg, B, Ti, steps, "free", True, K)
    took_single(ses, launched, B, Ti)
    assert ses.K == K
    ses.reset()                      # (memories, context tables and folded weights of the utterance stay in place)
    ses.replay()
    for _ in range(K):
        ses.run_step()
    ses.replay()
    torch.cuda.synchronize()
    ses.check()
    NO = ses.yout.shape[-1]
    for name, a, b in (("frames", ses.yout[:, 1:steps + 1].reshape(B * steps, NO), ref["yout"]), ("alignment1", ses.al1[:, :steps], ref["alignment1"])):
        e = rel_err(a.cpu().numpy(), b.cpu().numpy())
        print(name, e)
        assert e < BAR, (name, e)


# ---- 3: the shipped examples
@pytest.mark.parametrize("example", ["ljspeech", "vctk"])
def test_the_shipped_baseline_examples_take_the_kernel(example):
    from satt_amd import ops
    from satt_amd.engine import Engine
    from satt_amd.inference import infer, DecodeSession
    cfg = example_config(example)
    ops.set_precision("bf16")
    eng = Engine(cfg, "cuda", param_seed=3, rng_seed=7)
    B, Ti, steps = 1, 33, 9
    g = np.random.default_rng(5)
    batch = dict(source=g.integers(1, cfg.num_symbols, (B, Ti)).astype(np.int64), source_length=np.full((B,), Ti, np.int64))
    kw = dict(max_steps=steps, min_steps=10 ** 6)
    if cfg.num_speakers:
        kw["speaker_id"] = torch.as_tensor(np.array([cfg.speaker_offset + 3], np.int64))
    with switches(MEGA=True):
        new = infer(eng, batch["source"], batch["source_length"], **kw)
        ses = last_session(eng)          # (a new engine: the session is new)
        assert ses.mega is not None
        want = ops.MEGA_VAR_TABLES_LDS | ops.MEGA_VAR_SINGLE | (ops.MEGA_VAR_SPEAKER if example == "vctk" else 0)
        assert ops.dec_mega_variant(ses.mega) == want
        DecodeSession.MEGA = False
        old = infer(eng, batch["source"], batch["source_length"], **kw)
        assert last_session(eng).mega is None
    assert new["steps"] == old["steps"] == steps
    for k in KEYS:
        e = rel_err(new[k].cpu().numpy(), old[k].cpu().numpy())
        print(example, k, e)
        assert e < BAR, (k, e)


# ---- 4: LDS contents
@pytest.mark.parametrize("B,Ti", [(1, 33), (2, 57)])
def test_single_source_kernel_does_not_depend_on_what_the_lds_held_before_the_launch(B, Ti):
    """quiet NaN in every LDS word of every CU in front of every launch (satt_debug_poison_lds): the bits of the clean run - the
    start-of-launch zeroing covers the single form's own layout"""
    eng, cfg = engine("plain")
    clean, ses, launched = run(eng, cfg, B, Ti, 12, "free", True)
    took_single(ses, launched, B, Ti)
    dirty, _, _ = run(eng, cfg, B, Ti, 12, "free", True, poison=0x7fc00000)
    assert dirty["steps"] == clean["steps"]
    for k in KEYS:
        assert torch.equal(dirty[k], clean[k]), k
    assert torch.isfinite(clean["mel"]).all()


# ---- 5: what still falls back
@pytest.mark.parametrize("model", ["agent", "dropout"])
def test_baseline_with_options_stays_on_the_launch_per_layer_path(model):
    from satt_amd import ops
    eng, cfg = engine(model)
    out, ses, launched = run(eng, cfg, 1, 33, 9, "free", True)
    assert ses.mega is None and ses.graph is not None and not launched
    assert out["steps"] == 9 and torch.isfinite(out["mel"]).all()
    # and the plain baseline of the same shape does take the kernel
    eng0, cfg0 = engine("plain")
    _, ses0, launched0 = run(eng0, cfg0, 1, 33, 9, "free", True)
    took_single(ses0, launched0, 1, 33)
    assert ops.dec_mega_variant(ses0.mega) & ops.MEGA_VAR_SINGLE
