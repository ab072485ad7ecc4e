"""Multi-speaker synthesis on the persistent decode kernel (csrc/decode_mega2.hip, template flag SPK) against the launch-per-layer
path it replaces for these models (csrc/decode.hip) and against the float64 oracle.

MultiSpeakerPreNet (reference modules/multi_speaker_modules.py:27-32) is the first pre-net layer of a speaker model:
relu((relu(x W0 + b0) + softsign(s Ws + bs)) W2 + b2).  The speaker term is constant over the utterance (DecodeSession.sproj); the
kernel adds it behind the ReLU of pre-net 0 in BOTH of that layer's forms - the unfolded one on the fed frame (first step of every
launch, every teacher-fed step, every step with MEGA_FOLD_FEEDBACK off) and the folded feedback form (every other free-running
step) - and runs the second Dense as one more split product.  The cases are shaped so that a term added in one form only, a term
that is dropped, and a term that reaches the wrong row all show: MEGA_STEPS = 8 (several launches and a ragged last one within 19
steps, both forms), the fold off, one long launch; two DIFFERENT speakers in the two rows, swapped.

EVERY TEST HERE FAILS ON THE PARENT: there a speaker model never takes the kernel (`ses.mega is None`).
Bars: those of tests/test_inference_gpu.py test_persistent_decode_kernel_equals_the_launch_per_layer_path (2e-5 relative to the
largest element: same bf16 weights, same buffers, fp32 sums in another order, fed back through the steps)."""
import numpy as np
import pytest
import torch

from common import make_params, rel_err, small_batch
from decode_common import BAR, Engines, example_config, host_outputs, infer_kwargs, last_session, same, switches, traced_infer

pytestmark = pytest.mark.gpu

KEYS = ("mel", "stop", "alignment1", "alignment2")
SPK = dict(num_speakers=4, speaker_dim=16, speaker_offset=225)
# what the model is built with, per speaker source (test 3); "table" is the model of every other test
SOURCES = {"table": SPK, "resize": dict(SPK, speaker_proj_dim=24), "for_synthesis": dict(SPK, speaker_for_synthesis=227), "embed": SPK}
SHAPES = {1: (33, 9), 2: (57, 19)}            # B -> (Ti, steps)
IDS = {1: (226,), 2: (225, 227)}              # two DIFFERENT speakers in the two rows
FORMS = {"tables": (8, True), "nofold": (8, False), "tables32": (32, True)}          # -> (MEGA_STEPS, MEGA_FOLD_FEEDBACK)

engine = Engines(SOURCES, stats=True)
_runs = {}


def run(B, mode, mega, form="tables", ids=None, source="table", poison=None, fresh=False, **spk_kw):
    """one utterance; returns (outputs on the host, the instantiation of the persistent kernel that was LAUNCHED for it - None if
    none was).  Results are computed once and shared between the tests (fresh=True: computed again)."""
    ids = IDS[B] if ids is None else ids
    key = (B, mode, mega, form, ids, source, poison, tuple(sorted(spk_kw)))
    if key in _runs and not fresh:
        return _runs[key]
    eng, cfg, _, _ = engine(source, stop=(mode == "stop"))
    Ti, steps = SHAPES[B]
    batch = small_batch(cfg, B, Ti, steps * cfg.r, seed=6)
    kw = infer_kwargs(mode, steps, batch["mel"], ids if ("speaker_embed" not in spk_kw and ids != "none") else None)
    kw.update(spk_kw)
    K, fold = FORMS[form]
    out, _, launches = traced_infer(eng, batch["source"], batch["source_length"], dict(MEGA=mega, MEGA_STEPS=K, MEGA_FOLD_FEEDBACK=fold),
                                    poison, **kw)
    launched = {l.variant for l in launches}
    assert len(launched) <= 1
    _runs[key] = (host_outputs(out, KEYS), launched.pop() if launched else None)
    return _runs[key]


def took_the_speaker_kernel(var, B):
    from satt_amd import ops
    assert var is not None, "the speaker model did not take the persistent kernel"          # FAILS ON THE PARENT
    assert var & ops.MEGA_VAR_SPEAKER and bool(var & ops.MEGA_VAR_TWO_SAMPLES) == (B == 2)


# ---- 1: persistent against launch per layer
@pytest.mark.parametrize("form,mode,B", [("tables", m, B) for B in (1, 2) for m in ("free", "teacher", "stop")] +
                         [("nofold", "free", 2), ("tables32", "free", 2)])
def test_speaker_model_on_the_persistent_kernel_equals_the_launch_per_layer_path(form, mode, B):
    new, var = run(B, mode, True, form)
    took_the_speaker_kernel(var, B)
    old, none = run(B, mode, False)
    assert none is None
    assert new["steps"] == (7 if mode == "stop" else SHAPES[B][1])
    same(new, old, "%s %s B=%d" % (form, mode, B), KEYS)


# ---- 2: the term is live, and per row
@pytest.mark.parametrize("form", ["tables", "nofold"])
def test_the_speaker_term_is_live_and_belongs_to_its_row(form):
    """rows (text 0, speaker a), (text 1, speaker b), then the ids swapped ON THE CACHED SESSION (the speaker rows are rewritten in
    place, no pointer changes): the second run equals the launch-per-layer result for the swapped ids, and its row 0 - the same
    text with the other speaker - differs from the first run's row 0 by more than 100 bars.  A row mix-up fails the first, a
    term that is dropped or multiplied by zero the second."""
    a, b = IDS[2]
    first, var = run(2, "free", True, form)
    took_the_speaker_kernel(var, 2)
    swapped, _ = run(2, "free", True, form, ids=(b, a))
    old, _ = run(2, "free", False, ids=(b, a))
    same(swapped, old, form + " swapped ids", KEYS)
    for row in (0, 1):
        d = rel_err(swapped["mel"][row].numpy(), first["mel"][row].numpy())
        print("row %d: other speaker, same text: mel differs by %.3e (must exceed %.0e)" % (row, d, 100 * BAR))
        assert d > 100 * BAR, (row, d)
    again, _ = run(2, "free", True, form, fresh=True)            # ... and back: the first run's bits
    for k in KEYS:
        assert torch.equal(again[k], first[k]), k


# ---- 3: every speaker source reaches the kernel
@pytest.mark.parametrize("source", ["table", "resize", "for_synthesis", "embed"])
def test_every_speaker_source_reaches_the_kernel(source):
    """table lookup, the resize layer (speaker_embedding_projection_out_dim), speaker_for_synthesis without any speaker id, and a
    speaker embedding handed in by the caller: each fills DecodeSession.sproj before the first launch"""
    kw = {}
    ids = None
    if source == "for_synthesis":
        ids = "none"
    if source == "embed":
        kw["speaker_embed"] = torch.randn(1, 16, generator=torch.Generator().manual_seed(3)) * 0.5
    new, var = run(1, "free", True, "tables", ids=ids, source=source, **kw)
    took_the_speaker_kernel(var, 1)
    old, _ = run(1, "free", False, ids=ids, source=source, **kw)
    same(new, old, source, KEYS)
    if source in ("for_synthesis", "embed"):      # not the table row of the default id: the source was used
        other, _ = run(1, "free", True, "tables", source="table")
        assert rel_err(new["mel"].numpy(), other["mel"].numpy()) > 100 * BAR


# ---- 4: production widths
@pytest.mark.parametrize("nff,B,Ti,steps", [(2, 1, 33, 9), (2, 1, 140, 10), (1, 1, 33, 9), (1, 2, 57, 19), (1, 1, 140, 10)])
def test_vctk_example_widths_and_the_specialised_instantiation(nff, B, Ti, steps):
    """nff = 2: examples/vctk/self-attention-tacotron.json itself - 152 speakers from id 225 at the LJSpeech layer sizes, two fed-back
    frames per step (n_feed_frame = 2, feed = 160).  Those dimensions select the GENERIC instantiation (the compile-time
    specialisation is keyed on feed = 80, with and without speakers), here with the speaker flag; B = 1 with LDS-resident context
    tables (Ti <= 112) and with the tables in global memory (B = 2 generic: the tests above).
    nff = 1: the widths the specialisation is keyed on - it stays keyed on the dimensions, so a speaker model gets LJ AND SPK, in its
    three forms (B = 1 with LDS tables, B = 2, B = 1 with global tables)."""
    from satt_amd import ops
    from satt_amd.engine import Engine
    from satt_amd.inference import infer, DecodeSession
    want = example_config("self-attention-tacotron", "vctk")
    kw = dict(num_speakers=152, speaker_dim=16, speaker_offset=225, n_feed_frame=nff)
    cfg, P = make_params(kw, seed=4)
    for f in (("n_feed_frame",) if nff == 2 else ()) + ("num_speakers", "speaker_dim", "speaker_offset", "dec_prenet", "att_rnn_units", "att1_units", "att2_units", "dec_units",
              "dec_sa_units", "dec_sa_heads", "cbhg_out_units", "sa_units", "num_mels", "r", "att_kernel", "att_filters", "mem_speaker"):
        assert getattr(cfg, f) == getattr(want, f), f
    ops.set_precision("bf16")
    eng = Engine(cfg, "cuda", params=P, rng_seed=7)
    batch = small_batch(cfg, B, Ti, steps * cfg.r, seed=6)
    call = lambda: infer(eng, batch["source"], batch["source_length"], max_steps=steps, min_steps=10 ** 6,
                         speaker_id=torch.as_tensor([225 + 151, 225][:B]))
    form = {(1, 33): ops.MEGA_VAR_TABLES_LDS, (2, 57): ops.MEGA_VAR_TWO_SAMPLES, (1, 140): 0}[(B, Ti)]
    with switches(MEGA=True, MEGA_STEPS=8):
        new = call()
        ses = last_session(eng)          # (a new engine: the session is new)
        assert ses.mega is not None          # FAILS ON THE PARENT
        assert ops.dec_mega_variant(ses.mega) == form | (ops.MEGA_VAR_LJ if nff == 1 else 0) | ops.MEGA_VAR_SPEAKER
        DecodeSession.MEGA = False
        old = call()
        assert last_session(eng).mega is None
    same(host_outputs(new, KEYS), host_outputs(old, KEYS), "vctk widths, %d fed frame(s), B=%d Ti=%d" % (nff, B, Ti), KEYS)


# ---- 5: float64 oracle
def test_persistent_path_is_as_close_to_the_float64_oracle_as_the_launch_per_layer_path():
    """B = 2, 19 teacher-fed steps, two speakers.  Both paths multiply with the same bf16 weights, so their distance from the
    float64 oracle (fp32 parameters) is the rounding of the weights; the launch-per-layer path's distance, measured in the same
    run, is the yardstick (the behaviour before this kernel took speaker models), and the persistent path may be at most twice as
    far - fp32 sums in another order move it a little, a wrong speaker term moves it by orders of magnitude.
    Measured (MI355X): see profiles/decode_speaker_bench_and_kernel_times.txt."""
    from oracle import torch_ref
    eng, cfg, P, mv = engine("table")
    Ti, steps = SHAPES[2]
    batch = small_batch(cfg, 2, Ti, steps * cfg.r, seed=6)
    bt = torch_ref.batch_to_torch(batch)
    ref = torch_ref.infer(torch_ref.to_torch(P), bt["source"], bt["source_length"], torch_ref.Cfg(**SPK), None, mv,
                          speaker_id=torch.as_tensor(np.array(IDS[2], np.int64)), teacher=bt["mel"])
    new, var = run(2, "teacher", True, "tables")
    took_the_speaker_kernel(var, 2)
    old, _ = run(2, "teacher", False)
    assert ref["steps"] == new["steps"] == old["steps"] == steps
    bad = {}
    for k in KEYS:
        dn, do = rel_err(new[k].numpy(), ref[k].numpy()), rel_err(old[k].numpy(), ref[k].numpy())
        print("oracle distance %-10s persistent %.3e launch-per-layer %.3e ratio %.3f" % (k, dn, do, dn / do))
        if not dn <= 2 * do:
            bad[k] = (dn, do)
    assert not bad, bad


# ---- 6: LDS poison
def test_speaker_kernel_does_not_depend_on_what_the_lds_held_before_the_launch():
    """quiet NaN in every LDS word of every CU in front of every launch of the kernel (satt_debug_poison_lds, in process): the bits of
    the clean run.  The speaker term and the second Dense's bias live in registers, the second Dense reads the vector the first
    one's gather wrote and rows past P0 that the start-of-launch zeroing covers."""
    clean, var = run(2, "free", True, "tables")
    took_the_speaker_kernel(var, 2)
    dirty, _ = run(2, "free", True, "tables", poison=0x7fc00000)
    assert dirty["steps"] == clean["steps"]
    for k in KEYS:
        assert torch.equal(dirty[k], clean[k]), k
