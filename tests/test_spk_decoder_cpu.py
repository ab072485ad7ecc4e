"""CPU tests of speaker_embedd_to_decoder (reference models/models.py:366-372: the speaker vector concatenated to both attention
memories): configuration, parameter layout, validation, the example file, the C-ABI declarations of the two new kernels and the
float64 composition the GPU tests rest on."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import satt_amd  # noqa: F401
from satt_amd.hparams import hparams
from satt_amd.models.models import validate_params
from satt_amd.modules.attentions import UnsupportedConfiguration
from satt_amd.params import ModelConfig, init_params, layout, param_shapes
from oracle import torch_ref

import spk_decoder_common as sd
from common import MEDIUM, make_params, small_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the four shipped configurations + the resize example
EXAMPLES = [("ljspeech", "self-attention-tacotron.json"), ("ljspeech", "tacotron.json"), ("vctk", "self-attention-tacotron.json"),
            ("vctk", "tacotron.json"), ("vctk", "self-attention-tacotron-resize.json")]


def hp_from(corpus, name, **kw):
    hp = hparams.copy()
    hp.parse_json(open(os.path.join(ROOT, "examples", corpus, name)).read())
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


def _parent_param_shapes(c):
    """the oracle's list (oracle/torch_ref.py param_shapes, untouched by this feature) is the parent's layout"""
    kw = {k: getattr(c, k) for k in vars(torch_ref.Cfg()) if hasattr(c, k)}
    return torch_ref.param_shapes(torch_ref.Cfg(**kw))


@pytest.mark.parametrize("corpus,name", EXAMPLES)
def test_layouts_unchanged_with_the_flag_off(corpus, name):
    """flag off: names, shapes, offsets and the total size of the shipped configurations are what they were"""
    c = ModelConfig.from_hparams(hp_from(corpus, name))
    assert c.speaker_to_decoder is False and c.mem_speaker == 0
    shapes = param_shapes(c)
    parent = _parent_param_shapes(c)
    if c.speaker_resize:        # the oracle has no resize layer: its list lacks the two tensors and sizes Ws by the embedding
        shapes_cmp = [(n, s) for n, s in shapes if "speaker_resize" not in n and n != "dec.prenet0.Ws"]
        parent = [(n, s) for n, s in parent if n != "dec.prenet0.Ws"]
    else:
        shapes_cmp = shapes
    assert shapes_cmp == parent
    lay, total = layout(c)
    off = 0
    for n, shp in shapes:           # the packing rule of params.layout, restated
        assert lay[n] == (off, shp)
        off += (int(np.prod(shp)) + 7) // 8 * 8
    assert total == off
    d = dict(shapes)
    A, D, pn = c.att_rnn_units, c.dec_units, c.dec_prenet[-1]
    assert d["dec.att_lstm.W"] == (pn + c.cbhg_out_units + c.sa_units + A, 4 * A)
    assert d["dec.lstm1.W"] == (A + c.cbhg_out_units + c.sa_units + D, 4 * D)
    assert d["dec.att1.Wm"] == (c.cbhg_out_units, c.att1_units)


@pytest.mark.parametrize("rdim,S", [(-1, 16), (24, 24)])
def test_wide_shapes_with_the_flag_on(rdim, S):
    """FAILS ON THE PARENT (which refuses the key).  The four tensors sized by a memory width grow by S per source - S = the
    embedding's width, or the resize layer's - and nothing else moves: same names, same order, every other shape as with the flag off"""
    kw = dict(speaker_embedd_to_decoder=True, speaker_embedding_projection_out_dim=rdim)
    c = ModelConfig.from_hparams(hp_from("vctk", "self-attention-tacotron.json", **kw))
    off = ModelConfig.from_hparams(hp_from("vctk", "self-attention-tacotron.json", speaker_embedding_projection_out_dim=rdim))
    assert c.speaker_to_decoder is True and c.mem_speaker == S == c.speaker_feat
    d, d0 = dict(param_shapes(c)), dict(param_shapes(off))
    V1, V2, A, D, pn = 256, 32, 256, 256, 128
    assert d["dec.att1.Wm"] == (V1 + S, 224) and d["dec.att2.Wm"] == (V2 + S, 32)
    assert d["dec.att_lstm.W"] == (pn + V1 + S + V2 + S + A, 4 * A)
    assert d["dec.lstm1.W"] == (A + V1 + S + V2 + S + D, 4 * D)
    wide = ("dec.att1.Wm", "dec.att2.Wm", "dec.att_lstm.W", "dec.lstm1.W")
    assert [n for n, _ in param_shapes(c)] == [n for n, _ in param_shapes(off)]
    assert {n: s for n, s in d.items() if n not in wide} == {n: s for n, s in d0.items() if n not in wide}
    P = init_params(c, 0)
    assert all(P[n].shape == d[n] for n in wide)
    lay, total = layout(c)
    assert total > layout(off)[1] and all(o % 8 == 0 for o, _ in lay.values())


def test_example_resolves():
    a = json.load(open(os.path.join(ROOT, "examples", "vctk", "self-attention-tacotron-spk-decoder.json")))
    b = json.load(open(os.path.join(ROOT, "examples", "vctk", "self-attention-tacotron.json")))
    assert a == dict(b, speaker_embedd_to_decoder=True)
    hp = hp_from("vctk", "self-attention-tacotron-spk-decoder.json")
    validate_params(hp)
    c = ModelConfig.from_hparams(hp)
    assert (c.num_speakers, c.speaker_dim, c.speaker_offset, c.speaker_to_decoder, c.mem_speaker) == (152, 16, 225, True, 16)


def test_validation_outcomes():
    vctk = lambda **kw: hp_from("vctk", "self-attention-tacotron.json", **kw)
    lj = lambda **kw: hp_from("ljspeech", "self-attention-tacotron.json", **kw)
    validate_params(vctk(speaker_embedd_to_decoder=True))
    with pytest.raises(ValueError, match=r"speaker_embedd_to_decoder=True needs use_speaker_embedding"):
        validate_params(lj(speaker_embedd_to_decoder=True))
    with pytest.raises(UnsupportedConfiguration, match=r"speaker_embedd_to_decoder=True with use_forward_attention_transition_agent"):
        validate_params(vctk(speaker_embedd_to_decoder=True, use_forward_attention_transition_agent=True))
    validate_params(vctk(use_forward_attention_transition_agent=True))          # either one alone is built
    # the other speaker switches the reference tree cannot specify stay refused
    for flag in ("speaker_embedd_to_postnet", "channel_id_to_postnet", "use_external_speaker_embedding", "use_language_embedding"):
        with pytest.raises(UnsupportedConfiguration):
            validate_params(vctk(**{flag: True}))
    with pytest.raises(ValueError):
        ModelConfig(speaker_to_decoder=True)                 # no speaker embedding
    with pytest.raises(UnsupportedConfiguration):
        ModelConfig(num_speakers=4, speaker_to_decoder=True, transition_agent=True)


def test_baseline_model_ignores_the_key():
    """ExtendedTacotronV1Model's model_fn never reads speaker_embedd_to_decoder (reference models/models.py:20-226)"""
    for corpus in ("vctk", "ljspeech"):
        plain = ModelConfig.from_hparams(hp_from(corpus, "tacotron.json"))
        c = ModelConfig.from_hparams(hp_from(corpus, "tacotron.json", speaker_embedd_to_decoder=True))
        assert c.speaker_to_decoder is False and param_shapes(c) == param_shapes(plain)


def test_composed_reference_reduces_to_the_oracle():
    """s = 0 (a zero speaker table, no pre-net bias contribution changes: the table feeds the pre-net too, in both runs) and the
    speaker rows are then multiplied by zeros: the composed reference on the wide parameters reproduces torch_ref.forward on the
    narrow ones, which are the wide ones without their speaker rows"""
    kw = dict(MEDIUM, num_speakers=7, speaker_dim=16, speaker_offset=225)
    cfgw, Pw = make_params(dict(kw, speaker_to_decoder=True), seed=4)
    Pw["speaker_embedding"][:] = 0.0
    c = cfgw
    V1, V2, S, A, pn = c.cbhg_out_units, c.sa_units, 16, c.att_rnn_units, c.dec_prenet[-1]
    cut = lambda W, lead: np.concatenate([W[:lead + V1], W[lead + V1 + S:lead + V1 + S + V2], W[lead + V1 + V2 + 2 * S:]])
    Pn = dict(Pw)
    Pn["dec.att_lstm.W"], Pn["dec.lstm1.W"] = cut(Pw["dec.att_lstm.W"], pn), cut(Pw["dec.lstm1.W"], A)
    Pn["dec.att1.Wm"], Pn["dec.att2.Wm"] = Pw["dec.att1.Wm"][:V1], Pw["dec.att2.Wm"][:V2]
    batch = small_batch(c, 3, 11, 12, seed=8)
    batch["speaker_id"] = np.array([226, 231, 226], np.int64)
    bt = torch_ref.batch_to_torch(batch)
    ref = torch_ref.forward(torch_ref.to_torch(Pn, torch.float64), bt, torch_ref.Cfg(**kw), True, 5)
    out = sd.composed_forward(torch_ref.to_torch(Pw, torch.float64), bt, dict(kw, speaker_to_decoder=True), True, 5)
    for k in ("mel", "stop", "alignment1", "alignment2", "loss"):
        assert float((out[k] - ref[k]).abs().max()) < 1e-12, k
    # ... and with a speaker table the speaker rows matter, and every one of the wide tensors' speaker rows gets a gradient
    cfg2, P2 = make_params(dict(kw, speaker_to_decoder=True), seed=4)
    o2, _, g = sd.composed_run(dict(kw, speaker_to_decoder=True), P2, batch, True, 5)
    assert float((o2["mel"].detach() - ref["mel"]).abs().max()) > 1e-4
    assert np.abs(g["dec.att1.Wm"][V1:]).max() > 0 and np.abs(g["dec.att2.Wm"][V2:]).max() > 0
    for n, lead in (("dec.att_lstm.W", pn), ("dec.lstm1.W", A)):
        assert np.abs(g[n][lead + V1:lead + V1 + S]).max() > 0 and np.abs(g[n][lead + V1 + S + V2:lead + V1 + V2 + 2 * S]).max() > 0


def test_header_signatures_and_exports():
    """the two new entry points are declared, bound with matching arity and types, and exported by the built library"""
    from satt_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "satt_hip.h")).read(), flags=re.S)
    for name in ("satt_rows_bcast_add", "satt_rows_time_sum"):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(argtypes) == len(args), (name, len(argtypes), len(args))
        for a, t in zip(args, argtypes):        # pointer <-> c_void_p, int64_t <-> c_int64, int <-> c_int
            want = ctypes.c_void_p if "*" in a else (ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_int)
            assert t is want, (name, a, t)
    import __graft_entry__ as ge
    lib = ctypes.CDLL(ge.build())
    for name in ("satt_rows_bcast_add", "satt_rows_time_sum"):
        assert hasattr(lib, name), name
    # argument checks are host code: a bad leading dimension or range is refused before anything is launched
    lib.satt_rows_bcast_add.argtypes = _lib.SIGNATURES["satt_rows_bcast_add"][1]
    lib.satt_rows_time_sum.argtypes = _lib.SIGNATURES["satt_rows_time_sum"][1]
    assert lib.satt_rows_bcast_add(None, 8, None, 8, 1, 1, 8, 0, 1, None) == -1
    assert lib.satt_rows_bcast_add(16, 4, 16, 8, 1, 1, 8, 0, 1, None) == -1          # ld < N
    assert lib.satt_rows_bcast_add(16, 8, 16, 8, 1, 2, 8, 0, 3, None) == -1          # t1 > T
    assert lib.satt_rows_time_sum(16, 4, None, 16, 8, 1, 1, 8, 0, None) == -1        # ld < N
