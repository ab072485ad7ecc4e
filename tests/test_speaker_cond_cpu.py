"""CPU tests of speaker_embedding_projection_out_dim (the resize layer behind the speaker embedding, reference
models/models.py:307-312) and speaker_for_synthesis (:333-339): configuration, parameter layout, validation, the example file, the
C-ABI declarations and the float64 helper the GPU tests rest on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import satt_amd  # noqa: F401
from satt_amd.hparams import hparams
from satt_amd.models.models import validate_params
from satt_amd.params import ModelConfig, init_params, layout, param_shapes
from oracle import torch_ref

import speaker_common as sc
from common import MEDIUM, make_params, small_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLES = [("ljspeech", "self-attention-tacotron.json"), ("ljspeech", "tacotron.json"), ("ljspeech", "self-attention-tacotron-accent.json"),
            ("vctk", "self-attention-tacotron.json"), ("vctk", "tacotron.json")]


def hp_from(corpus, name, **kw):
    hp = hparams.copy()
    hp.parse_json(open(os.path.join(ROOT, "examples", corpus, name)).read())
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


def test_resize_layer_layout():
    """FAILS ON THE PARENT (which ignores the key): the two parameters sit right behind speaker_embedding, in the decoder range of
    the flat buffer, and the pre-net's speaker projection reads the resized width"""
    c = ModelConfig.from_hparams(hp_from("vctk", "self-attention-tacotron.json", speaker_embedding_projection_out_dim=64))
    assert c.speaker_proj_dim == 64 and c.speaker_resize and c.speaker_feat == 64 and c.speaker_for_synthesis == -1
    shapes = param_shapes(c)
    names = [n for n, _ in shapes]
    i = names.index("speaker_embedding")
    assert shapes[i:i + 3] == [("speaker_embedding", (152, 16)), ("speaker_resize.W", (16, 64)), ("speaker_resize.b", (64,))]
    assert dict(shapes)["dec.prenet0.Ws"] == (64, 256) and dict(shapes)["dec.prenet0.bs"] == (256,)
    lay, _ = layout(c)
    assert lay["speaker_embedding"][0] < lay["speaker_resize.W"][0] < lay["speaker_resize.b"][0] < lay["dec.prenet0.W"][0]
    assert lay["speaker_resize.W"][0] > lay["enc.sa.t.b"][0]          # decoder bucket: Engine.enc_end = offset of speaker_embedding
    # a Dense layer like the others: glorot-uniform kernel, zero bias
    P = init_params(c, 0)
    lim = np.sqrt(6.0 / (16 + 64))
    assert float(np.abs(P["speaker_resize.W"]).max()) <= lim and float(np.abs(P["speaker_resize.W"]).max()) > 0.8 * lim
    assert not P["speaker_resize.b"].any()
    assert c.l2_weight == 0.0       # L2 regularisation applies to the baseline model only, which never has the layer


def _parent_param_shapes(c):
    """the oracle's list (oracle/torch_ref.py param_shapes, untouched by this feature) is the parent's layout for every
    configuration it covers"""
    kw = {k: getattr(c, k) for k in vars(torch_ref.Cfg()) if hasattr(c, k)}
    return torch_ref.param_shapes(torch_ref.Cfg(**kw))


@pytest.mark.parametrize("corpus,name", EXAMPLES)
def test_layouts_unchanged_with_both_keys_off(corpus, name):
    """-1 / -1: names, shapes, offsets, total size and the initial values of the five shipped configurations are what they were"""
    c = ModelConfig.from_hparams(hp_from(corpus, name))
    assert c.speaker_proj_dim == -1 and c.speaker_for_synthesis == -1 and not c.speaker_resize and c.speaker_feat == c.speaker_dim
    shapes = param_shapes(c)
    assert not any("speaker_resize" in n for n, _ in shapes)
    parent = _parent_param_shapes(c)
    if c.accent:        # the oracle has no accent branch: its list lacks the accent tensors and feeds the bank the phoneme width only
        shapes_cmp = [(n, s) for n, s in shapes if "accent" not in n and not re.match(r"enc\.bank\d+\.W", n)]
        parent = [(n, s) for n, s in parent if not re.match(r"enc\.bank\d+\.W", n)]
    else:
        shapes_cmp = shapes
    assert shapes_cmp == parent
    lay, total = layout(c)
    off = 0
    for n, shp in shapes:           # the packing rule of params.layout, restated
        assert lay[n] == (off, shp)
        off += (int(np.prod(shp)) + 7) // 8 * 8
    assert total == off
    if c.num_speakers > 0 and not c.accent:        # same draws in the same order as the oracle's initialiser
        assert dict(shapes)["dec.prenet0.Ws"] == (c.speaker_dim, c.dec_prenet[0])


def test_validation_errors_name_the_number():
    vctk = lambda **kw: hp_from("vctk", "self-attention-tacotron.json", **kw)
    lj = lambda **kw: hp_from("ljspeech", "self-attention-tacotron.json", **kw)
    with pytest.raises(ValueError, match=r"speaker_embedding_projection_out_dim=64 needs use_speaker_embedding"):
        validate_params(lj(speaker_embedding_projection_out_dim=64))
    with pytest.raises(ValueError, match=r"speaker_for_synthesis=230 needs use_speaker_embedding"):
        validate_params(lj(speaker_for_synthesis=230))
    with pytest.raises(ValueError, match=r"speaker_embedding_projection_out_dim=0"):
        validate_params(vctk(speaker_embedding_projection_out_dim=0))
    for bad in (224, 377, 0, 5000):         # the table is [225, 225 + 152)
        with pytest.raises(ValueError, match=r"speaker_for_synthesis=%d is outside the speaker table \[225, 377\)" % bad):
            validate_params(vctk(speaker_for_synthesis=bad))
    for ok in (225, 376):
        validate_params(vctk(speaker_for_synthesis=ok))
        assert ModelConfig.from_hparams(vctk(speaker_for_synthesis=ok)).speaker_for_synthesis == ok


def test_baseline_model_ignores_both_keys():
    """ExtendedTacotronV1Model never reads either hparam (reference models/models.py:39-52)"""
    for corpus in ("vctk", "ljspeech"):
        plain = ModelConfig.from_hparams(hp_from(corpus, "tacotron.json"))
        c = ModelConfig.from_hparams(hp_from(corpus, "tacotron.json", speaker_embedding_projection_out_dim=64, speaker_for_synthesis=3))
        assert c.speaker_proj_dim == -1 and c.speaker_for_synthesis == -1
        assert param_shapes(c) == param_shapes(plain)


def test_resize_example_resolves():
    import json
    a = json.load(open(os.path.join(ROOT, "examples", "vctk", "self-attention-tacotron-resize.json")))
    b = json.load(open(os.path.join(ROOT, "examples", "vctk", "self-attention-tacotron.json")))
    assert a == dict(b, speaker_embedding_projection_out_dim=64)
    hp = hp_from("vctk", "self-attention-tacotron-resize.json")
    validate_params(hp)
    c = ModelConfig.from_hparams(hp)
    assert (c.num_speakers, c.speaker_dim, c.speaker_offset, c.speaker_proj_dim) == (152, 16, 225, 64)


def test_header_signatures_and_caps():
    """the two entry points are declared, bound with matching arity, exported, and the shape predicate (host code) states the cap"""
    from satt_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "satt_hip.h")).read(), flags=re.S)
    for name in ("satt_speaker_cond_supported", "satt_speaker_cond_fwd"):
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
    sup = lib.satt_speaker_cond_supported
    assert sup(32, 16, 64, 256) == 1 and sup(1, 16, 64, 256) == 1 and sup(5, 7, 13, 37) == 1      # VCTK sizes, B = 1, odd sizes
    assert sup(257, 16, 64, 256) == 0 and sup(32, 257, 64, 256) == 0 and sup(32, 16, 257, 256) == 0 and sup(32, 16, 64, 513) == 0
    assert sup(0, 16, 64, 256) == 0
    assert sup(256, 256, 256, 512) == 0         # inside every size cap, beyond the 64 KB LDS footprint: composed from generic ops


def test_float64_helper_matches_the_oracle_without_the_new_fields():
    """speaker_common.composed_forward with both fields off IS torch_ref.forward (bit for bit); with speaker_for_synthesis it equals
    the oracle run on a batch whose ids were all replaced; with the resize layer the decoder reads the resized vector"""
    kw = dict(MEDIUM, num_speakers=7, speaker_dim=16, speaker_offset=225)
    cfg, P = make_params(kw, seed=4)
    batch = small_batch(cfg, 3, 11, 12, seed=8)
    batch["speaker_id"] = np.array([226, 231, 226], np.int64)
    Pt = torch_ref.to_torch(P, torch.float64)
    bt = torch_ref.batch_to_torch(batch)
    ref = torch_ref.forward(Pt, bt, torch_ref.Cfg(**kw), True, 5)
    out = sc.composed_forward(Pt, bt, kw, True, 5)
    assert torch.equal(out["mel"], ref["mel"]) and torch.equal(out["loss"], ref["loss"])
    out2 = sc.composed_forward(Pt, bt, dict(kw, speaker_for_synthesis=229), True, 5)
    ref2 = torch_ref.forward(Pt, dict(bt, speaker_id=torch.full((3,), 229)), torch_ref.Cfg(**kw), True, 5)
    assert torch.equal(out2["mel"], ref2["mel"]) and not torch.equal(out2["mel"], ref["mel"])
    kw3 = dict(kw, speaker_proj_dim=24)
    cfg3, P3 = make_params(kw3, seed=4)
    assert P3["speaker_resize.W"].shape == (16, 24) and P3["dec.prenet0.Ws"].shape == (24, cfg3.dec_prenet[0])
    ref3, col, g = sc.composed_run(kw3, P3, batch, True, 5)
    for k in ("speaker_embedding", "speaker_resize.W", "speaker_resize.b", "dec.prenet0.Ws"):
        assert float(np.abs(g[k]).max()) > 0, k
    assert not g["speaker_embedding"][[0, 2, 3, 4, 5]].any()          # only the rows of ids 226 and 231 receive gradient


def test_tf_warm_start_leaves_the_resize_layer_to_the_variable_map():
    """the resize layer is an anonymous tf.layers.Dense of the model function: even where its shape is unique in a checkpoint it is
    not paired automatically - `tools/tf_checkpoint.py suggest` lists both tensors as needing a map entry"""
    from satt_amd.models.warm_start import MAP_ONLY, ShapeEngine, resolve_default_map

    class Reader:
        entries = {"model/dense/kernel": {"shape": [16, 64]}, "model/dense/bias": {"shape": [64]}}
    c = ModelConfig.from_hparams(hp_from("vctk", "self-attention-tacotron-resize.json"))
    vmap, unresolved = resolve_default_map(ShapeEngine(c), Reader())
    open_names = {t.get("param") for t in unresolved}
    assert set(MAP_ONLY) == {"speaker_resize.W", "speaker_resize.b"} <= open_names
    assert not any(t.get("param") in MAP_ONLY for t in vmap.values())
