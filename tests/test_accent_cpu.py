"""CPU tests of the accent-type input (SelfAttentionCBHGEncoderWithAccentType, reference modules/module.py:444-527): the
factory / validation surface, the parameter layout, the example configuration, the stream ids, and the substitution trick the
GPU tests' float64 reference rests on."""
import json
import os

import numpy as np
import pytest
import torch

import satt_amd  # noqa: F401
from satt_amd.hparams import hparams
from satt_amd.models.models import encoder_factory, validate_params
from satt_amd.modules.attentions import UnsupportedConfiguration
from satt_amd.params import ModelConfig, layout, param_shapes
from oracle import torch_ref

import accent_common as ac
from common import SMALL, make_params, small_batch

ROOT = ac.ROOT


def hp_from(name, corpus="ljspeech"):
    hp = hparams.copy()
    hp.parse_json(open(os.path.join(ROOT, "examples", corpus, name)).read())
    return hp


def accent_hp(**kw):
    hp = hp_from("self-attention-tacotron-accent.json")
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


def test_accent_example_resolves():
    hp = accent_hp()
    enc, dec, a1, a2 = validate_params(hp)
    assert enc.name == "SelfAttentionCBHGEncoderWithAccentType" and enc.prenet_out_units == (256, 112)
    c = ModelConfig.from_hparams(hp)
    assert (c.num_accent_type, c.accent_dim, c.accent_offset, c.accent_prenet) == (129, 32, 0x3100, (32, 16))
    assert c.enc_prenet == (256, 112) and c.prenet_width == 128 == c.cbhg_out_units // 2 == c.proj2
    shapes = dict(param_shapes(c))
    assert shapes["accent_embedding"] == (129, 32)
    assert shapes["enc.accent_prenet0.W"] == (32, 32) and shapes["enc.accent_prenet1.W"] == (32, 16)
    assert shapes["enc.accent_prenet0.b"] == (32,) and shapes["enc.accent_prenet1.b"] == (16,)
    assert shapes["enc.prenet1.W"] == (256, 112) and shapes["enc.bank3.W"] == (3, 128, 128)
    # the accent tensors lie in the encoder range of the flat buffer (the encoder's DP bucket, clip + Adam with no further change)
    lay, n = layout(c)
    enc_end = lay["dec.prenet0.W"][0]
    for k in ("accent_embedding", "enc.accent_prenet0.W", "enc.accent_prenet0.b", "enc.accent_prenet1.W", "enc.accent_prenet1.b"):
        assert lay[k][0] < enc_end, k
    from satt_amd.params import l2_regularized
    assert "accent_embedding" not in l2_regularized(c) and "enc.accent_prenet0.W" in l2_regularized(c)


def test_accent_refusals():
    # existing refusals stay
    with pytest.raises(ValueError):
        validate_params(accent_hp(encoder="SelfAttentionCBHGEncoder"))
    with pytest.raises(ValueError):
        validate_params(accent_hp(encoder="ZoneoutEncoderV1"))
    with pytest.raises(UnsupportedConfiguration):
        validate_params(accent_hp(use_accent_type=False))
    with pytest.raises(UnsupportedConfiguration):
        validate_params(accent_hp(encoder="EncoderV1WithAccentType"))
    # the reference's build-time assertions (modules/module.py:502-505), with the offending numbers
    with pytest.raises(UnsupportedConfiguration, match=r"encoder_prenet_out_units_if_accent\[0\]=224 must equal embedding_dim=256"):
        validate_params(accent_hp(encoder_prenet_out_units_if_accent=[224, 112]))
    with pytest.raises(UnsupportedConfiguration, match=r"accent_type_prenet_out_units\[0\]=24 must equal accent_type_embedding_dim=32"):
        validate_params(accent_hp(accent_type_prenet_out_units=[24, 16]))
    with pytest.raises(UnsupportedConfiguration, match=r"256 \+ 64 must equal embedding_dim \+ accent_type_embedding_dim = 256 \+ 32"):
        validate_params(accent_hp(self_attention_out_units=64, attention2_out_units=64))
    # the CBHG adjustment layer is not built: the pre-net widths must fill cbhg_out_units // 2 and projection2's width
    with pytest.raises(UnsupportedConfiguration, match=r"112 \+ 8 = 120 must equal cbhg_out_units // 2 = 128.*adjustment_layer"):
        validate_params(accent_hp(accent_type_prenet_out_units=[32, 8]))
    with pytest.raises(UnsupportedConfiguration, match=r"projection2_out_channels = 64.*adjustment_layer"):
        validate_params(accent_hp(projection2_out_channels=64))
    # the reference's DEFAULT accent sizes ((224,112)+(32,16), cbhg_out_units=224) need the adjustment layer
    with pytest.raises(UnsupportedConfiguration, match=r"112 \+ 16 = 128 must equal cbhg_out_units // 2 = 112"):
        validate_params(accent_hp(embedding_dim=224, encoder_prenet_out_units_if_accent=[224, 112], cbhg_out_units=224))
    # two dropout streams are declared for the accent pre-net: a third layer is refused
    with pytest.raises(UnsupportedConfiguration, match=r"at most 2 accent pre-net layers are built \(got 3\)"):
        validate_params(accent_hp(accent_type_prenet_out_units=[32, 32, 16]))
    with pytest.raises(ValueError, match="1 or 2 layers"):
        ModelConfig(num_accent_type=5, accent_prenet=(32, 32, 16))
    # the baseline model with the flag
    hp = hp_from("tacotron.json"); hp.use_accent_type = True
    with pytest.raises(ValueError):
        validate_params(hp)
    hp.encoder = "SelfAttentionCBHGEncoderWithAccentType"
    with pytest.raises(UnsupportedConfiguration):
        validate_params(hp)


def _parent_param_shapes(c):
    """param_shapes as it was before the accent fields existed, restated independently for the encoder front end: the oracle's list
    (oracle/torch_ref.py param_shapes, unchanged by this feature) is the parent's layout for every configuration it covers"""
    kw = {k: getattr(c, k) for k in vars(torch_ref.Cfg()) if hasattr(c, k)}
    return torch_ref.param_shapes(torch_ref.Cfg(**kw))


@pytest.mark.parametrize("corpus,name", [("ljspeech", "self-attention-tacotron.json"), ("ljspeech", "tacotron.json"),
                                         ("vctk", "self-attention-tacotron.json"), ("vctk", "tacotron.json")])
def test_existing_layouts_unchanged(corpus, name):
    """accent off (0 types): names, shapes, offsets and total size of the four shipped configurations are what they were"""
    c = ModelConfig.from_hparams(hp_from(name, corpus))
    assert c.num_accent_type == 0 and not c.accent and c.prenet_width == c.enc_prenet[-1]
    shapes = param_shapes(c)
    assert not any("accent" in n for n, _ in shapes)
    assert shapes == _parent_param_shapes(c)
    lay, total = layout(c)
    off = 0
    for n, shp in shapes:           # the packing rule of params.layout, restated
        assert lay[n] == (off, shp)
        off += (int(np.prod(shp)) + 7) // 8 * 8
    assert total == off
    if (corpus, name) == ("ljspeech", "self-attention-tacotron.json"):
        assert sum(int(np.prod(s)) for _, s in shapes) == 6246104


def test_stream_ids_match_header():
    from satt_amd import engine
    assert ac.accent_streams() == ac.S_ACCENT == (engine.S_ACCENT_PRENET0, engine.S_ACCENT_PRENET1)
    used = [getattr(torch_ref.rng, k) for k in dir(torch_ref.rng) if k.startswith("STREAM_")]
    assert not set(ac.S_ACCENT) & set(used) and all(s % engine.HOP_STREAM not in (engine.S_ENC_SA, engine.S_DEC_SA) for s in ac.S_ACCENT)


def test_composed_reference_reproduces_plain_forward():
    """the substitution (zero-layer pre-net, embedding := pre-net output, source := arange) with the accent branch removed gives
    torch_ref.forward bit for bit - outputs and gradients"""
    cfg, P = make_params(SMALL, seed=1)
    batch = small_batch(cfg, 3, 9, 12, seed=3)
    bt = torch_ref.batch_to_torch(batch)
    Pa = torch_ref.to_torch(P, torch.float64, requires_grad=True)
    Pb = torch_ref.to_torch(P, torch.float64, requires_grad=True)
    a = torch_ref.forward(Pa, bt, torch_ref.Cfg(**SMALL), True, 7)
    b = ac.composed_forward(Pb, bt, SMALL, True, 7)
    for k in ("lstm_out", "sa_out", "mel", "stop", "alignment1", "alignment2", "loss"):
        assert torch.equal(a[k], b[k]), k
    ga = torch.autograd.grad(a["loss"], list(Pa.values()), allow_unused=True)
    gb = torch.autograd.grad(b["loss"], list(Pb.values()), allow_unused=True)
    for k, x, y in zip(Pa, ga, gb):
        assert (x is None) == (y is None) and (x is None or torch.allclose(x, y, rtol=1e-12, atol=1e-15)), k


def test_composed_reference_sees_accent_parameters():
    cfg, P = make_params(ac.ACCENT_SMALL, seed=1)
    batch = ac.accent_batch(cfg, 3, 9, 12, seed=3)
    assert batch["accent_type"].min() >= cfg.accent_offset and batch["accent_type"].max() < cfg.accent_offset + cfg.num_accent_type
    out, col, g = ac.composed_run(ac.ACCENT_SMALL, P, batch, True, seed=7)
    assert np.isfinite(float(out["loss"].detach()))
    for k in ("accent_embedding", "enc.accent_prenet0.W", "enc.accent_prenet0.b", "enc.accent_prenet1.W", "enc.accent_prenet1.b"):
        assert np.abs(g[k]).max() > 0, k
