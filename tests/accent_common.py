"""Helpers of the accent-type tests: configurations extended with the accent fields, batches that carry `accent_type`, and the
float64 reference of SelfAttentionCBHGEncoderWithAccentType (reference modules/module.py:444-527) COMPOSED from the oracle's public
pieces without touching oracle/: x_p, x_a from torch_ref.prenet, x = cat(x_p, x_a), then torch_ref.encoder on a configuration copy
whose pre-net has zero layers and whose "embedding" table is x itself (source = arange): a zero-layer pre-net returns its input, so
the oracle's own CBHG / self-attention code runs on x and autograd carries the gradients back into every accent parameter.
test_accent_cpu.py checks that the substitution reproduces torch_ref.forward exactly when there is no accent branch."""
import re
import os

import numpy as np
import torch

from common import MEDIUM, SMALL, make_params, small_batch
from oracle import torch_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCENT_KEYS = ("num_accent_type", "accent_dim", "accent_offset", "accent_prenet")
# SMALL / MEDIUM with an accent branch whose width fills the CBHG input: Wp + Wa = cbhg_out_units // 2 = proj2
ACCENT_SMALL = dict(SMALL, enc_prenet=(16, 6), num_accent_type=5, accent_dim=6, accent_offset=3, accent_prenet=(6, 2))
ACCENT_MEDIUM = dict(MEDIUM, enc_prenet=(48, 32), num_accent_type=7, accent_dim=12, accent_offset=100, accent_prenet=(12, 8))
# examples/ljspeech/self-attention-tacotron-accent.json
ACCENT_SHIPPED = dict(enc_prenet=(256, 112), num_accent_type=129, accent_dim=32, accent_offset=0x3100, accent_prenet=(32, 16))


def accent_streams():
    """(stream of accent pre-net layer 0, layer 1) as csrc/common.h states them"""
    txt = open(os.path.join(ROOT, "self-attention-tacotron_amd", "csrc", "common.h")).read()
    return tuple(int(re.search(r"SATT_STREAM_ACCENT_PRENET%d\s*=\s*(\d+)u?;" % n, txt).group(1)) for n in (0, 1))


# plain integers, kept in step with the header by test_accent_cpu.test_stream_ids_match_header
S_ACCENT = (40, 41)


def accent_batch(cfg, B, Ti, Tm, seed=3, concentrate=None):
    """small_batch + accent_type [B, Ti] int64 in [offset, offset + num_accent_type), padded with the offset (table row 0)"""
    batch = small_batch(cfg, B, Ti, Tm, seed=seed)
    g = np.random.default_rng(seed + 1000)
    acc = g.integers(0, cfg.num_accent_type, (B, Ti)).astype(np.int64)
    if concentrate is not None:
        acc[g.random((B, Ti)) < 0.8] = concentrate
    pad = np.arange(Ti)[None, :] >= np.asarray(batch["source_length"])[:, None]
    acc[pad] = 0
    batch["accent_type"] = acc + cfg.accent_offset
    return batch


def oracle_kw(cfg_kw):
    return {k: v for k, v in cfg_kw.items() if k not in ACCENT_KEYS}


def composed_encoder(Pt, bt, cfg_kw, training, seed, collect=None, bn_moving=None):
    """(lstm_out, sa_out, enc_align) of the accent encoder; cfg_kw without accent fields: the plain encoder through the same trick"""
    kw = oracle_kw(cfg_kw)
    ocfg = torch_ref.Cfg(**kw)
    B, Ti = bt["source"].shape
    x = torch_ref.prenet(Pt["embedding"][bt["source"]], Pt, "enc.prenet", len(ocfg.enc_prenet), ocfg.enc_prenet_drop, training,
                         seed, (torch_ref.rng.STREAM_ENC_PRENET0, torch_ref.rng.STREAM_ENC_PRENET1))
    if cfg_kw.get("num_accent_type", 0) > 0:
        ea = Pt["accent_embedding"][bt["accent_type"] - cfg_kw["accent_offset"]]
        xa = torch_ref.prenet(ea, Pt, "enc.accent_prenet", len(cfg_kw["accent_prenet"]), ocfg.enc_prenet_drop, training, seed,
                              S_ACCENT)
        x = torch.cat([x, xa], dim=-1)
    cfg2 = torch_ref.Cfg(**dict(kw, enc_prenet=()))
    P2 = dict(Pt)
    P2["embedding"] = x.reshape(B * Ti, -1)
    src = torch.arange(B * Ti).reshape(B, Ti)
    return torch_ref.encoder(src, bt["source_length"], P2, cfg2, training, seed, bn_moving=bn_moving, collect=collect)


def composed_forward(Pt, bt, cfg_kw, training=True, seed=0, collect=None):
    """torch_ref.forward with the composed encoder (decoder and losses are the oracle's own, unchanged)"""
    ocfg = torch_ref.Cfg(**oracle_kw(cfg_kw))
    lstm_out, sa_out, enc_align = composed_encoder(Pt, bt, cfg_kw, training, seed, collect)
    mel, stop, al1, al2, dec_align = torch_ref.decoder(lstm_out, sa_out, bt["source_length"], bt["mel"], Pt, ocfg, training, seed,
                                                       None, collect)
    mel_loss, done_loss = torch_ref.losses(mel, stop, bt)
    return dict(mel=mel, stop=stop, alignment1=al1, alignment2=al2, enc_alignment=enc_align, dec_alignment=dec_align,
                lstm_out=lstm_out, sa_out=sa_out, mel_loss=mel_loss, done_loss=done_loss, loss=mel_loss + done_loss)


def composed_run(cfg_kw, P, batch, training=True, seed=0, dalign=None):
    """the counterpart of common.oracle_run for accent configurations: outputs, collected tensors, gradients of every parameter"""
    Pt = torch_ref.to_torch(P, torch.float64, requires_grad=True)
    bt = torch_ref.batch_to_torch(batch)
    col = {}
    out = composed_forward(Pt, bt, cfg_kw, training, seed, col)
    loss = out["loss"]
    if dalign is not None:
        loss = loss + (out["alignment1"] * torch.as_tensor(dalign[0])).sum() + (out["alignment2"] * torch.as_tensor(dalign[1])).sum()
    gl = torch.autograd.grad(loss, list(Pt.values()), allow_unused=True)
    g = {k: (v.numpy() if v is not None else np.zeros_like(P[k])) for k, v in zip(Pt.keys(), gl)}
    return out, col, g


def accent_prenet_ref(ids, table, offset, Ws, bs, rate, seed, dout=None):
    """float64 torch reference of the accent branch alone: y, and (dtable, dWs, dbs) for the output gradient dout"""
    table = torch.tensor(np.asarray(table), dtype=torch.float64, requires_grad=True)
    Pt = {}
    for n, (W, b) in enumerate(zip(Ws, bs)):
        Pt["p%d.W" % n] = torch.tensor(np.asarray(W), dtype=torch.float64, requires_grad=True)
        Pt["p%d.b" % n] = torch.tensor(np.asarray(b), dtype=torch.float64, requires_grad=True)
    e = table[torch.as_tensor(np.asarray(ids)) - offset]
    y = torch_ref.prenet(e, Pt, "p", len(Ws), rate, rate > 0, seed, S_ACCENT)
    if dout is None:
        return y.detach(), None
    gs = torch.autograd.grad((y * torch.as_tensor(np.asarray(dout), dtype=torch.float64)).sum(), [table] + list(Pt.values()))
    return y.detach(), (gs[0], [gs[1 + 2 * n] for n in range(len(Ws))], [gs[2 + 2 * n] for n in range(len(Ws))])
