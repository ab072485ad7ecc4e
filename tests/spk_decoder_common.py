"""Float64 reference of speaker_embedd_to_decoder (reference models/models.py:366-372), COMPOSED from the oracle's public pieces
without touching oracle/: torch_ref.encoder with the plain Cfg, the speaker vector (speaker_common.speaker_vector: lookup, resize
layer, speaker_for_synthesis) concatenated to both encoder outputs along the feature axis, then torch_ref.decoder with a Cfg copy
whose memory widths are V1 + S and V2 + S.  The oracle's decoder is shape-driven (keys = values Wm, attn of ctx_dim zeros, the
sequence mask over the WHOLE memory row), so it forms the wide memories exactly as the TF graph does - nothing of the engine's
folding (per-sample key / gate rows) is restated here."""
import numpy as np
import torch

import speaker_common as sc
from oracle import torch_ref

KEYS = sc.SPK_KEYS + ("speaker_to_decoder",)


def oracle_kw(cfg_kw):
    return {k: v for k, v in cfg_kw.items() if k not in KEYS}


def cfgs(cfg_kw, S):
    """(encoder Cfg, decoder Cfg with the widened memories)"""
    kw = oracle_kw(cfg_kw)
    enc = torch_ref.Cfg(**kw)
    dec = torch_ref.Cfg(**dict(kw, cbhg_out_units=enc.cbhg_out_units + S, sa_units=enc.sa_units + S))
    return enc, dec


def widen(lstm_out, sa_out, s):
    tile = s[:, None, :].expand(-1, lstm_out.shape[1], -1)
    return torch.cat([lstm_out, tile], dim=-1), torch.cat([sa_out, tile], dim=-1)


def composed_forward(Pt, bt, cfg_kw, training=True, seed=0, collect=None, speaker_embed=None, bn_moving=None, target=None):
    s = sc.speaker_vector(Pt, bt.get("speaker_id"), cfg_kw, speaker_embed=speaker_embed)
    ecfg, dcfg = cfgs(cfg_kw, s.shape[1])
    lstm_out, sa_out, enc_align = torch_ref.encoder(bt["source"], bt["source_length"], Pt, ecfg, training, seed, bn_moving=bn_moving,
                                                    collect=collect)
    m1, m2 = widen(lstm_out, sa_out, s)
    mel, stop, al1, al2, dec_align = torch_ref.decoder(m1, m2, bt["source_length"], bt["mel"] if target is None else target, Pt,
                                                       dcfg, training, seed, s, collect)
    out = dict(mel=mel, stop=stop, alignment1=al1, alignment2=al2, lstm_out=lstm_out, sa_out=sa_out)
    if target is None:
        mel_loss, done_loss = torch_ref.losses(mel, stop, bt)
        out.update(mel_loss=mel_loss, done_loss=done_loss, loss=mel_loss + done_loss)
    return out


def composed_run(cfg_kw, P, batch, training=True, seed=0):
    """outputs, collected tensors and the gradient of every parameter (the counterpart of speaker_common.composed_run)"""
    Pt = torch_ref.to_torch(P, torch.float64, requires_grad=True)
    bt = torch_ref.batch_to_torch(batch)
    col = {}
    out = composed_forward(Pt, bt, cfg_kw, training, seed, col)
    gl = torch.autograd.grad(out["loss"], list(Pt.values()), allow_unused=True)
    g = {k: (v.numpy() if v is not None else np.zeros_like(P[k])) for k, v in zip(Pt.keys(), gl)}
    return out, col, g


def composed_infer(cfg_kw, P, batch, bn_moving, steps=None, teacher=False):
    """evaluation-mode decode (BatchNorm on the moving statistics, dropout off, interpolating zoneout).  teacher=True: the
    teacher-fed pass = the composed decoder on the ground truth.  Otherwise a free run of `steps` steps: the decoder is causal, so
    step t of a free run is step t of a teacher-forced pass over the frames produced so far - the prefixes are replayed."""
    Pt = torch_ref.to_torch(P, torch.float64)
    bt = torch_ref.batch_to_torch(batch)
    with torch.no_grad():
        if teacher:
            return composed_forward(Pt, bt, cfg_kw, False, 0, bn_moving=bn_moving)
        B, nm = bt["mel"].shape[0], bt["mel"].shape[2]
        r = torch_ref.Cfg(**oracle_kw(cfg_kw)).r
        produced = torch.zeros(B, 0, nm, dtype=torch.float64)
        out = None
        for t in range(steps):
            tgt = torch.cat([produced, torch.zeros(B, r, nm, dtype=torch.float64)], dim=1)      # the last step's target is never fed
            out = composed_forward(Pt, bt, cfg_kw, False, 0, bn_moving=bn_moving, target=tgt)
            produced = out["mel"][:, :(t + 1) * r]
        return out
