"""Helpers of the speaker-conditioning tests (speaker_embedding_projection_out_dim, speaker_for_synthesis): configurations with the
two fields, and the float64 reference COMPOSED from the oracle's public pieces without touching oracle/.  torch_ref.decoder takes the
embedded speaker vector and multiplies it with P["dec.prenet0.Ws"] as it finds it, so the resize layer of reference
models/models.py:307-312 is restated here (relu(emb Wr + br)) and its output is what the decoder is fed; speaker_for_synthesis
(:333-339) replaces the ids before the lookup.  Encoder, decoder and losses are the oracle's own."""
import numpy as np
import torch

from oracle import torch_ref

SPK_KEYS = ("speaker_proj_dim", "speaker_for_synthesis")


def oracle_kw(cfg_kw):
    return {k: v for k, v in cfg_kw.items() if k not in SPK_KEYS}


def speaker_vector(Pt, speaker_id, cfg_kw, speaker_embed=None):
    """what the reference's composed `speaker_embedding(...)` returns for a batch: [B, R] with the resize layer, [B, E] without"""
    sfs = cfg_kw.get("speaker_for_synthesis", -1)
    if speaker_embed is not None:
        e = speaker_embed
    else:
        ids = torch.as_tensor(np.asarray(speaker_id))
        if sfs > -1:        # a Python scalar in the reference; the pre-net broadcasts it over the batch: the same numbers
            ids = torch.full_like(ids, sfs)
        e = Pt["speaker_embedding"][ids - cfg_kw.get("speaker_offset", 0)]
    if cfg_kw.get("speaker_proj_dim", -1) > -1:
        e = torch.relu(e @ Pt["speaker_resize.W"] + Pt["speaker_resize.b"])
    return e


def composed_forward(Pt, bt, cfg_kw, training=True, seed=0, collect=None):
    """torch_ref.forward with the composed speaker vector"""
    ocfg = torch_ref.Cfg(**oracle_kw(cfg_kw))
    spk = speaker_vector(Pt, bt["speaker_id"], cfg_kw)
    lstm_out, sa_out, enc_align = torch_ref.encoder(bt["source"], bt["source_length"], Pt, ocfg, training, seed, collect=collect)
    mel, stop, al1, al2, dec_align = torch_ref.decoder(lstm_out, sa_out, bt["source_length"], bt["mel"], Pt, ocfg, training, seed,
                                                       spk, collect)
    mel_loss, done_loss = torch_ref.losses(mel, stop, bt)
    return dict(mel=mel, stop=stop, alignment1=al1, alignment2=al2, enc_alignment=enc_align, dec_alignment=dec_align,
                lstm_out=lstm_out, sa_out=sa_out, mel_loss=mel_loss, done_loss=done_loss, loss=mel_loss + done_loss)


def composed_run(cfg_kw, P, batch, training=True, seed=0):
    """the counterpart of common.oracle_run: outputs, collected tensors, gradients of every parameter"""
    Pt = torch_ref.to_torch(P, torch.float64, requires_grad=True)
    bt = torch_ref.batch_to_torch(batch)
    col = {}
    out = composed_forward(Pt, bt, cfg_kw, training, seed, col)
    gl = torch.autograd.grad(out["loss"], list(Pt.values()), allow_unused=True)
    g = {k: (v.numpy() if v is not None else np.zeros_like(P[k])) for k, v in zip(Pt.keys(), gl)}
    return out, col, g


def speaker_cond_ref(speaker, table, offset, Wr, br, Ws, bs, ds, B):
    """float64 reference of the speaker term alone.  speaker: int (one id for all B rows), int64 [B] ids or float [B, E] embedding.
    Returns (semb, rs, sproj), dict(table, Wr, br, Ws, bs) of gradients for the output gradient ds (table: None for an embedding)"""
    d = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=True)
    table, Wr, br, Ws, bs = d(table), d(Wr), d(br), d(Ws), d(bs)
    if isinstance(speaker, int):
        semb = table[torch.full((B,), speaker - offset, dtype=torch.int64)]
    elif torch.as_tensor(speaker).is_floating_point():
        semb = torch.as_tensor(speaker).double()
    else:
        semb = table[torch.as_tensor(speaker) - offset]
    rs = torch.relu(semb @ Wr + br)
    s = rs @ Ws + bs
    sproj = s / (1.0 + s.abs())
    gs = torch.autograd.grad((sproj * torch.as_tensor(np.asarray(ds), dtype=torch.float64)).sum(), [table, Wr, br, Ws, bs],
                             allow_unused=True)
    return (semb.detach(), rs.detach(), sproj.detach()), dict(zip(("table", "Wr", "br", "Ws", "bs"), gs))
