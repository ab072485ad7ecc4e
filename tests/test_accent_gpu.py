"""GPU tests of the accent-type input: the two one-launch kernels (csrc/accent_prenet.hip) against float64 torch, the dropout
index of a GEMM epilogue with a strided output, and the full model (forward, every parameter gradient, optimiser steps, decode)
against the float64 reference composed in accent_common.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import accent_common as ac
from common import make_params, rel_err
from oracle import rng, torch_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
ACCENT_NAMES = ("accent_embedding", "enc.accent_prenet0.W", "enc.accent_prenet0.b", "enc.accent_prenet1.W", "enc.accent_prenet1.b")


def T(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32, device=DEV).contiguous()


def close(a, b, tol, what=""):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    err = float((a - b).abs().max() / (b.abs().max() + 1e-12))
    print("%-32s rel_err=%.3e" % (what, err))
    assert err < tol, (what, err)


def _branch(ops, ids, table, offset, Ws, bs, rate, seed_t, dout, Wp, fused):
    """forward into the trailing columns of a shared [M, Wp + Wa] buffer + backward from the same columns of its gradient"""
    M, Wa = ids.numel(), Ws[-1].shape[1]
    drops = [ops.Drop(rate, ac.S_ACCENT[n], seed_t) for n in range(len(Ws))]
    shared = torch.full((M, Wp + Wa), -7.0, device=DEV)
    dshared = torch.zeros(M, Wp + Wa, device=DEV); dshared[:, Wp:] = dout
    dt = torch.zeros_like(table); dWs = [torch.zeros_like(W) for W in Ws]; dbs = [torch.zeros_like(b) for b in bs]
    if fused:
        assert ops.accent_prenet_fwd(ids, table, offset, Ws, bs, shared[:, Wp:], drops)
        assert ops.accent_prenet_bwd(ids, table, offset, Ws, bs, dshared[:, Wp:], drops, dt, dWs, dbs)
    else:       # the composition the engine falls back to beyond the kernel's cap
        x = torch.empty(M, table.shape[1], device=DEV)
        ops.embedding_fwd(ids, table, x, offset=offset)
        acts = [x]
        for n in range(len(Ws)):
            y = shared[:, Wp:] if n == len(Ws) - 1 else torch.empty(M, Ws[n].shape[1], device=DEV)
            ops.linear(acts[-1], Ws[n], bs[n], y, act=ops.ACT_RELU, drop=drops[n])
            acts.append(y)
        dx = dshared[:, Wp:]
        for n in reversed(range(len(Ws))):
            dp = torch.empty(M, Ws[n].shape[1], device=DEV)
            ops.act_bwd(dx, acts[n + 1], dp, ops.ACT_RELU, drops[n].scale)
            ops.linear_dw(acts[n], dp, dWs[n], db=dbs[n])
            dx = torch.empty(M, acts[n].shape[1], device=DEV)
            ops.linear_dx(dp, Ws[n], dx)
        ops.embedding_bwd(ids, dx, dt, offset=offset)
    torch.cuda.synchronize()
    assert bool((shared[:, :Wp] == -7.0).all())          # the phoneme columns are not touched
    return shared[:, Wp:], dt, dWs, dbs


# shipped sizes at the benchmark's row count, and two odd shapes: rows not a multiple of either tile, one layer, widths 8 / 24
SHAPES = [((32, 160), 129, 32, (32, 16), 112), ((3, 37), 5, 8, (24,), 40), ((7, 11), 9, 24, (8, 24), 8)]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("spread", [True, False])
@pytest.mark.parametrize("rate", [0.0, 0.5])
@pytest.mark.parametrize("shape,ntypes,dim,widths,Wp", SHAPES)
def test_accent_prenet_ops(shape, ntypes, dim, widths, Wp, rate, spread, fused):
    """forward at 1e-6 relative (pure fp32, sums of <= 32 terms); atomically combined gradients at the bar tests/test_ops_gpu.py
    holds linear_dw and embedding_bwd to (1e-5).  The embedding_fwd + linear composition: the issue's 1e-6 is the FUSED kernel's
    forward bar; "the fallback gives the same result as the fused kernel to that bar" is read as the gradient bar (1e-5), and the
    composition's forward (GEMM kernel, another summation order) is held to 2e-6 against float64, well inside it"""
    from satt_amd import ops
    ops.set_precision("f32")
    g = torch.Generator().manual_seed(5)
    offset = 0x3100
    M = shape[0] * shape[1]
    ids = torch.randint(0, ntypes, shape, generator=g)
    if not spread:
        ids[torch.rand(shape, generator=g) < 0.85] = 2          # most tokens on one table row
    ids = ids + offset
    table = torch.randn(ntypes, dim, generator=g) * 0.5
    Ws, bs, i = [], [], dim
    for o in widths:
        Ws.append(torch.randn(i, o, generator=g) / np.sqrt(i)); bs.append(torch.randn(o, generator=g) * 0.1); i = o
    dout = torch.randn(M, widths[-1], generator=g)
    seed = 77
    seed_t = torch.tensor([seed], dtype=torch.int32, device=DEV)
    y, dt, dWs, dbs = _branch(ops, ids.to(DEV), T(table), offset, [T(W) for W in Ws], [T(b) for b in bs], rate, seed_t, T(dout), Wp,
                              fused)
    yr, (dtr, dWr, dbr) = ac.accent_prenet_ref(ids, table, offset, Ws, bs, rate, seed, dout.reshape(shape + (widths[-1],)))
    close(y, yr.reshape(M, -1), 1e-6 if fused else 2e-6, "accent pre-net forward")
    close(dt, dtr, 1e-5, "d accent_embedding")
    for n in range(len(Ws)):
        close(dWs[n], dWr[n], 1e-5, "dW%d" % n)
        close(dbs[n], dbr[n], 1e-5, "db%d" % n)
    assert float(dt.abs().max()) > 0


def test_accent_prenet_declines_beyond_cap():
    """wider than 64, three layers, or a table whose gradient accumulator does not fit in LDS: nothing launched, False returned"""
    from satt_amd import ops
    seed_t = torch.tensor([1], dtype=torch.int32, device=DEV)
    ids = torch.zeros(4, 5, dtype=torch.int64, device=DEV)
    for ntypes, dim, widths in ((5, 96, (96, 16)), (5, 8, (8, 8, 8)), (5, 16, (128,))):
        table = torch.zeros(ntypes, dim, device=DEV)
        Ws, bs, i = [], [], dim
        for o in widths:
            Ws.append(torch.zeros(i, o, device=DEV)); bs.append(torch.zeros(o, device=DEV)); i = o
        out = torch.full((20, widths[-1]), 3.0, device=DEV)
        drops = [ops.Drop(0.0, 40 + n, seed_t) for n in range(len(Ws))]
        assert ops.accent_prenet_fwd(ids, table, 0, Ws, bs, out, drops) is False
        torch.cuda.synchronize()
        assert bool((out == 3.0).all())
    # forward fits, the backward's table accumulator does not (4096 x 16 floats): the backward declines on its own
    table = torch.zeros(4096, 16, device=DEV); W = torch.zeros(16, 16, device=DEV); b = torch.zeros(16, device=DEV)
    out = torch.zeros(20, 16, device=DEV); d = [ops.Drop(0.0, 40, seed_t)]
    assert ops.accent_prenet_fwd(ids, table, 0, [W], [b], out, d) is True
    assert ops.accent_prenet_bwd(ids, table, 0, [W], [b], out, d, torch.zeros_like(table), [torch.zeros_like(W)],
                                 [torch.zeros_like(b)]) is False


def test_gemm_dropout_index_of_strided_output():
    """a GEMM epilogue that writes columns [0, N) of a wider buffer draws the dropout mask of a [M, N] tensor (index row*N + col, not
    row*ld + col): the phoneme pre-net's mask stays the one the oracle draws for [B, Ti, Wp]"""
    from satt_amd import ops
    g = torch.Generator().manual_seed(2)
    M, K, N, extra, seed, stream = 75, 24, 40, 16, 31, rng.STREAM_ENC_PRENET1
    x = torch.rand(M, K, generator=g) + 0.1; W = torch.rand(K, N, generator=g) + 0.1           # positive: ReLU keeps everything
    seed_t = torch.tensor([seed], dtype=torch.int32, device=DEV)
    for prec in ("f32", "bf16"):
        ops.set_precision(prec)
        shared = torch.zeros(M, N + extra, device=DEV)
        ops.linear(T(x), T(W), None, shared[:, :N], act=ops.ACT_RELU, drop=ops.Drop(0.5, stream, seed_t))
        torch.cuda.synchronize()
        keep = torch.from_numpy(rng.keep_mask(seed, stream, (M, N), 0.5))
        assert torch.equal(shared[:, :N].cpu() != 0, keep), prec
        assert bool((shared[:, N:] == 0).all())
    ops.set_precision("f32")


def run_engine(cfg, P, batch, seed, prec, dalign=None, fused=True):
    from satt_amd import ops
    from satt_amd.engine import Engine
    ops.set_precision(prec)
    eng = Engine(cfg, "cuda", params=P, rng_seed=seed)
    eng.fused_accent = fused
    b = eng.to_device_batch(batch)
    eng.zero_grad()
    ctx = eng.forward(b, training=True)
    assert ctx["accent_fused"] is fused
    if dalign is not None:
        ctx["dalign1"] = T(dalign[0]); ctx["dalign2"] = T(dalign[1])
    eng.backward(ctx)
    torch.cuda.synchronize()
    eng.check_clusters(ctx)
    out = {k: v.detach().float().cpu().numpy() for k, v in eng.outputs(ctx).items()}
    grads = {k: v.detach().cpu().numpy() for k, v in eng.G.items()}
    return eng, out, grads


def report(out, ref, grads, gref, keys):
    rows = [(k, rel_err(out[k], ref[k].detach().numpy() if hasattr(ref[k], "detach") else ref[k])) for k in keys]
    rows += [("grad:" + k, rel_err(grads[k], gref[k])) for k in grads]
    for k, e in rows:
        print("%-32s rel_err=%.3e" % (k, e))
    return dict(rows)


FWD_KEYS = ["lstm_out", "sa_out", "alignment1", "alignment2", "dec_out", "mel", "stop", "loss", "mel_loss", "done_loss"]


@pytest.mark.parametrize("cfg_kw,B,Ti,Tm,fused", [(ac.ACCENT_SMALL, 3, 9, 12, True), (ac.ACCENT_MEDIUM, 5, 37, 46, True),
                                                  (ac.ACCENT_MEDIUM, 5, 37, 46, False), (ac.ACCENT_SHIPPED, 2, 21, 24, True)])
def test_f32_parity_accent(cfg_kw, B, Ti, Tm, fused):
    """forward outputs and EVERY parameter gradient against the composed float64 reference, dropout and zoneout on: the bar of
    tests/test_model_gpu.py test_f32_parity_* (2e-4 on the same report); the accent parameters receive gradient"""
    cfg, P = make_params(cfg_kw, seed=1)
    batch = ac.accent_batch(cfg, B, Ti, Tm, seed=3)
    g = np.random.default_rng(0)
    Td = Tm // cfg.r
    dal = (g.normal(0, 0.05, (B, Td, Ti)), g.normal(0, 0.05, (B, Td, Ti)))
    ref, col, gref = ac.composed_run(cfg_kw, P, batch, True, seed=7, dalign=dal)
    eng, out, grads = run_engine(cfg, P, batch, 7, "f32", dalign=dal, fused=fused)
    errs = report(out, {**ref, "dec_out": col["dec_out"]}, grads, gref, FWD_KEYS)
    bad = {k: e for k, e in errs.items() if not (e < 2e-4)}
    assert not bad, bad
    for k in ACCENT_NAMES:
        assert float(np.abs(grads[k]).max()) > 0, k


@pytest.mark.parametrize("cfg_kw,B,Ti,Tm", [(ac.ACCENT_MEDIUM, 5, 37, 46), (ac.ACCENT_SHIPPED, 2, 21, 24)])
def test_bf16_parity_accent(cfg_kw, B, Ti, Tm):
    """the criteria of tests/test_model_gpu.py test_bf16_parity verbatim"""
    cfg, P = make_params(cfg_kw, seed=2)
    batch = ac.accent_batch(cfg, B, Ti, Tm, seed=4)
    ref, col, gref = ac.composed_run(cfg_kw, P, batch, True, seed=11)
    eng, out, grads = run_engine(cfg, P, batch, 11, "bf16")
    errs = report(out, {**ref, "dec_out": col["dec_out"]}, grads, gref, FWD_KEYS)
    assert abs(float(out["mel_loss"]) - float(ref["mel_loss"].detach())) < 1e-3
    assert errs["mel"] < 5e-2 and errs["alignment1"] < 5e-2
    bad = {}
    for k in grads:
        a, b = grads[k].astype(np.float64).ravel(), gref[k].astype(np.float64).ravel()
        cos = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))
        l2 = float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))
        print("%-32s cos=%.5f relL2=%.3e" % (k, cos, l2))
        if not (cos > 0.98 and l2 < 0.2):
            bad[k] = (cos, l2)
    assert not bad, bad


def test_accent_training_steps_match_oracle():
    """three optimisation steps against the oracle's clip_and_adam on the composed reference (the pattern and bars of
    test_training_trajectory_matches_oracle): the accent tensors are clipped and updated with everything else"""
    from satt_amd import ops
    from satt_amd.engine import Engine
    ops.set_precision("f32")
    cfg_kw, B, Ti, Tm = ac.ACCENT_MEDIUM, 5, 37, 46
    cfg, P0 = make_params(cfg_kw, seed=51)
    lr0, seed0, K = 2e-3, 61, 3
    eng = Engine(cfg, "cuda", params=P0, rng_seed=seed0, lr0=lr0, decay=False)
    Po = torch_ref.to_torch(P0, torch.float64)
    m = {k: torch.zeros_like(v) for k, v in Po.items()}; v = {k: torch.zeros_like(x) for k, x in Po.items()}
    rows = []
    for t in range(1, K + 1):
        batch = ac.accent_batch(cfg, B, Ti, Tm, seed=80 + t)
        Pt = {k: x.clone().requires_grad_(True) for k, x in Po.items()}
        out = ac.composed_forward(Pt, torch_ref.batch_to_torch(batch), cfg_kw, True, seed0 + t - 1)
        gl = torch.autograd.grad(out["loss"], list(Pt.values()), allow_unused=True)
        g = {k: (x if x is not None else torch.zeros_like(Po[k])) for k, x in zip(Pt.keys(), gl)}
        gn = torch_ref.clip_and_adam(Po, g, m, v, t, lr0)
        ctx = eng.train_step(eng.to_device_batch(batch))
        eng.optimizer_step()
        torch.cuda.synchronize()
        eng.check_clusters(ctx)
        le, lo, gne = float(eng.losses[2]), float(out["loss"].detach()), float(eng.opt_state[1])
        rows.append((t, lo, le, gn, gne))
        print("step %d  loss oracle %.6f engine %.6f  |g| oracle %.5f engine %.5f" % (t, lo, le, gn, gne))
    for t, lo, le, gn, gne in rows:
        assert abs(le - lo) < 2e-3 * lo and abs(gne - gn) < 1e-2 * gn, rows
    for k in Po:
        d_o = (Po[k].numpy() - np.asarray(P0[k], dtype=np.float64)).ravel()
        d_e = (eng.P[k].detach().cpu().numpy().astype(np.float64) - np.asarray(P0[k], dtype=np.float64)).ravel()
        no, ne = np.linalg.norm(d_o), np.linalg.norm(d_e)
        cos = float(d_o @ d_e / (no * ne + 1e-300))
        print("%-28s |dP| oracle %.4e engine %.4e  cos %.6f" % (k, no, ne, cos))
        assert abs(ne - no) < 0.05 * no and cos > 0.995, (k, no, ne, cos)
    for k in ACCENT_NAMES:
        assert np.linalg.norm(Po[k].numpy() - np.asarray(P0[k], dtype=np.float64)) > 0, k


def test_accent_missing_input_is_named():
    from satt_amd import ops
    from satt_amd.engine import Engine
    from satt_amd.inference import infer
    ops.set_precision("f32")
    cfg, P = make_params(ac.ACCENT_SMALL, seed=1)
    batch = ac.accent_batch(cfg, 3, 9, 12, seed=3)
    eng = Engine(cfg, "cuda", params=P, rng_seed=7)
    b = eng.to_device_batch({k: v for k, v in batch.items() if k != "accent_type"})
    with pytest.raises(KeyError, match="accent_type"):
        eng.forward(b, training=True)
    with pytest.raises(ValueError, match="accent_type"):
        infer(eng, b["source"], b["source_length"], max_steps=4)


def test_accent_decode_matches_reference():
    """evaluation-mode encoder (pre-net dropout off, as for the phoneme pre-net: the reference's PreNet gets is_training,
    modules/module.py:470-472) at the f32 bar, and the free-running DecodeSession against torch_ref.infer stepping on the composed
    encoder input, at the bar tests/test_inference_gpu.py test_free_running_decode_matches_oracle uses (5e-4)"""
    from satt_amd import ops
    from satt_amd.engine import Engine
    from satt_amd.inference import infer
    ops.set_precision("f32")
    cfg_kw, B, Ti, steps = ac.ACCENT_MEDIUM, 4, 33, 14
    cfg, P = make_params(cfg_kw, seed=2)
    batch = ac.accent_batch(cfg, B, Ti, 2 * cfg.r, seed=5)
    eng = Engine(cfg, "cuda", params=P, rng_seed=7)
    g = np.random.default_rng(11)
    mv = {}
    for name, (mean, var) in eng.bn.items():        # non-trivial moving statistics, shared with the reference
        m = g.normal(0, 0.2, mean.shape[0]).astype(np.float32); v = g.uniform(0.5, 1.5, var.shape[0]).astype(np.float32)
        mean.copy_(torch.as_tensor(m)); var.copy_(torch.as_tensor(v))
        mv[name] = (torch.as_tensor(m, dtype=torch.float64), torch.as_tensor(v, dtype=torch.float64))
    b = eng.to_device_batch(batch)
    out = infer(eng, b["source"], b["source_length"], max_steps=steps, min_steps=10 ** 6, accent_type=b["accent_type"])
    torch.cuda.synchronize()
    # reference: the composed pre-net output as the "embedding" of a zero-layer pre-net, then the oracle's own infer
    Pt = torch_ref.to_torch(P)
    bt = torch_ref.batch_to_torch(batch)
    kw = ac.oracle_kw(cfg_kw)
    ocfg = torch_ref.Cfg(**kw)
    x = torch_ref.prenet(Pt["embedding"][bt["source"]], Pt, "enc.prenet", 2, ocfg.enc_prenet_drop, False, 7, (1, 2))
    xa = torch_ref.prenet(Pt["accent_embedding"][bt["accent_type"] - cfg.accent_offset], Pt, "enc.accent_prenet", 2,
                          ocfg.enc_prenet_drop, False, 7, ac.S_ACCENT)
    P2 = dict(Pt); P2["embedding"] = torch.cat([x, xa], dim=-1).reshape(B * Ti, -1)
    ref = torch_ref.infer(P2, torch.arange(B * Ti).reshape(B, Ti), bt["source_length"], torch_ref.Cfg(**dict(kw, enc_prenet=())),
                          steps, mv, min_steps=10 ** 6)
    lstm_out, sa_out, _ = ac.composed_encoder(Pt, bt, cfg_kw, False, 7, bn_moving=mv)
    e1 = rel_err(out["lstm_out"].float().cpu().numpy().reshape(B, Ti, -1), lstm_out.numpy())
    e2 = rel_err(out["sa_out"].float().cpu().numpy().reshape(B, Ti, -1), sa_out.numpy())
    print("lstm_out %.3e  sa_out %.3e" % (e1, e2))
    assert e1 < 2e-4 and e2 < 2e-4
    assert out["steps"] == ref["steps"] == steps
    for k in ("mel", "stop", "alignment1", "alignment2"):
        e = rel_err(out[k].detach().cpu().numpy(), ref[k].numpy())
        print(k, e)
        assert e < 5e-4, (k, e)


def test_accent_encoder_module_takes_the_reference_tuple():
    """the callable encoder of an accent model takes inputs = (embedded, accent_embedded) as the reference's call does
    (modules/module.py:507-508) and gives what the id path gives; a bare tensor is refused"""
    from satt_amd import ops
    from satt_amd.engine import Engine
    from satt_amd.models.models import EncoderSpec
    ops.set_precision("f32")
    cfg, P = make_params(ac.ACCENT_MEDIUM, seed=2)
    batch = ac.accent_batch(cfg, 3, 17, 8, seed=5)
    eng = Engine(cfg, "cuda", params=P, rng_seed=7)
    b = eng.to_device_batch(batch)
    ctx = {"training": False, "batch": b}
    lstm_out, sa_out = eng._encode(b, False, ctx)
    enc = EncoderSpec("SelfAttentionCBHGEncoderWithAccentType", False, *([0] * (len(EncoderSpec._fields) - 2))).bind(eng)
    emb = torch.as_tensor(P["embedding"])[torch.as_tensor(batch["source"])]
    aemb = torch.as_tensor(P["accent_embedding"])[torch.as_tensor(batch["accent_type"]) - cfg.accent_offset]
    l2, s2, aligns = enc((emb, aemb), input_lengths=batch["source_length"])
    torch.cuda.synchronize()
    assert rel_err(l2.cpu().numpy().reshape(-1), lstm_out.cpu().numpy().reshape(-1)) < 1e-5
    assert rel_err(s2.cpu().numpy().reshape(-1), sa_out.cpu().numpy().reshape(-1)) < 1e-5
    with pytest.raises(ValueError, match="accent_embedded"):
        enc(emb, input_lengths=batch["source_length"])


def test_accent_kernels_run_clean_under_lds_poison():
    """SATT_DEBUG_POISON_LDS: every LDS word the two kernels read was written by the same launch - the op test at the shipped sizes
    in a child process with a NaN pattern in every LDS word of every CU before each launch"""
    env = dict(os.environ, SATT_DEBUG_POISON_LDS="7fc00000")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "test_accent_prenet_ops and shape0"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
