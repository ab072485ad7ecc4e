"""GPU tests of the speaker conditioning with the resize layer (speaker_embedding_projection_out_dim) and of speaker_for_synthesis:
the one-launch forward kernel (csrc/speaker_cond.hip) against float64 torch, the chain of generic ops it replaces and the chain
that is the term's backward, the full model
(forward, every parameter gradient) against the float64 composition of speaker_common.py, inference, evaluation, checkpoints."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import speaker_common as sc
from common import MEDIUM, make_params, rel_err, small_batch
from oracle import torch_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPK = dict(num_speakers=7, speaker_dim=16, speaker_offset=225)
RESIZE_NAMES = ("speaker_embedding", "speaker_resize.W", "speaker_resize.b", "dec.prenet0.Ws", "dec.prenet0.bs")


def T(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32, device=DEV).contiguous()


def close(a, b, tol, what=""):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    err = float((a - b).abs().max() / (b.abs().max() + 1e-12))
    print("%-32s rel_err=%.3e" % (what, err))
    assert err < tol, (what, err)


def _inputs(B, E, R, P0, nspk, seed):
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(nspk, E, generator=g) * 0.5
    Wr = torch.randn(E, R, generator=g) / np.sqrt(E); br = torch.randn(R, generator=g) * 0.1
    Ws = torch.randn(R, P0, generator=g) / np.sqrt(R); bs = torch.randn(P0, generator=g) * 0.1
    ds = torch.randn(B, P0, generator=g)
    return g, table, Wr, br, Ws, bs, ds


# (B, E, R, P0, speakers): the VCTK sizes with R = 64; odd sizes that are multiples of nothing; B = 1; a wide resize layer
SHAPES = [(32, 16, 64, 256, 152), (5, 7, 13, 37, 3), (1, 16, 64, 256, 152), (9, 21, 90, 130, 11)]


@pytest.mark.parametrize("mode", ["ids", "scalar", "embed"])
@pytest.mark.parametrize("B,E,R,P0,nspk", SHAPES)
def test_speaker_cond_kernel(B, E, R, P0, nspk, mode):
    """the forward kernel alone against float64 torch on the CPU at the bar tests/test_ops_gpu.py holds fp32 forward products to
    (2e-6, test_linear_fwd_bwd, f32); the gather is exact.  ids: duplicates in the batch and both ends of the table.  (The term's
    backward is a chain of generic ops: test_speaker_term_chain_and_kernel holds it to the gradient bars.)"""
    from satt_amd import ops
    assert ops.speaker_cond_supported(B, E, R, P0)
    offset = 225
    g, table, Wr, br, Ws, bs, ds = _inputs(B, E, R, P0, nspk, B * 7 + P0)
    if mode == "ids":
        ids = torch.randint(0, nspk, (B,), generator=g)
        ids[0] = nspk - 1                                   # last table row
        if B > 2:
            ids[1] = 0; ids[2] = 0                          # first table row, twice
            ids[B - 1] = ids[B // 2]                        # another duplicate
        speaker_ref = ids + offset
        speaker = speaker_ref.to(DEV)
    elif mode == "scalar":
        speaker = speaker_ref = offset + nspk - 1
    else:
        speaker_ref = torch.randn(B, E, generator=g) * 0.5
        speaker = T(speaker_ref)
    semb = torch.full((B, E), 9.0, device=DEV); rs = torch.full((B, R), 9.0, device=DEV); sproj = torch.full((B, P0), 9.0, device=DEV)
    assert ops.speaker_cond_fwd(speaker, T(table), offset, T(Wr), T(br), T(Ws), T(bs), semb, rs, sproj)
    (semb_r, rs_r, sproj_r), _ = sc.speaker_cond_ref(speaker_ref, table, offset, Wr, br, Ws, bs, ds, B)
    assert torch.equal(semb.cpu().double(), semb_r.float().double())        # a gather: exact
    close(rs, rs_r, 2e-6, "rs")
    close(sproj, sproj_r, 2e-6, "sproj")
    if mode == "scalar":        # the scalar mode is the ids mode with that id in every row, to the bit
        ids = torch.full((B,), speaker, dtype=torch.int64, device=DEV)
        s2 = torch.empty_like(semb); r2 = torch.empty_like(rs); p2 = torch.empty_like(sproj)
        assert ops.speaker_cond_fwd(ids, T(table), offset, T(Wr), T(br), T(Ws), T(bs), s2, r2, p2)
        assert torch.equal(p2, sproj) and torch.equal(r2, rs) and torch.equal(s2, semb)


def test_speaker_cond_declines_beyond_cap():
    """over a size limit nothing is launched and False is returned"""
    from satt_amd import ops
    for B, E, R, P0 in ((4, 16, 64, 520), (4, 16, 300, 64), (4, 300, 16, 64), (300, 4, 8, 16)):
        assert not ops.speaker_cond_supported(B, E, R, P0)
        g, table, Wr, br, Ws, bs, ds = _inputs(B, E, R, P0, 5, 1)
        ids = torch.zeros(B, dtype=torch.int64, device=DEV)
        semb = torch.full((B, E), 3.0, device=DEV); rs = torch.full((B, R), 3.0, device=DEV); sproj = torch.full((B, P0), 3.0, device=DEV)
        assert ops.speaker_cond_fwd(ids, T(table), 0, T(Wr), T(br), T(Ws), T(bs), semb, rs, sproj) is False
        torch.cuda.synchronize()
        assert bool((sproj == 3.0).all()) and bool((semb == 3.0).all()) and bool((rs == 3.0).all())


def _term(eng, speaker, ds, fused):
    """Engine.speaker_term + its backward on a fresh gradient buffer: (semb, rs, sproj, {name: gradient})"""
    c = eng.cfg
    B = ds.shape[0]
    eng.fused_speaker = fused        # forward: the kernel, or the chain; the backward is the chain either way
    eng.zero_grad()
    spk = dict(semb=torch.empty(B, c.speaker_dim, device=DEV), rs=torch.empty(B, c.speaker_proj_dim, device=DEV),
               sproj=torch.empty(B, c.dec_prenet[0], device=DEV))
    eng.speaker_term(speaker, spk)
    eng._speaker_term_bwd(spk, ds)
    torch.cuda.synchronize()
    return spk, {k: eng.G[k].detach().clone() for k in RESIZE_NAMES}


@pytest.mark.parametrize("mode", ["ids", "scalar"])
@pytest.mark.parametrize("R,supported", [(64, True), (300, False)])
def test_speaker_term_chain_and_kernel(R, supported, mode):
    """Engine.speaker_term and its backward.  The forward composed from generic ops (forced, and what the engine takes by itself over
    the kernel's limit: R = 300) and the forward kernel (R = 64) against float64 and against each other at the op bars of
    tests/test_ops_gpu.py (2e-6 forward); the backward - always the chain of generic ops - on the outputs of either forward against
    float64 at 1e-5 (linear_dw, embedding_bwd), duplicate ids and the one-speaker mode included"""
    from satt_amd import ops
    from satt_amd.engine import Engine
    ops.set_precision("f32")
    cfg, P = make_params(dict(MEDIUM, **SPK, speaker_proj_dim=R), seed=3)
    B = 6
    eng = Engine(cfg, "cuda", params=P, rng_seed=1)
    assert ops.speaker_cond_supported(B, 16, R, cfg.dec_prenet[0]) is supported
    ids_h = torch.tensor([231, 225, 228, 225, 231, 227])
    speaker_ref, speaker = (ids_h, ids_h.to(DEV)) if mode == "ids" else (228, 228)
    ds_h = torch.randn(B, cfg.dec_prenet[0], generator=torch.Generator().manual_seed(2))
    (semb_r, rs_r, sproj_r), gr = sc.speaker_cond_ref(speaker_ref, P["speaker_embedding"], 225, P["speaker_resize.W"],
                                                      P["speaker_resize.b"], P["dec.prenet0.Ws"], P["dec.prenet0.bs"], ds_h, B)
    chain, gc = _term(eng, speaker, T(ds_h), False)
    assert chain["fused"] is False
    close(chain["sproj"], sproj_r, 2e-6, "chain sproj"); close(chain["rs"], rs_r, 2e-6, "chain rs")
    for k, n in zip(RESIZE_NAMES, ("table", "Wr", "br", "Ws", "bs")):
        close(gc[k], gr[n], 1e-5, "chain d " + k)
    fused, gf = _term(eng, speaker, T(ds_h), True)
    assert fused["fused"] is supported          # over the limit the engine composes the chain by itself
    close(fused["sproj"], sproj_r, 2e-6, "kernel sproj"); close(fused["rs"], rs_r, 2e-6, "kernel rs")
    close(fused["sproj"], chain["sproj"], 2e-6, "kernel vs chain sproj"); close(fused["rs"], chain["rs"], 2e-6, "kernel vs chain rs")
    for k, n in zip(RESIZE_NAMES, ("table", "Wr", "br", "Ws", "bs")):
        close(gf[k], gr[n], 1e-5, "d %s behind the kernel" % k)
    if mode == "scalar":
        assert not gf["speaker_embedding"][[r for r in range(7) if r != 3]].any()


def run_engine(cfg, P, batch, seed, prec, fused=True):
    from satt_amd import ops
    from satt_amd.engine import Engine
    ops.set_precision(prec)
    eng = Engine(cfg, "cuda", params=P, rng_seed=seed)
    eng.fused_speaker = fused
    b = eng.to_device_batch(batch)
    eng.zero_grad()
    ctx = eng.forward(b, training=True)
    eng.backward(ctx)
    torch.cuda.synchronize()
    eng.check_clusters(ctx)
    out = {k: v.detach().float().cpu().numpy() for k, v in eng.outputs(ctx).items()}
    grads = {k: v.detach().cpu().numpy() for k, v in eng.G.items()}
    return eng, ctx, out, grads


def report(out, ref, grads, gref, keys):
    rows = [(k, rel_err(out[k], ref[k].detach().numpy() if hasattr(ref[k], "detach") else ref[k])) for k in keys]
    rows += [("grad:" + k, rel_err(grads[k], gref[k])) for k in grads]
    for k, e in rows:
        print("%-32s rel_err=%.3e" % (k, e))
    return dict(rows)


@pytest.mark.parametrize("cfg_kw,ns,B,fused", [(MEDIUM, 7, 4, True), (MEDIUM, 7, 4, False), (dict(), 152, 8, True)])
def test_f32_parity_resize_layer(cfg_kw, ns, B, fused):
    """full model with R = 64, dropout and zoneout on: the forward outputs and EVERY parameter gradient against the float64
    composition, cases and bar (2e-4) of tests/test_model_gpu.py test_f32_parity_multi_speaker_vctk; the second shape is
    examples/vctk/self-attention-tacotron-resize.json itself"""
    cfg_kw = dict(cfg_kw, num_speakers=ns, speaker_dim=16, speaker_offset=225, speaker_proj_dim=64)
    cfg, P = make_params(cfg_kw, seed=4)
    batch = small_batch(cfg, B, 21, 26, seed=8)
    batch["speaker_id"] = (np.random.default_rng(1).integers(0, ns, B) + 225).astype(np.int64)
    batch["speaker_id"][-1] = batch["speaker_id"][0]            # a duplicate
    ref, col, gref = sc.composed_run(cfg_kw, P, batch, True, seed=13)
    eng, ctx, out, grads = run_engine(cfg, P, batch, 13, "f32", fused)
    assert ctx["spk"]["fused"] is fused
    errs = report(out, {**ref, "dec_out": col["dec_out"]}, grads, gref, ["mel", "stop", "alignment1", "loss"])
    bad = {k: e for k, e in errs.items() if not (e < 2e-4)}
    assert not bad, bad
    assert set(RESIZE_NAMES) <= set(grads)
    for k in RESIZE_NAMES:
        assert float(np.abs(grads[k]).max()) > 0, k


def _teacher_infer(eng, b, spk):
    from satt_amd.inference import infer
    out = infer(eng, b["source"], b["source_length"], teacher=b["mel"], speaker_id=spk)
    torch.cuda.synchronize()
    return {k: out[k].detach().clone() for k in ("mel", "stop", "alignment1", "alignment2")}


@pytest.mark.parametrize("R", [-1, 24])
def test_speaker_for_synthesis_replaces_every_speaker(R):
    """FAILS ON THE PARENT (which ignores the key).  ids [a, b] with speaker_for_synthesis = c give, to the bit, what ids [c, c]
    give with the hparam unset - through a teacher-forced infer and through evaluate - and not what [a, b] give unset; a call
    without any speaker id works; one training step sends the whole embedding gradient to row c.  With and without the resize layer."""
    from satt_amd import ops
    from satt_amd.engine import Engine
    from satt_amd.inference import evaluate, infer
    ops.set_precision("f32")
    a, b_, c_ = 226, 231, 229
    kw = dict(MEDIUM, **SPK, speaker_proj_dim=R)
    cfg, P = make_params(kw, seed=4)
    cfg_c, _ = make_params(dict(kw, speaker_for_synthesis=c_), seed=4)
    batch = small_batch(cfg, 2, 17, 12, seed=8)
    plain = Engine(cfg, "cuda", params=P, rng_seed=5)
    forced = Engine(cfg_c, "cuda", params=P, rng_seed=5)
    b = plain.to_device_batch(batch)
    ab = torch.tensor([a, b_], device=DEV); cc = torch.tensor([c_, c_], device=DEV)
    want = _teacher_infer(plain, b, cc)
    other = _teacher_infer(plain, b, ab)
    got = _teacher_infer(forced, b, ab)
    none = _teacher_infer(forced, b, None)          # a record without a speaker id (predict_mel.py) is fine when the hparam is set
    for k in want:
        assert torch.equal(got[k], want[k]), k
        assert torch.equal(none[k], want[k]), k
    assert not torch.equal(got["mel"], other["mel"])
    # evaluate: the batch's own ids and an explicit speaker_id= are both overridden
    ev_want = evaluate(plain, dict(batch, speaker_id=np.array([c_, c_], np.int64)))
    ev_other = evaluate(plain, dict(batch, speaker_id=np.array([a, b_], np.int64)))
    ev_got = evaluate(forced, dict(batch, speaker_id=np.array([a, b_], np.int64)))
    ev_arg = evaluate(forced, dict(batch, speaker_id=np.array([a, b_], np.int64)), speaker_id=np.array([b_, a], np.int64))
    for k in ("mel", "mel_with_teacher", "stop", "alignment1"):
        assert torch.equal(ev_got[k], ev_want[k]) and torch.equal(ev_arg[k], ev_want[k]), k
    for k in ("loss", "loss_with_teacher", "mel_loss", "done_loss"):
        assert ev_got[k] == ev_want[k] == ev_arg[k], k
    assert not torch.equal(ev_got["mel"], ev_other["mel"])
    # one training step: the embedding gradient of all rows goes to table row c
    tb = forced.to_device_batch(dict(batch, speaker_id=np.array([a, b_], np.int64)))
    forced.zero_grad()
    ctx = forced.forward(tb, training=True)
    forced.backward(ctx)
    torch.cuda.synchronize()
    forced.check_clusters(ctx)
    g = forced.G["speaker_embedding"].detach().cpu()
    assert float(g[c_ - 225].abs().max()) > 0
    assert not g[[r for r in range(7) if r != c_ - 225]].any()
    # ... and equals the gradient of ids [c, c] without the hparam (same seed, same dropout masks), against float64 too
    pb = plain.to_device_batch(dict(batch, speaker_id=np.array([c_, c_], np.int64)))
    plain.zero_grad()
    pctx = plain.forward(pb, training=True)
    plain.backward(pctx)
    torch.cuda.synchronize()
    assert torch.equal(plain.G["speaker_embedding"].cpu(), g)
    ref, col, gref = sc.composed_run(dict(kw, speaker_for_synthesis=c_), P, dict(batch, speaker_id=np.array([a, b_], np.int64)), True, seed=5)
    assert rel_err(g.numpy(), gref["speaker_embedding"]) < 2e-4


def test_infer_and_decoder_contract_run_through_the_resize_layer():
    """free-running and teacher-fed decode against torch_ref.infer (bar of tests/test_inference_gpu.py: 5e-4).  The oracle looks the
    speaker up in P["speaker_embedding"] and feeds the row to the pre-net; the resize layer acts on rows, so the oracle is handed
    the RESIZED table relu(table Wr + br) - and, for a speaker_embed= passed in by the decoder call contract (the reference
    composes the resize behind the embedding: an embedding passed in is resized too), the resized vectors as a B-row table.
    Forced-alignment mode runs through the same term."""
    from satt_amd import ops
    from satt_amd.engine import Engine
    from satt_amd.inference import infer
    ops.set_precision("f32")
    kw = dict(MEDIUM, **SPK, speaker_proj_dim=24)
    cfg, P = make_params(kw, seed=6)
    B, Ti, steps = 3, 13, 9
    batch = small_batch(cfg, B, Ti, steps * cfg.r, seed=2)
    ids = np.array([231, 225, 231], np.int64)
    eng = Engine(cfg, "cuda", params=P, rng_seed=5)
    mv = {n: (m.double().cpu(), v.double().cpu()) for n, (m, v) in eng.bn.items()}
    b = eng.to_device_batch(batch)
    Pt = torch_ref.to_torch(P, torch.float64)
    bt = torch_ref.batch_to_torch(batch)
    ocfg = torch_ref.Cfg(**sc.oracle_kw(kw))
    emb = torch.randn(B, 16, generator=torch.Generator().manual_seed(3)) * 0.5
    all_ids = np.arange(7) + 225
    cases = (("ids", dict(speaker_id=torch.as_tensor(ids)), sc.speaker_vector(Pt, all_ids, kw), torch.as_tensor(ids)),
             ("embed", dict(speaker_embed=emb), sc.speaker_vector(Pt, None, kw, speaker_embed=emb.double()), torch.arange(B) + 225))
    for name, kwargs, table, oids in cases:
        P2 = dict(Pt); P2["speaker_embedding"] = table
        ref = torch_ref.infer(P2, bt["source"], bt["source_length"], ocfg, steps, mv, speaker_id=oids, min_steps=10 ** 6)
        out = infer(eng, b["source"], b["source_length"], max_steps=steps, min_steps=10 ** 6, **kwargs)
        reft = torch_ref.infer(P2, bt["source"], bt["source_length"], ocfg, None, mv, speaker_id=oids, teacher=bt["mel"])
        outt = infer(eng, b["source"], b["source_length"], teacher=b["mel"], **kwargs)
        torch.cuda.synchronize()
        for k in ("mel", "stop", "alignment1", "alignment2"):
            e, et = rel_err(out[k].cpu().numpy(), ref[k].numpy()), rel_err(outt[k].cpu().numpy(), reft[k].numpy())
            print(name, k, e, et)
            assert e < 5e-4 and et < 5e-4, (name, k, e, et)
    # forced-alignment mode: the free run that is handed the teacher-forced run's alignments
    first = infer(eng, b["source"], b["source_length"], teacher=b["mel"], speaker_id=torch.as_tensor(ids))
    second = infer(eng, b["source"], b["source_length"], max_steps=first["steps"], min_steps=1 << 30, speaker_id=torch.as_tensor(ids),
                   teacher_alignments=(first["alignment1"], first["alignment2"]))
    other = infer(eng, b["source"], b["source_length"], max_steps=first["steps"], min_steps=1 << 30,
                  speaker_id=torch.as_tensor(np.array([226, 226, 226])), teacher_alignments=(first["alignment1"], first["alignment2"]))
    torch.cuda.synchronize()
    assert torch.isfinite(second["mel"]).all() and not torch.equal(second["mel"], other["mel"])
    assert rel_err(second["alignment1"].cpu().numpy(), first["alignment1"].cpu().numpy()) < 1e-6


def test_checkpoint_round_trip_keeps_the_resize_layer(tmp_path):
    """native checkpoints carry the new parameters through the existing name-driven path"""
    from satt_amd import ops
    from satt_amd.hparams import hparams
    from satt_amd.models.models import tacotron_model_factory
    ops.set_precision("f32")
    hp = hparams.copy()
    hp.parse_json(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "vctk",
                                    "self-attention-tacotron-resize.json")).read())
    m = tacotron_model_factory(hp, str(tmp_path))
    eng = m.engine
    assert eng.P["speaker_resize.W"].shape == (16, 64) and eng.P["dec.prenet0.Ws"].shape == (64, 256)
    gen = torch.Generator().manual_seed(1)
    eng.P["speaker_resize.W"].copy_(torch.randn(16, 64, generator=gen)); eng.P["speaker_resize.b"].copy_(torch.randn(64, generator=gen))
    keep = {k: eng.P[k].detach().cpu().clone() for k in RESIZE_NAMES}
    m.global_step = 3
    m.save()
    m2 = tacotron_model_factory(hp, str(tmp_path))
    assert m2.global_step == 3
    for k in RESIZE_NAMES:
        assert torch.equal(m2.engine.P[k].cpu(), keep[k]), k
    # a checkpoint of the model WITHOUT the layer has another layout and is refused by the existing size check
    hp.speaker_embedding_projection_out_dim = -1
    with pytest.raises(ValueError, match="parameter layout"):
        tacotron_model_factory(hp, str(tmp_path))


@pytest.mark.parametrize("kw", [dict(MEDIUM), dict(MEDIUM, **SPK)])
def test_default_configurations_never_enter_the_new_path(kw):
    """both hparams at -1: one train step and one infer give bit-identical outputs with the fused path enabled and disabled, and
    the new entry point is never called"""
    from satt_amd import _lib, ops
    from satt_amd.engine import Engine
    from satt_amd.inference import infer
    ops.set_precision("f32")
    cfg, P = make_params(kw, seed=4)
    batch = small_batch(cfg, 3, 17, 12, seed=8)
    if cfg.num_speakers:
        batch["speaker_id"] = np.array([226, 231, 226], np.int64)
    calls = []
    real_f = ops.speaker_cond_fwd
    ops.speaker_cond_fwd = lambda *a, **k: calls.append("fwd") or real_f(*a, **k)
    res = []
    try:
        for fused in (True, False):
            eng = Engine(cfg, "cuda", params=P, rng_seed=5)
            eng.fused_speaker = fused
            b = eng.to_device_batch(batch)
            ctx = eng.train_step(b)
            torch.cuda.synchronize()
            eng.check_clusters(ctx)
            assert ctx["spk"] is None or "src" not in ctx["spk"]
            out = infer(eng, b["source"], b["source_length"], max_steps=6, min_steps=1 << 30, speaker_id=b.get("speaker_id"))
            torch.cuda.synchronize()
            res.append((eng.outputs(ctx)["mel"].clone(), eng.grad.clone(), float(eng.losses[2]), out["mel"].clone()))
    finally:
        ops.speaker_cond_fwd = real_f
    assert not calls
    assert torch.equal(res[0][0], res[1][0]) and res[0][2] == res[1][2] and torch.equal(res[0][3], res[1][3])
    # (the gradient buffer holds float-atomic sums of other kernels: equal to rounding, as between any two runs of one build)
    assert float((res[0][1] - res[1][1]).abs().max()) <= 1e-6 * float(res[1][1].abs().max())


def test_speaker_kernel_runs_clean_under_lds_poison():
    """SATT_DEBUG_POISON_LDS: every LDS word the kernel reads was written by the same launch - the kernel test in a child
    process with a NaN pattern in every LDS word of every CU before each launch; the outputs must still meet their bars"""
    env = dict(os.environ, SATT_DEBUG_POISON_LDS="7fc00000")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "test_speaker_cond_kernel"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
