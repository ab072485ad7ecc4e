"""GPU tests of speaker_embedd_to_decoder (the speaker vector concatenated to both attention memories, reference
models/models.py:366-372): the two kernels of csrc/speaker_cond.hip against float64 torch, the full model (forward, every parameter
gradient) against the float64 composition of spk_decoder_common.py, the step-0 rule, speaker_for_synthesis, decoding, the untouched
flag-off path, LDS discipline."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import spk_decoder_common as sd
from common import MEDIUM, make_params, rel_err, small_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPK = dict(num_speakers=7, speaker_dim=16, speaker_offset=225)
WIDE = ("dec.att1.Wm", "dec.att2.Wm", "dec.att_lstm.W", "dec.lstm1.W")

# (B, T, N, t0): one element; odd sizes with t0 = 1; the test width 16; the shipped gate width, more than one wave of time steps,
# t0 = 1; a width that is no multiple of 4 (the one-float-per-lane form) over more than one 64-column workgroup
SHAPES = [(1, 1, 4, 0), (3, 7, 72, 1), (2, 5, 16, 0), (4, 33, 1024, 1), (3, 9, 1030, 0)]


def _padded(rows, N, pad, gen):
    """a [rows, N] view with leading dimension N + pad of a buffer filled with a sentinel"""
    buf = torch.full((rows, N + pad), 7.0)
    buf[:, :N] = torch.randn(rows, N, generator=gen)
    return buf


@pytest.mark.parametrize("pad", [0, 8, 3])
@pytest.mark.parametrize("B,T,N,t0", SHAPES)
def test_rows_bcast_add(B, T, N, t0, pad):
    """y[b, t, :] += v[b, :] for t >= t0 is ONE fp32 addition per element: equal, to the bit, to the float64 sum rounded to fp32.
    Rows below t0 and the pad columns of a padded leading dimension stay as they were (pad 3 breaks the 16-byte rows)."""
    from satt_amd import ops
    g = torch.Generator().manual_seed(B * 100 + N)
    yh, vh = _padded(B * T, N, pad, g), _padded(B, N, pad, g)
    y, v = yh.to(DEV), vh.to(DEV)
    ops.rows_bcast_add(y[:, :N], v[:, :N], B, T, t0=t0)
    torch.cuda.synchronize()
    want = yh.clone().double().view(B, T, N + pad)
    want[:, t0:, :N] += vh[:, None, :N].double()
    assert torch.equal(y.cpu(), want.float().view(B * T, N + pad))
    # a chunk of the range
    if T > 2:
        y2 = yh.to(DEV)
        ops.rows_bcast_add(y2[:, :N], v[:, :N], B, T, t0=1, t1=T - 1)
        want = yh.clone().double().view(B, T, N + pad)
        want[:, 1:T - 1, :N] += vh[:, None, :N].double()
        assert torch.equal(y2.cpu(), want.float().view(B * T, N + pad))


@pytest.mark.parametrize("pad", [0, 8, 3])
@pytest.mark.parametrize("B,T,N,t0", SHAPES)
def test_rows_time_sum(B, T, N, t0, pad):
    """dv[b, :] = sum over t0 <= t < min(T, len_b) against float64 at 1e-6 (an fp32 sum of <= 33 terms in a fixed tree: a few ulp);
    with and without lengths (one sample of length 1, one of full length); two runs are bit-equal"""
    from satt_amd import ops
    g = torch.Generator().manual_seed(B * 100 + N + 1)
    dyh = _padded(B * T, N, pad, g)
    dy = dyh.to(DEV)
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0] = 1
    lens[-1] = T
    for L in (None, lens):
        outs = []
        for _ in range(2):
            dv = torch.full((B, N + pad), 5.0, device=DEV)
            ops.rows_time_sum(dy[:, :N], None if L is None else L.to(DEV), dv[:, :N], B, T, t0=t0)
            torch.cuda.synchronize()
            outs.append(dv.cpu())
        assert torch.equal(outs[0], outs[1])
        assert bool((outs[0][:, N:] == 5.0).all())
        want = torch.zeros(B, N, dtype=torch.float64)
        x = dyh.double().view(B, T, N + pad)
        for b in range(B):
            te = T if L is None else int(L[b])
            want[b] = x[b, t0:te, :N].sum(0)
        err = float((outs[0][:, :N].double() - want).abs().max() / (want.abs().max() + 1e-12))
        print("B=%d T=%d N=%d t0=%d pad=%d lengths=%s rel_err=%.3e" % (B, T, N, t0, pad, L is not None, err))
        assert err < 1e-6


def test_empty_range():
    """t0 = 1 with T = 1: the add leaves y unchanged, the sum is zeros"""
    from satt_amd import ops
    y = torch.randn(3, 16, device=DEV); v = torch.randn(3, 16, device=DEV)
    y0 = y.clone()
    ops.rows_bcast_add(y, v, 3, 1, t0=1)
    dv = torch.full((3, 16), 5.0, device=DEV)
    ops.rows_time_sum(y, None, dv, 3, 1, t0=1)
    torch.cuda.synchronize()
    assert torch.equal(y, y0) and not dv.any()


# ------------------------------------------------------------------------------------------------ the model
def _batch(cfg, B, Ti, Tm, seed, ids):
    batch = small_batch(cfg, B, Ti, Tm, seed=seed)
    batch["source_length"] = np.asarray(batch["source_length"]).copy()
    batch["source_length"][0] = Ti                          # a full-length sample ...
    batch["source_length"][1] = max(2, Ti // 2)             # ... and one of the minimum: the masked-row reduction matters
    batch["speaker_id"] = np.asarray(ids, np.int64)
    return batch


def run_engine(cfg, P, batch, seed):
    from satt_amd import ops
    from satt_amd.engine import Engine
    ops.set_precision("f32")
    eng = Engine(cfg, "cuda", params=P, rng_seed=seed)
    b = eng.to_device_batch(batch)
    eng.zero_grad()
    ctx = eng.forward(b, training=True)
    eng.backward(ctx)
    torch.cuda.synchronize()
    eng.check_clusters(ctx)
    out = {k: v.detach().float().cpu().numpy() for k, v in eng.outputs(ctx).items() if v is not None}
    grads = {k: v.detach().cpu().numpy() for k, v in eng.G.items()}
    return eng, ctx, out, grads


def _speaker_rows(cfg, name):
    V1, V2, S, A, pn = cfg.cbhg_out_units, cfg.sa_units, cfg.mem_speaker, cfg.att_rnn_units, cfg.dec_prenet[-1]
    if name == "dec.att1.Wm":
        return [slice(V1, V1 + S)]
    if name == "dec.att2.Wm":
        return [slice(V2, V2 + S)]
    lead = pn if name == "dec.att_lstm.W" else A
    return [slice(lead + V1, lead + V1 + S), slice(lead + V1 + S + V2, lead + V1 + V2 + 2 * S)]


@pytest.mark.parametrize("rdim", [-1, 24])
def test_f32_parity_speaker_to_decoder(rdim):
    """FAILS ON THE PARENT (which refuses the configuration).  Full model, dropout and zoneout on: mel, stop, both alignments, the
    loss and EVERY parameter gradient against the float64 composition; cases and bar (2e-4) of test_f32_parity_multi_speaker_vctk /
    test_f32_parity_resize_layer: MEDIUM, 7 speakers, B = 4, Ti = 21, Tm = 26; S = 16 (the embedding) and S = 24 (the resize layer)"""
    cfg_kw = dict(MEDIUM, **SPK, speaker_proj_dim=rdim, speaker_to_decoder=True)
    cfg, P = make_params(cfg_kw, seed=4)
    assert cfg.mem_speaker == (16 if rdim < 0 else 24)
    ids = np.random.default_rng(1).integers(0, 7, 4) + 225
    ids[-1] = ids[0]                                        # a duplicate
    batch = _batch(cfg, 4, 21, 26, 8, ids)
    ref, col, gref = sd.composed_run(cfg_kw, P, batch, True, seed=13)
    eng, ctx, out, grads = run_engine(cfg, P, batch, 13)
    rows = [(k, rel_err(out[k], ref[k].detach().numpy())) for k in ("mel", "stop", "alignment1", "alignment2", "loss")]
    rows += [("grad:" + k, rel_err(grads[k], gref[k])) for k in grads]
    for name in WIDE:           # the speaker rows on their own scale (they are smaller than the tensor's largest entries)
        for i, sl in enumerate(_speaker_rows(cfg, name)):
            rows.append(("grad:%s[speaker rows %d]" % (name, i), rel_err(grads[name][sl], gref[name][sl])))
            assert float(np.abs(grads[name][sl]).max()) > 0, name
    for k, e in rows:
        print("%-44s rel_err=%.3e" % (k, e))
    bad = {k: e for k, e in rows if not (e < 2e-4)}
    assert not bad, bad
    assert float(np.abs(grads["speaker_embedding"]).max()) > 0


def test_f32_parity_vctk_example_shape():
    """examples/vctk/self-attention-tacotron-spk-decoder.json itself (152 speakers, S = 16, the compile-time specialised cluster
    kernels, the folded first context, the chunked layer pipeline), B = 8, Ti = 21, Tm = 26: the case and bar (2e-4) that
    test_f32_parity_resize_layer holds its own example to"""
    cfg_kw = dict(num_speakers=152, speaker_dim=16, speaker_offset=225, speaker_to_decoder=True)
    cfg, P = make_params(cfg_kw, seed=4)
    ids = np.random.default_rng(1).integers(0, 152, 8) + 225
    ids[-1] = ids[0]
    batch = _batch(cfg, 8, 21, 26, 8, ids)
    ref, col, gref = sd.composed_run(cfg_kw, P, batch, True, seed=13)
    eng, ctx, out, grads = run_engine(cfg, P, batch, 13)
    rows = [(k, rel_err(out[k], ref[k].detach().numpy())) for k in ("mel", "stop", "alignment1", "alignment2", "loss")]
    rows += [("grad:" + k, rel_err(grads[k], gref[k])) for k in grads]
    for name in WIDE:
        for i, sl in enumerate(_speaker_rows(cfg, name)):
            rows.append(("grad:%s[speaker rows %d]" % (name, i), rel_err(grads[name][sl], gref[name][sl])))
    for k, e in rows:
        print("%-44s rel_err=%.3e" % (k, e))
    print("attention cluster size %d, LSTM cluster size %d, pipeline chunks %d" % (ctx["att_cluster"][0], ctx["cluster"][0], ctx["chunks"]))
    bad = {k: e for k, e in rows if not (e < 2e-4)}
    assert not bad, bad


def _forward_only(eng, b):
    ctx = eng.forward(b, training=True)
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in eng.outputs(ctx).items() if k in ("mel", "alignment1", "alignment2")}


def test_step_zero_gets_no_speaker_term():
    """the attention LSTM of step 0 reads the all-zero initial attention, speaker columns included: a Td = 1 batch equals the
    composed reference (bar of the parity test); on a Td = 3 batch, perturbing ONLY the speaker rows of dec.att_lstm.W leaves step
    0's alignment1 bit-identical and changes step 1's"""
    from satt_amd import ops
    from satt_amd.engine import Engine
    ops.set_precision("f32")
    cfg_kw = dict(MEDIUM, **SPK, speaker_to_decoder=True)
    cfg, P = make_params(cfg_kw, seed=4)
    one = _batch(cfg, 3, 13, cfg.r, 8, [226, 231, 226])
    ref, _, gref = sd.composed_run(cfg_kw, P, one, True, seed=5)
    eng, ctx, out, grads = run_engine(cfg, P, one, 5)
    for k in ("mel", "stop", "alignment1", "alignment2", "loss"):
        e = rel_err(out[k], ref[k].detach().numpy())
        print("Td=1 %-12s rel_err=%.3e" % (k, e))
        assert e < 2e-4, (k, e)
    for i, sl in enumerate(_speaker_rows(cfg, "dec.att_lstm.W")):
        assert not grads["dec.att_lstm.W"][sl].any()          # no step >= 1: the rows receive nothing
    assert rel_err(grads["dec.lstm1.W"], gref["dec.lstm1.W"]) < 2e-4
    three = _batch(cfg, 3, 13, 3 * cfg.r, 8, [226, 231, 226])
    eng = Engine(cfg, "cuda", params=P, rng_seed=5)
    b = eng.to_device_batch(three)
    base = _forward_only(eng, b)
    for sl in _speaker_rows(cfg, "dec.att_lstm.W"):
        eng.P["dec.att_lstm.W"][sl] += 0.5
    eng.refresh_shadows()
    moved = _forward_only(eng, b)
    assert torch.equal(moved["alignment1"][:, 0], base["alignment1"][:, 0])
    assert not torch.equal(moved["alignment1"][:, 1], base["alignment1"][:, 1])


def _teacher_infer(eng, b, spk):
    from satt_amd.inference import infer
    out = infer(eng, b["source"], b["source_length"], teacher=b["mel"], speaker_id=spk)
    torch.cuda.synchronize()
    return {k: out[k].detach().clone() for k in ("mel", "stop", "alignment1", "alignment2")}


def test_speaker_for_synthesis_reaches_the_memories():
    """ids [a, b] with speaker_for_synthesis = c give, to the bit, what ids [c, c] give with the hparam unset - in a training
    forward and in a teacher-fed infer - and not what [a, b] give"""
    from satt_amd import ops
    from satt_amd.engine import Engine
    ops.set_precision("f32")
    a, b_, c_ = 226, 231, 229
    kw = dict(MEDIUM, **SPK, speaker_to_decoder=True)
    cfg, P = make_params(kw, seed=4)
    cfg_c, _ = make_params(dict(kw, speaker_for_synthesis=c_), seed=4)
    batch = small_batch(cfg, 2, 17, 12, seed=8)
    plain = Engine(cfg, "cuda", params=P, rng_seed=5)
    forced = Engine(cfg_c, "cuda", params=P, rng_seed=5)
    ab, cc = np.array([a, b_], np.int64), np.array([c_, c_], np.int64)
    # (the infer calls first: a training forward moves the BatchNorm statistics that evaluation reads)
    b = plain.to_device_batch(batch)
    iw = _teacher_infer(plain, b, torch.as_tensor(cc, device=DEV))
    io = _teacher_infer(plain, b, torch.as_tensor(ab, device=DEV))
    ig = _teacher_infer(forced, b, torch.as_tensor(ab, device=DEV))
    for k in iw:
        assert torch.equal(ig[k], iw[k]), k
    assert not torch.equal(ig["mel"], io["mel"])
    want = _forward_only(plain, plain.to_device_batch(dict(batch, speaker_id=cc)))
    other = _forward_only(plain, plain.to_device_batch(dict(batch, speaker_id=ab)))
    got = _forward_only(forced, forced.to_device_batch(dict(batch, speaker_id=ab)))
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert not torch.equal(got["alignment1"], other["alignment1"])


@pytest.mark.parametrize("rdim", [-1, 24])
def test_decode_against_the_composed_reference(rdim):
    """teacher-fed infer and a 9-step free run, B = 3, Ti = 13, against the composed reference in evaluation mode at the bar of
    tests/test_inference_gpu.py (5e-4); forced-alignment mode reproduces the alignments it is given and depends on the speaker"""
    from satt_amd import ops
    from satt_amd.engine import Engine
    from satt_amd.inference import infer
    ops.set_precision("f32")
    kw = dict(MEDIUM, **SPK, speaker_proj_dim=rdim, speaker_to_decoder=True)
    cfg, P = make_params(kw, seed=6)
    B, Ti, steps = 3, 13, 9
    ids = np.array([231, 225, 231], np.int64)
    batch = _batch(cfg, B, Ti, steps * cfg.r, 2, ids)
    eng = Engine(cfg, "cuda", params=P, rng_seed=5)
    mv = {n: (m.double().cpu(), v.double().cpu()) for n, (m, v) in eng.bn.items()}
    b = eng.to_device_batch(batch)
    reft = sd.composed_infer(kw, P, batch, mv, teacher=True)
    reff = sd.composed_infer(kw, P, batch, mv, steps=steps)
    outt = infer(eng, b["source"], b["source_length"], teacher=b["mel"], speaker_id=b["speaker_id"])
    outf = infer(eng, b["source"], b["source_length"], max_steps=steps, min_steps=10 ** 6, speaker_id=b["speaker_id"])
    torch.cuda.synchronize()
    assert outf["steps"] == steps
    for k in ("mel", "stop", "alignment1", "alignment2"):
        et, ef = rel_err(outt[k].cpu().numpy(), reft[k].numpy()), rel_err(outf[k].cpu().numpy(), reff[k].numpy())
        print("%-12s teacher-fed rel_err=%.3e free run rel_err=%.3e" % (k, et, ef))
        assert et < 5e-4 and ef < 5e-4, (k, et, ef)
    second = infer(eng, b["source"], b["source_length"], max_steps=steps, min_steps=1 << 30, speaker_id=b["speaker_id"],
                   teacher_alignments=(outt["alignment1"], outt["alignment2"]))
    other = infer(eng, b["source"], b["source_length"], max_steps=steps, min_steps=1 << 30,
                  speaker_id=torch.as_tensor(np.array([226, 226, 226]), device=DEV),
                  teacher_alignments=(outt["alignment1"], outt["alignment2"]))
    torch.cuda.synchronize()
    assert torch.isfinite(second["mel"]).all() and not torch.equal(second["mel"], other["mel"])
    assert rel_err(second["alignment1"].cpu().numpy(), outt["alignment1"].cpu().numpy()) < 1e-6
    assert rel_err(second["alignment2"].cpu().numpy(), outt["alignment2"].cpu().numpy()) < 1e-6


@pytest.mark.parametrize("kw", [dict(MEDIUM), dict(MEDIUM, **SPK)])
def test_flag_off_never_enters_the_new_path(kw):
    """the default LJSpeech-like and VCTK-like configurations: a train step and an infer call neither of the two new entry points,
    the engine keeps no narrow copies, and the cell kernels the recurrent code reads ARE the parameters (same pointers)"""
    from satt_amd import ops
    from satt_amd.engine import Engine
    from satt_amd.inference import infer
    ops.set_precision("f32")
    cfg, P = make_params(kw, seed=4)
    batch = small_batch(cfg, 3, 17, 12, seed=8)
    if cfg.num_speakers:
        batch["speaker_id"] = np.array([226, 231, 226], np.int64)
    calls = []
    real = ops.rows_bcast_add, ops.rows_time_sum
    ops.rows_bcast_add = lambda *a, **k: calls.append("add") or real[0](*a, **k)
    ops.rows_time_sum = lambda *a, **k: calls.append("sum") or real[1](*a, **k)
    try:
        eng = Engine(cfg, "cuda", params=P, rng_seed=5)
        b = eng.to_device_batch(batch)
        ctx = eng.train_step(b)
        eng.optimizer_step()
        infer(eng, b["source"], b["source_length"], max_steps=6, min_steps=1 << 30, speaker_id=b.get("speaker_id"))
        torch.cuda.synchronize()
        eng.check_clusters(ctx)
    finally:
        ops.rows_bcast_add, ops.rows_time_sum = real
    assert not calls
    assert eng._ms == 0 and not eng._nw and not eng._spk_w
    for n in ("dec.att_lstm.W", "dec.lstm1.W"):
        assert eng.Pd(n).data_ptr() == eng.P[n].data_ptr() and eng.Wd(n) is eng.W(n)
    assert ctx["spk"] is None or "dec" not in ctx["spk"]


def test_runs_clean_under_lds_poison():
    """SATT_DEBUG_POISON_LDS: every LDS word a kernel reads was written by the same launch - the sum kernel's tests and one train
    step with the flag on (the S = 16 parity case) in a child process with a NaN pattern in every LDS word before each launch"""
    env = dict(os.environ, SATT_DEBUG_POISON_LDS="7fc00000")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "test_rows_time_sum or test_f32_parity_speaker_to_decoder and not 24"], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
