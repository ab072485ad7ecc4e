"""The single-workgroup attention kernels (csrc/attn_rnn.hip) as the GENERAL training path: attention=location_sensitive,
cumulative_weights and the transition agent on `use_clusters = False` and on problems the cluster kernels decline, and bf16
sentences whose key image does not fit LDS (keys read from global memory, rounded on load).  Against the float64 oracle
with dropout / zoneout on, at the bars the same comparisons have on the cluster path."""
import functools

import numpy as np
import pytest
import torch

from common import MEDIUM, SMALL, make_params, oracle_run, rel_err, small_batch
from test_model_gpu import report, run_engine, run_engine_chunked

pytestmark = pytest.mark.gpu

FWD_KEYS = ["lstm_out", "sa_out", "alignment1", "alignment2", "dec_out", "mel", "stop", "loss", "mel_loss", "done_loss"]
OPTIONS = {
    "location_sensitive": dict(attention="location_sensitive"),
    "location_sensitive+cumulative": dict(attention="location_sensitive", cumulative_weights=True),
    "forward+cumulative": dict(cumulative_weights=True),
    "agent": dict(transition_agent=True),
    "agent+cumulative": dict(transition_agent=True, cumulative_weights=True),
}
SIZES = {"small": SMALL, "medium": MEDIUM}


@functools.lru_cache(maxsize=None)
def problem(size, option, B, Ti, Tm):
    """config, parameters, batch, alignment gradients and the float64 reference of one case (computed once, shared, never written)"""
    kw = dict(SIZES[size], **OPTIONS[option])
    cfg, P = make_params(kw, seed=31)
    if "agent" in option:
        P["dec.att1.Wa"] = (3.0 * P["dec.att1.Wa"]).astype(np.float32)        # move u well away from 0.5
    batch = small_batch(cfg, B, Ti, Tm, seed=77)
    g = np.random.default_rng(4)
    Td = Tm // cfg.r
    dal = (g.normal(0, 0.05, (B, Td, Ti)), g.normal(0, 0.05, (B, Td, Ti)))
    ref, col, gref = oracle_run(kw, P, batch, True, seed=33, dalign=dal)
    return cfg, P, batch, dal, {**ref, "dec_out": col["dec_out"]}, gref


def assert_parity(out, ref, grads, gref, bar=2e-4):
    errs = report(out, ref, grads, gref, FWD_KEYS)
    bad = {k: e for k, e in errs.items() if not (e < bar)}
    assert not bad, bad


def assert_option_state(eng, out, option, agent_moved=True):
    ctx = eng.last_ctx
    if option.startswith("location_sensitive"):      # the returned alignments ARE the softmax probabilities
        assert np.allclose(out["alignment1"], ctx["a1"].cpu().numpy(), atol=1e-6)
    if "agent" in option and agent_moved:
        us = ctx["ustate"][:, 1:].float().cpu().numpy()
        print("max |u - 0.5| = %.3f" % np.abs(us - 0.5).max())
        assert np.abs(us - 0.5).max() > 0.02, "the agent never moved the transition probability"


@pytest.mark.parametrize("option", list(OPTIONS))
@pytest.mark.parametrize("size,B,Ti,Tm", [("medium", 5, 37, 46), ("small", 3, 9, 12)])
def test_f32_parity_on_the_single_workgroup_kernels(size, B, Ti, Tm, option):
    """ragged lengths, Ti no multiple of the wave-row stride (37) / fewer rows than waves (9): every forward tensor and every
    parameter gradient, non-zero gradients on both alignments"""
    cfg, P, batch, dal, ref, gref = problem(size, option, B, Ti, Tm)
    eng, out, grads = run_engine(cfg, P, batch, 33, "f32", dalign=dal, clusters=False)
    assert eng.last_ctx["att_cluster"][0] == 0
    assert_option_state(eng, out, option)
    assert_parity(out, ref, grads, gref)


# gradients that attn_param_grads_k adds with fp32 atomics in ARRIVAL order (both families use it in exact-fp32 mode)
ATOMIC_SUMS = ("dec.att1.v", "dec.att1.b", "dec.att1.U", "dec.att2.v")


@pytest.mark.parametrize("option", ["location_sensitive", "forward+cumulative", "agent"])
def test_both_kernel_families_agree(option):
    """cluster kernels against single-workgroup kernels on one batch, f32.  Every gradient agrees to 1e-5 (the bar of the
    chunked-versus-unchunked comparison) - except the four tensors of ATOMIC_SUMS, whose bar is 2e-5: they are heavily
    cancelling sums added with fp32 atomics in arrival order, so each RUN carries its own noise.  Measured on one MI355X, worst
    of those tensors, three repeats: two runs of the SAME single-workgroup kernels differ by up to 5.4e-6 (agent; plain forward
    at the parent commit: 2.6e-6), so two independent runs can differ by about 1e-5 through the atomics alone, on top of the
    1e-5 allowed between the families.  Measured between the families: agent 7.7e-6 .. 8.4e-6, location_sensitive 2.7e-6 ..
    3.8e-6, forward+cumulative 3.2e-6 .. 4.1e-6; plain forward on the same batch 4.4e-6 .. 5.8e-6 (parent commit: 4.8e-6 ..
    5.9e-6).  Every other tensor measured below 3.3e-6."""
    cfg, P, batch, dal, ref, gref = problem("medium", option, 8, 29, 34)
    e1, o1, g1 = run_engine(cfg, P, batch, 33, "f32", dalign=dal, clusters=True)
    assert e1.last_ctx["att_cluster"][0] > 0
    e2, o2, g2 = run_engine(cfg, P, batch, 33, "f32", dalign=dal, clusters=False)
    assert e2.last_ctx["att_cluster"][0] == 0
    errs = {k: rel_err(g2[k], g1[k]) for k in g1}
    for k, e in sorted(errs.items(), key=lambda kv: -kv[1])[:8]:
        print("%-28s rel_err=%.3e" % (k, e))
    bad = {k: e for k, e in errs.items() if not (e < (2e-5 if k in ATOMIC_SUMS else 1e-5))}
    assert not bad, bad


def test_chunked_schedule_on_the_single_workgroup_kernels(monkeypatch):
    """agent + cumulative through the chunked-launch driver with the cluster kernels off: the single-workgroup kernels walk all
    steps in ONE launch whatever the pipeline settings (d u and the accumulated conv-input gradient never leave the kernel), so
    the gradients equal the plain run's"""
    from satt_amd.engine import Engine
    cfg, P, batch, dal, ref, gref = problem("medium", "agent+cumulative", 8, 29, 34)
    eng, out, grads = run_engine(cfg, P, batch, 33, "f32", dalign=dal, clusters=False)
    monkeypatch.setattr(Engine, "use_clusters", False)
    eng2, _, grads2 = run_engine_chunked(cfg, P, batch, 33, dal)
    assert eng2.use_clusters is False
    errs = {k: rel_err(grads2[k], grads[k]) for k in grads}
    print("worst: %s" % (max(errs.items(), key=lambda kv: kv[1]),))
    bad = {k: e for k, e in errs.items() if not (e < 1e-5)}
    assert not bad, bad
    assert_parity(out, ref, grads, gref)


@pytest.mark.parametrize("option", ["location_sensitive", "agent+cumulative"])
def test_a_sentence_the_cluster_kernels_decline(option):
    """Ti = 400 > 384 memory rows: `use_clusters` stays at its default and the engine falls back by itself"""
    cfg, P, batch, dal, ref, gref = problem("medium", option, 2, 400, 8)
    eng, out, grads = run_engine(cfg, P, batch, 33, "f32", dalign=dal, clusters=True)
    assert eng.use_clusters and eng.last_ctx["att_cluster"][0] == 0, "the cluster path was taken"
    assert_option_state(eng, out, option, agent_moved=False)      # (4 decoder steps: too few for u to travel)
    assert_parity(out, ref, grads, gref)


# ---- bf16: the LDS-key rule
def lds_bytes(cfg, Ti, backward, klds, F=5, ANT=512):
    """carve_fwd / carve_bwd of csrc/attn_rnn.hip in bytes"""
    u = lambda x: (x + 3) & ~3
    A, CT, UQ, KW = cfg.att_rnn_units, cfg.cbhg_out_units + cfg.sa_units, cfg.att1_units + cfg.att2_units, cfg.att_kernel
    if backward:
        o = 4 * A + u(CT + A) + u(A) + 2 * u(UQ) + u(CT) + 9 * u(Ti) + 2 * u(Ti * F) + u(KW * F) + ANT * 8 + 4
    else:
        o = u(CT + A) + 4 * A + u(A) + u(UQ) + 5 * u(Ti) + u(Ti * F) + u(KW * F) + u(F) + ANT * 8
    return 4 * (o + (u((Ti * UQ + 1) // 2) if klds else 0))


@pytest.mark.parametrize("Ti", [64, 400])
def test_bf16_parity_keys_in_lds_and_keys_from_global(Ti):
    """production widths (U1 + U2 = 256), plain forward attention, cluster kernels off.  Ti = 64: the bf16 keys are staged in LDS.
    Ti = 400: their image (400 x 256 x 2 = 204800 bytes alone) is over the 160 KB limit, the kernels read them from global
    memory and round them on load.  Same bars as test_bf16_parity_baseline_tacotron_production_dims."""
    kw = dict()
    cfg, P = make_params(kw, seed=31)
    over = max(lds_bytes(cfg, Ti, False, True), lds_bytes(cfg, Ti, True, True)) > 160 * 1024
    assert over == (Ti == 400)
    assert lds_bytes(cfg, Ti, True, False) <= 160 * 1024
    batch = small_batch(cfg, 2, Ti, 8, seed=32)
    ref, col, gref = oracle_run(kw, P, batch, True, seed=33)
    eng, out, grads = run_engine(cfg, P, batch, 33, "bf16", clusters=False)
    assert eng.last_ctx["att_cluster"][0] == 0
    errs = report(out, {**ref, "dec_out": col["dec_out"]}, grads, gref,
                  ["lstm_out", "alignment1", "alignment2", "dec_out", "mel", "stop", "loss", "mel_loss", "done_loss"])
    assert errs["mel"] < 5e-2 and errs["alignment1"] < 5e-2 and errs["alignment2"] < 5e-2
    bad = {}
    for k in grads:
        a, b = grads[k].astype(np.float64).ravel(), gref[k].astype(np.float64).ravel()
        cos = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))
        l2 = float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))
        print("%-28s cos=%.5f l2=%.4f" % (k, cos, l2))
        if not (cos > 0.98 and l2 < 0.2):
            bad[k] = (cos, l2)
    assert not bad, bad


def test_global_keys_rounded_on_load_equal_the_lds_image_bit_for_bit(monkeypatch):
    """the two bf16 key forms of the loop kernels on the same inputs, at a length where both can be launched
    (SATT_ATTN_RNN_GLOBAL_KEYS, read at every call, forces the global form): every output of both passes is bit-identical"""
    from satt_amd import ops
    from satt_amd.engine import Engine
    cfg, P = make_params(dict(), seed=31)
    batch = small_batch(cfg, 2, 64, 8, seed=32)
    ops.set_precision("bf16")
    eng = Engine(cfg, "cuda", params=P, rng_seed=33)
    eng.use_clusters = False
    ctx = eng.forward(eng.to_device_batch(batch), training=True)
    ap = ctx["att_params"]
    assert ap.keys_lds_bf16 == 1 and ctx["att_cluster"][0] == 0
    B, Ti, Td, _ = ctx["dims"]
    A, CT, UQ = cfg.att_rnn_units, cfg.cbhg_out_units + cfg.sa_units, cfg.att1_units + cfg.att2_units
    fwd_outs = [ctx[k] for k in ("att_out", "al1", "al2", "a1", "pq", "flb")] + list(ctx["att_saved"])
    g = torch.Generator(device="cuda").manual_seed(5)
    # (the engine does not keep the cell's input projection beyond its forward pass: a stand-in that this test owns)
    xg = 0.5 * torch.randn(B * Td, 4 * A, device="cuda", generator=g)
    ap.xg = xg.data_ptr()
    dout = 0.1 * torch.randn(B * Td, A + CT, device="cuda", generator=g)
    dal1, dal2 = (0.05 * torch.randn(B, Td, Ti, device="cuda", generator=g) for _ in range(2))
    names = ("dxg", "dctx", "dpq", "de1", "de2", "dfl")
    shapes = ((B * Td, 4 * A), (B * Td, CT), (B * Td, UQ), (B, Td, Ti), (B, Td, Ti), (B * Td * Ti, cfg.att_filters))

    def both_passes():
        for t in fwd_outs:
            t.fill_(float("nan"))
        ops.attn_rnn_fwd(ap)
        bw = {n: torch.full(s, float("nan"), device="cuda") for n, s in zip(names, shapes)}
        ops.attn_rnn_bwd(ap, WrecT=eng.shadow["att.Wrec.T"], WqT=eng.shadow["att.Wq.T"], dout=dout, dalign1=dal1, dalign2=dal2, **bw)
        torch.cuda.synchronize()
        return [t.clone() for t in fwd_outs] + [bw[n] for n in names]

    monkeypatch.delenv("SATT_ATTN_RNN_GLOBAL_KEYS", raising=False)
    lds = both_passes()
    monkeypatch.setenv("SATT_ATTN_RNN_GLOBAL_KEYS", "1")
    glob = both_passes()
    for i, (x, y) in enumerate(zip(lds, glob)):
        assert bool(torch.isfinite(x).all()), i
        assert torch.equal(x, y), (i, float((x - y).abs().max()))
