"""infer(stop="each"): free-running batches in which every utterance ends on its own (satt_dec_ends_scan behind every launch or
replay), end to end on all three decode paths - the persistent kernel at B = 2, its group mode at B = 3 .. 16, the hipGraph of
launch-per-layer steps for everything else - and step by step without a graph.

Every case first decodes the batch at full length (stop="each", min_steps out of reach) and takes the stop logits of that run.  The
threshold is then chosen ON THE HOST from the gaps of those values (decode_ends_common.pick_threshold) so that at least two samples end
at different steps, one end lies behind the first launch and no logit lies within 1e-3 of the threshold's logit - a condition on the
inputs; a case that cannot meet it fails.  The models are randomly initialised: their stop logits move by a few hundredths over a
run, so the stop column of the output projection is scaled by STOP_SCALE[model] - the sign is the one with which the logits RISE
behind min_steps (measured: the dual and the baseline model rise to a plateau around step 25, the VCTK model falls to one), so
that ends can lie in a later launch.  The stop logit is not fed back: the frames do not change.
The run with that threshold and min_steps = 10 must then end every sample where the NumPy model of the scan ends it on the full-length
logits, stop at the last of them, and return rows that are BIT-IDENTICAL to the full-length run's (same launch length in both runs;
tests/test_inference_gpu.py asserts run-to-run and graph-to-eager identity of the launch-per-layer path, so that path is held to
bits as well).  Every test of stop="each" fails on the parent, which has neither the argument nor the kernel."""
import contextlib

import numpy as np
import pytest
import torch

from decode_common import BASELINE, Engines, inputs, keys_of, traced_infer
from decode_ends_common import MARGIN, ends_of_logits, margin_ok, pick_threshold

pytestmark = pytest.mark.gpu

TD, K, MIN_STEPS = 48, 8, 10          # steps at the most, steps per launch on every path (the graph path: check_every)
STOP_SCALE = {"dual": 16.0, "baseline": 16.0, "vctk": -16.0}
MODELS = {"dual": dict(), "baseline": BASELINE,
          "vctk": dict(num_speakers=152, speaker_dim=16, speaker_offset=225, n_feed_frame=2)}          # examples/vctk/self-attention-tacotron.json
engines = Engines(MODELS)


def engine(model):
    if (model, False) not in engines._params:          # once per model, before its engine is built
        _, P = engines.params(model)
        W = np.array(P["dec.out.W"], dtype=np.float32).copy()
        W[:, -1] *= np.float32(STOP_SCALE[model])
        P["dec.out.W"] = W
    return engines(model)


@contextlib.contextmanager
def scans():
    """yields the list of (t0, nsteps) of the ops.dec_ends_scan calls made inside the body"""
    from satt_amd import ops
    real, calls = ops.dec_ends_scan, []

    def scan(yout, B, rows, NO, t0, nsteps, *rest):
        calls.append((int(t0), int(nsteps)))
        return real(yout, B, rows, NO, t0, nsteps, *rest)
    ops.dec_ends_scan = scan
    try:
        yield calls
    finally:
        ops.dec_ends_scan = real


def speakers(cfg, B):
    return dict(speaker_id=torch.as_tensor((np.arange(B) * 5 % 152 + 225).astype(np.int64))) if cfg.num_speakers else {}


PATHS = {"persistent": lambda s: s.mega is not None and s.mega_groups is None and s.graph is None,
         "groups": lambda s: s.mega_groups is not None and s.mega is None and s.graph is None,
         "graph": lambda s: s.graph is not None and s.mega is None and s.mega_groups is None,
         "eager": lambda s: s.graph is None and s.mega is None and s.mega_groups is None}


@pytest.mark.parametrize("model,B,Ti,path,sw,use_graph", [
    ("dual", 2, 33, "persistent", {}, True),
    ("dual", 3, 57, "groups", {}, True),                               # odd: the padding sample is not scanned
    ("dual", 5, 33, "groups", {}, True),
    ("dual", 16, 57, "groups", {}, True),                              # all eight XCDs, every wave of the scan takes four samples
    ("dual", 5, 57, "graph", dict(MEGA_GROUPS=False), True),
    ("dual", 17, 33, "graph", {}, True),                               # more samples than the group mode takes
    ("dual", 5, 33, "eager", {}, False),
    ("baseline", 5, 57, "groups", {}, True),
    ("vctk", 5, 57, "groups", {}, True)])
def test_each_utterance_ends_where_the_scan_of_the_full_run_ends_it(model, B, Ti, path, sw, use_graph):
    eng, cfg = engine(model)
    src, sl, _ = inputs(cfg, B, Ti, TD)
    sw = dict(MEGA_STEPS=K, MEGA_GROUPS_STEPS=K, **sw)
    kw = dict(max_steps=TD, stop="each", check_every=K, use_graph=use_graph, **speakers(cfg, B))
    full, ses_full, _ = traced_infer(eng, src, sl, sw, min_steps=10 ** 6, **kw)
    assert PATHS[path](ses_full) and ses_full.stop_each, path
    launch = ses_full.K
    assert launch == K          # (B = 2 takes the GROUP launch length, not MEGA_STEPS: the overshoot stays bounded)
    assert full["steps"] == TD and full["steps_each"].tolist() == [TD] * B and full["steps_each"].dtype == np.int64
    logits = full["stop"][:, :, 0].cpu().numpy()
    assert logits.shape == (B, TD)
    thr = pick_threshold(logits, MIN_STEPS, launch)
    assert thr is not None, "no gap of the stop logits gives two different ends with one behind the first launch"
    want = ends_of_logits(logits, MIN_STEPS, thr, TD)
    inside = want[want < TD]
    assert margin_ok(logits, thr) and len(set(inside.tolist())) >= 2 and inside.max() > launch          # the conditions on the inputs
    with scans() as scanned:
        cut, ses, launches = traced_infer(eng, src, sl, sw, min_steps=MIN_STEPS, stop_threshold=thr, **kw)
    assert PATHS[path](ses) and ses.stop_each and ses is not ses_full and ses.K == launch
    print("%s B=%d Ti=%d %s thr=%.6f steps_each=%s steps=%d scans=%s" % (model, B, Ti, path, thr, cut["steps_each"].tolist(), cut["steps"], scanned))
    assert cut["steps_each"].dtype == np.int64 and cut["steps_each"].tolist() == want.tolist()
    steps = cut["steps"]
    assert steps == int(want.max())
    # the windows tile the steps from 0 on, and the host is at most one launch behind the flag
    run = scanned[1:] if path in ("persistent", "groups") else scanned          # (in front: the warm-up launch of the new session)
    assert run[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(run[:-1], run[1:])), scanned
    done = run[-1][0] + run[-1][1]
    assert steps <= done <= min(TD, (-(-steps // launch) + 1) * launch), (steps, scanned)
    if path in ("persistent", "groups"):
        assert len(launches) == len(scanned) and {l.nsteps for l in launches} == {launch}
    r = cfg.r
    for k in keys_of(cfg):
        n = steps * r if k == "mel" else steps
        assert cut[k].shape[:2] == (B, n), (k, cut[k].shape)
        assert torch.equal(cut[k], full[k][:, :n]), k
    assert torch.isfinite(cut["mel"]).all()


def test_each_at_batch_one_is_the_rule_of_all():
    eng, cfg = engine("dual")
    src, sl, _ = inputs(cfg, 1, 33, TD)
    sw = dict(MEGA_STEPS=K)
    full, _, _ = traced_infer(eng, src, sl, sw, max_steps=TD, min_steps=10 ** 6)
    lg = full["stop"][:, :, 0].cpu().numpy()
    vals = np.unique(lg)          # a threshold in the widest gap of the logits that the sample crosses inside the run
    thr = None
    for gap, x in sorted(((hi - lo, 0.5 * (lo + hi)) for lo, hi in zip(vals[:-1], vals[1:])), reverse=True):
        t = float(np.float32(1.0 / (1.0 + np.exp(-x))))
        if gap >= 2.5 * MARGIN and margin_ok(lg, t) and MIN_STEPS + 1 < ends_of_logits(lg, MIN_STEPS, t, 0)[0] < TD:
            thr = t
            break
    assert thr is not None
    outs = {}
    for stop in ("all", "each"):
        with scans() as scanned:
            out, ses, launches = traced_infer(eng, src, sl, sw, max_steps=TD, min_steps=MIN_STEPS, stop_threshold=thr, stop=stop)
        assert not scanned and not ses.stop_each and ses.mega is not None and ses.K == K
        outs[stop] = (out, ses)
    a, e = outs["all"][0], outs["each"][0]
    assert outs["each"][1] is outs["all"][1]          # the SAME session: at B = 1 the key says "all"
    assert a["steps"] == e["steps"] == int(ends_of_logits(lg, MIN_STEPS, thr, TD)[0]) < TD
    assert e["steps_each"].tolist() == [e["steps"]] and "steps_each" not in a
    for k in keys_of(cfg):
        assert a[k].cpu().numpy().tobytes() == e[k].cpu().numpy().tobytes(), k


@pytest.mark.parametrize("B,name", [(2, "dec_mega"), (4, "dec_mega_groups"), (17, None)])
def test_stop_all_launches_what_it_launched_before(B, name):
    """the default and stop="all" are one call: the same session, the launches of the batch rule, no per-utterance scan"""
    from satt_amd.inference import DecodeSession
    eng, cfg = engine("dual")
    src, sl, _ = inputs(cfg, B, 33, 24)
    res = []
    for kw in ({}, dict(stop="all")):
        with scans() as scanned:
            out, ses, launches = traced_infer(eng, src, sl, {}, max_steps=24, min_steps=10 ** 6, **kw)
        assert not scanned and not ses.stop_each and ses.ends is None and "steps_each" not in out and out["steps"] == 24
        res.append((ses, [l.name for l in launches]))
    assert res[0][0] is res[1][0]
    ses, names = res[1]
    want = DecodeSession.MEGA_STEPS if B == 2 else DecodeSession.MEGA_GROUPS_STEPS if B == 4 else 8
    assert ses.K == want and set(names) == ({name} if name else set())
    assert len(names) == (0 if name is None else -(-24 // want))
    if B == 2:          # the in-kernel rule is still wired: the block carries the flag
        assert ses.mega.flag


def test_stop_each_is_free_running_only():
    from satt_amd.inference import infer
    eng, cfg = engine("dual")
    src, sl, mel = inputs(cfg, 3, 33, 12)
    ta = torch.full((3, 12, 33), 1.0 / 33)
    with pytest.raises(ValueError):
        infer(eng, src, sl, teacher=mel, stop="each")
    with pytest.raises(ValueError):
        infer(eng, src, sl, max_steps=12, teacher_alignments=(ta, ta), stop="each")
    with pytest.raises(ValueError):
        infer(eng, src, sl, max_steps=12, stop="every")
