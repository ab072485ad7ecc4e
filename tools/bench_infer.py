#!/usr/bin/env python
"""BASELINE.json config 5: free-running decode (B=1, Ti=100, LJSpeech config) - decoder steps per second.
--hparams-json: another model, e.g. examples/vctk/self-attention-tacotron.json (speaker ids: the first B of the table).
--hparams "k=v,...": overrides on top of it (on the LJSpeech example's file when no --hparams-json is given), e.g.
use_forward_attention_transition_agent=True or apply_dropout_on_inference=True.
--batch 3 .. 16 takes the persistent kernel in group mode (one pair of samples per XCD); --no-groups: the hipGraph of launch-per-layer
steps such batches ran on before.
--forced: forced-alignment synthesis (infer(..., teacher_alignments=...), the second pass of predict_mel.py's
use_forced_alignment_mode): one free-running utterance produces the alignments, the timed utterances replay them.
--forced --batch 3 .. 16: the forced instantiations in group mode (path "persistent, groups, forced"); --no-groups returns it to the
hipGraph path as well.
--stop-each: the per-utterance stop rule (infer(..., stop="each"): satt_dec_ends_scan behind every launch; B = 2 takes launches of
MEGA_GROUPS_STEPS steps) with min_steps out of reach like every run here, so both rules decode the same number of steps.
usage: python tools/bench_infer.py [--steps 200] [--batch 1] [--no-groups] [--forced] [--stop-each] [--hparams-json FILE] [--hparams "k=v,..."] [--repeat N]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import satt_amd  # noqa: F401
from satt_amd import ops
from satt_amd.engine import Engine
from satt_amd.params import ModelConfig
from satt_amd.inference import infer

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--precision", default="bf16")
ap.add_argument("--steps-per-graph", type=int, default=8)
ap.add_argument("--no-graph", action="store_true")
ap.add_argument("--mega-max-b", type=int, default=None, help="largest batch that takes the persistent step kernel (default: the session's)")
ap.add_argument("--no-groups", action="store_true", help="DecodeSession.MEGA_GROUPS = False: batches of 3 .. 16 on the launch-per-layer path")
ap.add_argument("--forced", action="store_true", help="time forced-alignment utterances fed the alignments of one free-running utterance")
ap.add_argument("--stop-each", action="store_true", help='time infer(..., stop="each"), the per-utterance stop rule of free-running batches')
ap.add_argument("--hparams-json", default=None, help="hparams file of the model (default: the LJSpeech dimensions)")
ap.add_argument("--hparams", default=None, help='comma-separated name=value overrides of the model\'s hparams')
ap.add_argument("--repeat", type=int, default=1, help="timed utterances (one JSON line each)")
a = ap.parse_args()
ops.set_precision(a.precision)
if a.mega_max_b is not None:
    from satt_amd.inference import DecodeSession
    DecodeSession.MEGA_MAX_B = a.mega_max_b
if a.batch < 1 or a.batch > 16:
    ap.error("--batch: 1 .. 16")
if a.stop_each and a.forced:
    ap.error("--stop-each is the stop rule of a free-running decode")
if a.no_groups:
    from satt_amd.inference import DecodeSession
    DecodeSession.MEGA_GROUPS = False
if a.hparams_json or a.hparams:
    from satt_amd.hparams import hparams
    hp = hparams.copy()
    hp.parse_json(open(a.hparams_json or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "ljspeech",
                                                      "self-attention-tacotron.json")).read())
    hp.parse(a.hparams)
    cfg = ModelConfig.from_hparams(hp)
else:
    cfg = ModelConfig()
eng = Engine(cfg, "cuda", param_seed=0, rng_seed=1)
g = np.random.default_rng(1234)
B, Ti = a.batch, 100
src = g.integers(1, 68, (B, Ti)); src[:, 0] = 0; src[:, -1] = 0
sl = np.full((B,), Ti, dtype=np.int64)
ap_kw = dict(max_steps=a.steps, min_steps=10 ** 6, check_every=a.steps_per_graph, use_graph=not a.no_graph)
if a.stop_each:
    ap_kw["stop"] = "each"
if cfg.num_speakers > 0:
    ap_kw["speaker_id"] = (np.arange(B) % cfg.num_speakers + cfg.speaker_offset).astype(np.int64)
if a.forced:                            # the alignments of one free-running utterance; the forced session is built by the warm-up below
    free = infer(eng, src, sl, **ap_kw)
    ap_kw["teacher_alignments"] = (free["alignment1"], free["alignment2"])
infer(eng, src, sl, **ap_kw)            # warm-up: builds the session of this shape (buffers + captured hipGraph)
torch.cuda.synchronize()
for _ in range(a.repeat):
    t0 = time.perf_counter()
    out = infer(eng, src, sl, **ap_kw)      # encoder + memories + every decoder step + result copies
    torch.cuda.synchronize()
    dt_all = time.perf_counter() - t0
    dt = out["decode_ms"] * 1e-3            # the decoder steps alone (HIP events around the replay loop)
    al = out["alignment1"]
    ses = eng._decode_sessions[next(reversed(eng._decode_sessions))]
    path = "persistent, groups, forced" if (getattr(ses, "mega_groups", None) is not None and getattr(ses, "mega_forced", None) is not None) else \
        "persistent, forced" if getattr(ses, "mega_forced", None) is not None else "persistent" if getattr(ses, "mega", None) is not None else \
        ("persistent, groups" if getattr(ses, "mega_groups", None) is not None else "launch-per-layer")
    frames = a.steps * cfg.r * B
    print(json.dumps({"metric": "forced-alignment decode" if a.forced else "free-running decode (config 5)", "model": (a.hparams_json or "ljspeech") + (" + " + a.hparams if a.hparams else ""), "path": path, "stop": "each" if a.stop_each else "all", "batch": B, "Ti": Ti, "decoder_steps": out["steps"],
                      "ms_per_step": 1e3 * dt / a.steps, "utterance_ms_incl_encoder": 1e3 * dt_all,
                      "steps_per_graph": a.steps_per_graph, "graph": not a.no_graph,
                      "mel_frames_per_sec": frames / dt,
                      "realtime_factor": (dt / B) / (a.steps * cfg.r * 0.0125), "dtype": a.precision,
                      "alignment_rows_sum_to_one": bool(torch.allclose(al.sum(-1), torch.ones_like(al.sum(-1)), atol=1e-4)),
                      "finite": bool(torch.isfinite(out["mel"]).all())}))
