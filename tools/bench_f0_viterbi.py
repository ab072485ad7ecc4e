"""Time of the Viterbi pitch tracker's two kernels (csrc/yin.hip satt_yin_candidates, csrc/f0_viterbi.hip) at the sizes of a corpus
evaluation: 64 utterances of about 6 s at the LJSpeech parameters (22050 Hz, hop 275) and at the VCTK parameters (48000 Hz, hop
600), with the defaults of utils/pitch.py:
  candidates:  ops.yin_candidates alone, device-resident signal, tables and outputs, HIP events around `calls` back-to-back launches;
  viterbi:     ops.f0_viterbi alone over the candidates and the gate of the same batch, the same way;
  batch:       Audio.f0_batch(tracker="viterbi") on the hip backend from host signals to host tracks (both launches, the copies both
               ways and the gate on the host between them; at 48000 Hz the batch exceeds MAX_LAUNCH_SAMPLES and goes out in three);
  numpy16:     the float32 NumPy backend over the same signals in a pool of 16 worker processes, as context (a host figure).
    python tools/bench_f0_viterbi.py [--utts 64] [--seconds 6] [--calls 5] [--repeat 5] [--no-numpy]
Every shape is warmed up first; `repeat` windows, the timed things alternating.  Prints one JSON line per case.  Under
`rocprofv3 --kernel-trace --stats -- python tools/bench_f0_viterbi.py --no-numpy` the kernels appear as yin_k<.., true> and
f0_viterbi_k.  The Viterbi kernel is a serial chain of T steps per utterance, one workgroup each: its time is that of the longest
utterance, not of the batch."""
import argparse
import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_yin import CASES  # noqa: E402


def _numpy_signal(job):
    import satt_amd  # noqa: F401
    from satt_amd.utils import pitch
    y, sr, hop = job
    return pitch.track_f0([y], sr, hop, tracker="viterbi")[0][0].sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=6.0)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    # the workers are fresh processes that never open the GPU, started before this one does
    pool = None if a.no_numpy else multiprocessing.get_context("spawn").Pool(16)
    import torch
    import satt_amd  # noqa: F401
    from satt_amd import ops
    from satt_amd.hparams import hparams
    from satt_amd.utils import audio, pitch
    if not torch.cuda.is_available():
        raise SystemExit("bench_f0_viterbi.py needs a GPU (the numpy figure is context for the GPU ones)")
    dev = "cuda:0"
    g = np.random.default_rng(0)

    def speechlike(n, sr):
        """a gliding three-harmonic tone with unvoiced gaps and a noise floor"""
        k = np.arange(n)
        f = (100.0 + 120.0 * g.random()) * (1.0 + 0.3 * np.sin(2 * np.pi * k / sr * (0.5 + g.random())))
        ph = 2.0 * np.pi * np.cumsum(f) / sr
        y = sum(0.3 / h * np.sin(h * ph + h) for h in (1, 2, 3)) * (np.sin(2 * np.pi * k / sr * 1.3 + 6 * g.random()) > -0.3)
        return (y + 2e-3 * g.standard_normal(n)).astype(np.float32)

    for name, sr, hop, hp_text in CASES:
        hp = hparams.copy()
        hp.parse(hp_text)
        au = audio.Audio(hp, backend="hip", device=dev)
        assert au.tables.hop == hop
        W, tau_min, tau_max = pitch.yin_check(sr, hop)
        ys = [speechlike(int(sr * a.seconds * (0.8 + 0.4 * g.random())), sr) for _ in range(a.utts)]
        lens = np.asarray([len(y) for y in ys], np.int64)
        T = 1 + lens // hop
        off = lambda c: torch.from_numpy(np.concatenate([[0], np.cumsum(c)]).astype(np.int64)).to(dev)
        x = torch.from_numpy(np.concatenate(ys)).to(dev)
        io, fo = off(lens), off(T)
        frames = int(T.sum())
        per, val = (torch.empty((frames, pitch.F0_CANDIDATES), dtype=torch.float32, device=dev) for _ in range(2))
        power, f0 = (torch.empty(frames, dtype=torch.float32, device=dev) for _ in range(2))
        state = torch.empty(frames, dtype=torch.uint8, device=dev)
        cost = torch.empty(len(ys), dtype=torch.float32, device=dev)
        ops.yin_candidates(x, io, fo, W, tau_min, tau_max, hop, per, val, power)
        pw = power.cpu().numpy()
        bounds = np.concatenate([[0], np.cumsum(T)])
        gate = torch.from_numpy(np.concatenate([pitch.silence_gate(pw[bounds[u]:bounds[u + 1]]) for u in range(len(ys))]).astype(np.uint8)).to(dev)
        costs = (pitch.JUMP_COST, pitch.SWITCH_COST, pitch.THRESHOLD, pitch.LAG_BIAS)

        def timed(launch):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                launch()
            e1.record(); e1.synchronize()
            return e0.elapsed_time(e1) / a.calls               # ms per launch

        def candidates():
            return timed(lambda: ops.yin_candidates(x, io, fo, W, tau_min, tau_max, hop, per, val, power))

        def viterbi():
            return timed(lambda: ops.f0_viterbi(per, val, gate, fo, int(T.max()), tau_max, sr, *costs, f0, state, cost))

        def batch():
            t0 = time.perf_counter()
            res = au.f0_batch(ys, tracker="viterbi")
            assert len(res) == len(ys)
            return 1e3 * (time.perf_counter() - t0)

        def numpy16():
            t0 = time.perf_counter()
            pool.map(_numpy_signal, [(y, sr, hop) for y in ys], chunksize=1)
            return 1e3 * (time.perf_counter() - t0)

        fns = dict(candidates=candidates, viterbi=viterbi, batch=batch)
        if pool is not None:
            fns["numpy16"] = numpy16
        for fn in fns.values():
            fn()                                                # warm-up of every shape (and of the pool's imports)
        res = {k: [] for k in fns}
        for _ in range(a.repeat):
            for k, fn in fns.items():
                res[k].append(round(fn(), 3))
        med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
        voiced = int(sum(r["voiced"].sum() for r in au.f0_batch(ys, tracker="viterbi")))
        used = int((per > 0).sum().item())
        print(json.dumps({"what": "F0 Viterbi, ms per batch", "case": name, "sample_rate": sr, "hop": hop, "window": W, "tau_min": tau_min,
                          "tau_max": tau_max, "utts": len(ys), "samples": int(lens.sum()), "frames": frames, "longest_frames": int(T.max()),
                          "used_slots_per_frame": round(used / frames, 2), "voiced_frames": voiced, "windows_ms": res, "median_ms": med,
                          "viterbi_us_per_step_of_the_longest": round(1e3 * med["viterbi"] / int(T.max()), 3),
                          "audio_s_per_s": {k: round(int(lens.sum()) / sr / (v * 1e-3), 1) for k, v in med.items()}}), flush=True)
    if pool is not None:
        pool.close()
        pool.join()


if __name__ == "__main__":
    main()
