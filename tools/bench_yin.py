"""Time of the YIN pitch tracker (csrc/yin.hip) at the sizes of a corpus evaluation: 64 utterances of about 6 s at the LJSpeech
parameters (22050 Hz, hop 275) and at the VCTK parameters (48000 Hz, hop 600), with the defaults of utils/pitch.py:
  kernel:  ops.yin alone, device-resident signal, tables and outputs, HIP events around `calls` back-to-back launches;
  batch:   Audio.f0_batch on the hip backend from host signals to host tracks (concatenation, copies both ways, one launch at
           22050 Hz; at 48000 Hz the batch exceeds MAX_LAUNCH_SAMPLES and goes out in three, the voicing on the host);
  numpy:   the float32 NumPy backend over the same signals in a pool of 16 worker processes, as context (a host figure).
    python tools/bench_yin.py [--utts 64] [--seconds 6] [--calls 5] [--repeat 5] [--no-numpy]
Every shape is warmed up first; `repeat` windows, the timed things alternating.  Prints one JSON line per case.  Under
`rocprofv3 --kernel-trace --stats -- python tools/bench_yin.py --no-numpy` the kernel appears as yin_k.
Work per frame: (tau_max + 1) W differences, products and sums, W products and sums for the power, and a chain of tau_max sums."""
import argparse
import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("LJSpeech", 22050, 275, "num_freq=1025,sample_rate=22050,frame_length_ms=50.0,frame_shift_ms=12.5,num_mels=80"),
         ("VCTK", 48000, 600, "num_freq=2049,sample_rate=48000,frame_length_ms=50.0,frame_shift_ms=12.5,num_mels=80")]


def _numpy_signal(job):
    import satt_amd  # noqa: F401
    from satt_amd.utils import pitch
    y, sr, hop = job
    return pitch.yin_numpy(y, sr, hop)[0].sum()


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
        raise SystemExit("bench_yin.py needs a GPU (the numpy figure is context for the GPU ones)")
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
        off = lambda c: torch.from_numpy(np.concatenate([[0], np.cumsum(c)]).astype(np.int64)).to(dev)
        x = torch.from_numpy(np.concatenate(ys)).to(dev)
        io, fo = off(lens), off(1 + lens // hop)
        frames = int((1 + lens // hop).sum())
        out = [torch.empty(frames, dtype=torch.float32, device=dev) for _ in range(3)]

        def kernel():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                ops.yin(x, io, fo, W, tau_min, tau_max, hop, sr, pitch.THRESHOLD, *out)
            e1.record(); e1.synchronize()
            return e0.elapsed_time(e1) / a.calls               # ms per launch

        def batch():
            t0 = time.perf_counter()
            res = au.f0_batch(ys)
            assert len(res) == len(ys)
            return 1e3 * (time.perf_counter() - t0)

        def numpy16():
            t0 = time.perf_counter()
            pool.map(_numpy_signal, [(y, sr, hop) for y in ys], chunksize=1)
            return 1e3 * (time.perf_counter() - t0)

        fns = dict(kernel=kernel, batch=batch)
        if pool is not None:
            fns["numpy16"] = numpy16
        for fn in fns.values():
            fn()                                                # warm-up of every shape (and of the pool's imports)
        res = {k: [] for k in fns}
        for _ in range(a.repeat):
            for k, fn in fns.items():
                res[k].append(round(fn(), 3))
        med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
        terms = frames * (tau_max + 1) * W
        voiced = int(sum(r["voiced"].sum() for r in au.f0_batch(ys)))
        launches, count = 1, 0                                  # yin_hip's cut at MAX_LAUNCH_SAMPLES
        for n in lens:
            if count and count + n > audio.MAX_LAUNCH_SAMPLES:
                launches, count = launches + 1, 0
            count += int(n)
        print(json.dumps({"what": "YIN, ms per batch", "case": name, "sample_rate": sr, "hop": hop, "window": W, "tau_min": tau_min,
                          "tau_max": tau_max, "utts": len(ys), "samples": int(lens.sum()), "frames": frames, "voiced_frames": voiced,
                          "launches_per_batch": launches, "windows_ms": res, "median_ms": med,
                          "terms": terms, "gterms_per_s": {k: round(terms / (v * 1e-3) / 1e9, 2) for k, v in med.items()},
                          "audio_s_per_s": {k: round(int(lens.sum()) / sr / (v * 1e-3), 1) for k, v in med.items()}}), flush=True)
    if pool is not None:
        pool.close()
        pool.join()


if __name__ == "__main__":
    main()
