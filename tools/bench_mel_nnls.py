"""Time of the non-negative mel inversion (csrc/mel_nnls.hip) at the sizes of a corpus evaluation: 64 utterances of 800 frames at the
LJSpeech parameters (n_fft 2048, 80 mels) and at the VCTK parameters (n_fft 4096, 80 mels), K = 64 iterations:
  kernel:  ops.mel_nnls alone, device-resident amplitudes, starts, tables and output, HIP events around `calls` back-to-back
           launches of all 51 200 frames;
  batch:   audio.mel_to_linear_batch(inversion="nnls") on the hip backend from host dB mels to host magnitudes (the pseudo-inverse
           start on the host, copies both ways, the launches cut at MAX_LAUNCH_SAMPLES // hop frames, the float64 floor);
  numpy:   the float32 NumPy backend over the same frames in a pool of 16 worker processes, one utterance a task (a host figure).
    python tools/bench_mel_nnls.py [--utts 64] [--frames 800] [--iters 64] [--calls 3] [--repeat 7] [--numpy-repeat 3] [--no-numpy]
Every shape is warmed up first; the timed things alternate within a repeat.  Prints one JSON line per case: every window, the
median and the spread (min, max).  There is no earlier kernel to compare with: the two columns stand beside each other, nothing more.
Work per frame and iteration: one product and sum per weight of the banded basis and of its transposed table, 7 operations per bin."""
import argparse
import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, (sample_rate, n_fft, win, hop, num_mels)
CASES = [("LJSpeech", (22050, 2048, 1102, 275, 80)), ("VCTK", (48000, 4096, 2400, 600, 80))]


def _numpy_utterance(job):
    import satt_amd  # noqa: F401
    from satt_amd.utils import audio
    cfg, a, x0, iters = job
    if cfg not in _numpy_utterance.tables:
        _numpy_utterance.tables[cfg] = audio.mel_nnls_tables(audio.MelspecTables(*cfg))
    return float(audio.mel_nnls_numpy(_numpy_utterance.tables[cfg], a, x0, iters).sum())


_numpy_utterance.tables = {}


def speechlike(n, sr, g):
    """a gliding harmonic tone under a moving spectral envelope, with unvoiced gaps and a noise floor"""
    k = np.arange(n)
    f = (100.0 + 120.0 * g.random()) * (1.0 + 0.3 * np.sin(2 * np.pi * k / sr * (0.5 + g.random())))
    ph = 2.0 * np.pi * np.cumsum(f) / sr
    y = sum(0.3 / h ** (0.7 + 0.6 * g.random()) * np.sin(h * ph + h) for h in range(1, 25))
    y = y * (np.sin(2 * np.pi * k / sr * 1.3 + 6 * g.random()) > -0.3)
    return (y + 2e-3 * g.standard_normal(n)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--numpy-repeat", type=int, default=3)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    # the workers are fresh processes that never open the GPU, started before this one does
    pool = None if a.no_numpy else multiprocessing.get_context("spawn").Pool(16)
    import torch
    import satt_amd  # noqa: F401
    from satt_amd import ops
    from satt_amd.utils import audio
    if not torch.cuda.is_available():
        raise SystemExit("bench_mel_nnls.py needs a GPU (the numpy figure stands beside the GPU ones)")
    dev = "cuda:0"
    g = np.random.default_rng(0)
    for name, cfg in CASES:
        sr, n_fft, win, hop, num_mels = cfg
        t = audio.MelspecTables(*cfg)
        nt = audio.mel_nnls_tables(t)
        # eight different utterances, each used utts / 8 times: the kernel's time does not depend on the data
        distinct = [audio.melspec_numpy(t, speechlike((a.frames - 1) * hop, sr, g), 20.0) for _ in range(min(8, a.utts))]
        Ss = [distinct[u % len(distinct)] for u in range(a.utts)]
        assert all(len(S) == a.frames for S in Ss)
        pairs = [audio._mel_amp_and_start(t, S, 20.0) for S in distinct]
        amps = [p[0].astype(np.float32) for p in pairs]
        x0s = [np.maximum(1e-10, p[1]).astype(np.float32) for p in pairs]
        amp = np.concatenate([amps[u % len(distinct)] for u in range(a.utts)])
        x0 = np.concatenate([x0s[u % len(distinct)] for u in range(a.utts)])
        d = nt.device(dev)
        ta, tx = torch.from_numpy(amp).to(dev), torch.from_numpy(x0).to(dev)
        beta = torch.from_numpy(np.ascontiguousarray(nt.beta(a.iters))).to(dev)
        out = torch.empty_like(tx)
        tabs = [d[k] for k in ("band_start", "band_offset", "band_weight", "bin_first", "bin_offset", "bin_weight")]

        def kernel():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                ops.mel_nnls(ta, tx, beta, float(nt.step), *tabs, out)
            e1.record(); e1.synchronize()
            return e0.elapsed_time(e1) / a.calls               # ms per launch

        def batch():
            t0 = time.perf_counter()
            res = audio.mel_to_linear_batch(t, Ss, 20.0, inversion="nnls", nnls_iters=a.iters, backend="hip", device=dev)
            assert len(res) == len(Ss)
            return 1e3 * (time.perf_counter() - t0)

        def numpy16():
            t0 = time.perf_counter()
            pool.map(_numpy_utterance, [(cfg, amps[u % len(distinct)], x0s[u % len(distinct)], a.iters) for u in range(a.utts)], chunksize=1)
            return 1e3 * (time.perf_counter() - t0)

        fns = dict(kernel=kernel, batch=batch)
        if pool is not None:
            fns["numpy16"] = numpy16
        for fn in fns.values():
            fn()                                                # warm-up of every shape (and of the pool's imports and tables)
        res = {k: [] for k in fns}
        for r in range(a.repeat):
            for k, fn in fns.items():
                if k != "numpy16" or r < a.numpy_repeat:
                    res[k].append(round(fn(), 3))
        med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
        # the launch's result against the NumPy backend on the first utterance, at the size that was timed
        same = out[:a.frames].cpu().numpy().tobytes() == audio.mel_nnls_numpy(nt, amps[0], x0s[0], a.iters).tobytes()
        frames = len(amp)
        terms = frames * a.iters * (len(nt.band_weight) + len(nt.bin_weight))
        print(json.dumps({"what": "mel NNLS, ms per batch", "case": name, "n_fft": n_fft, "num_mels": num_mels, "bins": nt.num_bins,
                          "weights": len(nt.band_weight), "transposed_weights": len(nt.bin_weight), "iters": a.iters, "utts": a.utts,
                          "frames": frames, "launches_per_batch": -(-frames // max(1, audio.MAX_LAUNCH_SAMPLES // hop)),
                          "bits_equal_numpy_first_utterance": same, "windows_ms": res, "median_ms": med,
                          "spread_ms": {k: [min(v), max(v)] for k, v in res.items()},
                          "gterms_per_s": {k: round(terms / (v * 1e-3) / 1e9, 2) for k, v in med.items()},
                          "frames_per_s": {k: round(frames / (v * 1e-3)) for k, v in med.items()}}), flush=True)
    if pool is not None:
        pool.close()
        pool.join()


if __name__ == "__main__":
    main()
