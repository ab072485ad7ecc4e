"""Time of the DTW alignment (csrc/dtw.hip) at the sizes of a corpus evaluation: 64 pairs of about 800 x 800 frames at K = 13 (with
and without the path), and one pair of 2048 x 2048:
  kernel:  ops.dtw alone, device-resident inputs, outputs and workspace, HIP events around `calls` back-to-back launches;
  batch:   Audio.mel_distance_batch on the hip backend from normalised host mels to host results (de-normalisation, cepstra,
           concatenation, copies both ways, one launch);
  numpy:   the float32 NumPy backend over the same pairs in a pool of 16 worker processes, as context (a host figure).
    python tools/bench_dtw.py [--pairs 64] [--frames 800] [--calls 5] [--repeat 5] [--no-numpy]
Every shape is warmed up first; `repeat` windows, the timed things alternating.  Prints one JSON line per case.  Under
`rocprofv3 --kernel-trace --stats -- python tools/bench_dtw.py --no-numpy` the kernel appears as dtw_k.
Work per cell: K subtractions, K multiplications, K additions and a square root, then three comparisons; Ta + Tb - 1 barriers a pair."""
import argparse
import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _numpy_pair(pair):
    import satt_amd  # noqa: F401
    from satt_amd.utils import mel_distance as md
    return md.dtw_numpy(pair[0], pair[1], True)[:2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--frames", type=int, default=800)
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
    from satt_amd.utils import audio
    from satt_amd.utils import mel_distance as md
    if not torch.cuda.is_available():
        raise SystemExit("bench_dtw.py needs a GPU (the numpy figure is context for the GPU ones)")
    dev = "cuda:0"
    hp = hparams.copy()
    hp.parse("num_freq=513,sample_rate=16000,frame_length_ms=50.0,frame_shift_ms=12.5,num_mels=80")
    hp.set("average_mel_level_db", [-40.0 - 0.1 * m for m in range(80)])
    hp.set("stddev_mel_level_db", [10.0 + 0.05 * m for m in range(80)])
    au = audio.Audio(hp, backend="hip", device=dev)
    g = np.random.default_rng(0)

    def mels(n_ref):
        """a smooth random normalised mel and a time-warped, noised copy of another length"""
        ref = np.cumsum(0.2 * g.standard_normal((n_ref, 80)), axis=0).astype(np.float32)
        n_pred = max(1, min(md.DTW_MAX_FRAMES, int(n_ref * (0.9 + 0.2 * g.random()))))
        idx = np.clip(np.round(np.linspace(0, n_ref - 1, n_pred) + g.normal(0, 2, n_pred)), 0, n_ref - 1).astype(int)
        idx.sort()
        return (ref[idx] + 0.1 * g.standard_normal((n_pred, 80))).astype(np.float32), ref

    cases = [("%d pairs of ~%d x %d" % (a.pairs, a.frames, a.frames),
              [mels(int(a.frames * (0.8 + 0.4 * g.random()))) for _ in range(a.pairs)]),
             ("one pair of 2048 x 2048", [(mels(2048)[1], mels(2048)[1])])]
    for name, pairs in cases:
        feats = [(md.mel_cepstrum(au.denormalize_mel(p.astype(np.float64)), 13), md.mel_cepstrum(au.denormalize_mel(r.astype(np.float64)), 13))
                 for p, r in pairs]
        ta = np.asarray([len(x) for x, _ in feats], np.int64)
        tb = np.asarray([len(y) for _, y in feats], np.int64)
        off = lambda c: torch.from_numpy(np.concatenate([[0], np.cumsum(c)]).astype(np.int64)).to(dev)
        A = torch.from_numpy(np.concatenate([x for x, _ in feats])).to(dev)
        B = torch.from_numpy(np.concatenate([y for _, y in feats])).to(dev)
        ao, bo, do, po = off(ta), off(tb), off(ta * tb), off(ta + tb - 1)
        cost = torch.empty(len(feats), dtype=torch.float32, device=dev)
        steps = torch.empty(len(feats), dtype=torch.int32, device=dev)
        dirs = torch.empty(int((ta * tb).sum()), dtype=torch.uint8, device=dev)
        path = torch.empty((int((ta + tb - 1).sum()), 2), dtype=torch.int32, device=dev)

        def kernel(with_path):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                if with_path:
                    ops.dtw(A, B, ao, bo, int(ta.max()), int(tb.max()), cost, steps, dirs, do, path, po)
                else:
                    ops.dtw(A, B, ao, bo, int(ta.max()), int(tb.max()), cost, steps)
            e1.record(); e1.synchronize()
            return e0.elapsed_time(e1) / a.calls               # ms per launch

        def batch():
            t0 = time.perf_counter()
            out = au.mel_distance_batch([p for p, _ in pairs], [r for _, r in pairs])
            assert len(out) == len(pairs)
            return 1e3 * (time.perf_counter() - t0)

        def numpy16():
            t0 = time.perf_counter()
            pool.map(_numpy_pair, feats, chunksize=1)
            return 1e3 * (time.perf_counter() - t0)

        fns = dict(kernel=lambda: kernel(False), kernel_path=lambda: kernel(True), batch=batch)
        if pool is not None:
            fns["numpy16"] = numpy16
        for fn in fns.values():
            fn()                                                # warm-up of every shape (and of the pool's imports)
        res = {k: [] for k in fns}
        for _ in range(a.repeat):
            for k, fn in fns.items():
                res[k].append(round(fn(), 3))
        med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
        cells = int((ta * tb).sum())
        print(json.dumps({"what": "DTW, ms per batch", "case": name, "K": 13, "pairs": len(feats), "cells": cells,
                          "diagonals_longest_pair": int((ta + tb - 1).max()), "windows_ms": res, "median_ms": med,
                          "cells_per_s": {k: round(cells / (v * 1e-3)) for k, v in med.items()},
                          "us_per_diagonal_longest_pair": {k: round(1e3 * med[k] / int((ta + tb - 1).max()), 3) for k in ("kernel", "kernel_path")}}),
              flush=True)
    if pool is not None:
        pool.close()
        pool.join()


if __name__ == "__main__":
    main()
