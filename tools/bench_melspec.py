"""Time of the log-mel extraction (csrc/melspec.hip) at the two example configurations, for a batch of 64 utterances of about 6 s:
  kernel:  ops.melspec alone, device-resident inputs and outputs, HIP events around `calls` back-to-back launches;
  batch:   Audio.melspectrogram_batch on the hip backend from host arrays to host arrays (concatenation, copies both ways, launch);
  numpy:   the float32 NumPy / scipy.fft backend on 16 threads, as context (a host figure, not a GPU one).
    python tools/bench_melspec.py [--utts 64] [--seconds 6] [--calls 20] [--repeat 5] [--no-numpy]
Every shape is warmed up first; `repeat` windows, the three alternating.  Prints one JSON line per configuration.  Under
`rocprofv3 --kernel-trace --stats -- python tools/bench_melspec.py --no-numpy` the kernel appears as melspec_k<2048> / melspec_k<4096>.
Work per frame (for rates): an n_fft-point real transform is ~2.5 n_fft log2(n_fft) flop; bytes: hop samples in, num_mels out."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"ljspeech": (22050, 2048, 1102, 275, 80), "vctk": (48000, 4096, 2400, 600, 80)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=6.0)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    import torch
    import satt_amd  # noqa: F401
    from satt_amd import ops
    from satt_amd.hparams import hparams
    from satt_amd.utils import audio
    if not torch.cuda.is_available():
        raise SystemExit("bench_melspec.py needs a GPU (the numpy figure is context for the GPU ones)")
    dev = "cuda:0"
    for name, (sr, n_fft, win, hop, mels) in CONFIGS.items():
        hp = hparams.copy()
        hp.parse("num_freq=%d,sample_rate=%d,frame_length_ms=50.0,frame_shift_ms=12.5,num_mels=%d" % (n_fft // 2 + 1, sr, mels))
        au = audio.Audio(hp, backend="hip", device=dev)
        assert (au.tables.n_fft, au.tables.hop, au.tables.win) == (n_fft, hop, win)
        g = np.random.default_rng(0)
        ys = [(0.1 * g.standard_normal(int(sr * a.seconds * (0.8 + 0.4 * g.random())))).astype(np.float32) for _ in range(a.utts)]
        lens = np.asarray([len(y) for y in ys], np.int64)
        so = np.concatenate([[0], np.cumsum(lens)])
        fo = np.concatenate([[0], np.cumsum(1 + lens // hop)])
        frames = int(fo[-1])
        d = au.tables.device(dev)
        sig = torch.from_numpy(np.concatenate(ys)).to(dev)
        so_d, fo_d = torch.from_numpy(so).to(dev), torch.from_numpy(fo).to(dev)
        mel = torch.empty((frames, mels), dtype=torch.float32, device=dev)

        def kernel():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                ops.melspec(sig, so_d, fo_d, n_fft, win, hop, d["window"], d["twiddle"], d["band_start"], d["band_offset"],
                            d["band_weight"], hp.ref_level_db, mel)
            e1.record(); e1.synchronize()
            return e0.elapsed_time(e1) / a.calls               # ms per launch

        def batch():
            t0 = time.perf_counter()
            out = au.melspectrogram_batch(ys)                   # ends in the device-to-host copy of the result
            assert len(out) == a.utts
            return 1e3 * (time.perf_counter() - t0)

        nb = audio.Audio(hp, backend="numpy")

        def numpy16():
            t0 = time.perf_counter()
            with ThreadPoolExecutor(max_workers=16) as pool:
                list(pool.map(lambda y: nb.melspectrogram_batch([y]), ys))
            return 1e3 * (time.perf_counter() - t0)

        fns = dict(kernel=kernel, batch=batch)
        if not a.no_numpy:
            fns["numpy16"] = numpy16
        for fn in fns.values():
            fn()                                                # warm-up of every shape
        res = {k: [] for k in fns}
        for _ in range(a.repeat):
            for k, fn in fns.items():
                res[k].append(round(fn(), 3))
        med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
        flop = frames * 2.5 * n_fft * np.log2(n_fft)
        print(json.dumps({"what": "log-mel extraction, ms per batch", "config": name, "n_fft": n_fft, "hop": hop, "win": win,
                          "utts": a.utts, "samples": int(so[-1]), "frames": frames, "windows_ms": res, "median_ms": med,
                          "frames_per_s": {k: round(frames / (v * 1e-3)) for k, v in med.items()},
                          "kernel_fft_gflops": round(flop / (med["kernel"] * 1e-3) / 1e9, 1),
                          "kernel_signal_GBps": round(4.0 * (int(so[-1]) + frames * mels) / (med["kernel"] * 1e-3) / 1e9, 2)}), flush=True)


if __name__ == "__main__":
    main()
