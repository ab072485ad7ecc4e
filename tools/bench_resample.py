"""Time of the sample-rate conversion (csrc/resample.hip) for a batch of 64 utterances of about 6 s, 22050 -> 16000 and 48000 -> 16000:
  kernel:  ops.resample alone, device-resident inputs and outputs, HIP events around `calls` back-to-back launches;
  batch:   Audio.resample_batch on the hip backend from host arrays to host arrays (concatenation, copies both ways, launch);
  numpy:   the float32 NumPy backend on 16 threads, as context (a host figure, not a GPU one).
    python tools/bench_resample.py [--utts 64] [--seconds 6] [--calls 20] [--repeat 5] [--no-numpy]
Every shape is warmed up first; `repeat` windows, the three alternating.  Prints one JSON line per conversion.  Under
`rocprofv3 --kernel-trace --stats -- python tools/bench_resample.py --no-numpy` the kernel appears as resample_k.
Work per output: `taps` multiply-adds; bytes: down / up samples in, one out (the table rows come from the caches)."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIRS = [(22050, 16000), (48000, 16000)]


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
        raise SystemExit("bench_resample.py needs a GPU (the numpy figure is context for the GPU ones)")
    dev = "cuda:0"
    for src, dst in PAIRS:
        hp = hparams.copy()
        hp.parse("num_freq=513,sample_rate=%d,frame_length_ms=50.0,frame_shift_ms=12.5,num_mels=80" % dst)
        au = audio.Audio(hp, backend="hip", device=dev, resample=True)
        t = audio.resample_tables(src, dst)
        g = np.random.default_rng(0)
        ys = [(0.1 * g.standard_normal(int(src * a.seconds * (0.8 + 0.4 * g.random())))).astype(np.float32) for _ in range(a.utts)]
        lens = np.asarray([len(y) for y in ys], np.int64)
        io = np.concatenate([[0], np.cumsum(lens)])
        oo = np.concatenate([[0], np.cumsum((lens * t.up + t.down - 1) // t.down)])
        outputs = int(oo[-1])
        x = torch.from_numpy(np.concatenate(ys)).to(dev)
        io_d, oo_d, table = torch.from_numpy(io).to(dev), torch.from_numpy(oo).to(dev), t.device(dev)
        y = torch.empty(outputs, dtype=torch.float32, device=dev)

        def kernel():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                ops.resample(x, io_d, oo_d, t.up, t.down, table, y)
            e1.record(); e1.synchronize()
            return e0.elapsed_time(e1) / a.calls               # ms per launch

        def batch():
            t0 = time.perf_counter()
            out = au.resample_batch(ys, [src] * a.utts)         # ends in the device-to-host copy of the result
            assert len(out) == a.utts
            return 1e3 * (time.perf_counter() - t0)

        def numpy16():
            t0 = time.perf_counter()
            with ThreadPoolExecutor(max_workers=16) as pool:
                list(pool.map(lambda s: audio.resample_numpy(t, s), ys))
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
        print(json.dumps({"what": "sample-rate conversion, ms per batch", "src": src, "dst": dst, "up": t.up, "down": t.down,
                          "taps": t.taps, "utts": a.utts, "samples_in": int(io[-1]), "samples_out": outputs, "windows_ms": res,
                          "median_ms": med, "outputs_per_s": {k: round(outputs / (v * 1e-3)) for k, v in med.items()},
                          "kernel_gflops": round(2.0 * outputs * t.taps / (med["kernel"] * 1e-3) / 1e9, 1),
                          "kernel_signal_GBps": round(4.0 * (int(io[-1]) + outputs) / (med["kernel"] * 1e-3) / 1e9, 2)}), flush=True)


if __name__ == "__main__":
    main()
