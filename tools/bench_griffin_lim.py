"""Time of Griffin-Lim (csrc/griffin_lim.hip) at the two example configurations: 60 iterations at alpha = 0.99 on utterances of
800 frames, batches of 1 and 16:
  call:    ops.griffin_lim alone, device-resident state, HIP events around `calls` back-to-back entry calls (2 iters + 2 launches each);
  numpy:   the float32 NumPy / scipy.fft backend, one utterance a thread on up to 16 threads, as context (a host figure).
    python tools/bench_griffin_lim.py [--frames 800] [--iters 60] [--calls 3] [--repeat 5] [--no-numpy]
Every shape is warmed up first; `repeat` windows, the two alternating.  Prints one JSON line per configuration and batch.  Under
`rocprofv3 --kernel-trace --stats -- python tools/bench_griffin_lim.py --no-numpy` the kernels appear as gl_synth_k<N>,
gl_analysis_k<N> and gl_signal_k<N>.  Work per frame and iteration (for rates): two n_fft-point real transforms of ~2.5 n_fft
log2(n_fft) flop each."""
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
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    import torch
    import satt_amd  # noqa: F401
    from satt_amd import ops
    from satt_amd.utils import audio
    if not torch.cuda.is_available():
        raise SystemExit("bench_griffin_lim.py needs a GPU (the numpy figure is context for the GPU ones)")
    dev = "cuda:0"
    for name, cfg in CONFIGS.items():
        _, n_fft, win, hop, _ = cfg
        t = audio.MelspecTables(*cfg)
        g = np.random.default_rng(0)
        y = (0.1 * g.standard_normal((a.frames - 1) * hop)).astype(np.float32)
        mag1 = audio.melspec_numpy(t, y, 20.0, want_mag=True)[1]                        # a real magnitude spectrogram, [frames, NF]
        ang1 = np.exp(2j * np.pi * g.random(mag1.shape)).astype(np.complex64)
        d = t.griffin_lim_device(dev)
        env = d["envelope"]
        for utts in (1, 16):
            fo = torch.arange(utts + 1, dtype=torch.int64, device=dev) * a.frames
            so = torch.arange(utts + 1, dtype=torch.int64, device=dev) * ((a.frames - 1) * hop)
            mag = torch.from_numpy(np.concatenate([mag1] * utts)).to(dev)
            ang0 = torch.view_as_real(torch.from_numpy(np.concatenate([ang1] * utts)).to(dev)).contiguous()
            ang, prev = ang0.clone(), torch.zeros_like(ang0)
            signal = torch.empty(utts * (a.frames - 1) * hop, dtype=torch.float32, device=dev)
            ws = torch.empty(ops.griffin_lim_workspace_bytes(n_fft, utts * a.frames) // 4, dtype=torch.float32, device=dev)

            def call():
                ang.copy_(ang0); prev.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    ops.griffin_lim(mag, ang, prev, signal, so, fo, n_fft, win, hop, a.iters, 0.99, d["window"], d["twiddle"], env, ws)
                e1.record(); e1.synchronize()
                return e0.elapsed_time(e1) / a.calls               # ms per entry call

            def numpy16():
                t0 = time.perf_counter()
                with ThreadPoolExecutor(max_workers=min(16, utts)) as pool:
                    list(pool.map(lambda _: audio.griffin_lim_numpy(t, mag1, ang1, a.iters, 0.99), range(utts)))
                return 1e3 * (time.perf_counter() - t0)

            fns = dict(call=call)
            if not a.no_numpy:
                fns["numpy16"] = numpy16
            for fn in fns.values():
                fn()                                                # warm-up of every shape
            res = {k: [] for k in fns}
            for _ in range(a.repeat):
                for k, fn in fns.items():
                    res[k].append(round(fn(), 3))
            med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
            assert bool(torch.isfinite(signal).all())
            flop = utts * a.frames * (2 * a.iters + 1) * 2.5 * n_fft * np.log2(n_fft)
            print(json.dumps({"what": "Griffin-Lim, ms per entry call", "config": name, "n_fft": n_fft, "hop": hop, "win": win,
                              "utts": utts, "frames": utts * a.frames, "iters": a.iters, "launches": 2 * a.iters + 2, "windows_ms": res,
                              "median_ms": med, "us_per_launch": round(1e3 * med["call"] / (2 * a.iters + 2), 2),
                              "call_fft_gflops": round(flop / (med["call"] * 1e-3) / 1e9, 1)}), flush=True)


if __name__ == "__main__":
    main()
