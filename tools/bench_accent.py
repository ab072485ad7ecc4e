"""Step time of a model built from an hparams JSON file at the benchmark shape (B=32, Ti=160, Tm=800, synthetic batch, bf16),
timed the way bench.py times its workload: warm-up steps, then HIP events around every timed step (train_step + optimizer_step)
and a host clock around the timed region ending in a device synchronise.  bench.py's --model list is fixed, so configurations
outside it - examples/ljspeech/self-attention-tacotron-accent.json - are timed here; the numbers come from THIS script, not from
bench.py.  Prints one JSON line per run.

    python tools/bench_accent.py [--config FILE] [--steps 50] [--warmup 10] [--repeat 3] [--composed]

--composed builds the accent branch from embedding_fwd + linear (the fallback beyond the fused kernels' cap) instead of the two
one-launch kernels (csrc/accent_prenet.hip).  Under `rocprofv3 --kernel-trace --stats -- python tools/bench_accent.py ...` the
two kernels appear as accent_prenet_fwd_k / accent_prenet_bwd_k."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(ROOT, "examples", "ljspeech", "self-attention-tacotron-accent.json"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=3, help="timed windows after one warm-up")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--composed", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import satt_amd  # noqa: F401
    from satt_amd import ops
    from satt_amd.datasets.synthetic import synthetic_batch
    from satt_amd.engine import Engine
    from satt_amd.hparams import hparams
    from satt_amd.params import ModelConfig
    if not torch.cuda.is_available():
        raise SystemExit("bench_accent.py needs a GPU (no CPU fallback)")
    hp = hparams.copy()
    hp.parse_json(open(a.config).read())
    cfg = ModelConfig.from_hparams(hp)
    ops.set_precision("bf16")
    eng = Engine(cfg, "cuda:0", param_seed=0, rng_seed=3)
    eng.fused_accent = not a.composed
    B, Ti, Tm = a.batch, 160, 800
    host = synthetic_batch(B, Ti, Tm, seed=1234)
    if cfg.accent:
        acc = np.random.default_rng(5).integers(0, cfg.num_accent_type, (B, Ti)).astype(np.int64)
        acc[np.arange(Ti)[None, :] >= np.asarray(host["source_length"])[:, None]] = 0
        host["accent_type"] = acc + cfg.accent_offset
    batch = eng.to_device_batch(host)

    def step():
        ctx = eng.train_step(batch)
        eng.optimizer_step()
        return ctx
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    for rep in range(a.repeat):
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
        marks[0].record()
        t0 = time.perf_counter()
        for i in range(a.steps):
            ctx = step()
            marks[i + 1].record()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        per = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(a.steps))
        eng.check_clusters(ctx)
        print(json.dumps({"config": os.path.relpath(a.config, ROOT), "accent": bool(cfg.accent),
                          "accent_branch": ("fused" if ctx.get("accent_fused") else "composed") if cfg.accent else None,
                          "window": rep, "steps": a.steps, "warmup": a.warmup, "ms_per_step": 1e3 * dt / a.steps,
                          "ms_per_step_median": per[len(per) // 2], "ms_min": per[0], "ms_max": per[-1],
                          "loss": float(eng.losses[2]), "batch": B, "Ti": Ti, "Tm": Tm, "dtype": "bf16"}), flush=True)


if __name__ == "__main__":
    main()
