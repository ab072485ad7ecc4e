"""Times of speaker_embedd_to_decoder (the speaker vector fed to the decoder memories): the two kernels of csrc/speaker_cond.hip
at the shapes of examples/vctk/self-attention-tacotron-spk-decoder.json, and whole training steps of that example against the plain
VCTK example in one process (bench.py's method and the VCTK shape: B = 32, Ti = 160, Tm = 800, bf16).

    python tools/bench_spk_decoder.py [--batch 32] [--calls 2000] [--repeat 5] [--step] [--steps 40]

Kernel figures: time per call of `calls` back-to-back calls on one stream between two HIP events (launch overhead included), after a
warm-up of the same length; `repeat` windows, alternating.  One JSON line per result."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step_bench(a):
    import torch
    from satt_amd import ops
    from satt_amd.datasets.synthetic import synthetic_batch
    from satt_amd.engine import Engine
    from satt_amd.hparams import hparams
    from satt_amd.params import ModelConfig
    ops.set_precision("bf16")
    engs = {}
    for name in ("self-attention-tacotron.json", "self-attention-tacotron-spk-decoder.json"):
        hp = hparams.copy()
        hp.parse_json(open(os.path.join(ROOT, "examples", "vctk", name)).read())
        cfg = ModelConfig.from_hparams(hp)
        eng = Engine(cfg, "cuda:0", param_seed=0, rng_seed=3)
        batch = eng.to_device_batch(synthetic_batch(a.batch, 160, 800, seed=1234, num_speakers=cfg.num_speakers,
                                                    speaker_offset=cfg.speaker_offset, min_source_length=30, min_target_steps=90))
        engs[name] = (eng, batch)

    def step(eng, batch):
        ctx = eng.train_step(batch)
        eng.optimizer_step()
        return ctx
    for eng, batch in engs.values():
        for _ in range(10):
            step(eng, batch)
    torch.cuda.synchronize()
    for rep in range(a.repeat):
        for name, (eng, batch) in engs.items():         # alternating
            t0 = time.perf_counter()
            for _ in range(a.steps):
                ctx = step(eng, batch)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            eng.check_clusters(ctx)
            print(json.dumps({"what": "train step", "example": "vctk/" + name, "speaker_to_decoder": eng.cfg.speaker_to_decoder,
                              "window": rep, "steps": a.steps, "ms_per_step": round(1e3 * dt / a.steps, 4), "loss": float(eng.losses[2]),
                              "chunks": ctx["chunks"], "batch": a.batch, "dtype": "bf16"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=40)
    a = ap.parse_args()
    import torch
    import satt_amd  # noqa: F401
    from satt_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_spk_decoder.py needs a GPU (no CPU fallback)")
    if a.step:
        return step_bench(a)
    dev = "cuda:0"
    B, Td, Ti, G4, U1, U2 = a.batch, 400, 160, 1024, 224, 32       # gate rows [B * Td, 4 * 256], key rows [B * Ti, 224 | 32]
    r = lambda *s: torch.randn(*s, device=dev)
    xg, keys1, keys2 = r(B * Td, G4), r(B * Ti, U1), r(B * Ti, U2)
    gs, ks1, ks2 = r(B, G4), r(B, U1), r(B, U2)
    dgs, dks1, dks2 = torch.empty(B, G4, device=dev), torch.empty(B, U1, device=dev), torch.empty(B, U2, device=dev)
    lens = torch.randint(30, Ti + 1, (B,), device=dev)
    fns = {
        "bcast_add gates [B*Td, 1024] t0=1": lambda: ops.rows_bcast_add(xg, gs, B, Td, t0=1),
        "bcast_add keys1 [B*Ti, 224]": lambda: ops.rows_bcast_add(keys1, ks1, B, Ti),
        "bcast_add keys2 [B*Ti, 32]": lambda: ops.rows_bcast_add(keys2, ks2, B, Ti),
        "time_sum gates [B*Td, 1024] t0=1": lambda: ops.rows_time_sum(xg, None, dgs, B, Td, t0=1),
        "time_sum keys1 [B*Ti, 224] lengths": lambda: ops.rows_time_sum(keys1, lens, dks1, B, Ti),
        "time_sum keys2 [B*Ti, 32] lengths": lambda: ops.rows_time_sum(keys2, lens, dks2, B, Ti),
    }

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record(); e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / a.calls          # us per call

    for fn in fns.values():
        window(fn)
    res = {k: [] for k in fns}
    for _ in range(a.repeat):
        for k, fn in fns.items():
            res[k].append(round(window(fn), 3))
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    print(json.dumps({"what": "speaker_to_decoder kernels, us per call (launch overhead included)", "B": B, "Td": Td, "Ti": Ti,
                      "calls": a.calls, "windows": res, "median_us": med}), flush=True)


if __name__ == "__main__":
    main()
