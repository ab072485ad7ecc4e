"""Time of the forward of the speaker term with the resize layer (speaker_embedding_projection_out_dim): the one-launch kernel of
csrc/speaker_cond.hip against the chain of generic ops the engine composes beyond its cap (embedding_fwd + 2 x linear), at the VCTK
sizes with R = 64 and B = 32 (E = 16, P0 = 256, 152 speakers), fp32 operands as the engine's f32 parity mode and the kernel use
them.  The backward of the term has no kernel of its own (the chain of generic ops measured faster than a one-workgroup kernel:
profiles/speaker_cond_bench_and_kernel_times.txt); it is timed here as `chain_bwd` for the record.

    python tools/bench_speaker_cond.py [--batch 32] [--resize 64] [--calls 2000] [--repeat 5] [--step] [--composed]

Each figure is the time per call of `calls` back-to-back calls on one stream between two HIP events (launch overhead included: the
chain is launch-bound, which is what the kernel removes), after a warm-up of the same length; `repeat` windows, alternating.
Prints one JSON line.  --step times whole training steps of examples/vctk/self-attention-tacotron-resize.json instead (bench.py's
method and shape; --composed takes the chain in the forward too).  Under `rocprofv3 --kernel-trace --stats -- python
tools/bench_speaker_cond.py` the kernel appears as speaker_cond_fwd_k."""
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
    hp = hparams.copy()
    hp.parse_json(open(os.path.join(ROOT, "examples", "vctk", "self-attention-tacotron-resize.json")).read())
    hp.speaker_embedding_projection_out_dim = a.resize
    cfg = ModelConfig.from_hparams(hp)
    ops.set_precision("bf16")
    eng = Engine(cfg, "cuda:0", param_seed=0, rng_seed=3)
    eng.fused_speaker = not a.composed
    batch = eng.to_device_batch(synthetic_batch(a.batch, 160, 800, seed=1234, num_speakers=cfg.num_speakers,
                                                speaker_offset=cfg.speaker_offset))

    def step():
        ctx = eng.train_step(batch)
        eng.optimizer_step()
        return ctx
    for _ in range(10):
        step()
    torch.cuda.synchronize()
    for rep in range(a.repeat):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            ctx = step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        eng.check_clusters(ctx)
        print(json.dumps({"what": "train step, vctk resize example", "speaker_term_forward": "kernel" if ctx["spk"]["fused"] else "chain",
                          "window": rep, "steps": a.steps, "ms_per_step": 1e3 * dt / a.steps, "loss": float(eng.losses[2]),
                          "batch": a.batch, "R": a.resize, "dtype": "bf16"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--resize", type=int, default=64)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--composed", action="store_true")
    a = ap.parse_args()
    import torch
    import satt_amd  # noqa: F401
    from satt_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_speaker_cond.py needs a GPU (no CPU fallback)")
    if a.step:
        return step_bench(a)
    ops.set_precision("f32")
    dev = "cuda:0"
    B, E, R, P0, ns, off = a.batch, 16, a.resize, 256, 152, 225
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    table, Wr, br, Ws, bs, ds = r(ns, E), r(E, R) / 4, r(R) / 10, r(R, P0) / 8, r(P0) / 10, r(B, P0)
    ids = (torch.randint(0, ns, (B,), generator=g) + off).to(dev)
    semb, rs, sproj = torch.empty(B, E, device=dev), torch.empty(B, R, device=dev), torch.empty(B, P0, device=dev)
    G = [torch.zeros_like(x) for x in (table, Wr, br, Ws, bs)]
    dsp, drs, dx_r, dx_e = torch.empty(B, P0, device=dev), torch.empty(B, R, device=dev), torch.empty(B, R, device=dev), torch.empty(B, E, device=dev)
    assert ops.speaker_cond_supported(B, E, R, P0)

    def fused_fwd():
        ops.speaker_cond_fwd(ids, table, off, Wr, br, Ws, bs, semb, rs, sproj)

    def chain_fwd():
        ops.embedding_fwd(ids, table, semb, offset=off)
        ops.linear(semb, Wr, br, rs, act=ops.ACT_RELU)
        ops.linear(rs, Ws, bs, sproj, act=ops.ACT_SOFTSIGN)

    def chain_bwd():
        ops.act_bwd(ds, sproj, dsp, ops.ACT_SOFTSIGN)
        ops.linear_dw(rs, dsp, G[3], db=G[4])
        ops.linear_dx(dsp, Ws, dx_r)
        ops.act_bwd(dx_r, rs, drs, ops.ACT_RELU)
        ops.linear_dw(semb, drs, G[1], db=G[2])
        ops.linear_dx(drs, Wr, dx_e)
        ops.embedding_bwd(ids, dx_e, G[0], offset=off)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record(); e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / a.calls          # us per call

    fns = dict(fused_fwd=fused_fwd, chain_fwd=chain_fwd, chain_bwd=chain_bwd)
    fused_fwd()
    for fn in fns.values():
        window(fn)                                           # warm-up of every shape the timed windows use
    res = {k: [] for k in fns}
    for _ in range(a.repeat):
        for k, fn in fns.items():                            # alternating
            res[k].append(round(window(fn), 3))
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    print(json.dumps({"what": "speaker term, us per call (launch overhead included)", "B": B, "E": E, "R": R, "P0": P0,
                      "calls": a.calls, "windows": res, "median_us": med, "launches": {"fused_fwd": 1, "chain_fwd": 3, "chain_bwd": 7}}), flush=True)


if __name__ == "__main__":
    main()
