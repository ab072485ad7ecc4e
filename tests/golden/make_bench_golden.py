"""Freezes the float64 oracle (oracle/torch_ref.py) at the EXACT benchmark workloads into compact fixtures.

BASELINE.json configs[1] (LJSpeech, B=32, Ti=160, Tm=800) and configs[3] (VCTK, B=32, Ti=80, Tm=500, 152 speakers): the
batches bench.py times (`synthetic_batch(32, 160, 800, seed=1234)`, VCTK `seed=4321`), fp32 master weights straight from
`init_params` (no slice made bf16-representable), dropout / zoneout ON with the counter-based masks of oracle/rng.py.
The full tensors are too large to commit (gradient: 25 MB, alignments: 8 MB), so each fixture keeps:

  * the three losses, the per-sample masked mel-L1 and stop-token BCE;
  * the argmax path of both alignments ([B, Td] int16) and NROW sampled (sample, step) rows of alignment1 / alignment2,
    mel (both frames of the step), stop logits and the decoder self-attention output; sampled encoder rows;
  * per parameter tensor: the gradient's L2 norm, the full gradient where the tensor has <= FULL_MAX elements, and a
    SKETCH_T-dimensional count sketch otherwise; plus one SKETCH_G-dimensional count sketch of the flat gradient.
    A count sketch is a sparse random projection (bucket h(i), sign s(i), both from a seeded numpy generator - see
    `sketch_plan`): ||S(a) - S(b)|| estimates ||a - b|| to a few percent, which is what the GPU test bounds.

The reference (TF1 + tacotron2@6af04c7) cannot run here and holds no vectors: this pins the build's own
restatement - "parity unpinned" with respect to TF stays true.  CPU only, ~15 min and ~25 GB for the LJSpeech case:
    python tests/golden/make_bench_golden.py [ljspeech] [vctk] [ljspeech_sharp_lo] [ljspeech_sharp_hi]
The converged-regime fixtures also carry their bf16 floor (`floor`: the same oracle with bf16-rounded weight matrices, measured by
`frozen_distances`; ~30 s of CPU per fixture with 4-6 threads), added to an existing fixture without touching its other keys by
    python tests/golden/make_bench_golden.py --floor [ljspeech_sharp_lo] [ljspeech_sharp_hi]
"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NROW = 64
FULL_MAX = 2048
SKETCH_T = 1024
SKETCH_G = 4096
PARAM_SEED = 3
RNG_SEED = 5

# The converged regime (r6): training drives alignment 1 towards one-hot rows that ride on the `+1e-7` floor of the forward recursion
# (reference modules/forward_attention.py:107-121) with large energies, while everything init_params produces is diffuse (mean row
# entropy 2.95 nats of log 160 = 5.08, max alpha 0.51).  `sharpen` reshapes the location-sensitive score of the SAME random model so
# that its rows are sharp, on both sides of the kernels' softmax-form switch at sum|v| = 30 (csrc/attn_cluster.hip: constant shift /
# lazy normalisation below it, the in-chain maximum above):
#   sharp_lo: v concentrated on its first 4 units and scaled to sum|v| = 29.5, query layer and keys x 8 (saturated tanh: neighbouring
#             energies differ by several units) - mean entropy ~0.4 nats, max alpha > 0.95 on ~45 % of the rows (what sum|v| < 30 allows
#             a random network);
#   sharp_hi: v x 24 (sum|v| = 443), query layer and keys x 4 - mean entropy ~0.2 nats, max alpha > 0.95 on ~70 % of the rows.
CASES = {
    "ljspeech": dict(cfg=dict(), batch=dict(B=32, Ti=160, Tm=800, seed=1234)),
    "ljspeech_sharp_lo": dict(cfg=dict(), batch=dict(B=32, Ti=160, Tm=800, seed=1234), sharpen=dict(keep=4, sv=1.6, sq=8.0, sk=8.0)),
    "ljspeech_sharp_hi": dict(cfg=dict(), batch=dict(B=32, Ti=160, Tm=800, seed=1234), sharpen=dict(keep=0, sv=24.0, sq=4.0, sk=4.0)),
    "vctk": dict(cfg=dict(num_speakers=152, speaker_offset=225),
                 batch=dict(B=32, Ti=80, Tm=500, seed=4321, min_source_length=30, min_target_steps=90, num_speakers=152,
                            speaker_offset=225)),
}


FLOOR_CASES = ("ljspeech_sharp_lo", "ljspeech_sharp_hi")     # fixtures that also carry the bf16-weight floor (`floor`)


def sample_rows(B, Td, seed):
    """NROW (sample, decoder step) pairs: the first / last steps of a few samples plus uniform draws"""
    g = np.random.default_rng(seed)
    b = g.integers(0, B, NROW)
    t = g.integers(0, Td, NROW)
    t[:4] = 0
    t[4:8] = Td - 1
    t[8:12] = 1
    return b.astype(np.int32), t.astype(np.int32)


def crc_of(arrays):
    """CRC-32 over the bytes of a dict of arrays in key order (pins the seeded inputs the vectors belong to)"""
    import zlib
    c = 0
    for k in sorted(arrays):
        c = zlib.crc32(np.ascontiguousarray(arrays[k]).tobytes(), zlib.crc32(k.encode(), c))
    return c


def make_batch(kw):
    from satt_amd.datasets.synthetic import synthetic_batch
    kw = dict(kw)
    return synthetic_batch(kw.pop("B"), kw.pop("Ti"), kw.pop("Tm"), **kw)


def sharpen_params(P, keep=0, sv=1.0, sq=1.0, sk=1.0):
    """the `sharpen` transformation of a parameter dict (a copy): dec.att1.v concentrated on its first `keep` units (0: all) and scaled
    to sv x its initial sum of magnitudes, the fused query layer dec.att.Wq x sq, the key layer dec.att1.Wm x sk"""
    P = dict(P)
    v0 = np.asarray(P["dec.att1.v"], dtype=np.float64)
    v = v0.copy()
    if keep > 0:
        v[int(keep):] = 0.0
    v *= sv * np.abs(v0).sum() / np.abs(v).sum()
    P["dec.att1.v"] = v.astype(np.float32)
    P["dec.att.Wq"] = (np.asarray(P["dec.att.Wq"], dtype=np.float64) * sq).astype(np.float32)
    P["dec.att1.Wm"] = (np.asarray(P["dec.att1.Wm"], dtype=np.float64) * sk).astype(np.float32)
    return P


def frozen_distances(r, z, batch):
    """Distances of one run from the frozen fixture z - the ONE definition that tests/test_pinned_gpu.py (the engine's run) and
    `floor` below (the float64 oracle with bf16-rounded weight matrices) both use.  r: loss, mel_loss, mel [B,T,nm], al1 / al2
    [B,Td,Ti], stop, dec_out [B,Td,.], lstm_out / sa_out [B,Ti,.], G {name: gradient}.  Returns (got: {metric: value},
    tensor: per-tensor relative distances aligned with z["grad_names"] (NaN where the fixture's gradient is zero),
    extra: row distances, largest path offset, |g| / |g_ref|)."""
    from common import count_sketch
    B, Td = batch["done"].shape
    got = {}
    got["mel_loss"] = abs(float(r["mel_loss"]) - float(z["mel_loss"]))
    got["loss"] = abs(float(r["loss"]) - float(z["loss"]))
    w = batch["spec_loss_mask"].astype(np.float64)
    per = (np.abs(np.asarray(r["mel"], dtype=np.float64) - batch["mel"]).mean(-1) * w).sum(-1) / np.maximum(w.sum(-1), 1.0)
    got["per_sample"] = float(np.abs(per - z["per_sample_mel_l1"]).max())
    sb, st = z["rows_b"], z["rows_t"]
    got["al1"] = float(np.abs(r["al1"][sb, st] - z["align1_rows"]).max())
    got["al2"] = float(np.abs(r["al2"][sb, st] - z["align2_rows"]).max())
    # argmax paths: compared where the run's maximum is not a near-tie (two memory rows within 2 % of each other flip freely)
    p1 = r["al1"].argmax(-1)
    top2 = np.sort(r["al1"], -1)[..., -2:]
    clear = top2[..., 1] > 1.02 * top2[..., 0]
    got["path"] = float((p1[clear] == z["path1"][clear]).mean())
    off = int(np.abs(p1.astype(np.int64) - z["path1"]).max())
    rel = lambda a, b: float(np.abs(np.asarray(a, np.float64) - b).max() / (np.abs(b).max() + 1e-12))
    rows = dict(mel=rel(np.asarray(r["mel"]).reshape(B, Td, -1)[sb, st], z["mel_rows"]),
                stop=rel(np.asarray(r["stop"]).reshape(B, Td)[sb, st], z["stop_rows"]),
                dec_out=rel(np.asarray(r["dec_out"])[sb, st], z["dec_out_rows"]),
                lstm_out=rel(np.asarray(r["lstm_out"])[z["enc_b"], z["enc_t"]], z["lstm_out_rows"]),
                sa_out=rel(np.asarray(r["sa_out"])[z["enc_b"], z["enc_t"]], z["sa_out_rows"]))
    got["rows"] = max(rows.values())
    names = [str(n) for n in z["grad_names"]]
    G = {k: np.asarray(r["G"][k], dtype=np.float64) for k in names}
    flat = np.concatenate([G[k].ravel() for k in names])
    ref_sk = z["grad_sketch_all"]
    got["grad"] = float(np.linalg.norm(count_sketch(flat, int(z["meta.sketch_g"]), 0) - ref_sk) / np.linalg.norm(ref_sk))
    gn = float(np.linalg.norm(flat) / float(z["grad_norm_all"]))
    tensor = np.full(len(names), np.nan)
    for i, k in enumerate(names):
        nrm = float(z["grad_norms"][i])
        if nrm == 0.0:
            continue
        if ("grad_full." + k) in z.files:
            tensor[i] = np.linalg.norm(G[k] - z["grad_full." + k]) / nrm
        else:
            tensor[i] = np.linalg.norm(count_sketch(G[k], int(z["meta.sketch_t"]), i + 1) - z["grad_sketch." + k]) / nrm
    # the worst tensor among those with gradient signal (>= 1e-6 of the total norm: nothing to be relative to below)
    live = np.asarray(z["grad_norms"], dtype=np.float64) >= 1e-6 * float(z["grad_norm_all"])
    got["tensor"] = float(np.nanmax(np.where(live, tensor, np.nan)))
    return got, tensor, dict(rows=rows, off=off, gn=gn)


def bf16_weights(P):
    """every weight matrix (ndim >= 2) rounded to bf16, the rest as it is - the rule of make_decode_golden.py"""
    return {k: (torch.as_tensor(np.asarray(v, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()
                if np.asarray(v).ndim >= 2 else v) for k, v in P.items()}


def floor(name):
    """The bf16 floor of a fixture: the SAME float64 oracle with every weight matrix rounded to bf16, measured against the fixture by
    `frozen_distances`.  Adds floor.<metric> scalars and floor.tensor (aligned with grad_names) to bench_<name>.npz and leaves
    every other key as it is."""
    import satt_amd  # noqa: F401
    from satt_amd.params import ModelConfig, init_params
    from common import oracle_run
    path = os.path.join(HERE, "bench_%s.npz" % name)
    z = np.load(path)
    keep = {k: z[k] for k in z.files if not k.startswith("floor.")}
    case = CASES[name]
    P = init_params(ModelConfig(**case["cfg"]), PARAM_SEED)
    if "sharpen" in case:
        P = sharpen_params(P, **case["sharpen"])
    batch = make_batch(case["batch"])
    assert int(z["meta.batch_crc"]) == crc_of(batch) and int(z["meta.param_crc"]) == crc_of(P)
    t0 = time.time()
    out, col, g = oracle_run(case["cfg"], bf16_weights(P), batch, True, seed=RNG_SEED)
    print("%s: bf16-weight oracle forward + backward %.0f s" % (name, time.time() - t0), flush=True)
    r = dict(loss=out["loss"].detach(), mel_loss=out["mel_loss"].detach(), mel=out["mel"].detach().numpy(),
             al1=out["alignment1"].detach().numpy(), al2=out["alignment2"].detach().numpy(), stop=out["stop"].detach().numpy(),
             dec_out=col["dec_out"].detach().numpy(), lstm_out=out["lstm_out"].detach().numpy(), sa_out=out["sa_out"].detach().numpy(),
             G=g)
    got, tensor, extra = frozen_distances(r, z, batch)
    names = [str(n) for n in z["grad_names"]]
    print("%s floor: " % name + " ".join("%s=%.3e" % kv for kv in got.items()) + " | rows %s" % extra["rows"], flush=True)
    print("%s floor, largest tensors: " % name + " ".join("%s=%.3e" % (names[i], tensor[i]) for i in np.argsort(-np.nan_to_num(tensor))[:8]))
    keep.update({"floor." + k: np.float64(v) for k, v in got.items() if k != "tensor"})     # (the worst tensor: max of floor.tensor)
    keep["floor.tensor"] = tensor
    np.savez_compressed(path, **keep)
    print("%s: wrote %s (%.0f KB)" % (name, path, os.path.getsize(path) / 1024), flush=True)


def build(name):
    import satt_amd  # noqa: F401
    from satt_amd.params import ModelConfig, init_params
    from common import count_sketch, oracle_run
    case = CASES[name]
    cfg = ModelConfig(**case["cfg"])
    P = init_params(cfg, PARAM_SEED)
    if "sharpen" in case:
        P = sharpen_params(P, **case["sharpen"])
    batch = make_batch(case["batch"])
    t0 = time.time()
    out, col, g = oracle_run(case["cfg"], P, batch, True, seed=RNG_SEED)
    print("%s: oracle forward + backward %.0f s, loss %.9f" % (name, time.time() - t0, float(out["loss"])), flush=True)
    B, Td = batch["done"].shape
    r = cfg.r
    mel = out["mel"].detach().numpy()
    stop = out["stop"].detach().numpy().reshape(B, Td)
    al1, al2 = out["alignment1"].detach().numpy(), out["alignment2"].detach().numpy()
    tgt = np.asarray(batch["mel"], dtype=np.float64)
    w = np.asarray(batch["spec_loss_mask"], dtype=np.float64)
    per_mel = (np.abs(mel - tgt).mean(-1) * w).sum(-1) / np.maximum(w.sum(-1), 1.0)
    sb, st = sample_rows(B, Td, 99)
    eb = np.random.default_rng(98).integers(0, B, NROW).astype(np.int32)
    et = np.array([np.random.default_rng(97 + i).integers(0, int(batch["source_length"][b])) for i, b in enumerate(eb)], dtype=np.int32)
    keep = dict(loss=np.float64(out["loss"].detach()), mel_loss=np.float64(out["mel_loss"].detach()),
                done_loss=np.float64(out["done_loss"].detach()), per_sample_mel_l1=per_mel,
                path1=al1.argmax(-1).astype(np.int16), path2=al2.argmax(-1).astype(np.int16),
                rows_b=sb, rows_t=st, align1_rows=al1[sb, st].astype(np.float32), align2_rows=al2[sb, st].astype(np.float32),
                mel_rows=mel.reshape(B, Td, r * cfg.num_mels)[sb, st].astype(np.float32), stop_rows=stop[sb, st].astype(np.float32),
                dec_out_rows=col["dec_out"].detach().numpy()[sb, st].astype(np.float32),
                enc_b=eb, enc_t=et, lstm_out_rows=out["lstm_out"].detach().numpy()[eb, et].astype(np.float32),
                sa_out_rows=out["sa_out"].detach().numpy()[eb, et].astype(np.float32),
                align1_mean_entropy=np.float64(-(al1 * np.log(np.maximum(al1, 1e-300))).sum(-1).mean()),
                align1_max_mean=np.float64(al1.max(-1).mean()), align1_frac_max_above_095=np.float64((al1.max(-1) > 0.95).mean()),
                att1_v_abs_sum=np.float64(np.abs(np.asarray(P["dec.att1.v"], dtype=np.float64)).sum()))
    print("%s: alignment-1 mean row entropy %.3f nats, mean max %.3f, rows with max > 0.95: %.3f, sum|v| = %.1f"
          % (name, keep["align1_mean_entropy"], keep["align1_max_mean"], keep["align1_frac_max_above_095"], keep["att1_v_abs_sum"]), flush=True)
    names = list(g.keys())
    flat = np.concatenate([np.asarray(g[k], dtype=np.float64).ravel() for k in names])
    keep["grad_names"] = np.array(names)
    keep["grad_norms"] = np.array([np.linalg.norm(np.asarray(g[k], dtype=np.float64)) for k in names])
    keep["grad_norm_all"] = np.float64(np.linalg.norm(flat))
    keep["grad_sketch_all"] = count_sketch(flat, SKETCH_G, 0)
    for i, k in enumerate(names):
        a = np.asarray(g[k], dtype=np.float64)
        if a.size <= FULL_MAX:
            keep["grad_full." + k] = a.astype(np.float32)
        else:
            keep["grad_sketch." + k] = count_sketch(a, SKETCH_T, i + 1).astype(np.float32)
    meta = dict(param_seed=PARAM_SEED, rng_seed=RNG_SEED, nrow=NROW, full_max=FULL_MAX, sketch_t=SKETCH_T, sketch_g=SKETCH_G,
                batch_crc=crc_of(batch), param_crc=crc_of(P))
    path = os.path.join(HERE, "bench_%s.npz" % name)
    np.savez_compressed(path, **{"meta." + k: np.int64(v) for k, v in meta.items()}, **keep)
    print("%s: wrote %s (%.0f KB)" % (name, path, os.path.getsize(path) / 1024), flush=True)


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("SATT_ORACLE_THREADS", "6")))
    args = sys.argv[1:]
    if args[:1] == ["--floor"]:          # the bf16 floor of existing fixtures (default: the converged-regime ones)
        for n in (args[1:] or FLOOR_CASES):
            floor(n)
    else:
        for n in (args or list(CASES)):
            build(n)
            if n in FLOOR_CASES:
                floor(n)
