"""single-workgroup attention kernels: forward / backward launch time per option at B=32, Ti=160, Tm=800 (bf16, cluster kernels off).
usage: python tools/attn_general_times.py <tree root> <option,option,...>"""
import os
import sys

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import torch  # noqa: E402
import satt_amd  # noqa: E402,F401
from satt_amd import ops  # noqa: E402
from satt_amd.engine import Engine  # noqa: E402
from satt_amd.params import ModelConfig  # noqa: E402
from satt_amd.datasets.synthetic import synthetic_batch  # noqa: E402

OPTIONS = {
    "forward": dict(),
    "location_sensitive": dict(attention="location_sensitive"),
    "forward+cumulative": dict(cumulative_weights=True),
    "agent": dict(transition_agent=True),
    "agent+cumulative": dict(transition_agent=True, cumulative_weights=True),
}
B, Ti, Tm = 32, 160, 800
ops.set_precision("bf16")
batch = synthetic_batch(B, Ti, Tm, seed=5)
for name in sys.argv[2].split(","):
    eng = Engine(ModelConfig(**OPTIONS[name]), "cuda:0", param_seed=0, rng_seed=3)
    eng.use_clusters = False
    b = eng.to_device_batch(batch)
    for _ in range(2):
        ctx = eng.train_step(b); eng.optimizer_step()
    torch.cuda.synchronize()
    assert ctx["att_cluster"][0] == 0
    Td = ctx["dims"][2]
    rounds = []
    for r in range(3):          # three rounds of 3 steps: the spread between rounds is the run-to-run spread
        eng.timing = {}
        for _ in range(3):
            eng.train_step(b); eng.optimizer_step()
        torch.cuda.synchronize()
        ts = eng.timing_summary()
        rounds.append(tuple(ts[k][0] / ts[k][1] for k in ("attn_rnn_fwd", "attn_rnn_bwd")))
        eng.timing = None
    print("%-20s %s  fwd ms/launch %s  bwd ms/launch %s  | per decoder step (us): fwd %.2f bwd %.2f" % (
        name, os.path.basename(root), " ".join("%.3f" % f for f, _ in rounds), " ".join("%.3f" % g for _, g in rounds),
        1e3 * min(f for f, _ in rounds) / Td, 1e3 * min(g for _, g in rounds) / Td), flush=True)
    del eng, ctx
    torch.cuda.empty_cache()
