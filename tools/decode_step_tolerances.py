"""The float32 deviation of every reference of tests/decode_step_common.py from its float64 form, over the cases of
tests/test_decode_step_gpu.py: plain torch on the CPU, same inputs, same bf16-rounded weights, relative to the tensor maximum
(common.rel_err).  The tests' bounds are 8 x the worst figure per operation, or the bound tests/test_ops_gpu.py grants the training
kernel of the same function where that is wider (decode_step_common.DEV32, FLOOR, bound).
    python tools/decode_step_tolerances.py          (profiles/decode_step_tolerances.txt holds a recorded run)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import decode_step_common as ds  # noqa: E402
from common import rel_err  # noqa: E402

F32, F64 = torch.float32, torch.float64


def flat(x):
    """the tensors of a reference's result, in order"""
    if isinstance(x, torch.Tensor):
        return [x]
    if isinstance(x, dict):
        return [v for v in x.values() if v is not None]
    return [t for v in x for t in flat(v)]


def deviation(ref, case):
    return max(rel_err(a.numpy(), b.numpy()) for a, b in zip(flat(ref(case, F32)), flat(ref(case, F64))))


def self_attn_cases():
    p = ds.SA_PROD
    for t in ds.SA_PROD_T:
        yield "self_attn", ds.sa_cache(p["B"], p["Td"], p["D"], p["heads"]), t, p["D"], p["heads"]
    yield "self_attn", ds.sa_cache(p["B"], p["Td"], p["D"], p["heads"], "sharp"), ds.SA_REGIME_T, p["D"], p["heads"]
    yield "self_attn_offset", ds.sa_cache(p["B"], p["Td"], p["D"], p["heads"], "offset"), ds.SA_REGIME_T, p["D"], p["heads"]
    b = ds.SA_BIG
    yield "self_attn", ds.sa_cache(b["B"], b["Td"], b["D"], b["heads"]), b["t"], b["D"], b["heads"]
    for D, heads in ds.SA_ANY:
        for t in ds.SA_ANY_T:
            yield "self_attn", ds.sa_cache(ds.SA_ANY_B, ds.SA_ANY_TD, D, heads), t, D, heads


def main():
    worst = {k: 0.0 for k in ds.DEV32}

    def note(op, e):
        worst[op] = max(worst[op], e)
    for c in ds.LIN_CASES + [ds.DROP_CASE]:
        note("dense", deviation(ds.lin_ref, c))
    for c in ds.LSTM_CASES:
        note("lstm", deviation(ds.lstm_case_ref, c))
    for c in ds.L2_CASES:
        note("linear2", deviation(ds.l2_ref, c))
    for c in ds.CHAIN_CASES:
        note("chain" if c.main == "plain" else "chain_lstm", deviation(ds.chain_ref, c))
    for op, kvq, t, D, heads in self_attn_cases():
        note(op, rel_err(ds.self_attn_ref(kvq, t, D, heads, F32).numpy(), ds.self_attn_ref(kvq, t, D, heads, F64).numpy()))
    keys = dict(attn_align=("align1", "align2"), attn_ctx=("ctx",), attn_state=("a_state", "alpha_state"), attn_pq=("pq",))
    for c in ds.ATT_CASES:
        r32, r64 = ds.att_ref(c, F32), ds.att_ref64(c)
        forced = c.mode.startswith("forced")          # the rows are given (exact), only the contexts are computed
        for op, ks in keys.items():
            for s32, s64 in zip(r32, r64):
                for k in ks:
                    if s64[k] is not None and (k == "ctx" or not forced):
                        note(op, rel_err(s32[k].numpy(), s64[k].numpy()))
    print("%-18s %-12s %-12s %-12s %-12s %s" % ("operation", "float32 dev", "8 x dev", "ops_gpu", "recorded", "bound"))
    for op, e in worst.items():
        print("%-18s %-12.3e %-12.3e %-12.1e %-12.1e %.2e" % (op, e, 8 * e, ds.FLOOR[op], ds.DEV32[op], ds.bound(op)))
        if e > ds.DEV32[op]:
            print("    (above decode_step_common.DEV32: record it there)")


if __name__ == "__main__":
    main()
