"""CPU checks of tests/decode_step_common.py: the references of tests/test_decode_step_gpu.py against the oracle's own functions,
the LSTM column regrouping against the expression DecodeSession.refresh_folded uses, and every case list against the coverage
conditions it was written to meet.  No GPU, no library call."""
import numpy as np
import torch

import decode_step_common as ds
from common import SMALL, make_params, small_batch
from oracle import torch_ref


def test_self_attention_reference_is_the_last_row_of_sdpa():
    for (D, heads), t in zip(((16, 2), (96, 3), (256, 2)), (0, 5, 12)):
        B, Td, hd = 2, 13, D // heads
        kvq = ds.sa_cache(B, Td, D, heads).double()
        got = ds.self_attn_ref(kvq, t, D, heads)
        split = lambda x: x.reshape(B, t + 1, heads, hd).permute(0, 2, 1, 3)
        rows = kvq[:, :t + 1]
        # every row's own query, causal mask: row t sees rows 0 .. t
        out, _ = torch_ref.sdpa(split(rows[:, :, 2 * D:]), split(rows[:, :, :D]), split(rows[:, :, D:2 * D]), True, 0.0, False, 0, 0)
        want = out[:, :, -1].reshape(B, D)
        assert float((got - want).abs().max()) < 1e-13


def test_lstm_regrouping_is_the_sessions_permutation():
    for H in (8, 64, 256):
        K = 5
        W = torch.arange(K * 4 * H, dtype=torch.float32).reshape(K, 4 * H)
        Wg = ds.regroup_lstm(W, H)
        dst = torch.empty(K, 4 * H)          # satt_amd/inference.py DecodeSession.refresh_folded, the statement itself
        dst.view(K, H // 8, 4, 8).copy_(W.view(K, 4, H // 8, 8).permute(0, 2, 1, 3))
        assert torch.equal(Wg, dst)
        idx = ds.regroup_index(H)          # column gate * H + u -> (u // 8) * 32 + gate * 8 + u % 8
        assert sorted(idx.tolist()) == list(range(4 * H))
        assert torch.equal(Wg[:, torch.as_tensor(idx)], W)
        assert torch.equal(ds.ungroup_lstm(Wg, H), W)


def test_chained_attention_reference_reproduces_the_oracles_decode():
    """the alignments of torch_ref.infer (SMALL, 6 steps) from the queries it formed, through attention_chain"""
    cfg, P = make_params(SMALL, seed=1)
    batch = small_batch(cfg, 3, 9, 12, seed=3)
    mv = {n: (torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64))
          for n, c in (("bank", cfg.max_filter_width * cfg.conv_channels), ("proj1", cfg.proj1), ("proj2", cfg.proj2))}
    Pt = torch_ref.to_torch(P)
    seen = dict(q=[])
    real1, real2 = torch_ref.forward_attention_step, torch_ref.additive_attention_step

    def spy1(query, keys, state, P_, lengths, mode="forward", cumulative=False, values=None, agent=False):
        seen["q"].append(query); seen.update(keys1=keys, values1=values, lens=lengths, mode=mode, cumulative=cumulative, agent=agent)
        return real1(query, keys, state, P_, lengths, mode, cumulative, values, agent)

    def spy2(query, keys, P_, lengths):
        seen["keys2"] = keys
        return real2(query, keys, P_, lengths)
    torch_ref.forward_attention_step, torch_ref.additive_attention_step = spy1, spy2
    try:
        ref = torch_ref.infer(Pt, torch.as_tensor(batch["source"]), torch.as_tensor(batch["source_length"]), torch_ref.Cfg(**SMALL), 6, mv,
                              min_steps=10 ** 6)
    finally:
        torch_ref.forward_attention_step, torch_ref.additive_attention_step = real1, real2
    assert ref["steps"] == 6 and len(seen["q"]) == 6
    values2 = seen["keys2"].new_zeros(seen["keys2"].shape[0], seen["keys2"].shape[1], 4)
    steps = ds.attention_chain(seen["keys1"], seen["values1"], seen["keys2"], values2, torch.stack(seen["q"]), Pt, seen["lens"],
                               seen["mode"], seen["cumulative"], seen["agent"])
    for t, s in enumerate(steps):
        assert float((s["align1"] - ref["alignment1"][:, t]).abs().max()) < 1e-14
        assert float((s["align2"] - ref["alignment2"][:, t]).abs().max()) < 1e-14
        assert float((s["align1"].sum(-1) - 1).abs().max()) < 1e-12


def test_case_lists_meet_their_coverage_conditions():
    ds.lin_coverage(ds.LIN_CASES)
    ds.lstm_coverage(ds.LSTM_CASES)
    ds.l2_coverage(ds.L2_CASES)
    ds.chain_coverage(ds.CHAIN_CASES)
    ds.att_coverage(ds.ATT_CASES)
    assert ds.DROP_CASE.step == 3 and ds.DROP_CASE.B == 3 and ds.LIN_SHAPES[ds.DROP_CASE.shape][1] == 161 and ds.DROP_T == 7
    assert set(ds.DROP_RATES) == {0.5, 0.1}
    t = {c.name: c for c in ds.STOP_CASES}
    assert t["t0"].t == 0 and [t[n].t - 1 - ds.STOP_MIN for n in ("t-1=min-1", "t-1=min", "t-1=min+1")] == [-1, 0, 1]
    assert [t[n].want for n in ("t-1=min-1", "t-1=min", "t-1=min+1")] == [0, 0, ds.STOP_MIN + 2]
    assert t["B70_one_low"].B == 70 and list(t["B70_one_low"].logits) == [69] and t["sticky"].flag0 != 0
    assert set(ds.SA_PROD_T) == {0, 1, 63, 64, 255, 256, 257, 1023, 1024, 1030} and ds.SA_PROD["Td"] % 4 != 0
    assert all(ds.bound(op) >= ds.FLOOR[op] and ds.bound(op) <= max(ds.FLOOR[op], 8 * ds.DEV32[op]) for op in ds.DEV32)


def test_stop_threshold_equality_logit():
    """the logit of the `equal` case: its float32 sigmoid, formed as the kernel forms it, IS the threshold"""
    x = np.float32(ds.STOP_EQUAL_LOGIT)
    sgm = np.float32(1) / (np.float32(1) + np.exp(-x, dtype=np.float32))
    assert sgm == np.float32(ds.STOP_THRESHOLD) and not (sgm > np.float32(ds.STOP_THRESHOLD))
    case = next(c for c in ds.STOP_CASES if c.name == "equal")
    z = ds.stop_logits(case, case.t + 1)
    assert float(z[1, case.t - 1]) == 0.0 and bool((z[[0, 2], case.t - 1] > 0).all())


def test_agent_cases_are_not_vacuous():
    """the transition agent moves the float64 alignments of every agent case by more than 1e-3"""
    for c in (c for c in ds.ATT_CASES if c.mode == "agent"):
        on, off = ds.att_ref64(c), ds.att_ref(c, agent=False)
        moved = max(float((a["align1"] - b["align1"]).abs().max()) for a, b in zip(on, off))
        assert moved > 1e-3, (c, moved)


def test_attention_regimes_and_references():
    """the regimes of the self-attention cases are what their names say; the dense reference honours mask, scale and residual order"""
    p = ds.SA_PROD
    D, heads, t = p["D"], p["heads"], ds.SA_REGIME_T
    hd = D // heads
    for regime in ("sharp", "offset"):
        kvq = ds.sa_cache(p["B"], p["Td"], D, heads, regime).double()
        k = kvq[:, :t + 1, :D].reshape(p["B"], t + 1, heads, hd)
        s = torch.einsum("bhd,bjhd->bhj", kvq[:, t, 2 * D:].reshape(p["B"], heads, hd), k) / np.sqrt(hd)
        if regime == "sharp":
            assert float(torch.softmax(s, -1).max(-1).values.min()) > 0.999
        else:
            assert float(s.min()) > 90 and float(s.max()) < 110
    x, W = torch.ones(2, 3), torch.ones(3, 2)
    keep = torch.tensor([[True, False], [False, True]])
    y = ds.dense_ref([x], W, None, ds.ACT_NONE, keep, 2.0, torch.full((2, 2), 10.0))
    assert y.tolist() == [[16.0, 10.0], [10.0, 16.0]]
