"""The float64 loop of tests/lstm_common.py - the reference of tests/test_lstm_gpu.py - is right, and the inputs of the case tables
are fair to the kernels.  No GPU, no library.

What the bars of test_lstm_gpu.py (1e-5 on everything the forward writes, 5e-5 on dxg; max-abs error over max-abs of the reference,
per tensor and direction) can and cannot resolve, measured with the loop itself (test_bar_resolves_the_second_row_of_the_split, H = 128,
B = 4, T = 13, both directions):
  - fp32 arithmetic instead of float64, every table case (H = 8 .. 1024, T = 1 .. 23, xg scale 1 and 6): at most 3e-7 on every tensor
    (test_inputs_are_well_conditioned asserts a quarter of the bars; the kernels compute in fp32, so this is their floor);
  - the state that enters the recurrent product cut to TWO of the three bf16 rows of the exact split of csrc/mfma_rec.h (xs_put):
    hout moves by 1.4e-6 - under the bar: a kernel that lost the third row would pass;
  - cut to ONE row (plain bf16 state): 1.1e-3 - a hundred times the bar.
So the bar catches the loss of the second row of the split (and anything coarser: a wrong mask bit, a stale state, a step stored to the
wrong row), not the loss of the third."""
import numpy as np
import pytest
import torch

import lstm_common as lc
from lstm_common import Case
from oracle import torch_ref


def _case(ndir, lengths, mode, H=8, B=3, T=6, seed=11):
    return Case(H, B, T, ndir, lengths, mode, 1.0, 0, 0, seed)


@pytest.mark.parametrize("mode", [lc.Z_TRAIN, lc.Z_EVAL, lc.Z_TRAIN_0H], ids=["train", "eval", "train0h"])
@pytest.mark.parametrize("lengths", [None, (6, 2, 5), (1, 6, 0)], ids=["nolen", "len", "len0"])
@pytest.mark.parametrize("ndir", [1, 2])
def test_reference_equals_the_oracle(ndir, lengths, mode):
    """hout and the gradient wrt xg against oracle.torch_ref.zoneout_lstm_seq (identity input weights: xg enters as the input)"""
    case = _case(ndir, lengths, mode)
    inp, ref = lc.inputs(case), lc.reference(case)
    H, (training, zc, zh) = case.H, mode
    sc, sh = lc.streams(case)
    xr = torch.tensor(inp.xg, dtype=torch.float64, requires_grad=True)
    outs = []
    for d in range(ndir):
        W = torch.cat([torch.eye(4 * H, dtype=torch.float64), torch.tensor(inp.Wh[d], dtype=torch.float64)], 0)
        outs.append(torch_ref.zoneout_lstm_seq(xr[d], W, torch.zeros(4 * H, dtype=torch.float64), H,
                                               None if lengths is None else torch.tensor(inp.lengths), d == 1, zc, zh, training,
                                               case.seed, (sc[d], sh[d])))
    y = torch.cat(outs, -1)
    y.backward(torch.tensor(inp.dh, dtype=torch.float64))
    lc.close("hout", ref["hout"], y, 1e-12, ndir, "reference vs oracle")
    lc.close("dxg", ref["dxg"], xr.grad, 1e-12, ndir, "reference vs oracle")


def test_dxg_matches_central_differences():
    case = Case(8, 2, 3, 2, (3, 2), lc.Z_EVAL, 1.0, 0, 0, 5)
    inp, ref = lc.inputs(case), lc.reference(case)
    dh = torch.tensor(inp.dh, dtype=torch.float64)
    masks = lc.keep_masks(case)

    def f(x):
        return float((lc.reference_from(x, inp.Wh, None, inp.lengths, case.mode, masks)["hout"] * dh).sum())

    x0 = inp.xg.astype(np.float64)
    fd = np.zeros_like(x0)
    eps = 1e-5
    for i in range(x0.size):
        xp, xm = x0.copy(), x0.copy()
        xp.flat[i] += eps
        xm.flat[i] -= eps
        fd.flat[i] = (f(xp) - f(xm)) / (2 * eps)
    lc.close("dxg", ref["dxg"], torch.tensor(fd), 1e-6, case.ndir, "autograd vs central differences")


def test_saved_tensor_semantics_of_the_reference():
    case = Case(24, 3, 5, 2, (5, 0, 3), lc.Z_TRAIN, 1.0, 0, 0, 9)
    ref, masks = lc.reference(case), lc.keep_masks(case)
    H = case.H
    hout = torch.stack(ref["hout"].chunk(2, dim=-1))          # [ndir, B, T, H]
    for b, L in enumerate(case.lengths):
        for n in lc.SAVED + ("dxg",):
            assert float(ref[n][:, b, L:].abs().max() if L < case.T else 0.0) == 0.0, (n, b)
        assert float(hout[:, b, L:].abs().max() if L < case.T else 0.0) == 0.0
        if L == 0:
            assert all(float(ref[n][:, b].abs().max()) == 0.0 for n in lc.SAVED + ("dxg",)) and float(hout[:, b].abs().max()) == 0.0
    kept = 0
    for d in range(2):
        kc, kh = (torch.from_numpy(m) for m in masks[d])
        for b, L in enumerate(case.lengths):
            mh, mc = kh[b, :L], kc[b, :L]
            assert torch.equal(ref["hstate"][d, b, :L][mh], hout[d, b, :L][mh])          # kept: the new value, exactly
            assert torch.equal(ref["cstate"][d, b, :L][mc], ref["cnew"][d, b, :L][mc])
            assert not torch.equal(ref["hstate"][d, b, :L][~mh], hout[d, b, :L][~mh]) or int((~mh).sum()) == 0
            kept += int(mh.sum())
            # not kept: the state of the step walked before (zero in front of the first)
            order = [L - 1 - s if d == 1 else s for s in range(L)]
            for s, t in enumerate(order):
                prev = ref["hstate"][d, b, order[s - 1]] if s > 0 else torch.zeros(H, dtype=torch.float64)
                assert torch.equal(ref["hstate"][d, b, t][~kh[b, t]], prev[~kh[b, t]])
    assert kept > 0
    # gates are the four activations: inside their ranges, the forget gate carries the + 1
    assert float(ref["gates"].min()) >= -1.0 and float(ref["gates"].max()) <= 1.0


@pytest.mark.parametrize("case", lc.ALL_RECURRENT, ids=lc.case_id)
def test_inputs_are_well_conditioned(case):
    """the loop in numpy fp32 stays under a quarter of the bars against float64 on every case of the tables - a kernel that computes in
    fp32 has three quarters of the bar for its own order of operations; the numpy loop in float64 (backward written out by hand, as
    the kernels do it) agrees with the autograd reference to rounding"""
    ref = lc.reference(case)
    f32, f64 = lc.case_numpy(case, np.float32), lc.case_numpy(case, np.float64)
    for n in lc.FWD_NAMES + ("dxg",):
        lc.close(n, f64[n], ref[n], 1e-12, case.ndir, "numpy f64 vs reference")
        lc.close(n, f32[n], ref[n], lc.bar(n) / 4, case.ndir, "numpy f32 vs reference")
        assert bool(torch.isfinite(ref[n]).all())


def test_bar_resolves_the_second_row_of_the_split():
    case = next(c for c in lc.SINGLE if c.H == 128 and c.T == 13 and c.scale == 1.0)
    ref = lc.reference(case)
    one = max(lc.rel_errs("hout", lc.case_numpy(case, np.float64, state_rows=1)["hout"], ref["hout"], case.ndir))
    two = max(lc.rel_errs("hout", lc.case_numpy(case, np.float64, state_rows=2)["hout"], ref["hout"], case.ndir))
    three = max(lc.rel_errs("hout", lc.case_numpy(case, np.float64, state_rows=3)["hout"], ref["hout"], case.ndir))
    print("hout moved by: one row %.3e, two rows %.3e, three rows %.3e (bar %.1e)" % (one, two, three, lc.BAR_FWD))
    assert one > lc.BAR_FWD          # the bar sees a state cut to plain bf16
    assert three < lc.BAR_FWD / 4    # and the exact split costs what fp32 costs
