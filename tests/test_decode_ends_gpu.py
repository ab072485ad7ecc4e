"""satt_dec_ends_scan (csrc/decode_ends.hip), the per-utterance stop behind a decode launch, against its NumPy model
(tests/decode_ends_common.py: numpy_ends) on synthetic yout buffers.  Integers must be EQUAL.  Every input keeps its stop logits at
least 1e-3 away from logit(threshold) (asserted by the builder), so the fp32 sigmoid of the kernel and the float64 comparison of
the model cannot disagree about a step.

What can go wrong in the kernel: which wave owns which sample (b = wave, wave + 4, ...: B = 1 .. 33), which lane owns which step
(strides of 64: windows of 1 .. 300 steps), the wave-wide minimum (the FIRST qualifying step wins, wherever its lane sits), the
min_steps boundary, stickiness across calls, and the flag (all samples ended, the maximum, written once)."""
import numpy as np
import pytest
import torch

from decode_ends_common import logit, margin_ok, numpy_ends, synthetic_yout

pytestmark = pytest.mark.gpu

THR = 0.5


def scan(y, windows, min_steps, thr=THR, ends=None, flag=0):
    """the kernel over the consecutive `windows` (t0, n) of yout `y`, against the model after EVERY call; returns [(ends, flag)]"""
    from satt_amd import ops
    B, rows, NO = y.shape
    yd = torch.as_tensor(y).cuda()
    e_ref = np.zeros(B, np.int64) if ends is None else np.array(ends, np.int64)
    f_ref = int(flag)
    ed = torch.as_tensor(e_ref.astype(np.int32)).cuda()
    fd = torch.full((1,), f_ref, dtype=torch.int32, device="cuda")
    seen = []
    for t0, n in windows:
        ops.dec_ends_scan(yd, B, rows, NO, t0, n, min_steps, thr, ed, fd)
        e_ref, f_ref = numpy_ends(y, t0, n, min_steps, thr, e_ref, f_ref)
        e, f = ed.cpu().numpy().astype(np.int64), int(fd.item())
        assert np.array_equal(e, e_ref) and f == f_ref, ("window", t0, n, e.tolist(), e_ref.tolist(), f, f_ref)
        seen.append((e, f))
    assert torch.equal(yd.cpu(), torch.as_tensor(y))          # the scan writes nothing but ends and flag
    return seen


@pytest.mark.parametrize("nsteps", [1, 32, 63, 64, 65, 128, 300])
@pytest.mark.parametrize("B", [1, 2, 3, 5, 16, 17, 33])
def test_one_window(B, nsteps):
    """random ends: per sample none, one or two qualifying steps anywhere in the window (first and last step included); then the
    same with every sample ending, which raises the flag"""
    g = np.random.default_rng(1000 * B + nsteps)
    t0 = int(g.integers(0, 5))
    rows = t0 + nsteps + 1 + int(g.integers(0, 3))
    for everyone in (False, True):
        fires = []
        for b in range(B):
            k = int(g.integers(1, 3)) if everyone else int(g.integers(0, 3))
            if b == 0 and everyone:
                fires.append((b, t0 + nsteps - 1))                        # the last step of the window
            elif b == 1 and everyone:
                fires += [(b, t0), (b, t0 + nsteps - 1)]                  # the first step (and a later one)
            else:
                fires += [(b, t0 + int(s)) for s in g.integers(0, nsteps, k)]
        y = synthetic_yout(g, B, rows, 161, THR, fires)
        (e, f), = scan(y, [(t0, nsteps)], -1)
        if everyone:
            assert (e > 0).all() and f == e.max()
            assert e[0] == t0 + nsteps and (B < 2 or e[1] == t0 + 1)
        print("B=%d nsteps=%d t0=%d everyone=%s ends=%s flag=%d" % (B, nsteps, t0, everyone, e.tolist(), f))


@pytest.mark.parametrize("NO", [161, 5])
def test_min_steps_boundary_and_first_of_two(NO):
    g = np.random.default_rng(NO)
    # sample 0 qualifies AT min_steps (must not fire) and again later; sample 1 at min_steps + 1 (must); sample 2 three times: in the
    # whole-run window steps 75 and 77 sit in lanes 11 and 13, step 130 in lane 2 - the minimum is over steps, not over lanes
    y = synthetic_yout(g, 3, 140, NO, THR, [(0, 20), (0, 90), (1, 21), (2, 75), (2, 77), (2, 130)])
    for windows in ([(0, 139)], [(0, 20), (20, 1), (21, 1), (22, 100), (122, 17)], [(15, 10), (25, 114)]):
        seen = scan(y, windows, 20)
        e, f = seen[-1]
        assert e.tolist() == [91, 22, 76] and f == 91, (windows, e, f)
    e, f = scan(y, [(20, 1)], 20)[0]          # t0 + s == min_steps alone: nothing
    assert not e.any() and f == 0
    e, f = scan(y, [(21, 1)], 20)[0]
    assert e.tolist() == [0, 22, 0] and f == 0


def test_ends_over_three_calls_are_sticky_and_the_flag_comes_last():
    g = np.random.default_rng(7)
    B = 6
    # ends in launches 1, 2 and 3 (32 steps each); samples that ended qualify AGAIN later, which must not move them
    fires = [(0, 12), (0, 40), (1, 31), (1, 95), (2, 32), (3, 63), (3, 64), (4, 70), (5, 95), (2, 80)]
    y = synthetic_yout(g, B, 129, 161, THR, fires)
    seen = scan(y, [(0, 32), (32, 32), (64, 32), (96, 32)], 10)
    assert seen[0][0].tolist() == [13, 32, 0, 0, 0, 0] and seen[0][1] == 0
    assert seen[1][0].tolist() == [13, 32, 33, 64, 0, 0] and seen[1][1] == 0
    assert seen[2][0].tolist() == [13, 32, 33, 64, 71, 96] and seen[2][1] == 96          # the call in which the last sample ends
    assert np.array_equal(seen[3][0], seen[2][0]) and seen[3][1] == 96                    # a call after the flag fired changes nothing
    # ... even one whose window would end a sample earlier or whose ends are still open: the flag is looked at first
    open_ends = [13, 0, 33, 64, 71, 96]
    (e, f), = scan(y, [(0, 128)], 10, ends=open_ends, flag=96)
    assert e.tolist() == open_ends and f == 96


def test_a_sample_that_never_ends_keeps_the_flag_down():
    g = np.random.default_rng(8)
    for B, never in ((1, 0), (5, 4), (5, 0), (17, 16), (33, 7)):
        fires = [(b, 5 + 3 * b) for b in range(B) if b != never]
        y = synthetic_yout(g, B, 120, 5, THR, fires)
        seen = scan(y, [(0, 64), (64, 55)], 0)
        e, f = seen[-1]
        assert e[never] == 0 and f == 0 and all(e[b] == 6 + 3 * b for b in range(B) if b != never)


def test_rows_bound():
    """the last row a window may read is rows - 1 (t0 + nsteps < rows); one step more is refused before any launch"""
    from satt_amd import _lib, ops
    g = np.random.default_rng(9)
    y = synthetic_yout(g, 2, 9, 161, THR, [(0, 7), (1, 7)])
    (e, f), = scan(y, [(0, 8)], 0)
    assert e.tolist() == [8, 8] and f == 8
    yd = torch.as_tensor(y).cuda()
    ed, fd = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    for t0, n in ((0, 9), (1, 8), (8, 1)):
        with pytest.raises(_lib.SattError):
            ops.dec_ends_scan(yd, 2, 9, 161, t0, n, 0, THR, ed, fd)
    torch.cuda.synchronize()
    assert not ed.any() and not fd.any()


def test_other_thresholds_use_the_step_loops_expression():
    """thresholds away from 0.5, logits placed 2e-3 on either side of logit(thr): the decision is sigmoid(x) > thr in fp32"""
    g = np.random.default_rng(10)
    for thr in (0.1, 0.3, 0.9, 0.999):
        x = logit(thr)
        y = synthetic_yout(g, 4, 40, 161, thr)
        y[0, 11, -1] = np.float32(x + 2e-3)
        y[1, 12, -1] = np.float32(x - 2e-3); y[1, 20, -1] = np.float32(x + 2e-3)
        y[2, 13, -1] = np.float32(x + 2e-3)
        y[3, 14, -1] = np.float32(x + 2e-3)
        assert margin_ok(y[:, :, -1], thr)
        (e, f), = scan(y, [(0, 39)], 5, thr=thr)
        assert e.tolist() == [11, 20, 13, 14] and f == 20, (thr, e, f)
