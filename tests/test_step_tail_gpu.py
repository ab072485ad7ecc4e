"""The tail of every training step, kernel by kernel against float64: the two loss forms (loss_sums_k + loss_grad_k and the
one-launch loss_fused_k) with spec_loss_type l1 and mse, the L2 regulariser, the fixed-order sum of squares, and
adam_prepare_k + adam_k (clip, data-parallel gradient scale, rate schedule, bias correction, eps placement, skip counters).

References are float64: oracle/torch_ref.py's losses + autograd, and adam_ref below.  adam_ref takes the hyper-parameters as
the kernel receives them (rounded to fp32): with exact 0.9 / 0.999 the float64 lr_t differs from ANY fp32 evaluation by up to
1e-5 at t = 2, which is a property of the constants, not of the kernel.

Bars: 2e-6 (relative to the largest reference magnitude) for the loss values and gradients; LONG_SUM_BAR for the loss values
of the cases whose fp32 sum runs over more than 4096 decoder steps (measured, profiles/step_tail_tests.txt); 1e-5 for the sum
of squares, for lr_t and the clip scale (3 x the 3.4e-6 of an fp32 evaluation of adam_prepare_k's formulas over steps
0 .. 1e6) and for p, m, v."""
import functools
import math

import numpy as np
import pytest
import torch

import satt_amd  # noqa: F401
from oracle import torch_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 12345.0          # fill of everything a kernel must leave alone
# loss values of the long sums (> 4096 decoder steps, or the 2.1 M-element two-kernel case): 3 x the largest error measured on
# the MI355X against the float64 reference - 3.65e-7 over 32 figures, the atomics' order moves it from call to call
# (profiles/step_tail_tests.txt) -, which stays under the cap of 2e-5 and under the 2e-6 of the short sums
LONG_SUM_BAR = 1.1e-6


def T(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32, device=DEV).contiguous()


def rel(a, b):
    """max |a - b| / max |b|, no floor: the optimiser cases with 1e-9 gradients have moments of 1e-21"""
    a = a.detach().double().cpu() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))
    b = b.detach().double().cpu() if isinstance(b, torch.Tensor) else torch.as_tensor(np.asarray(b, dtype=np.float64))
    assert a.shape == b.shape, (a.shape, b.shape)
    den = float(b.abs().max())
    assert den > 0 and bool(torch.isfinite(b).all())
    if not bool(torch.isfinite(a).all()):
        return float("inf")
    return float((a - b).abs().max()) / den


def close(a, b, tol, what):
    err = rel(a, b)
    print("%-44s rel_err=%.3e (bar %.1e)" % (what, err, tol))
    assert err < tol, (what, err, tol)
    return err


# ---------------------------------------------------------------------------------------------- losses
class LossCase:
    """one seeded problem in the decoder head's layout: y [B*Td, r*nm + 1] = [mel frames of the step | stop logit]"""

    def __init__(self, B, Td, r, nm, seed, mask="random"):
        g = np.random.default_rng(seed)
        self.B, self.Td, self.r, self.nm, self.Tm, self.rn, self.NO = B, Td, r, nm, Td * r, r * nm, r * nm + 1
        self.rows = B * Td
        tgt = g.normal(0, 1, (B, self.Tm, nm)).astype(np.float32)
        # the differences come from a continuous distribution bounded away from zero: the L1 gradient is sign(d), and an
        # element within fp32 rounding of zero would make the bar measure the reference's rounding, not the kernel
        d = (0.01 + g.exponential(0.8, tgt.shape)) * (g.integers(0, 2, tgt.shape) * 2 - 1)
        mel = (tgt.astype(np.float64) + d).astype(np.float32)
        stop = g.normal(0, 2, (B, Td)).astype(np.float32)
        self.y = np.concatenate([mel.reshape(self.rows, self.rn), stop.reshape(self.rows, 1)], 1)
        self.tgt = tgt
        self.sm = (g.random((B, self.Tm)) > 0.3).astype(np.float32)
        self.bm = (g.random((B, Td)) > 0.3).astype(np.float32)
        self.done = (g.random((B, Td)) > 0.7).astype(np.float32)
        if mask == "sample_masked":             # one sample contributes nothing, to either loss
            self.sm[B - 1] = 0; self.bm[B - 1] = 0
        elif mask == "last_frame":              # the mask is per FRAME: exactly the last frame of every second step is off
            assert r >= 2
            self.sm[:] = 1
            self.sm.reshape(B, Td, r)[:, 1::2, r - 1] = 0
        else:
            assert mask == "random"
        assert self.sm.sum() > 0 and self.bm.sum() > 0
        # checked on the float64 side, over EVERY element (none is left out of the comparison below)
        d64 = self.y[:, :self.rn].astype(np.float64).reshape(B, self.Tm, nm) - tgt.astype(np.float64)
        assert d64.size == B * self.Tm * nm and float(np.abs(d64).min()) > 1e-3

    @functools.lru_cache(maxsize=None)
    def ref(self, loss_type):
        """float64 [mel_loss, done_loss, loss] and d loss / d y of torch_ref.losses"""
        yr = torch.tensor(self.y, dtype=torch.float64, requires_grad=True)
        mel = yr[:, :self.rn].reshape(self.B, self.Tm, self.nm)
        stop = yr[:, self.rn:].reshape(self.B, self.Td, 1)
        f64 = lambda a: torch.tensor(a, dtype=torch.float64)
        bt = dict(mel=f64(self.tgt), spec_loss_mask=f64(self.sm), done=f64(self.done), binary_loss_mask=f64(self.bm))
        ml, dl = torch_ref.losses(mel, stop, bt, loss_type)
        (ml + dl).backward()
        return torch.stack([ml, dl, ml + dl]).detach(), yr.grad

    @functools.lru_cache(maxsize=None)
    def dev(self):
        return T(self.y), T(self.tgt), T(self.sm), T(self.done), T(self.bm)


@functools.lru_cache(maxsize=None)
def loss_case(B, Td, r, nm, seed=9, mask="random"):
    return LossCase(B, Td, r, nm, seed, mask)


def check_loss(c, loss_type, losses, dmel, dstop, what, loss_bar=2e-6):
    lref, gref = c.ref(loss_type)
    errs = [close(losses, lref, loss_bar, what + " losses")]
    if dmel is not None:
        errs.append(close(dmel, gref[:, :c.rn], 2e-6, what + " d mel"))
    if dstop is not None:
        errs.append(close(dstop, gref[:, c.rn:], 2e-6, what + " d stop"))
    return errs


def two_kernel(c, l2, want_dmel=True, want_dstop=True, postnet_layout=False):
    """satt_loss_fwd_bwd.  postnet_layout: the mel rows are a buffer of their own (leading dimension r*nm) and the stop logits
    are read from another one, as in the PostNetV2 call."""
    from satt_amd import ops
    y, tgt, sm, done, bm = c.dev()
    rn, NO = c.rn, c.NO
    losses = torch.full((3,), SENT, device=DEV); ws = torch.full((4,), SENT, device=DEV)
    if postnet_layout:
        mel, mel_ld = y[:, :rn].contiguous(), rn
        stopb = torch.full((c.rows, 3), SENT, device=DEV); stopb[:, 0] = y[:, rn]
        stop, stop_ld = stopb, 3
    else:
        mel, mel_ld, stop, stop_ld = y, NO, y[:, rn:], NO
    dy = torch.full((c.rows, NO), SENT, device=DEV)
    dmel = dy if want_dmel else None
    dstop = dy[:, rn:] if want_dstop else None
    ops.loss_fwd_bwd(mel, mel_ld, tgt, sm, stop, stop_ld, done, bm, c.B, c.Tm, c.nm, c.Td, l2, losses, dmel, NO,
                     dstop, NO if want_dstop else 0, ws)
    torch.cuda.synchronize()
    if not want_dmel:
        assert bool((dy[:, :rn] == SENT).all())
    if not want_dstop:
        assert bool((dy[:, rn:] == SENT).all())
    return losses, (dy[:, :rn] if want_dmel else None), (dy[:, rn:] if want_dstop else None)


def fused(c, l2, layout):
    """satt_loss_mask_sums + satt_loss_fwd_bwd_presummed.
    tight: rows of r*nm + 1;  padded: the engine's rows [mel | stop | pad] of whole 8-column groups, pad pre-filled with NaN;
    split: d stop in a buffer of its own and a d mel buffer with 5 spare columns per row."""
    from satt_amd import ops
    y, tgt, sm, done, bm = c.dev()
    rn, NO, rows = c.rn, c.NO, c.rows
    losses = torch.full((3,), SENT, device=DEV); ws = torch.full((8,), SENT, device=DEV)
    ops.loss_mask_sums(sm, bm, c.B, c.Tm, c.Td, ws)
    if layout == "padded":
        NOp = NO + (-NO) % 8
        assert NOp > NO
        yp = torch.full((rows, NOp), float("nan"), device=DEV); yp[:, :NO] = y
        dyp = torch.full((rows, NOp), float("nan"), device=DEV)
        ops.loss_fwd_bwd_presummed(yp, NOp, tgt, sm, yp[:, rn:], NOp, done, bm, c.B, c.Tm, c.nm, c.Td, l2, losses,
                                   dyp, NOp, dyp[:, rn:], NOp, ws)
        torch.cuda.synchronize()
        assert bool((dyp[:, NO:] == 0).all()), "the pad columns come back exactly 0"
        return losses, dyp[:, :rn], dyp[:, rn:NO]
    if layout == "split":
        dm = torch.full((rows, rn + 5), SENT, device=DEV); ds = torch.full((rows, 3), SENT, device=DEV)
        ops.loss_fwd_bwd_presummed(y, NO, tgt, sm, y[:, rn:], NO, done, bm, c.B, c.Tm, c.nm, c.Td, l2, losses,
                                   dm, rn + 5, ds, 3, ws)
        torch.cuda.synchronize()
        # no pad promise in this form: nothing of a gradient row outside [0, r*nm) and the stop column is touched
        assert bool((dm[:, rn:] == SENT).all()) and bool((ds[:, 1:] == SENT).all())
        return losses, dm[:, :rn], ds[:, :1]
    assert layout == "tight"
    dy = torch.full((rows, NO), SENT, device=DEV)
    ops.loss_fwd_bwd_presummed(y, NO, tgt, sm, y[:, rn:], NO, done, bm, c.B, c.Tm, c.nm, c.Td, l2, losses,
                               dy, NO, dy[:, rn:], NO, ws)
    torch.cuda.synchronize()
    return losses, dy[:, :rn], dy[:, rn:]


LT = {False: "l1", True: "mse"}
# (r, num_mels): (2, 5) puts a frame boundary inside one 64-column block; r*nm = 64, 65, 192, 193 sit on and beside the ends of
# the 64-column block and of the 192-column pass of loss_fused_k; (3, 70) is the shape of test_ops_gpu.test_loss_kernels.
# pad columns of the engine's rows: 5, 7, 6, 7, 6, 5
ROW_SHAPES = [(2, 5), (1, 64), (1, 65), (3, 64), (1, 193), (3, 70)]


@pytest.mark.parametrize("l2", [False, True])
@pytest.mark.parametrize("r,nm", ROW_SHAPES)
def test_loss_row_shapes(r, nm, l2):
    """both API forms at B*Td = 21 decoder steps (two workgroups of the fused kernel), every gradient layout"""
    c = loss_case(3, 7, r, nm)
    check_loss(c, LT[l2], *two_kernel(c, l2), "two-kernel")
    for layout in ("tight", "padded", "split"):
        check_loss(c, LT[l2], *fused(c, l2, layout), "fused " + layout)


@pytest.mark.parametrize("l2", [False, True])
@pytest.mark.parametrize("mask", ["sample_masked", "last_frame"])
def test_loss_masks(mask, l2):
    """a sample that is masked out entirely (its gradient rows are exactly zero), and a spectrogram mask that is off on exactly
    the last frame of a decoder step: the mask is indexed per frame, not per step"""
    c = loss_case(3, 7, 2, 5, mask=mask)
    outs = [two_kernel(c, l2), fused(c, l2, "tight"), fused(c, l2, "padded")]
    for what, o in zip(("two-kernel", "fused tight", "fused padded"), outs):
        check_loss(c, LT[l2], *o, what + " " + mask)
        if mask == "sample_masked":
            assert bool((o[1][-c.Td:] == 0).all()) and bool((o[2][-c.Td:] == 0).all())
        else:
            dm = o[1].reshape(c.B, c.Td, c.r, c.nm)
            assert bool((dm[:, 1::2, c.r - 1] == 0).all()) and bool((dm[:, 1::2, 0] != 0).all())


# B*Td of the fused kernel at num_mels = 3, r = 2 (rows of 7 floats, one pad column in the engine's layout): one wave per
# decoder step, 16 waves per workgroup, at most 256 workgroups = 4096 waves; a wave unrolls 4 rows that are 4096 apart
FUSED_STEPS = [(3, 5), (2, 8), (1, 17),         # 15, 16, 17: one workgroup not full, full, and a second one
               (4, 1024), (17, 241),            # 4096 and 4097: the grid reaches its cap; the unroll's second row starts
               (1, 8191),                       # a partial unroll: rows 0, 1 and some of 2 of every wave's four
               (5, 3277)]                       # 16385: a second pass of the row0 loop, whose prefetch clamps at nrows - 1


@pytest.mark.parametrize("l2", [False, True])
@pytest.mark.parametrize("B,Td", FUSED_STEPS)
def test_loss_fused_step_counts(B, Td, l2):
    c = loss_case(B, Td, 2, 3, seed=B * Td)
    assert c.rows == B * Td and c.NO == 7
    bar = LONG_SUM_BAR if c.rows > 4096 else 2e-6
    for layout in ("tight", "padded"):
        check_loss(c, LT[l2], *fused(c, l2, layout), "fused %s B*Td=%d" % (layout, c.rows), loss_bar=bar)


@pytest.mark.parametrize("l2", [False, True])
@pytest.mark.parametrize("r,nm", [(2, 5), (1, 64)])
def test_loss_two_kernel_optional_gradients(r, nm, l2):
    """dstop = NULL with the mel rows in a buffer of their own (the PostNetV2 call), and no gradient at all (losses only)"""
    c = loss_case(3, 7, r, nm)
    check_loss(c, LT[l2], *two_kernel(c, l2, want_dstop=False, postnet_layout=True), "two-kernel, no d stop")
    check_loss(c, LT[l2], *two_kernel(c, l2, want_dmel=False, want_dstop=False), "two-kernel, losses only")
    check_loss(c, LT[l2], *two_kernel(c, l2, want_dmel=False, want_dstop=False, postnet_layout=True),
               "two-kernel, losses only, own mel buffer")


@pytest.mark.parametrize("l2", [False, True])
def test_loss_two_kernel_stride_loops(l2):
    """B*Tm*nm = 2 112 000: above the 131 072 threads of loss_sums_k's capped grid (16 elements per thread) and above 2 097 152,
    where loss_grad_k's loop takes a second element"""
    c = loss_case(33, 400, 2, 80, seed=33)
    assert c.B * c.Tm * c.nm > 2097152
    check_loss(c, LT[l2], *two_kernel(c, l2), "two-kernel 2.1 M", loss_bar=LONG_SUM_BAR)
    check_loss(c, LT[l2], *two_kernel(c, l2, want_dstop=False, postnet_layout=True), "two-kernel 2.1 M, no d stop",
               loss_bar=LONG_SUM_BAR)


def test_loss_presummed_twice_without_new_mask_sums():
    """include/satt_hip.h promises the presummed form's results only behind a satt_loss_mask_sums on the same workspace, which
    also resets the accumulators.  A second presummed call without one is outside that promise, and nothing of it is asserted."""
    from satt_amd import ops
    c = loss_case(3, 7, 2, 5)
    y, tgt, sm, done, bm = c.dev()
    rn, NO = c.rn, c.NO
    ws = torch.full((8,), SENT, device=DEV)
    args = lambda losses, dy: (y, NO, tgt, sm, y[:, rn:], NO, done, bm, c.B, c.Tm, c.nm, c.Td, False, losses, dy, NO, dy[:, rn:],
                               NO, ws)
    l1, l2_ = torch.full((3,), SENT, device=DEV), torch.full((3,), SENT, device=DEV)
    d1, d2 = torch.full((c.rows, NO), SENT, device=DEV), torch.full((c.rows, NO), SENT, device=DEV)
    ops.loss_mask_sums(sm, bm, c.B, c.Tm, c.Td, ws)
    ops.loss_fwd_bwd_presummed(*args(l1, d1))
    ops.loss_fwd_bwd_presummed(*args(l2_, d2))
    torch.cuda.synchronize()
    check_loss(c, "l1", l1, d1[:, :rn], d1[:, rn:], "presummed, first call")
    # Observed (and what the code says): the second call's gradients are right - they need only the mask sums - but its three
    # loss values are never written: the arrival counter in ws[4] goes on from the first call's count, so no workgroup sees
    # itself as the last one, and the numerators in ws[0] and ws[2] hold the sum of both calls.
    print("second call without mask sums: losses", l2_.tolist(), "ws", ws.tolist(),
          "gradients equal the first call's:", bool(torch.equal(d1, d2)))
    # the promise: mask sums again, and the workspace is good for the next step
    l3, d3 = torch.full((3,), SENT, device=DEV), torch.full((c.rows, NO), SENT, device=DEV)
    ops.loss_mask_sums(sm, bm, c.B, c.Tm, c.Td, ws)
    ops.loss_fwd_bwd_presummed(*args(l3, d3))
    torch.cuda.synchronize()
    check_loss(c, "l1", l3, d3[:, :rn], d3[:, rn:], "presummed, behind new mask sums")


# ---------------------------------------------------------------------------------------------- sum of squares
# 1 .. 5: below, on and above one float4; 255, 1023, 1025: a partial wave, a partial workgroup and one element more than one;
# 3*4096 + 2: four workgroups with a two-element scalar tail; 2048*4096 + 4099: past the 2048-partial cap (a workgroup sums
# several strides) with a three-element tail
SUMSQ_N = [1, 3, 4, 5, 255, 1023, 1025, 3 * 4096 + 2, 2048 * 4096 + 4099]


def run_sumsq(gd):
    from satt_amd import ops
    state = ops.opt_state(DEV)
    state[:4] = SENT
    ops.sumsq(gd, state)
    torch.cuda.synchronize()
    return state[0].clone()


@pytest.mark.parametrize("n", SUMSQ_N)
def test_sumsq(n):
    g = np.random.default_rng(n)
    vals = {"N(0,1)": g.normal(0, 1, n)}
    if n == 3 * 4096 + 2:
        vals["1e-6 .. 1e3"] = 10.0 ** g.uniform(-6, 3, n) * (g.integers(0, 2, n) * 2 - 1)
    for name, a in vals.items():
        a = a.astype(np.float32)
        gd = T(a)
        s1, s2 = run_sumsq(gd), run_sumsq(gd)
        want = float((a.astype(np.float64) ** 2).sum())
        err = abs(float(s1) - want) / want
        print("sumsq n=%d %s rel_err=%.3e" % (n, name, err))
        assert err < 1e-5, (n, name, float(s1), want)
        # the fixed summation order data parallelism relies on: the same buffer gives the same bits
        assert s1.view(torch.int32).item() == s2.view(torch.int32).item()
    # only the LAST element is non-zero: its square comes back exactly (the scalar tail and the ends of the strides, no tolerance)
    x = np.float32(1.7)
    z = torch.zeros(n, device=DEV); z[n - 1] = float(x)
    assert float(run_sumsq(z)) == float(x * x)


def test_sumsq_rejects_a_misaligned_buffer():
    """the float4 loads need 16-byte alignment: a view that starts at element 1 is the documented bad-argument error (a host
    return code: nothing is launched)"""
    from satt_amd import _lib, ops
    state = ops.opt_state(DEV)
    state[0] = SENT
    buf = torch.ones(1024 + 1, device=DEV)
    with pytest.raises(_lib.SattError, match="bad argument"):
        ops.sumsq(buf[1:], state)
    torch.cuda.synchronize()
    assert float(state[0]) == SENT


# ---------------------------------------------------------------------------------------------- Adam
def f32(x):
    return float(np.float32(x))


HP = dict(lr0=5e-4, decay=True, step_factor=1.0, b1=0.9, b2=0.999, eps=1e-8, clip=1.0, grad_scale=1.0)


def adam_ref(p, m, v, g, step, hp):
    """tf.clip_by_global_norm + tf.train.AdamOptimizer (epsilon on the UNcorrected sqrt(v)) + the reference's rate schedule, in
    float64 on float64 arrays; `step` is the 0-based global step before the update.  The hyper-parameters are rounded to fp32
    first, as the kernel receives them.  Returns p, m, v and (global norm, lr_t, gradient scale) = state[1..3]."""
    lr0, sf, b1, b2, eps, clip, gs = (f32(hp[k]) for k in ("lr0", "step_factor", "b1", "b2", "eps", "clip", "grad_scale"))
    norm = math.sqrt(float((g ** 2).sum())) * gs
    lr = lr0
    if hp["decay"]:
        s = step * sf + 1.0
        lr = lr0 * math.sqrt(4000.0) * min(s * 4000.0 ** -1.5, s ** -0.5)
    t = step + 1
    lr_t = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    scale = gs * (1.0 / max(1.0, norm / clip) if clip > 0 else 1.0)
    gr = g * scale
    m = b1 * m + (1.0 - b1) * gr
    v = b2 * v + (1.0 - b2) * gr * gr
    p = p - lr_t * m / (np.sqrt(v) + eps)
    return p, m, v, (norm, lr_t, scale)


def adam_run(n, hp, gstd, step0=0, steady=False, pscale=None, steps=3, seed=0, gfix=None):
    """`steps` updates on the device and in adam_ref, compared after each.  The parameters start at the size of the updates
    (10 lr_t) unless pscale says otherwise: at |p| ~ 1 an update of lr_t ~ 1e-7 is below the bar, and nothing would be tested.
    steady: the moments start at their stationary values for gradients of size gstd (m ~ g, v ~ g^2)."""
    from satt_amd import ops
    g = np.random.default_rng(seed + n)
    draw = (lambda: gfix(g, n)) if gfix else (lambda: g.normal(0, gstd, n))
    grads = [draw().astype(np.float32) for _ in range(steps)]
    zero = np.zeros(n)
    _, _, _, (_, lr_t0, _) = adam_ref(zero, zero, zero, grads[0].astype(np.float64), step0, hp)
    p = (g.normal(0, 1, n) * (10 * lr_t0 if pscale is None else pscale)).astype(np.float32)
    m = (g.normal(0, gstd, n) if steady else zero).astype(np.float32)
    v = ((g.normal(0, gstd, n) ** 2 + 0.1 * gstd ** 2) if steady else zero).astype(np.float32)
    pd_, md, vd = T(p), T(m), T(v)
    p, m, v = p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    state = ops.opt_state(DEV)
    step = torch.full((1,), step0, dtype=torch.int32, device=DEV)
    seedt = torch.full((1,), 40, dtype=torch.int32, device=DEV)
    out = []
    for k, gr in enumerate(grads):
        p, m, v, st = adam_ref(p, m, v, gr.astype(np.float64), step0 + k, hp)
        gd = T(gr)
        ops.sumsq(gd, state)
        ops.adam_step(pd_, gd, md, vd, state, step, seedt, hp["lr0"], hp["decay"], hp["step_factor"], hp["b1"], hp["b2"],
                      hp["eps"], hp["clip"], hp["grad_scale"])
        torch.cuda.synchronize()
        tag = "n=%d step %d: " % (n, step0 + k)
        got = [float(x) for x in state[1:5].cpu()]
        for name, a, b in zip(("norm", "lr_t", "scale"), got, st):
            e = abs(a - b) / abs(b)
            print("%-44s rel_err=%.3e (bar 1.0e-05)  %.9g" % (tag + name, e, b))
            assert e < 1e-5, (tag + name, a, b)
        assert got[3] == 0.0, "an update that took place leaves state[4] = 0"
        close(pd_, p, 1e-5, tag + "p"); close(md, m, 1e-5, tag + "m"); close(vd, v, 1e-5, tag + "v")
        # both counters advance by exactly one per call
        assert int(step) == step0 + k + 1 and int(seedt) == 40 + k + 1
        out.append((got, st))
    assert [float(x) for x in state[-2:].cpu()] == [0.0, 0.0]
    return out


@pytest.mark.parametrize("n", [1, 5, 1025])
@pytest.mark.parametrize("case", ["above_clip", "below_clip", "clip_off", "dp_above", "dp_below", "no_decay"])
def test_adam_clip_scale_and_decay(case, n):
    """the global-norm clip on both sides of its threshold, switched off, and behind the data-parallel gradient scale"""
    # gradient norms ~ gstd * sqrt(n): chosen per n so that the norm is on the side of the clip the case names
    rt = math.sqrt(n)
    hp, gstd, side = {
        "above_clip": (dict(HP), 6.0 / rt, "above"),
        "below_clip": (dict(HP), 0.2 / rt, "below"),
        "clip_off": (dict(HP, clip=0.0), 6.0 / rt, "off"),
        "dp_above": (dict(HP, grad_scale=0.25), 24.0 / rt, "above"),       # scaled norm ~ 6
        "dp_below": (dict(HP, grad_scale=0.25), 2.4 / rt, "below"),        # norm 2.4 > clip, scaled norm 0.6 < clip
        "no_decay": (dict(HP, decay=False), 6.0 / rt, "above"),
    }[case]
    fix = None
    if n <= 5:      # a handful of elements: fix the magnitudes so the norm cannot wander across the clip
        fix = lambda g, n_: gstd * g.uniform(0.8, 1.2, n_) * (g.integers(0, 2, n_) * 2 - 1)
    for got, st in adam_run(n, hp, gstd, gfix=fix):
        gs = f32(hp["grad_scale"])
        if side == "above":
            assert st[0] > 1.5 * hp["clip"] and got[2] < gs / 1.5
        elif side == "below":
            assert st[0] < hp["clip"] / 1.2
            if case == "dp_below":          # only the scaling brings the norm under the clip
                assert st[0] / gs > 1.2 * hp["clip"]
            assert got[2] == gs, "below the clip the scale is the data-parallel factor, exactly"
        else:
            assert st[0] > 1.5 and got[2] == gs
        if case == "no_decay":
            assert st[1] > 1e-4         # lr0 itself, not the warm-up's 1e-7


@pytest.mark.parametrize("step_factor", [1.0, 700.0])
@pytest.mark.parametrize("step0", [0, 3998, 3999, 4000, 4001, 100000])
def test_adam_rate_schedule(step0, step_factor):
    """the warm-up / decay kink of the schedule at step * step_factor + 1 = 4000, and far out, where the bias correction has
    died out"""
    adam_run(1025, dict(HP, step_factor=step_factor), 6.0 / 32, step0=step0)


def test_adam_late_step_with_live_moments():
    """step 100000 with non-zero m and v: both bias corrections are 1 to fp32 (0.999^100001 < 1e-43)"""
    for k, (got, st) in enumerate(adam_run(1025, HP, 6.0 / 32, step0=100000, steady=True)):
        lr = torch_ref.learning_rate(f32(HP["lr0"]), 100000 + k)
        assert abs(st[1] / lr - 1) < 1e-12 and abs(got[1] / lr - 1) < 1e-5      # lr_t is the schedule's rate itself


@pytest.mark.parametrize("steady", [False, True])
def test_adam_epsilon_placement(steady):
    """gradients of size 1e-9 with the clip off: eps = 1e-8 decides the step.
    From zero moments at t = 1 the update is lr * sqrt(1-b2) g / (sqrt(1-b2) |g| + eps) ~ lr * 3.2e-3: with eps on the
    bias-CORRECTED sqrt(v) (Kingma & Ba's form) it would be lr * |g| / (|g| + eps) ~ lr * 0.09, 29 times as large.
    With stationary moments at step 100000 (sqrt(v) ~ |g|, eps = 10 sqrt(v)) the update is ~ lr / 11: with eps moved INSIDE
    the square root it would be lr * |g| / sqrt(g^2 + eps) = lr * 1e-5, about 9000 times smaller."""
    hp = dict(HP, clip=0.0, decay=False)
    fix = lambda g, n_: 1e-9 * g.uniform(0.5, 2.0, n_) * (g.integers(0, 2, n_) * 2 - 1)
    if steady:
        out = adam_run(1025, hp, 1e-9, step0=100000, steady=True, gfix=fix)
    else:
        out = adam_run(1025, hp, 1e-9, gfix=fix)
    assert all(got[2] == 1.0 for got, _ in out)


def test_adam_stride_loop():
    """n = 2 097 152 + 3: adam_k's workgroups take a second element, and sumsq_k a three-element tail"""
    adam_run(2097152 + 3, HP, 6.0 / 1448, steps=1)


def test_adam_full_size_parameters():
    """parameters of size 1 (the usual case; the update is then near the fp32 resolution of p and only m, v and the state words
    test the arithmetic): p keeps its value, it is not rebuilt from the update"""
    adam_run(1025, dict(HP, decay=False), 6.0 / 32, pscale=1.0)


def test_adam_skipped_steps_and_sticky_counters():
    """A non-finite gradient, or a set cluster error word, skips the update on the device: p, m and v keep their bits,
    state[4] = 1, and the sticky counters at the end of the state count (skipped updates, those skipped for a non-finite gradient
    alone).  step_dev and seed_dev DO advance on a skipped step (adam_prepare_k increments unconditionally), as the host's mirror
    Engine.global_step does: test_engine_counts_a_skipped_step_like_the_device."""
    from satt_amd import ops
    n = 1025
    g = np.random.default_rng(5)
    pd_, md, vd = T(g.normal(0, 1e-6, n)), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    state = ops.opt_state(DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV); seedt = torch.zeros(1, dtype=torch.int32, device=DEV)
    err = torch.zeros(16, dtype=torch.int32, device=DEV)
    words = [err[0:1].data_ptr(), err[5:6].data_ptr(), err[9:10].data_ptr()]
    good = T(g.normal(0, 0.2, n))

    def update(gd, err_words=()):
        ops.sumsq(gd, state)
        ops.adam_step(pd_, gd, md, vd, state, step, seedt, 5e-4, True, 1.0, 0.9, 0.999, 1e-8, 1.0, 1.0, err_words=err_words)
        torch.cuda.synchronize()
        return float(state[4]), [float(x) for x in state[-2:].cpu()], int(step), int(seedt)

    assert update(good, words) == (0.0, [0.0, 0.0], 1, 1)
    before = (pd_.clone(), md.clone(), vd.clone())
    same = lambda: torch.equal(pd_, before[0]) and torch.equal(md, before[1]) and torch.equal(vd, before[2])
    assert bool(md.abs().max() > 0) and bool(vd.max() > 0)
    bad = good.clone(); bad[n - 1] = float("nan")           # one NaN, in the scalar tail of the sum of squares
    assert update(bad, words) == (1.0, [1.0, 1.0], 2, 2) and same()
    assert update(bad) == (1.0, [2.0, 2.0], 3, 3) and same()                # no error words given at all
    err[5] = 1                                                              # a timed-out cluster kernel, finite gradient
    assert update(good, words) == (1.0, [3.0, 2.0], 4, 4) and same()
    assert update(bad, words) == (1.0, [4.0, 2.0], 5, 5) and same()         # both reasons: not "for the gradient alone"
    err[5] = 0
    assert update(good, words) == (0.0, [4.0, 2.0], 6, 6) and not same()    # a clean step: state[4] resets, the counters stay


def test_engine_counts_a_skipped_step_like_the_device():
    """the host's mirror of the step counter (Engine.global_step, which the rate shown in the logs is computed from) advances
    unconditionally: so does the device's, also on a skipped step"""
    from common import SMALL, make_params, small_batch
    from satt_amd import ops
    from satt_amd.engine import Engine
    cfg, P = make_params(SMALL, seed=1)
    ops.set_precision("f32")
    eng = Engine(cfg, DEV, params=P, rng_seed=7)
    b = eng.to_device_batch(small_batch(cfg, 3, 9, 12, seed=3))
    eng.train_step(b)
    eng.grad[eng.grad.numel() - 1] = float("nan")
    before = eng.flat.clone()
    eng.optimizer_step()
    torch.cuda.synchronize()
    assert torch.equal(eng.flat, before) and [float(x) for x in eng.opt_state[-2:].cpu()] == [1.0, 1.0]
    assert int(eng.step_dev) == eng.global_step == 1
    eng.train_step(b)
    eng.optimizer_step()
    torch.cuda.synchronize()
    assert not torch.equal(eng.flat, before) and float(eng.opt_state[4]) == 0.0
    assert int(eng.step_dev) == eng.global_step == 2


# ---------------------------------------------------------------------------------------------- L2 regulariser
L2_N = 40000
L2_TABLES = {
    "one": [(100, 5000)],
    "five_odd_offsets": [(1, 7), (13, 300), (1001, 2500), (5003, 1), (9999, 12001)],
    # one element; less than a wave; a workgroup and one element; one element more than the 8192 threads of a segment's grid
    "counts": [(3, 1), (10, 63), (101, 257), (1003, 8193)],
}


@pytest.mark.parametrize("with_total", [True, False])
@pytest.mark.parametrize("table", list(L2_TABLES))
def test_l2_reg(table, with_total):
    from satt_amd import ops
    segs = L2_TABLES[table]
    g = np.random.default_rng(len(segs))
    w = g.normal(0, 0.5, L2_N).astype(np.float32); g0 = g.normal(0, 1, L2_N).astype(np.float32)
    scale = 1e-2
    inside = np.zeros(L2_N, dtype=bool)
    for off, cnt in segs:
        assert not inside[off:off + cnt].any() and off + cnt <= L2_N
        inside[off:off + cnt] = True
    w64 = w.astype(np.float64)
    want_reg = f32(scale) * float((w64[inside] ** 2).sum()) / 2
    wd, gd = T(w), T(g0)
    tab = torch.tensor(segs, dtype=torch.int64, device=DEV).contiguous()
    reg = torch.zeros(1, device=DEV)
    total = torch.full((1,), 2.5, device=DEV) if with_total else None
    for call in (1, 2):             # the header leaves zeroing *reg to the caller: a second call adds to it, and to the gradient
        ops.l2_reg(wd, gd, tab, len(segs), scale, reg, total)
        torch.cuda.synchronize()
        e = abs(float(reg) - call * want_reg) / (call * want_reg)
        print("l2_reg %s call %d: reg rel_err=%.3e" % (table, call, e))
        assert e < 1e-5, (float(reg), call * want_reg)
        if with_total:
            assert abs(float(total) - (2.5 + call * want_reg)) / (2.5 + call * want_reg) < 1e-5
        got = gd.cpu().numpy()
        close(torch.as_tensor(got[inside]), torch.as_tensor(g0.astype(np.float64)[inside] + call * f32(scale) * w64[inside]), 1e-6,
              "l2_reg %s call %d: gradient" % (table, call))
        assert np.array_equal(got[~inside].view(np.int32), g0[~inside].view(np.int32)), "outside the segments: bit-identical"
    assert np.array_equal(wd.cpu().numpy().view(np.int32), w.view(np.int32))
