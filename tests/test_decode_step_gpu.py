"""The launch-per-layer decode kernels of csrc/decode.hip, each called directly (ops.dec_linear, dec_linear2, dec_linear_chain,
dec_self_attn, dec_attention) and compared with a float64 reference of the same operation (tests/decode_step_common.py): one to
three launches per case at the shapes where the kernels take another path.  Every output is NaN before the launch, every history
row and parity buffer a launch must not write holds a sentinel and is compared bit for bit afterwards.  The bounds are
decode_step_common.bound (profiles/decode_step_tolerances.txt); zero patterns, flags and untouched rows are exact.

Paths of csrc/decode.hip that no test with a reference behind it had run, and the cases that reach them:
  dec_attn_context_k   the loop over memories longer than 256 rows and the second pass of the softmax / recursion strides:
                       test_dec_attention at Ti = 257, 513, 1100 (sample 0 has the full length).  Rows >= 256 carry weight in the
                       location_sensitive and forced cases and in the second mechanism's context columns of every dual case; a
                       forward recursion three steps from onehot(0) weights them with ~1e-7.
  dec_attn_energy_k    Ti = 513: 64 slices of 9 rows, slices 57 .. 63 start beyond the memory; Ti = 1100: the slice count pushed
                       from 64 to 69.  Kernel widths 6 (even: one more tap right than left) and 31 beside the 10 of the examples.
  dec_self_attn_k<128> t = 1024, 1030 and 12999: the second pass of the softmax stride loop; Td = 1031: no multiple of 4;
                       Td = 13000: 68 KB of dynamic LDS, the opt-in; t = 255, 256, 257: either side of the 256-row score pass;
                       the sharp and offset regimes: one row with all the weight, and scores that overflow without the maximum.
  dec_self_attn_any_k  head depths 8, 16, 32, 256, 1024 at t = 0, 37, 69.
  dec_linear_k         B = 9, 17: groups of 8 with a ragged last one; K = 1024; N = 8 < 32; the scalar instantiations on ldw = 161
                       and on a view one element into its allocation (f32 and bf16); N = 161 on rows of 168 whose padding is NaN
                       (the vector path, a row ending inside a 4-column group); softsign; the stop rule at sigmoid == threshold,
                       at t - 1 == min_steps and either side, 70 samples with only sample 69 low, a flag already set; step_out;
                       the LSTM form at H = 8, 64, 256 with zc != zh; dropout masks against oracle/rng.py.
  dec_linear2_k        the three shapes incl. (5, 12, 161) on rows of 12 and 164, dropout on both layers.
  dec_chain_k          B = 5, 9: groups of 4 with a ragged last one; one pre-layer in front of the plain N = 161 layer; one and two
                       pre-layers in front of the H = 256 LSTM form; pre[j].y.
None of them showed a defect (measured errors: profiles/decode_step_tolerances.txt)."""
import math

import pytest
import torch

import satt_amd  # noqa: F401
import decode_step_common as ds
from common import rel_err
from decode_step_common import SENTINEL, Holder

pytestmark = pytest.mark.gpu
NAN = float("nan")


def close(op, got, want, what, bar=None):
    bar = ds.bound(op) if bar is None else bar
    e = rel_err(got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy())
    print("DSTEP %-16s %-58s rel_err=%.3e (bound %.2e)" % (op, what, e, bar))
    assert e < bar, (op, what, e, bar)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def untouched(buf, row_axis_index, what):
    """every row of a [B, rows, n] history but `row_axis_index` still holds the sentinel"""
    keep = [r for r in range(buf.shape[1]) if r != row_axis_index]
    assert bool((buf[:, keep] == SENTINEL).all()), what


def word(hold, value):
    return hold(torch.tensor([value], dtype=torch.int32))


def history(hold, B, rows, n, step):
    """a [B, rows, n] history of sentinels whose row `step` - the one the launch addresses - is NaN"""
    y = hold.full((B, rows, n), SENTINEL)
    y[:, step] = NAN
    return y


def parity_state(hold, init, par):
    """a [2, B, n] state: buffer `par` is read (and must stay as it is), buffer par ^ 1 is the output (NaN)"""
    d = hold(init)
    d[par ^ 1] = NAN
    return d


def code_of(err):
    return int(str(err.value).rsplit("(", 1)[1].rstrip(")"))


# ---------------------------------------------------------------------------------------------------------------- 1. plain form
def plain_block(hold, case, z, **kw):
    from satt_amd import ops
    B, N, rows = case.B, z["N"], z["rows"]
    W = hold.matrix(z["W"], z["ldw"], case.wdt, z["off1"])
    align = 8 if case.wdt == "bf16" else 16
    assert (W.data_ptr() % align != 0) == z["off1"]
    y = history(hold, B, rows, N, case.step)
    res = None if z["res"] is None else hold(z["res"])
    p = ops.dec_linear_params([hold.seg(s) for s in z["segs"]], W, (y, rows * N, N), bias=None if z["b"] is None else hold(z["b"]),
                              act=case.act, res=None if res is None else (res, rows * N, N), step=word(hold, case.step), B=B, **kw)
    return hold.keep(p), y


@pytest.mark.parametrize("case", ds.LIN_CASES, ids=lambda c: "%s-B%d-%s-act%d-b%d-r%d-t%d" % (c.shape, c.B, c.wdt, c.act, c.bias, c.res, c.step))
def test_dec_linear_plain(case):
    from satt_amd import ops
    hold, z = Holder(), ds.lin_inputs(case)
    p, y = plain_block(hold, case, z)
    ops.dec_linear(p)
    torch.cuda.synchronize()
    close("dense", y[:, case.step], ds.lin_ref(case), "dec_linear %s" % (case,))
    untouched(y, case.step, case)


# ---------------------------------------------------------------------------------------------------------------- 2. LSTM form
def lstm_block(hold, case, z, x0=None, **kw):
    """x0: the first segment's entry (a chained layer's output) instead of the case's own history"""
    from satt_amd import ops
    H, B, rows, par = case.H, case.B, z["rows"], case.step & 1
    W = hold.matrix(ds.regroup_lstm(z["W"], H), 4 * H, case.wdt)
    c, h = parity_state(hold, z["c"], par), parity_state(hold, z["h"], par)
    y = history(hold, B, rows, H, case.step)
    segs = z["segs"]
    xs = [hold.seg(segs[0]) if x0 is None else x0] + [hold.seg(s) for s in segs[1:-1]] + [(h.view(-1), H, H, 0, B * H)]
    p = ops.dec_linear_params(xs, W, (y, rows * H, H), bias=hold(z["b"]), step=word(hold, case.step), B=B,
                              lstm=(H, c, h, ds.LSTM_ZC, ds.LSTM_ZH), **kw)
    return hold.keep(p), y, c, h


def check_lstm(op, case, got, want, c0, h0, what):
    y, c, h = got
    par = case.step & 1
    close(op, y[:, case.step], want[0], what + " y = the cell output before zoneout")
    close(op, c[par ^ 1], want[1], what + " c state")
    close(op, h[par ^ 1], want[2], what + " h state")
    assert same_bits(c[par], c0[par].to(c.device)) and same_bits(h[par], h0[par].to(h.device)), "the states read were written"
    untouched(y, case.step, what)


@pytest.mark.parametrize("case", ds.LSTM_CASES, ids=lambda c: "H%d-B%d-t%d-%s" % c)
def test_dec_linear_lstm(case):
    from satt_amd import ops
    hold, z = Holder(), ds.lstm_inputs(case)
    p, y, c, h = lstm_block(hold, case, z)
    ops.dec_linear(p)
    torch.cuda.synchronize()
    check_lstm("lstm", case, (y, c, h), ds.lstm_case_ref(case), z["c"], z["h"], "lstm %s" % (case,))


# ---------------------------------------------------------------------------------------------------------------- 3. dropout
@pytest.mark.parametrize("rate", ds.DROP_RATES)
def test_dec_linear_dropout_on_inference(rate):
    from satt_amd import ops
    case = ds.DROP_CASE
    hold, z = Holder(), ds.lin_inputs(case)
    seed = hold(torch.tensor([ds.DROP_SEED], dtype=torch.int32))
    p, y = plain_block(hold, case, z, drop=ops.Drop(rate, ds.DROP_STREAM, seed), drop_T=ds.DROP_T)
    ops.dec_linear(p)
    torch.cuda.synchronize()
    got, res = y[:, case.step].cpu(), z["res"][:, case.step]
    keep = ds.keep_rows(ds.DROP_SEED, ds.DROP_STREAM, case.B, ds.DROP_T, z["N"], rate, case.step)
    assert 0 < int(keep.sum()) < keep.numel()
    # the residual is added AFTER the mask: a dropped element is 0 + res, bit for bit; a kept one is not (tanh(.) * scale != 0)
    assert torch.equal(got == res, ~keep), "the zero pattern is not the oracle's mask"
    plain = ds.dense_ref([ds.seg_rows(s, case.B, case.step) for s in z["segs"]], z["W"], z["b"], case.act)
    want = torch.where(keep, plain * (1.0 / (1.0 - rate)), torch.zeros_like(plain)) + res.double()
    close("dense", got, want, "dropout rate %.1f" % rate)
    untouched(y, case.step, rate)


# ---------------------------------------------------------------------------------------------------------------- 4. bookkeeping
@pytest.mark.parametrize("case", ds.STOP_CASES, ids=lambda c: c.name)
def test_dec_linear_step_bookkeeping(case):
    from satt_amd import ops
    lin = ds.LinCase("n8", case.B, "f32", ds.ACT_NONE, False, False, case.t)
    hold, z = Holder(), ds.lin_inputs(lin)
    rows = z["rows"]
    logits = hold(ds.stop_logits(case, rows))
    flag, out = word(hold, case.flag0), word(hold, -1)
    p, y = plain_block(hold, lin, z, step_out=(out, 3), stop=(logits, rows, 1, flag, ds.STOP_THRESHOLD, ds.STOP_MIN))
    ops.dec_linear(p)
    torch.cuda.synchronize()
    assert int(out) == case.t + 3
    assert int(flag) == case.want, (case.name, int(flag))
    close("dense", y[:, lin.step], ds.lin_ref(lin), "bookkeeping %s" % case.name)


# ---------------------------------------------------------------------------------------------------------------- 5. dec_linear2
def l2_blocks(hold, case, z):
    from satt_amd import ops
    K1, N1, N2, ld1, ld2 = case.shape
    B, rows = case.B, z["rows"]
    seed = hold(torch.tensor([ds.DROP_SEED], dtype=torch.int32))
    mid, y = hold.full((B, N1), NAN), history(hold, B, rows, N2, case.step)
    step = word(hold, case.step)
    drop = [ops.Drop(rate, stream, seed) for rate, stream in ds.L2_DROP]
    p1 = ops.dec_linear_params([hold.seg(z["x"])], hold.matrix(z["W1"], ld1, "bf16"), (mid, N1, 0), bias=hold(z["b1"]), act=case.act1,
                               res=(hold(z["res1"]), N1, 0), step=step, B=B, drop=drop[0], drop_T=ds.L2_DROP_T)
    p2 = ops.dec_linear_params([(mid, N1, N1, 0)], hold.matrix(z["W2"], ld2, "bf16"), (y, rows * N2, N2), bias=hold(z["b2"]), act=case.act2,
                               step=step, B=B, drop=drop[1], drop_T=ds.L2_DROP_T)
    hold.keep(p1, p2)
    return p1, p2, mid, y


@pytest.mark.parametrize("case", ds.L2_CASES, ids=lambda c: "K%d-N%d-N%d-B%d-t%d" % (c.shape[0], c.shape[1], c.shape[2], c.B, c.step))
def test_dec_linear2(case):
    from satt_amd import ops
    hold, z = Holder(), ds.l2_inputs(case)
    mid64, y64 = ds.l2_ref(case)
    p1, p2, mid, y = l2_blocks(hold, case, z)
    assert ops.dec_linear2(p1, p2) is True
    torch.cuda.synchronize()
    close("linear2", y[:, case.step], y64, "linear2 fused %s" % (case,))
    assert bool(torch.isnan(mid).all()), "the fused form writes no intermediate vector"
    untouched(y, case.step, case)
    q1, q2, mid1, y1 = l2_blocks(hold, case, z)          # the same two layers, one launch each, on buffers of their own
    ops.dec_linear(q1)
    ops.dec_linear(q2)
    torch.cuda.synchronize()
    close("linear2", mid1, mid64, "linear2 layer 1 alone")
    close("linear2", y1[:, case.step], y64, "linear2 one by one")
    close("linear2", y[:, case.step], y1[:, case.step], "linear2 fused against one by one", ds.FORMS)
    assert torch.equal(y[:, case.step] == 0, y1[:, case.step] == 0), "the two forms drop different elements"


# ---------------------------------------------------------------------------------------------------------------- 6. dec_linear_chain
def chain_blocks(hold, case, z):
    from satt_amd import ops
    B, rows = case.B, z["rows"]
    step = word(hold, case.step)
    pre, mids, x = [], [], hold.seg(z["x"])
    for q, (K, N) in zip(z["pre"], ds.CHAIN_PRE[case.npre]):
        mid = hold.full((B, N), NAN)
        pre.append(ops.dec_linear_params([x], hold.matrix(q["W"], N, "bf16"), (mid, N, 0), bias=hold(q["b"]), act=ds.ACT_RELU, step=step, B=B))
        mids.append(mid)
        x = (mid, N, N, 0)
    if case.main == "plain":
        y = history(hold, B, rows, 161, case.step)
        main = ops.dec_linear_params([x], hold.matrix(z["W"], 168, "bf16"), (y, rows * 161, 161), bias=hold(z["b"]), act=ds.ACT_TANH,
                                     res=(hold(z["res"]), rows * 161, 161), step=step, B=B)
        out = (y,)
    else:
        lc = ds.LstmCase(ds.CHAIN_H, B, case.step, "bf16")
        main, y, c, h = lstm_block(hold, lc, dict(z, segs=[None] + z["segs"]), x0=x)
        out = (y, c, h)
    hold.keep(*pre, main)
    return pre, main, mids, out


@pytest.mark.parametrize("case", ds.CHAIN_CASES, ids=lambda c: "pre%d-%s-B%d-t%d" % c)
def test_dec_linear_chain(case):
    from satt_amd import ops
    hold, z = Holder(), ds.chain_inputs(case)
    mids64, main64 = ds.chain_ref(case)
    op = "chain" if case.main == "plain" else "chain_lstm"
    lc = ds.LstmCase(ds.CHAIN_H, case.B, case.step, "bf16")

    def check(mids, out, what):
        for j, (m, m64) in enumerate(zip(mids, mids64)):
            close(op, m, m64, "%s pre[%d].y" % (what, j))
        if case.main == "plain":
            close(op, out[0][:, case.step], main64, what + " y")
            untouched(out[0], case.step, what)
        else:
            check_lstm(op, lc, out, main64, z["c"], z["h"], what)
    pre, main, mids, out = chain_blocks(hold, case, z)
    assert ops.dec_linear_chain(pre, main) is True
    torch.cuda.synchronize()
    check(mids, out, "chain %s" % (case,))
    pre1, main1, mids1, out1 = chain_blocks(hold, case, z)          # the same layers through dec_linear
    for p in pre1 + [main1]:
        ops.dec_linear(p)
    torch.cuda.synchronize()
    check(mids1, out1, "one by one")
    if case.main == "plain":
        close(op, out[0][:, case.step], out1[0][:, case.step], "chain against one by one", ds.FORMS)
    else:
        par = case.step & 1
        for a, b, what in ((out[0][:, case.step], out1[0][:, case.step], "y"), (out[1][par ^ 1], out1[1][par ^ 1], "c"), (out[2][par ^ 1], out1[2][par ^ 1], "h")):
            close(op, a, b, "chain against one by one " + what, ds.FORMS)


# ---------------------------------------------------------------------------------------------------------------- 7. declines
def raises_code(fn, code):
    from satt_amd import _lib
    with pytest.raises(_lib.SattError) as err:
        fn()
    assert code_of(err) == code, str(err.value)


def test_dec_linear_declines():
    from satt_amd import ops
    hold = Holder()
    g = ds.gen(7)
    B = 3
    # sum k = 1025
    x, y = hold(ds.randn(g, B, 1025)), hold.full((B, 8), NAN)
    p = ops.dec_linear_params([(x, 1000, 1025, 0), (x.view(-1)[1000:], 25, 1025, 0)], hold(ds.randn(g, 1025, 8)), (y, 8, 0), B=B)
    raises_code(lambda: ops.dec_linear(hold.keep(p)), ds.E_UNSUPPORTED)

    def lstm(H, **kw):
        xs = [(hold(ds.randn(g, B, 20)), 20, 20, 0), (hold(ds.randn(g, 2, B, H)), H, H, 0, B * H)]
        c, h, yy = hold(ds.randn(g, 2, B, H)), hold(ds.randn(g, 2, B, H)), hold.full((B, H), NAN)
        c[1] = NAN; h[1] = NAN
        return hold.keep(ops.dec_linear_params(xs, hold(ds.randn(g, 20 + H, 4 * H)), (yy, H, 0), bias=hold(ds.randn(g, 4 * H)), B=B,
                                               lstm=(H, c, h, 0.1, 0.1), **kw)), (yy, c[1], h[1])
    seed = hold(torch.tensor([1], dtype=torch.int32))
    outs = [y]
    for H, kw in ((12, {}), (16, dict(res=(hold(ds.randn(g, B, 64)), 64, 0))), (16, dict(drop=ops.Drop(0.5, 8, seed), drop_T=4))):
        p, o = lstm(H, **kw)
        raises_code(lambda: ops.dec_linear(p), ds.E_BADARG)
        outs += o
    p, o = lstm(16)          # (the block itself is a valid one)
    ops.dec_linear(p)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in o)
    assert all(bool(torch.isnan(t).all()) for t in outs), "a declined call wrote its output"


def test_dec_linear2_and_chain_decline():
    from satt_amd import ops
    hold = Holder()
    g = ds.gen(77)
    B = 3

    def layer(K, N, ldw, wdt, x=None):
        y = hold.full((B, N), NAN)
        x = hold(ds.randn(g, B, K)) if x is None else x
        return hold.keep(ops.dec_linear_params([(x, K, K, 0)], hold.matrix(ds.weight(g, K, N, wdt), ldw, wdt), (y, N, 0), B=B)), y
    outs = []
    for (K1, N1, ld1, w1), (N2, ld2, w2) in (((64, 32, 32, "f32"), (16, 16, "f32")),          # f32 weights
                                             ((64, 260, 260, "bf16"), (16, 16, "bf16")),      # N = 260
                                             ((64, 32, 32, "bf16"), (16, 18, "bf16"))):       # ldw % 4 != 0
        a, ya = layer(K1, N1, ld1, w1)
        b, yb = layer(N1, N2, ld2, w2, x=ya)
        assert ops.dec_linear2(a, b) is False
        outs += [ya, yb]
    a, ya = layer(64, 32, 32, "bf16")
    b, yb = layer(32, 16, 16, "bf16", x=ya)
    assert ops.dec_linear2(a, b) is True          # (the pair itself is a valid one)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(yb).all())
    # chain: the pre-layer yields 32 features, the main layer's first segment takes 48
    a, ya = layer(64, 32, 32, "bf16")
    b, yb = layer(48, 16, 16, "bf16")
    raises_code(lambda: ops.dec_linear_chain([a], b), ds.E_BADARG)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs + [ya, yb]), "a declined call wrote its output"


def test_dec_self_attn_declines():
    from satt_amd import ops
    hold = Holder()
    B, Td, D, heads = 2, 8, 48, 2          # head depth 24
    kvq, out = hold(ds.sa_cache(B, Td, D, heads)), hold.full((B, D), NAN)
    raises_code(lambda: ops.dec_self_attn(kvq, out, word(hold, 3), B, Td, D, heads, 1.0 / math.sqrt(24)), ds.E_UNSUPPORTED)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ---------------------------------------------------------------------------------------------------------------- 8. dec_self_attn
_SA_DEVICE = {}


def sa_device(B, Td, D, heads, regime="normal"):
    """the finite cache on the device, once per shape (every case clones it and poisons its own rows)"""
    key = (B, Td, D, heads, regime)
    if key not in _SA_DEVICE:
        if len(_SA_DEVICE) >= 3:
            _SA_DEVICE.clear()
        host = ds.sa_cache(B, Td, D, heads, regime)
        _SA_DEVICE[key] = (host, host.cuda())
    return _SA_DEVICE[key]


def run_self_attn(op, B, Td, D, heads, t, regime="normal"):
    from satt_amd import ops
    hold = Holder()
    host, base = sa_device(B, Td, D, heads, regime)
    kvq = hold.keep(base.clone())
    kvq[:, t + 1:] = NAN          # the rows the step has not written yet
    out, step = hold.full((B, D), NAN), word(hold, t)
    ops.dec_self_attn(kvq, out, step, B, Td, D, heads, 1.0 / math.sqrt(D // heads))
    torch.cuda.synchronize()
    close(op, out, ds.self_attn_ref(host, t, D, heads), "self_attn D%d h%d Td%d t%d %s" % (D, heads, Td, t, regime))
    assert torch.equal(kvq[:, :t + 1], base[:, :t + 1]) and bool(torch.isnan(kvq[:, t + 1:]).all())


@pytest.mark.parametrize("t", ds.SA_PROD_T)
def test_dec_self_attn_production(t):
    p = ds.SA_PROD
    run_self_attn("self_attn", p["B"], p["Td"], p["D"], p["heads"], t)


@pytest.mark.parametrize("regime", ["sharp", "offset"])
def test_dec_self_attn_regimes(regime):
    p = ds.SA_PROD
    run_self_attn("self_attn_offset" if regime == "offset" else "self_attn", p["B"], p["Td"], p["D"], p["heads"], ds.SA_REGIME_T, regime)


def test_dec_self_attn_large_dynamic_lds():
    b = ds.SA_BIG
    assert 4 * (b["Td"] + 32 * 128 + 16) > 64 * 1024          # beyond the default dynamic LDS limit: the launcher opts in
    run_self_attn("self_attn", b["B"], b["Td"], b["D"], b["heads"], b["t"])
    _SA_DEVICE.clear()          # (40 MB that no other case uses)


@pytest.mark.parametrize("t", ds.SA_ANY_T)
@pytest.mark.parametrize("D,heads", ds.SA_ANY)
def test_dec_self_attn_any_depth(D, heads, t):
    assert D // heads != 128
    run_self_attn("self_attn", ds.SA_ANY_B, ds.SA_ANY_TD, D, heads, t)


# ---------------------------------------------------------------------------------------------------------------- 9. dec_attention
def att_device(hold, z, widths, Ti, KW, mode, wq, filters=5):
    from satt_amd import ops
    A, U1, V1, U2, V2 = widths
    B, Td, UQ, CT = ds.ATT_B, ds.ATT_TD, widths[1] + widths[3], widths[2] + widths[4]
    forced, dual = mode.startswith("forced"), U2 > 0
    d = dict(lengths=hold(z["lens"]), hq=hold.full((B, A), NAN), keys1=hold(z["keys1"]), values1=hold(z["values1"]),
             locF=hold(z["F"]), locFb=hold(z["bF"]), locU=hold(z["U"]), v1=hold(z["v1"]), b1=hold(z["b1"]),
             e1=hold.full((B, Ti), NAN), ctx=hold.full((2, B, CT), NAN), pq_out=hold.full((2, B, UQ), NAN),
             a_state=hold.full((2, B, Ti), SENTINEL), alpha_state=hold.full((2, B, Ti), SENTINEL),
             align1=hold.full((B, Td, Ti), SENTINEL), step=word(hold, 0))
    d["a_state"][0] = 0.0          # include/satt_hip.h: buffer 0 starts at 0 and onehot(0)
    d["alpha_state"][0] = 0.0
    d["alpha_state"][0, :, 0] = 1.0
    if dual:
        d.update(keys2=hold(z["keys2"]), values2=hold(z["values2"]), v2=hold(z["v2"]), e2=hold.full((B, Ti), NAN),
                 align2=hold.full((B, Td, Ti), SENTINEL))
    d["Wqb" if wq == "bf16" else "Wq"] = hold(z["Wq"], dtype=torch.bfloat16 if wq == "bf16" else torch.float32)
    if mode == "agent":
        d.update(agentW=hold(z["Wa"]), agentb=hold(z["ba"]))
    if forced:
        d["teach1"] = hold(z["teach1"])
        if z["teach2"] is not None:
            d["teach2"] = hold(z["teach2"])
    p = ops.dec_attention_params(B=B, Td=Td, Ti=Ti, U1=U1, V1=V1, U2=U2, V2=V2, kernel=KW, filters=filters, A=A,
                                 att1_mode=int(mode == "location_sensitive"), cumulative=int(mode == "cumulative"), **d)
    return hold.keep(p), d


@pytest.mark.parametrize("case", ds.ATT_CASES, ids=lambda c: "%s-k%d-Ti%d-%s-%s" % c)
def test_dec_attention(case):
    from satt_amd import ops
    hold, z, ref = Holder(), ds.att_inputs(case), ds.att_ref64(case)
    widths = ds.ATT_WIDTHS[case.widths]
    p, d = att_device(hold, z, widths, case.Ti, case.kernel, case.mode, case.wq)
    forced, dual = case.mode.startswith("forced"), widths[3] > 0
    if case.mode == "agent":          # not vacuous: in float64 the agent moves the alignments of this input
        moved = max(float((a["align1"] - b["align1"]).abs().max()) for a, b in zip(ref, ds.att_ref(case, agent=False)))
        assert moved > 1e-3, moved
    state =("a_state", "alpha_state", "ctx", "pq_out", "align1") + (("align2",) if dual else ())
    for t in range(ds.ATT_STEPS):
        par, want = t & 1, ref[t]
        d["step"].fill_(t)
        d["hq"].copy_(z["hq"][t])
        for k in ("a_state", "alpha_state"):          # outputs of the step: NaN
            d[k][par ^ 1] = NAN
        for k in ("ctx", "pq_out"):
            d[k][par] = NAN
        for k in ("e1", "e2", "align1", "align2"):
            if k in d:
                (d[k] if k[0] == "e" else d[k][:, t]).fill_(NAN)
        before = {k: d[k].clone() for k in state}
        ops.dec_attention(p)
        torch.cuda.synchronize()
        what = "%s step %d " % (case, t)
        close("attn_align", d["align1"][:, t], want["align1"], what + "align1")
        if dual:
            close("attn_align", d["align2"][:, t], want["align2"], what + "align2")
        close("attn_ctx", d["ctx"][par], want["ctx"], what + "ctx")
        close("attn_state", d["a_state"][par ^ 1], want["a_state"], what + "a_state")
        close("attn_state", d["alpha_state"][par ^ 1], want["alpha_state"], what + "alpha_state")
        if forced:          # the rows are the ones given, bit for bit; no query layer runs
            assert torch.equal(d["align1"][:, t].cpu(), z["teach1"][:, t])
            assert bool(torch.isnan(d["pq_out"]).all())
        else:
            close("attn_pq", d["pq_out"][par], want["pq"], what + "pq_out")
        # everything the step does not own is as it was, bit for bit
        for k in ("a_state", "alpha_state"):
            assert same_bits(d[k][par], before[k][par]), (what, k)
        for k in ("ctx", "pq_out"):
            assert same_bits(d[k][par ^ 1], before[k][par ^ 1]), (what, k)
        for k in ("align1", "align2"):
            if k in d:
                rows = [r for r in range(ds.ATT_TD) if r != t]
                assert same_bits(d[k][:, rows], before[k][:, rows]), (what, k)


@pytest.mark.parametrize("widths,filters", [((256, 258, 256, 0, 0), 5), ((64, 30, 64, 0, 0), 5), ((64, 32, 64, 8, 32), 4)],
                         ids=["U1=258", "U1%4", "filters=4"])
def test_dec_attention_declines(widths, filters):
    from satt_amd import ops
    hold = Holder()
    z = ds.att_make(widths, 9, 10, "forward", 1000 + widths[1] + filters)
    if filters != 5:
        z["F"], z["bF"], z["U"] = z["F"][:, :, :filters].contiguous(), z["bF"][:filters].contiguous(), z["U"][:filters].contiguous()
    p, d = att_device(hold, z, widths, 9, 10, "forward", "f32", filters)
    d["hq"].copy_(z["hq"][0])
    before = {k: d[k].clone() for k in ("a_state", "alpha_state", "ctx", "pq_out", "align1", "e1")}
    raises_code(lambda: ops.dec_attention(p), ds.E_UNSUPPORTED)
    torch.cuda.synchronize()
    assert all(same_bits(d[k], v) for k, v in before.items()), "a declined call wrote"
