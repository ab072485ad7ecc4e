"""Helpers of the direct tests of the launch-per-layer decode kernels (csrc/decode.hip; tests/test_decode_step_{cpu,gpu}.py,
tools/decode_step_tolerances.py): the case lists with their coverage conditions, seeded inputs, float64 references built from
oracle/torch_ref.py and plain torch, and - GPU half - a holder that keeps every tensor a parameter block points to alive.

Every reference takes a dtype: float64 is the yardstick, float32 (same inputs, same bf16-rounded weights) is what the tolerance
tool measures.  bf16 weights are common.bf16_round values, multiplied as they are in both: only the fp32 accumulation (and the
fast exp / tanh / sigmoid of csrc/common.h) separates a kernel from its reference.  Importing this module touches no GPU."""
import collections
import functools
import math

import numpy as np
import torch

from common import bf16_round
from decode_common import teacher_rows
from oracle import rng, torch_ref

ACT_NONE, ACT_RELU, ACT_TANH, ACT_SOFTSIGN = 0, 1, 2, 4          # include/satt_hip.h SATT_ACT_*
SENTINEL = 7.25          # history rows and parity buffers a launch must not write
E_BADARG, E_UNSUPPORTED = -1, -2

# ---- tolerances.  DEV32: the worst float32 deviation of each reference over the cases below, relative to the tensor maximum
# (common.rel_err), as tools/decode_step_tolerances.py prints it (profiles/decode_step_tolerances.txt), rounded up to two digits.
# A bound is 8 x that - the margin of the mel and Griffin-Lim suites, for the kernel's other summation order - or, where that is
# tighter, what tests/test_ops_gpu.py grants the training kernel of the same function (FLOOR): linear / activation 2e-6, softmax
# rows 1e-6, LSTM output 1e-5.  The kernels evaluate exp, tanh and the sigmoid with the fast forms of csrc/common.h, as those do.
DEV32 = dict(dense=8.0e-7, lstm=5.9e-7, linear2=1.3e-6, chain=4.1e-7, chain_lstm=6.6e-7, self_attn=1.8e-6, self_attn_offset=9.2e-6,
             attn_align=3.5e-7, attn_ctx=4.7e-7, attn_state=3.5e-7, attn_pq=9.5e-7)
FLOOR = dict(dense=2e-6, lstm=1e-5, linear2=2e-6, chain=2e-6, chain_lstm=1e-5, self_attn=2e-6, self_attn_offset=2e-6, attn_align=1e-6,
             attn_ctx=2e-6, attn_state=1e-6, attn_pq=2e-6)
FORMS = 1e-5          # two launch forms of the same layers (tests/test_inference_gpu.py test_bf16_decode_chained_launches)


def bound(op):
    return max(8.0 * DEV32[op], FLOOR[op])


def gen(*seed):
    return torch.Generator().manual_seed(int(np.random.SeedSequence([int(s) for s in seed]).generate_state(1)[0]))


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def weight(g, K, N, wdt):
    """[K, N] float32 values of a layer's weight; "bf16": bf16-representable ones (the kernel's matrix holds exactly these)"""
    W = randn(g, K, N) / math.sqrt(K)
    return torch.as_tensor(bf16_round(W.numpy())) if wdt == "bf16" else W


def act_fn(z, act):
    if act == ACT_RELU:
        return torch.relu(z)
    if act == ACT_TANH:
        return torch.tanh(z)
    if act == ACT_SOFTSIGN:
        return z / (1.0 + z.abs())
    assert act == ACT_NONE
    return z


def keep_rows(seed, stream, B, drop_T, N, rate, step):
    """bool [B, N]: row `step` of the oracle's mask over a [B, drop_T, N] activation"""
    return torch.from_numpy(rng.keep_mask(seed, stream, (B, drop_T, N), rate)[:, step, :].copy())


def dense_ref(xs, W, b, act, keep=None, scale=1.0, res=None, dtype=torch.float64):
    """act(cat(xs) @ W + b), then the dropout mask (kept values times scale), then + res"""
    z = torch.cat([x.to(dtype) for x in xs], dim=-1) @ W.to(dtype)
    if b is not None:
        z = z + b.to(dtype)
    y = act_fn(z, act)
    if keep is not None:
        y = torch.where(keep, y * scale, torch.zeros_like(y))
    return y if res is None else y + res.to(dtype)


def lstm_ref(xs, c, h, W, b, zc, zh, dtype=torch.float64):
    """(cell output before zoneout, next c state, next h state) of the ZoneoutLSTMCell in inference mode; W [sum k + H, 4 H] in the
    ORIGINAL gate-column order, xs the segments in front of h"""
    x = torch.cat([t.to(dtype) for t in xs], dim=-1)
    c, h = c.to(dtype), h.to(dtype)
    cn, hn = torch_ref.lstm_cell(x, c, h, W.to(dtype), b.to(dtype))
    return hn, torch_ref.zoneout(cn, c, zc, False, None), torch_ref.zoneout(hn, h, zh, False, None)


def regroup_lstm(W, H):
    """gate column gate * H + u -> (u // 8) * 32 + gate * 8 + u % 8 (include/satt_hip.h, LSTM form of satt_dec_linear)"""
    K = W.shape[0]
    return W.reshape(K, 4, H // 8, 8).permute(0, 2, 1, 3).reshape(K, 4 * H).contiguous()


def ungroup_lstm(Wg, H):
    K = Wg.shape[0]
    return Wg.reshape(K, H // 8, 4, 8).permute(0, 2, 1, 3).reshape(K, 4 * H).contiguous()


def regroup_index(H):
    """the destination column of every source column, from the expression itself"""
    col = np.arange(4 * H)
    gate, u = col // H, col % H
    return (u // 8) * 32 + gate * 8 + u % 8


# ---------------------------------------------------------------------------------------------------------------- addressing
# A segment of a layer's input is (flat float32 buffer, features, offset, batch stride, step stride, parity stride): sample b of the
# launch with step word t reads buffer[offset + b * bs + t * ss + (t & 1) * ps + (0 .. k)]
Seg = collections.namedtuple("Seg", "buf k off bs ss ps")


def seg_rows(s, B, step):
    idx = s.off + torch.arange(B)[:, None] * s.bs + step * s.ss + (step & 1) * s.ps + torch.arange(s.k)[None, :]
    return s.buf.reshape(-1)[idx]


def hist_seg(g, B, rows, k):
    """rows of a per-step history [B, rows, k]"""
    return Seg(randn(g, B, rows, k), k, 0, rows * k, k, 0)


def parity_seg(g, B, k, negative):
    """a state double-buffered by step parity [2, B, k]; negative: the buffer of the OTHER parity, as the attention LSTM reads the
    contexts (base at buffer 1, parity stride -B k)"""
    buf = randn(g, 2, B, k)
    return Seg(buf, k, B * k, k, 0, -B * k) if negative else Seg(buf, k, 0, k, 0, B * k)


# ---------------------------------------------------------------------------------------------------------------- 1. dec_linear, plain form
LinCase = collections.namedtuple("LinCase", "shape B wdt act bias res step")
LIN_SHAPES = {           # name -> (segments, N, ldw, weight view offset by one element)
    "k1024": ((1024,), 256, 256, False),
    "n8": ((33,), 8, 8, False),
    "three": ((128, 288, 256), 1024, 1024, False),          # segment 1 with the negative parity stride, segment 2 with the positive one
    "n161": ((256,), 161, 161, False),                      # ldw % 4 != 0: the scalar path
    "n161_pad": ((256,), 161, 168, False),                  # the vector path; the padding columns hold NaN
    "n161_off1": ((256,), 161, 168, True),                  # the view starts one element in: the pointer fails the 16 / 8 byte test
}
LIN_B = (1, 2, 3, 5, 8, 9, 17)
LIN_STEPS = (0, 1, 5)
_LIN_ROWS = [("k1024", 8, ACT_RELU, True, False, 1), ("k1024", 1, ACT_NONE, False, True, 0),
             ("n8", 2, ACT_TANH, True, True, 5), ("n8", 17, ACT_SOFTSIGN, False, False, 1),
             ("three", 3, ACT_NONE, True, True, 0), ("three", 9, ACT_RELU, True, False, 1),
             ("n161", 9, ACT_TANH, True, True, 5), ("n161", 17, ACT_NONE, True, False, 0), ("n161", 5, ACT_SOFTSIGN, False, True, 1),
             ("n161_pad", 9, ACT_SOFTSIGN, True, False, 1), ("n161_pad", 17, ACT_RELU, False, True, 5), ("n161_pad", 1, ACT_TANH, True, False, 0),
             ("n161_off1", 5, ACT_RELU, True, True, 1), ("n161_off1", 8, ACT_NONE, False, False, 5)]
LIN_CASES = [LinCase(s, B, wdt, act, bias, res, step) for wdt in ("f32", "bf16") for (s, B, act, bias, res, step) in _LIN_ROWS]


def lin_coverage(cases):
    """the conditions the case list must meet (tests/test_decode_step_cpu.py)"""
    assert {c.B for c in cases} == set(LIN_B)
    assert {c.step for c in cases} == set(LIN_STEPS)
    for wdt in ("f32", "bf16"):
        mine = [c for c in cases if c.wdt == wdt]
        assert {c.shape for c in mine} == set(LIN_SHAPES), wdt
        assert {c.act for c in mine} == {ACT_NONE, ACT_RELU, ACT_TANH, ACT_SOFTSIGN}
        assert {c.bias for c in mine} == {True, False} and {c.res for c in mine} == {True, False}
        for shape in ("n161", "n161_pad"):
            assert {9, 17} <= {c.B for c in mine if c.shape == shape}, (wdt, shape)


@functools.lru_cache(maxsize=None)
def lin_inputs(case):
    """segments, weight values [K, N], bias, residual history [B, rows, N] (or None) and the number of history rows"""
    segs_k, N, ldw, off1 = LIN_SHAPES[case.shape]
    g = gen(1, LIN_CASES.index(case)) if case in LIN_CASES else gen(1, 999)
    rows = case.step + 2
    segs = [hist_seg(g, case.B, rows, segs_k[0])]
    if len(segs_k) == 3:
        segs += [parity_seg(g, case.B, segs_k[1], True), parity_seg(g, case.B, segs_k[2], False)]
    W = weight(g, sum(segs_k), N, case.wdt)
    b = 0.3 * randn(g, N) if case.bias else None
    res = randn(g, case.B, rows, N) if case.res else None
    return dict(segs=segs, W=W, b=b, res=res, rows=rows, N=N, ldw=ldw, off1=off1)


def lin_ref(case, dtype=torch.float64):
    z = lin_inputs(case)
    return dense_ref([seg_rows(s, case.B, case.step) for s in z["segs"]], z["W"], z["b"], case.act,
                     res=None if z["res"] is None else z["res"][:, case.step], dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------- 2. dec_linear, LSTM form
LstmCase = collections.namedtuple("LstmCase", "H B step wdt")
LSTM_SEGS = {8: (5, 12), 64: (33, 40), 256: (128, 288)}          # the two segments in front of h (three segments in all)
LSTM_ZC, LSTM_ZH = 0.1, 0.25
LSTM_CASES = [LstmCase(H, B, step, wdt) for (H, B, step, wdt) in
              [(8, 1, 0, "f32"), (8, 9, 1, "bf16"), (8, 3, 1, "f32"), (64, 3, 0, "bf16"), (64, 8, 1, "f32"), (64, 9, 0, "f32"),
               (256, 1, 1, "bf16"), (256, 8, 0, "bf16"), (256, 9, 1, "f32"), (256, 3, 0, "f32")]]


def lstm_coverage(cases):
    assert {c.H for c in cases} == {8, 64, 256} and {c.B for c in cases} == {1, 3, 8, 9} and {c.step for c in cases} == {0, 1}
    assert {c.wdt for c in cases} == {"f32", "bf16"} and LSTM_ZC != LSTM_ZH
    for H in (8, 64, 256):
        assert {c.step for c in cases if c.H == H} == {0, 1}


@functools.lru_cache(maxsize=None)
def lstm_inputs(case):
    g = gen(2, LSTM_CASES.index(case))
    k0, k1 = LSTM_SEGS[case.H]
    rows = case.step + 2
    h = parity_seg(g, case.B, case.H, False)          # the h state IS the third segment
    segs = [hist_seg(g, case.B, rows, k0), parity_seg(g, case.B, k1, True), h]
    W = weight(g, k0 + k1 + case.H, 4 * case.H, case.wdt)
    return dict(segs=segs, W=W, b=0.3 * randn(g, 4 * case.H), c=randn(g, 2, case.B, case.H), h=h.buf, rows=rows)


def lstm_case_ref(case, dtype=torch.float64):
    z = lstm_inputs(case)
    par = case.step & 1
    xs = [seg_rows(s, case.B, case.step) for s in z["segs"][:2]]
    return lstm_ref(xs, z["c"][par], z["h"][par], z["W"], z["b"], LSTM_ZC, LSTM_ZH, dtype)


# ---------------------------------------------------------------------------------------------------------------- 3. dropout on inference
DROP_RATES = (0.5, 0.1)
DROP_T, DROP_STEP, DROP_B, DROP_SEED, DROP_STREAM = 7, 3, 3, 12345, 8
DROP_CASE = LinCase("n161_pad", DROP_B, "bf16", ACT_TANH, True, True, DROP_STEP)

# ---------------------------------------------------------------------------------------------------------------- 4. step bookkeeping
# The kernel's sigmoid is 1 / (1 + __expf(-x)) in fp32.  Threshold 0.5 and the logit 0.0: exp(-0.0) is exactly 1 in any evaluation,
# 1 / (1 + 1) is exactly 0.5 - the float32 logit whose sigmoid EQUALS the threshold (np.float32(1) / (np.float32(1) +
# np.exp(np.float32(-0.0))) == np.float32(0.5), checked in tests/test_decode_step_cpu.py).  The rule is strict: no flag.
STOP_THRESHOLD, STOP_EQUAL_LOGIT, STOP_MIN = 0.5, 0.0, 3
StopCase = collections.namedtuple("StopCase", "name B t logits flag0 want")          # logits: "high", or {sample: logit} over "high"
STOP_CASES = [StopCase("t0", 3, 0, "high", 0, 0),
              StopCase("t-1=min-1", 3, STOP_MIN, "high", 0, 0),
              StopCase("t-1=min", 3, STOP_MIN + 1, "high", 0, 0),
              StopCase("t-1=min+1", 3, STOP_MIN + 2, "high", 0, STOP_MIN + 2),
              StopCase("equal", 3, STOP_MIN + 3, {1: STOP_EQUAL_LOGIT}, 0, 0),
              StopCase("B70_one_low", 70, STOP_MIN + 3, {69: -2.0}, 0, 0),
              StopCase("B70_all_high", 70, STOP_MIN + 3, "high", 0, STOP_MIN + 3),
              StopCase("sticky", 3, STOP_MIN + 3, "high", 2, 2)]


def stop_logits(case, rows):
    """[B, rows]: row t - 1 holds the case's logits; every OTHER row holds what would give the opposite answer"""
    fired = case.want == case.t and case.flag0 == 0
    z = torch.full((case.B, rows), -4.0 if fired else 4.0)
    if case.t >= 1:
        z[:, case.t - 1] = 4.0
        if case.logits != "high":
            for b, v in case.logits.items():
                z[b, case.t - 1] = v
    return z


# ---------------------------------------------------------------------------------------------------------------- 5. dec_linear2
L2_SHAPES = ((160, 256, 128, 256, 128), (256, 256, 256, 256, 256), (5, 12, 161, 12, 164))          # K1, N1, N2, ldw1, ldw2
L2_B = (1, 3, 8)
L2Case = collections.namedtuple("L2Case", "shape B act1 act2 step")
L2_CASES = [L2Case(L2_SHAPES[0], 1, ACT_RELU, ACT_RELU, 0), L2Case(L2_SHAPES[0], 8, ACT_RELU, ACT_TANH, 1),
            L2Case(L2_SHAPES[1], 3, ACT_TANH, ACT_NONE, 1), L2Case(L2_SHAPES[1], 8, ACT_SOFTSIGN, ACT_RELU, 0),
            L2Case(L2_SHAPES[2], 3, ACT_RELU, ACT_SOFTSIGN, 0), L2Case(L2_SHAPES[2], 1, ACT_TANH, ACT_TANH, 1)]
L2_DROP = ((0.5, 8), (0.1, 9))          # (rate, stream) of the two layers
L2_DROP_T = 4


def l2_coverage(cases):
    assert {c.shape for c in cases} == set(L2_SHAPES) and {c.B for c in cases} == set(L2_B)
    assert L2_DROP[0][1] != L2_DROP[1][1]


@functools.lru_cache(maxsize=None)
def l2_inputs(case):
    K1, N1, N2, _, _ = case.shape
    g = gen(5, L2_CASES.index(case))
    rows = case.step + 2
    return dict(x=hist_seg(g, case.B, rows, K1), W1=weight(g, K1, N1, "bf16"), b1=0.3 * randn(g, N1), res1=randn(g, case.B, N1),
                W2=weight(g, N1, N2, "bf16"), b2=0.3 * randn(g, N2), rows=rows)


def l2_ref(case, dtype=torch.float64):
    """(intermediate vector, output)"""
    K1, N1, N2, _, _ = case.shape
    z = l2_inputs(case)
    k1 = keep_rows(DROP_SEED, L2_DROP[0][1], case.B, L2_DROP_T, N1, L2_DROP[0][0], case.step)
    k2 = keep_rows(DROP_SEED, L2_DROP[1][1], case.B, L2_DROP_T, N2, L2_DROP[1][0], case.step)
    h = dense_ref([seg_rows(z["x"], case.B, case.step)], z["W1"], z["b1"], case.act1, k1, 1.0 / (1.0 - L2_DROP[0][0]), z["res1"], dtype)
    return h, dense_ref([h], z["W2"], z["b2"], case.act2, k2, 1.0 / (1.0 - L2_DROP[1][0]), None, dtype)


# ---------------------------------------------------------------------------------------------------------------- 6. dec_linear_chain
CHAIN_PRE = {1: ((160, 128),), 2: ((80, 256), (256, 128))}          # (K, N) of the pre-layers; the last N is the main layer's first segment
CHAIN_B = (1, 2, 3, 4, 5, 9)
ChainCase = collections.namedtuple("ChainCase", "npre main B step")          # main: "plain" ([128 chained], 161, 168) or "lstm" (H = 256)
CHAIN_CASES = [ChainCase(n, m, B, s) for (n, m, B, s) in
               [(1, "plain", 1, 0), (1, "plain", 5, 1), (1, "plain", 9, 0), (1, "plain", 4, 1), (1, "lstm", 2, 1), (1, "lstm", 3, 0),
                (2, "plain", 2, 1), (2, "plain", 3, 0), (2, "lstm", 1, 0), (2, "lstm", 4, 1), (2, "lstm", 5, 0), (2, "lstm", 9, 1)]]
CHAIN_H, CHAIN_LSTM_SEGS = 256, (288, 256)


def chain_coverage(cases):
    assert {c.npre for c in cases} == {1, 2} and {c.B for c in cases} == set(CHAIN_B)
    assert {(c.npre, c.main) for c in cases} == {(n, m) for n in (1, 2) for m in ("plain", "lstm")}
    for m in ("plain", "lstm"):          # a ragged last group of four samples in both main forms
        assert {c.B for c in cases if c.main == m} & {5, 9}
    assert any(c.npre == 1 and c.main == "plain" for c in cases)          # NPRE = 1 in front of a plain layer with N % 32 != 0


@functools.lru_cache(maxsize=None)
def chain_inputs(case):
    g = gen(6, CHAIN_CASES.index(case))
    rows = case.step + 2
    pre = [dict(W=weight(g, K, N, "bf16"), b=0.3 * randn(g, N)) for K, N in CHAIN_PRE[case.npre]]
    z = dict(x=hist_seg(g, case.B, rows, CHAIN_PRE[case.npre][0][0]), pre=pre, rows=rows)
    if case.main == "plain":
        z.update(W=weight(g, 128, 161, "bf16"), b=0.3 * randn(g, 161), res=randn(g, case.B, rows, 161))
    else:
        H = CHAIN_H
        h = parity_seg(g, case.B, H, False)
        z.update(segs=[parity_seg(g, case.B, CHAIN_LSTM_SEGS[0], True), h], W=weight(g, 128 + 288 + H, 4 * H, "bf16"),
                 b=0.3 * randn(g, 4 * H), c=randn(g, 2, case.B, H), h=h.buf)
    return z


def chain_ref(case, dtype=torch.float64):
    """(the intermediate vectors, the main layer's result: y, or (y, c state, h state))"""
    z = chain_inputs(case)
    v, mids = seg_rows(z["x"], case.B, case.step), []
    for q in z["pre"]:
        v = dense_ref([v], q["W"], q["b"], ACT_RELU, dtype=dtype)
        mids.append(v)
    if case.main == "plain":
        return mids, dense_ref([v], z["W"], z["b"], ACT_TANH, res=z["res"][:, case.step], dtype=dtype)
    par = case.step & 1
    return mids, lstm_ref([v, seg_rows(z["segs"][0], case.B, case.step)], z["c"][par], z["h"][par], z["W"], z["b"], LSTM_ZC, LSTM_ZH, dtype)


# ---------------------------------------------------------------------------------------------------------------- 8. dec_self_attn
SA_PROD = dict(D=256, heads=2, B=2, Td=1031)
SA_PROD_T = (0, 1, 63, 64, 255, 256, 257, 1023, 1024, 1030)
SA_REGIME_T = 257
SA_BIG = dict(D=256, heads=2, B=1, Td=13000, t=12999)
SA_ANY = ((16, 2), (64, 4), (96, 3), (256, 1), (1024, 1))
SA_ANY_TD, SA_ANY_T, SA_ANY_B = 70, (0, 37, 69), 2


@functools.lru_cache(maxsize=4)
def sa_cache(B, Td, D, heads, regime="normal", seed=0):
    """the K | V | Q cache [B, Td, 3 D] (every row finite: the test poisons the rows above t).
    sharp: every query is 4 x key row SA_REGIME_T // 2 - that row's score (~45) stands ten deviations above the rest;
    offset: keys = one direction + small noise and the queries along it, every score within ~1 of +100"""
    g = gen(8, B, Td, D, heads, seed)
    kvq = randn(g, B, Td, 3 * D)
    hd = D // heads
    if regime == "sharp":
        kvq[:, :, 2 * D:] = 4.0 * kvq[:, SA_REGIME_T // 2, None, :D]
    elif regime == "offset":
        d = randn(g, B, 1, D)
        d = d.reshape(B, 1, heads, hd)
        d = (d / d.norm(dim=-1, keepdim=True)).reshape(B, 1, D)          # unit direction per head
        kvq[:, :, :D] = 10.0 * d + 0.1 * kvq[:, :, :D]
        kvq[:, :, 2 * D:] = (10.0 * math.sqrt(hd)) * d
    return kvq


def self_attn_ref(kvq, t, D, heads, dtype=torch.float64):
    """softmax(q K^T / sqrt(hd)) V of the query of row t over cache rows 0 .. t, per head: [B, D]"""
    B, hd = kvq.shape[0], D // heads
    x = kvq[:, :t + 1].to(dtype)
    k = x[:, :, :D].reshape(B, t + 1, heads, hd)
    v = x[:, :, D:2 * D].reshape(B, t + 1, heads, hd)
    q = x[:, t, 2 * D:].reshape(B, heads, hd)
    s = torch.einsum("bhd,bjhd->bhj", q, k) * (1.0 / math.sqrt(hd))
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bhj,bjhd->bhd", p, v).reshape(B, D)


# ---------------------------------------------------------------------------------------------------------------- 9. dec_attention
ATT_WIDTHS = {"prod": (256, 224, 256, 32, 32), "small": (64, 32, 64, 8, 32), "single": (256, 128, 256, 0, 0)}          # A, U1, V1, U2, V2
ATT_KERNELS = (10, 6, 31)
ATT_TI = (1, 7, 9, 17, 100, 256, 257, 513, 1100)
ATT_MODES = ("forward", "cumulative", "location_sensitive", "agent", "forced1", "forced2")
ATT_MODE_TI = (9, 257, 1100)
ATT_B, ATT_STEPS, ATT_TD = 3, 3, 4
AttCase = collections.namedtuple("AttCase", "widths kernel Ti mode wq")


def _att_cases():
    cases = [AttCase("prod", 10, Ti, "forward", ("f32", "bf16")[i % 2]) for i, Ti in enumerate(ATT_TI)]
    n = 0
    for mode in ATT_MODES[1:]:
        for Ti in ATT_MODE_TI:
            w = ("small", "single", "prod")[n % 3]
            if mode == "forced2" and w == "single":          # a second teacher history needs a second source
                w = "small"
            cases.append(AttCase(w, ATT_KERNELS[(n // 3 + n) % 3], Ti, mode, ("bf16", "f32")[n % 2]))
            n += 1
    cases += [AttCase("small", 6, 17, "forward", "f32"), AttCase("single", 31, 100, "forward", "bf16")]
    return cases


ATT_CASES = _att_cases()


def att_coverage(cases):
    assert {c.Ti for c in cases if c.mode == "forward" and c.widths == "prod"} == set(ATT_TI)
    for mode in ATT_MODES:
        assert set(ATT_MODE_TI) <= {c.Ti for c in cases if c.mode == mode}, mode
    assert {c.widths for c in cases} == set(ATT_WIDTHS) and {c.kernel for c in cases} == set(ATT_KERNELS)
    assert {c.wq for c in cases} == {"f32", "bf16"}
    assert not any(c.mode == "forced2" and ATT_WIDTHS[c.widths][3] == 0 for c in cases)
    assert len(set(cases)) == len(cases)


def att_lengths(Ti):
    return torch.tensor([Ti, Ti // 2 + 1, 1], dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def att_inputs(case):
    return att_make(ATT_WIDTHS[case.widths], case.Ti, case.kernel, case.mode, ATT_CASES.index(case))


def att_make(widths, Ti, KW, mode, seed):
    """the host tensors of an attention problem of ATT_B samples, ATT_STEPS queries and ATT_TD history rows"""
    A, U1, V1, U2, V2 = widths
    B = ATT_B
    g = gen(9, seed)
    lens = att_lengths(Ti)
    mask = (torch.arange(Ti)[None, :] < lens[:, None]).float()[:, :, None]
    z = dict(lens=lens, hq=torch.tanh(randn(g, ATT_STEPS, B, A)), Wq=torch.as_tensor(bf16_round((randn(g, A, U1 + U2) / math.sqrt(A)).numpy())),
             keys1=randn(g, B, Ti, U1), values1=randn(g, B, Ti, V1) * mask,          # the values beyond the length are zero (masked memory)
             F=0.3 * randn(g, KW, 1, 5), bF=0.1 * randn(g, 5), U=0.3 * randn(g, 5, U1), v1=2.0 * randn(g, U1) / math.sqrt(U1),
             b1=0.1 * randn(g, U1))
    if U2:
        z.update(keys2=randn(g, B, Ti, U2), values2=randn(g, B, Ti, V2) * mask, v2=2.0 * randn(g, U2) / math.sqrt(U2))
    if mode == "agent":          # scaled as in tests/test_inference_gpu.py test_transition_agent_decode: 3 x an initialised Wa
        z.update(Wa=3.0 * randn(g, V1 + U1, 1) / math.sqrt(V1 + U1), ba=0.1 * randn(g, 1))
    if mode.startswith("forced"):
        t1, t2 = teacher_rows(B, ATT_TD, Ti, lens, True, masked=True, seed=seed, sharp=3)
        z.update(teach1=t1, teach2=t2 if mode == "forced2" else None)
    return z


def att_P(z, dtype, agent=True):
    names = {"Wq": "dec.att.Wq", "F": "dec.att1.F", "bF": "dec.att1.bF", "U": "dec.att1.U", "v1": "dec.att1.v", "b1": "dec.att1.b",
             "v2": "dec.att2.v"}
    if agent:
        names.update(Wa="dec.att1.Wa", ba="dec.att1.ba")
    return {n: z[k].to(dtype) for k, n in names.items() if k in z}


def attention_chain(keys1, values1, keys2, values2, queries, P, lens, mode="forward", cumulative=False, agent=False, teach=None):
    """torch_ref.forward_attention_step / additive_attention_step chained over the queries [steps, B, A] from the initial state
    (zeros, onehot(0), u = 0.5); teach = (rows1, rows2 or None): the alignments are the teacher rows.  Per step a dictionary:
    align1, align2 (None: single source), ctx, a_state (the next location-conv input), alpha_state, pq (None when forced)"""
    B, Ti = keys1.shape[0], keys1.shape[1]
    dual = keys2 is not None
    zero = keys1.new_zeros(B, Ti)
    state = (zero, torch.cat([keys1.new_ones(B, 1), keys1.new_zeros(B, Ti - 1)], dim=1), 0.5)
    out = []
    for t in range(queries.shape[0]):
        q = queries[t]
        if teach is not None:
            a1 = teach[0][:, t].to(keys1.dtype)
            a2 = (teach[1][:, t].to(keys1.dtype) if teach[1] is not None else zero) if dual else None
            nxt, pq = a1, None
        else:
            a1, state = torch_ref.forward_attention_step(q, keys1, state, P, lens, mode, cumulative, values1, agent)
            a2 = torch_ref.additive_attention_step(q, keys2, P, lens) if dual else None
            nxt, pq = state[0], q @ P["dec.att.Wq"]
        ctx = (a1[:, :, None] * values1).sum(1)
        if dual:
            ctx = torch.cat([ctx, (a2[:, :, None] * values2).sum(1)], dim=-1)
        out.append(dict(align1=a1, align2=a2, ctx=ctx, a_state=nxt, alpha_state=a1, pq=pq))
    return out


def att_ref(case, dtype=torch.float64, agent=None):
    z = att_inputs(case)
    agent = (case.mode == "agent") if agent is None else agent
    c = lambda k: z[k].to(dtype) if k in z else None
    teach = (z["teach1"], z["teach2"]) if case.mode.startswith("forced") else None
    return attention_chain(c("keys1"), c("values1"), c("keys2"), c("values2"), z["hq"].to(dtype), att_P(z, dtype, agent), z["lens"],
                           "location_sensitive" if case.mode == "location_sensitive" else "forward", case.mode == "cumulative", agent, teach)


@functools.lru_cache(maxsize=None)
def att_ref64(case):
    return att_ref(case)


# ---------------------------------------------------------------------------------------------------------------- GPU half
class Holder:
    """keeps every device tensor a parameter block points to alive until the test drops it (behind torch.cuda.synchronize())"""

    def __init__(self, device="cuda"):
        self.device, self.kept = device, []

    def __call__(self, t, dtype=None):
        """a contiguous device copy of a host tensor"""
        d = torch.as_tensor(t).to(device=self.device, dtype=dtype).contiguous().clone()
        self.kept.append(d)
        return d

    def full(self, shape, value, dtype=torch.float32):
        d = torch.full(shape, value, dtype=dtype, device=self.device)
        self.kept.append(d)
        return d

    def keep(self, *objs):
        self.kept.extend(objs)
        return objs[0]

    def matrix(self, W, ldw, wdt, off1=False):
        """the device matrix of a layer: [K, N] view of rows of ldw elements whose padding columns hold NaN; off1: the view starts
        one element into its allocation"""
        K, N = W.shape
        dt = torch.bfloat16 if wdt == "bf16" else torch.float32
        flat = torch.full((K * ldw + 1,), float("nan"), dtype=dt, device=self.device)
        self.kept.append(flat)
        m = flat[1 if off1 else 0:][:K * ldw].view(K, ldw)[:, :N]
        m.copy_(W.to(self.device))
        return m

    def seg(self, s):
        """the (tensor, features, batch stride, step stride, parity stride) entry of ops.dec_linear_params for a Seg"""
        d = self(s.buf)
        return (d.view(-1)[s.off:], s.k, s.bs, s.ss, s.ps)
