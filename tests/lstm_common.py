"""Shared by tests/test_lstm_cpu.py and tests/test_lstm_gpu.py: a plain float64 loop of the recurrent ZoneoutLSTM as
include/satt_hip.h states it (the reference of the kernels in csrc/lstm.hip and csrc/lstm_cluster.hip), the same loop in numpy at a
chosen precision (the conditioning check of the inputs and the sensitivity figures of the bars), the input generator, the comparison
helper and the case tables.

The recurrence (gate order i, j, f, o; xg holds the input's share of the gate pre-activations, Wh the bf16-rounded recurrent weights):
    z = xg[t] + h Wh;  gi = sigmoid(z_i), gj = tanh(z_j), gf = sigmoid(z_f + 1), go = sigmoid(z_o)
    c' = gf c + gi gj;  h' = go tanh(c');  hout[t] = h' (pre-zoneout)
    training: c = keep_c[b, t] ? c' : c, h = keep_h[b, t] ? h' : h   (oracle.rng.keep_mask(seed, stream, (B, T, H), rate); rate 0 keeps all)
    eval:     c = (1 - zc) c' + zc c,    h = (1 - zh) h' + zh h
Direction 1 walks t = len - 1 .. 0.  At t >= len nothing runs: the state is frozen and every tensor written there is zero.
Saved tensors: gates = (gi, gj, gf, go) [ndir, B, T, 4H], cnew = c', cstate = c, hstate = h [ndir, B, T, H]; hout [B, T, ndir * H] with
direction d at columns d * H; dxg [ndir, B, T, 4H] = the gradient of sum(hout * dh) wrt xg.

No import of the package: the module loads on a machine without the library."""
import collections
import functools
import math

import numpy as np
import torch

from oracle import rng

BAR_FWD = 1e-5       # everything the forward writes (tests/test_ops_gpu.py: test_lstm_fwd_bwd, test_lstm_cluster_fwd_bwd)
BAR_DXG = 5e-5       # dxg (same tests)
SAVED = ("gates", "cnew", "cstate", "hstate")
FWD_NAMES = ("hout",) + SAVED

# zoneout modes: (training, zc, zh)
Z_TRAIN = (True, 0.1, 0.15)
Z_TRAIN_00 = (True, 0.0, 0.0)          # the zct == 0 / zht == 0 short-cuts
Z_TRAIN_0H = (True, 0.0, 0.5)          # one short-cut, one mask
Z_EVAL = (False, 0.1, 0.15)
Z_MODES = (Z_TRAIN, Z_TRAIN_00, Z_TRAIN_0H, Z_EVAL)

Case = collections.namedtuple("Case", "H B T ndir lengths mode scale pad C seed")


def case_id(c):
    s = "H%d-B%d-T%d-d%d" % (c.H, c.B, c.T, c.ndir)
    if c.C:
        s += "-C%d" % c.C
    if c.lengths is not None:
        s += "-L" + ".".join(str(v) for v in c.lengths)
    s += "-%s%g.%g" % ("tr" if c.mode[0] else "ev", c.mode[1], c.mode[2])
    if c.scale != 1.0:
        s += "-s%g" % c.scale
    if c.pad:
        s += "-pad%d" % c.pad
    return s


def _mk(table, H, B, T, ndir, lengths=None, mode=Z_TRAIN, scale=1.0, pad=0, C=0):
    assert lengths is None or (len(lengths) == B and max(lengths) <= T)
    table.append(Case(H, B, T, ndir, None if lengths is None else tuple(lengths), mode, scale, pad, C, 1000 + len(table)))


# ---- single-workgroup kernels (satt_lstm_fwd / satt_lstm_bwd) ------------------------------------------------------------------
LEN_A = (6, 9, (9, 1, 2, 3, 4, 5))       # every len % 4, len 1, len == T (T % 4 == 1)
LEN_B = (4, 13, (13, 8, 7, 6))           # more than one group of four steps in both walks
LEN_C = (3, 5, (5, 0, 3))                # a sample of length 0
LEN_S = (3, 5, (5, 1, 3))                # streaming form

SINGLE = []
for _H in (8, 24, 40, 104, 128):         # register-resident form (H <= 128): a unit count below one wave tile, ragged tiles, the limit
    for _B, _T, _L in (LEN_A, LEN_B, LEN_C):
        _mk(SINGLE, _H, _B, _T, 2, _L)
    for _T in (1, 3, 4, 5):              # T below, at and above one group of four steps
        _mk(SINGLE, _H, 2, _T, 1)
for _H in (136, 256):                    # streaming form (H > 128)
    _mk(SINGLE, _H, *LEN_S[:2], 2, LEN_S[2])
    _mk(SINGLE, _H, 2, 1, 1)
_mk(SINGLE, 1024, 2, 3, 2, (3, 2))       # the launchers' limit: KS = 2 forward, KS = 8 backward
for _H in (24, 128, 136):                # zoneout modes (Z_TRAIN is in the groups above)
    for _m in (Z_TRAIN_00, Z_TRAIN_0H, Z_EVAL):
        _B, _T, _L = LEN_C if _H <= 128 else LEN_S
        _mk(SINGLE, _H, _B, _T, 2, _L, mode=_m)
_mk(SINGLE, 128, *LEN_B[:2], 2, LEN_B[2], scale=6.0)      # saturated gates
_mk(SINGLE, 136, *LEN_S[:2], 2, LEN_S[2], scale=6.0)
_mk(SINGLE, 40, *LEN_A[:2], 2, LEN_A[2], pad=8)           # ld_hout / ld_dhout = ndir * H + 8
_mk(SINGLE, 136, *LEN_S[:2], 2, LEN_S[2], pad=8)

# H the forward launcher accepts and the backward launcher declines (H % 8 != 0): forward only, eval mode
SINGLE_FWD_ONLY = []
_mk(SINGLE_FWD_ONLY, 12, *LEN_C[:2], 2, LEN_C[2], mode=Z_EVAL)
_mk(SINGLE_FWD_ONLY, 132, *LEN_C[:2], 2, LEN_C[2], mode=Z_EVAL)

# ---- cluster kernels (satt_lstm_cluster_fwd / _bwd): ndir = 1, no lengths -------------------------------------------------------
CLUSTER_HC = ((16, 2), (48, 2), (128, 2), (64, 8), (192, 4), (256, 4), (256, 8))
CLUSTER = []
for _H, _C in CLUSTER_HC:
    _mk(CLUSTER, _H, 3, 7, 1, C=_C)
for _H, _C in ((256, 4), (64, 8)):
    for _B in (1, 8):
        for _T in (1, 2, 7):
            _mk(CLUSTER, _H, _B, _T, 1, C=_C)
for _H, _C in ((256, 4), (48, 2)):
    for _m in (Z_TRAIN_00, Z_TRAIN_0H, Z_EVAL):
        _mk(CLUSTER, _H, 3, 7, 1, mode=_m, C=_C)
_mk(CLUSTER, 256, 3, 7, 1, pad=8, C=4)

CHUNKS = ((0, 1), (1, 2), (2, 18), (18, 23))
CLUSTER_CHUNKED = []
for _m in (Z_TRAIN, Z_EVAL):
    _mk(CLUSTER_CHUNKED, 256, 3, 23, 1, mode=_m, C=4)

PACK_STRIDE = ((256, 4), (48, 2))

# ---- fused input projection (satt_lstm_cluster_pack_in / satt_lstm_cluster_fwd_x) ----------------------------------------------
FusedCase = collections.namedtuple("FusedCase", "H C B T Kin xpad bias seed")
FUSED_CHUNKS = ((0, 1), (1, 17), (17, 37))
FUSED = [FusedCase(H, C, 3, 37, Kin, xpad, bias, 2000 + i)
         for i, (H, C, Kin, xpad, bias) in enumerate((H, C, Kin, xpad, bias) for H, C in ((256, 4), (64, 8))
                                                     for Kin in (4, 36, 100, 256, 544) for xpad in (0, 12) for bias in (True, False))]


def fused_id(c):
    return "H%d-C%d-K%d-ldx%d-%s" % (c.H, c.C, c.Kin, c.Kin + c.xpad, "bias" if c.bias else "nobias")


ALL_RECURRENT = SINGLE + SINGLE_FWD_ONLY + CLUSTER + CLUSTER_CHUNKED       # every case that is compared with the float64 loop


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def bf16_round(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


Inputs = collections.namedtuple("Inputs", "xg Wh dh lengths")


@functools.lru_cache(maxsize=None)
def inputs(case):
    """xg ~ N(0, scale) fp32 [ndir, B, T, 4H], Wh ~ N(0, 1/sqrt(H)) bf16-rounded fp32 [ndir, H, 4H], dh ~ N(0, 1) fp32 [B, T, ndir * H]"""
    g = np.random.default_rng(case.seed)
    xg = g.normal(0, case.scale, (case.ndir, case.B, case.T, 4 * case.H)).astype(np.float32)
    Wh = bf16_round(g.normal(0, 1.0 / math.sqrt(case.H), (case.ndir, case.H, 4 * case.H)))
    dh = g.normal(0, 1, (case.B, case.T, case.ndir * case.H)).astype(np.float32)
    lens = np.full(case.B, case.T, dtype=np.int64) if case.lengths is None else np.asarray(case.lengths, dtype=np.int64)
    for a in (xg, Wh, dh, lens):
        a.setflags(write=False)
    return Inputs(xg, Wh, dh, lens)


def streams(case):
    """zoneout stream ids (cell, hidden) per direction: the encoder's for the single-workgroup kernels, LSTM1's for the cluster form"""
    if case.C:
        return (rng.STREAM_LSTM1_C,), (rng.STREAM_LSTM1_H,)
    return (rng.STREAM_ENC_LSTM_FW_C, rng.STREAM_ENC_LSTM_BW_C)[:case.ndir], (rng.STREAM_ENC_LSTM_FW_H, rng.STREAM_ENC_LSTM_BW_H)[:case.ndir]


def keep_masks(case):
    """[ndir][2] boolean (B, T, H) keep masks (cell, hidden); None where everything is kept or the mode is eval"""
    training, zc, zh = case.mode
    sc, sh = streams(case)
    shape = (case.B, case.T, case.H)
    out = []
    for d in range(case.ndir):
        out.append((rng.keep_mask(case.seed, sc[d], shape, zc) if training and zc > 0 else None,
                    rng.keep_mask(case.seed, sh[d], shape, zh) if training and zh > 0 else None))
    return out


# ---- the float64 reference (torch: autograd gives dxg) ---------------------------------------------------------------------------
def reference_from(xg, Wh, dh, lens, mode, masks):
    """xg [ndir, B, T, 4H], Wh [ndir, H, 4H], dh [B, T, ndir * H] (or None: no dxg), lens [B]; float64 torch tensors out"""
    training, zc, zh = mode
    ndir, B, T, G = xg.shape
    H = G // 4
    x = torch.tensor(np.array(xg), dtype=torch.float64).requires_grad_(dh is not None)
    W = torch.tensor(np.array(Wh), dtype=torch.float64)
    zH, zG = torch.zeros(H, dtype=torch.float64), torch.zeros(G, dtype=torch.float64)
    res = {n: [] for n in FWD_NAMES}
    for d in range(ndir):
        kc, kh = (None if m is None else torch.from_numpy(m) for m in masks[d])
        per = {n: [] for n in FWD_NAMES}
        for b in range(B):
            L = int(lens[b])
            rows = {n: [zG if n == "gates" else zH] * T for n in FWD_NAMES}
            c, h = zH, zH
            for s in range(L):
                t = L - 1 - s if d == 1 else s
                z = x[d, b, t] + h @ W[d]
                gi, gj = torch.sigmoid(z[:H]), torch.tanh(z[H:2 * H])
                gf, go = torch.sigmoid(z[2 * H:3 * H] + 1.0), torch.sigmoid(z[3 * H:])
                cn = gf * c + gi * gj
                hn = go * torch.tanh(cn)
                if training:
                    c = cn if kc is None else torch.where(kc[b, t], cn, c)
                    h = hn if kh is None else torch.where(kh[b, t], hn, h)
                else:
                    c = (1.0 - zc) * cn + zc * c
                    h = (1.0 - zh) * hn + zh * h
                rows["hout"][t], rows["gates"][t], rows["cnew"][t] = hn, torch.cat([gi, gj, gf, go]), cn
                rows["cstate"][t], rows["hstate"][t] = c, h
            for n in FWD_NAMES:
                per[n].append(torch.stack(rows[n]))
        for n in FWD_NAMES:
            res[n].append(torch.stack(per[n]))
    out = {n: torch.stack(res[n]) for n in SAVED}
    out["hout"] = torch.cat(res["hout"], dim=-1)
    if dh is not None:
        (out["hout"] * torch.tensor(np.array(dh), dtype=torch.float64)).sum().backward()
        out["dxg"] = x.grad
    return {n: v.detach() for n, v in out.items()}


@functools.lru_cache(maxsize=None)
def reference(case):
    """the float64 result of a table case, computed once and shared (callers must not write into it)"""
    inp = inputs(case)
    return reference_from(inp.xg, inp.Wh, inp.dh, inp.lengths, case.mode, keep_masks(case))


# ---- the same loop in numpy at a chosen precision, backward by hand --------------------------------------------------------------
def split_rows(v, rows):
    """the sum of the first `rows` bf16 rows of the three-way split of fp32 `v` (csrc/mfma_rec.h, xs_put); rows = 3 is v itself"""
    v = np.asarray(v, dtype=np.float32)
    acc = np.zeros_like(v)
    rem = v.copy()
    for _ in range(rows):
        part = bf16_round(rem)
        acc = acc + part
        rem = rem - part
    return acc


def numpy_loop(xg, Wh, dh, lens, mode, masks, dtype, state_rows=None):
    """the recurrence and its backward in `dtype` arithmetic; state_rows: the h that enters the recurrent product is cut to that many
    bf16 rows of its fp32 split (what the register-resident kernels would compute if they dropped rows of the split)"""
    training, zc, zh = mode
    ndir, B, T, G = xg.shape
    H = G // 4
    dt = np.dtype(dtype).type
    one, zc, zh = dt(1), dt(zc), dt(zh)
    x, W, dho = xg.astype(dtype), Wh.astype(dtype), dh.astype(dtype)
    sig = lambda v: one / (one + np.exp(-v))
    out = {"hout": np.zeros((B, T, ndir * H), dtype), "gates": np.zeros((ndir, B, T, G), dtype), "dxg": np.zeros((ndir, B, T, G), dtype)}
    for n in ("cnew", "cstate", "hstate"):
        out[n] = np.zeros((ndir, B, T, H), dtype)
    for d in range(ndir):
        kc, kh = masks[d]
        for b in range(B):
            L = int(lens[b])
            order = [L - 1 - s if d == 1 else s for s in range(L)]
            c, h = np.zeros(H, dtype), np.zeros(H, dtype)
            for t in order:
                hin = h if state_rows is None else split_rows(h, state_rows).astype(dtype)
                z = x[d, b, t] + hin @ W[d]
                gi, gj, gf, go = sig(z[:H]), np.tanh(z[H:2 * H]), sig(z[2 * H:3 * H] + one), sig(z[3 * H:])
                cn = gf * c + gi * gj
                hn = go * np.tanh(cn)
                if training:
                    c = cn if kc is None else np.where(kc[b, t], cn, c)
                    h = hn if kh is None else np.where(kh[b, t], hn, h)
                else:
                    c = (one - zc) * cn + zc * c
                    h = (one - zh) * hn + zh * h
                out["hout"][b, t, d * H:(d + 1) * H] = hn
                out["gates"][d, b, t] = np.concatenate([gi, gj, gf, go])
                out["cnew"][d, b, t], out["cstate"][d, b, t], out["hstate"][d, b, t] = cn, c, h
            dc, dhs = np.zeros(H, dtype), np.zeros(H, dtype)          # gradients wrt the carried (post-zoneout) state
            for s in range(L - 1, -1, -1):
                t = order[s]
                if training:
                    kcv = np.ones(H, dtype) if kc is None else kc[b, t].astype(dtype)
                    khv = np.ones(H, dtype) if kh is None else kh[b, t].astype(dtype)
                    pcv, phv = one - kcv, one - khv
                else:
                    kcv, pcv, khv, phv = one - zc, zc, one - zh, zh
                gi, gj, gf, go = np.split(out["gates"][d, b, t], 4)
                cn = out["cnew"][d, b, t]
                cp = out["cstate"][d, b, order[s - 1]] if s > 0 else np.zeros(H, dtype)
                dhn = dho[b, t, d * H:(d + 1) * H] + khv * dhs
                tc = np.tanh(cn)
                dcn = dhn * go * (one - tc * tc) + kcv * dc
                dz = np.concatenate([dcn * gj * gi * (one - gi), dcn * gi * (one - gj * gj), dcn * cp * gf * (one - gf),
                                     dhn * tc * go * (one - go)])
                dc = dcn * gf + pcv * dc
                out["dxg"][d, b, t] = dz
                dhs = dz @ W[d].T + phv * dhs
    return out


def case_numpy(case, dtype, state_rows=None):
    inp = inputs(case)
    return numpy_loop(inp.xg, inp.Wh, inp.dh, inp.lengths, case.mode, keep_masks(case), dtype, state_rows)


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def by_direction(name, t, ndir):
    """[ndir, ...] view of a result: hout's directions are column blocks"""
    t = torch.as_tensor(t).detach().double().cpu()
    if name == "hout":
        return torch.stack(t.chunk(ndir, dim=-1)).reshape(ndir, -1)
    return t.reshape(ndir, -1)


def rel_errs(name, got, want, ndir):
    """max |got - want| / max |want| per direction"""
    g, w = by_direction(name, got, ndir), by_direction(name, want, ndir)
    return [float((g[d] - w[d]).abs().max() / (w[d].abs().max() + 1e-12)) for d in range(ndir)]


def close(name, got, want, tol, ndir=1, what=""):
    errs = rel_errs(name, got, want, ndir)
    for d, err in enumerate(errs):
        print("%-40s rel_err=%.3e (bar %.1e)" % ("%s %s d%d" % (what, name, d), err, tol))
    for d, err in enumerate(errs):
        assert err < tol, (what, name, d, err, tol)       # (a NaN fails: NaN < tol is false)
    return max(errs)


def bar(name):
    return BAR_DXG if name == "dxg" else BAR_FWD
