"""The deferred attention gradients (csrc/attn_rnn.hip: attn_param_grads_k, attn_param_grads_saf_k, attn_param_grads_finish_k)
against a float64 reference written from the energy arguments themselves.

    x1 = keys1 + b1 + pq1 + fl . U        x2 = keys2 + pq2        (per sample, step, memory row, unit)
    g = d e * v * (1 - tanh^2 x):  d keys = sum_t g,  d b = sum g,  d U = sum fl g,  d v = sum d e tanh x

The saved-factor kernel reads the fp16 factors the folded forward kernel stores (satt_attn_rnn_params.saf) instead of x; this
test builds them from x in float64 with the forward kernel's encoding and rounding (`encode_saf`).  Two bars per tensor:
  * arithmetic: against the same sums over the DECODED fp16 factors, max-norm 1e-5 of the tensor's scale (the kernel's own work);
  * representation: against the exact float64 derivative, relative L2 3e-3 (a few x 2^-11: what fp16 RELATIVE rounding of the
    factors allows) - in every energy regime, the saturated one included (|x| 3 .. 10: 1 - tanh^2 spans 1e-2 .. 1e-8), where
    converged training runs."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F = 5
ARITH_BAR = 1e-5
REPR_BAR = 3e-3
NAMES = ("dkeys1", "dkeys2", "dv1", "db1", "dU", "dv2")


def encode_saf(x, U1):
    """fp16 words of the saved factors for energy arguments x (float64), as the folded forward kernel stores them
    (csrc/attn_common.h, saf_encode): q = +m where tanh x >= 0, -m otherwise, m = min(r, 1 - r), r = 1 / (1 + e^(2x)),
    in fp16: units [0, U1) (source 1) rounded toward zero - the packed conversion of the store -, the others to nearest.  m carries
    relative precision where tanh saturates; tanh = sign(q) (1 - 2 m), r (1 - r) = m (1 - m)."""
    m = 1.0 / (1.0 + np.exp(2.0 * np.abs(x)))
    q = np.where(x >= 0, m, -m)
    h = q.astype(np.float16)
    rtz = np.where(np.abs(h.astype(np.float64)) > np.abs(q), np.nextafter(h, np.float16(0)), h)
    return np.concatenate([rtz[..., :U1], h[..., U1:]], axis=-1)


def decode_saf(q):
    """(tanh, 1 - tanh^2) in float64 from the fp16 words"""
    q = q.astype(np.float64)
    m = np.abs(q)
    return np.copysign(1.0 - 2.0 * m, q), 4.0 * m * (1.0 - m)


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def make_problem(B, Td, Ti, U1, U2, lengths, regime, seed):
    """inputs whose energy arguments sit in `regime`: 'diffuse' (|x| <~ 1), 'saturated' (|x| 3 .. 10 per (row, unit), random sign,
    +- 0.2 of step-to-step variation) or 'mixed' (each (row, unit) pair one or the other)"""
    g = np.random.default_rng(seed)
    UQ = U1 + U2

    def base(shape):
        if regime == "diffuse":
            return g.normal(0, 0.4, shape)
        sat = g.uniform(3.0, 10.0, shape) * g.choice([-1.0, 1.0], shape)
        return sat if regime == "saturated" else np.where(g.random(shape) < 0.5, sat, g.normal(0, 0.4, shape))
    step = 1.0 if regime == "diffuse" else 0.25          # scale of the step-dependent terms
    b1 = g.normal(0, 0.1, U1).astype(np.float32)
    x01 = base((B, Ti, U1))
    keys1 = _bf16(x01 - b1)                                # bf16-representable: keys_lds_bf16 changes nothing
    keys2 = _bf16(base((B, Ti, U2)))
    pq = (g.normal(0, 0.2, (B, Td, UQ)) * step).astype(np.float32)
    fl = (g.normal(0, 0.5, (B, Td, Ti, F)) * step).astype(np.float32)
    locU = g.normal(0, 0.1, (F, U1)).astype(np.float32)
    v1 = g.normal(0, 1, U1).astype(np.float32)
    v2 = g.normal(0, 1, U2).astype(np.float32)
    de1 = (g.normal(0, 0.1, (B, Td, Ti))).astype(np.float32)
    de2 = (g.normal(0, 0.1, (B, Td, Ti))).astype(np.float32)
    D = lambda a: a.astype(np.float64)
    x1 = D(keys1)[:, None] + D(b1) + D(pq)[:, :, None, :U1] + np.einsum("btik,ku->btiu", D(fl), D(locU))
    x2 = D(keys2)[:, None] + D(pq)[:, :, None, U1:]
    return dict(B=B, Td=Td, Ti=Ti, U1=U1, U2=U2, lengths=np.asarray(lengths, dtype=np.int64), b1=b1, keys1=keys1, keys2=keys2,
                pq=pq, fl=fl, locU=locU, v1=v1, v2=v2, de1=de1, de2=de2, x1=x1, x2=x2)


def reference(P, th1, dth1, th2, dth2):
    """float64 sums from (tanh, 1 - tanh^2) of both mechanisms; rows at or beyond the source length contribute nothing and
    their d keys are zero"""
    Ti = P["Ti"]
    m = (np.arange(Ti)[None, :] < P["lengths"][:, None]).astype(np.float64)
    d1 = P["de1"].astype(np.float64) * m[:, None, :]
    d2 = P["de2"].astype(np.float64) * m[:, None, :]
    g1 = d1[..., None] * P["v1"].astype(np.float64) * dth1
    g2 = d2[..., None] * P["v2"].astype(np.float64) * dth2
    return dict(dkeys1=g1.sum(1), dkeys2=g2.sum(1), dv1=(d1[..., None] * th1).sum((0, 1, 2)), db1=g1.sum((0, 1, 2)),
                dU=np.einsum("btik,btiu->ku", P["fl"].astype(np.float64), g1), dv2=(d2[..., None] * th2).sum((0, 1, 2)))


def exact(P):
    c1, c2 = np.cosh(P["x1"]), np.cosh(P["x2"])
    return reference(P, np.tanh(P["x1"]), 1.0 / (c1 * c1), np.tanh(P["x2"]), 1.0 / (c2 * c2))


def saturated_fraction(P):
    """fraction of (live row, step, unit) energies with 1 - tanh^2 < 1e-3"""
    live = np.arange(P["Ti"])[None, :] < P["lengths"][:, None]
    c = np.cosh(np.concatenate([P["x1"], P["x2"]], axis=-1).transpose(0, 2, 1, 3)[live])
    return float(np.mean(1.0 / (c * c) < 1e-3))


def assert_regime(P, regime):
    fr = saturated_fraction(P)
    print("%s: fraction of energies with 1 - tanh^2 < 1e-3: %.3f" % (regime, fr))
    if regime == "diffuse":
        assert fr < 0.01 and np.abs(P["x1"]).mean() < 1.0, fr
    elif regime == "saturated":
        assert fr > 0.7, fr
    else:
        assert 0.25 < fr < 0.6, fr


class Run:
    """device tensors + satt_attn_rnn_params of one problem; saf: fp16 words [B,Td,Ti,UQ] or None"""

    def __init__(self, P, saf):
        from satt_amd import ops
        self.ops, self.P = ops, P
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.t = {k: T(P[k]) for k in ("keys1", "keys2", "pq", "fl", "locU", "v1", "v2", "b1", "de1", "de2", "lengths")}
        self.saf = None if saf is None else T(saf)
        single = P["U2"] == 0
        t = self.t
        self.ap = ops.attn_rnn_params(
            B=P["B"], Td=P["Td"], Ti=P["Ti"], A=256, U1=P["U1"], V1=256, U2=P["U2"], V2=0 if single else 32, kernel=10, filters=F,
            training=1, keys_lds_bf16=1, lengths=t["lengths"], keys1=t["keys1"], keys2=None if single else t["keys2"],
            v1=t["v1"], v2=None if single else t["v2"], b1=t["b1"], locU=t["locU"], pq=t["pq"], fl=t["fl"], saf=self.saf)
        self.single = single

    def outputs(self):
        P = self.P
        z = lambda *s: torch.zeros(*s, device="cuda")
        nan = lambda *s: torch.full(s, float("nan"), device="cuda")      # rows beyond the length must be written (zeros)
        o = dict(dkeys1=nan(P["B"], P["Ti"], P["U1"]), dkeys2=None if self.single else nan(P["B"], P["Ti"], P["U2"]),
                 dv1=z(P["U1"]), db1=z(P["U1"]), dU=z(F, P["U1"]), dv2=None if self.single else z(P["U2"]))
        return o

    def de2(self):
        return None if self.single else self.t["de2"]

    def full(self):
        """satt_attn_param_grads: all steps in one call"""
        o = self.outputs()
        lib = self.ops._lib.lib()
        rc = lib.satt_attn_param_grads(C.byref(self.ap), self.t["de1"].data_ptr(), self.ops._p(self.de2()),
                                       *[self.ops._p(o[k]) for k in NAMES], self.ops._s())
        assert rc == 0, rc
        return o

    def ranged(self, t0, pad):
        """satt_attn_param_grads_range over [0, t0) then [t0, Td) with accumulate"""
        o = self.outputs()
        for a, b, acc in ((0, t0, False), (t0, self.P["Td"], True)):
            self.ops.attn_param_grads(self.ap, self.t["de1"], self.de2(), *[o[k] for k in NAMES], a, b, accumulate=acc, lds_pad=pad)
        return o

    def acc(self, t0, pad):
        """satt_attn_param_grads_acc over [0, t0) then [t0, Td) + satt_attn_param_grads_finish"""
        o = self.outputs()
        buf = self.ops.attn_param_grads_acc_buffer(self.ap, "cuda")
        buf.fill_(float("nan"))                                    # the first call overwrites its slots
        for a, b, ac in ((0, t0, False), (t0, self.P["Td"], True)):
            self.ops.attn_param_grads_acc(self.ap, self.t["de1"], self.de2(), o["dkeys1"], o["dkeys2"], buf, a, b, accumulate=ac,
                                          lds_pad=pad)
        self.ops.attn_param_grads_finish(self.ap, buf, o["dv1"], o["db1"], o["dU"], o["dv2"])
        return o


def host(o):
    torch.cuda.synchronize()
    return {k: v.double().cpu().numpy() for k, v in o.items() if v is not None}


def max_rel(a, r):
    return float(np.abs(a - r).max() / (np.abs(r).max() + 1e-30))


def l2_rel(a, r):
    return float(np.linalg.norm(a - r) / (np.linalg.norm(r) + 1e-30))


def judge(label, got, arith, ex, arith_bar=ARITH_BAR):
    """both bars for every tensor of `got`; arith None: no fp16 factors (recomputing kernel), its arithmetic is judged against
    the exact reference"""
    bad = []
    for k, a in got.items():
        assert np.isfinite(a).all(), (label, k)
        ea = max_rel(a, (arith if arith is not None else ex)[k])
        er = l2_rel(a, ex[k])
        print("%-28s %-7s arithmetic max-rel %.2e   vs exact float64: L2-rel %.2e" % (label, k, ea, er))
        if not (ea < arith_bar):
            bad.append((k, "arithmetic", ea))
        if not (er < REPR_BAR):
            bad.append((k, "representation", er))
    assert not bad, (label, bad)


SHAPES = {          # B, Td, Ti, U1, U2, source lengths
    "Ti160": (4, 20, 160, 224, 32, [160, 1, 131, 97]),
    "Ti97": (3, 17, 97, 224, 32, [97, 1, 50]),
    "single": (3, 16, 160, 256, 0, [160, 1, 77]),           # baseline model: one source, U2 = 0 (single_source_fixup)
}
REGIMES = ("diffuse", "saturated", "mixed")


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_saved_factor_param_grads(shape, regime):
    """attn_param_grads_saf_k (U1 + U2 = 256 and saved factors): every entry point, step ranges with accumulate, LDS pad 0 and
    96 KB, the float64-slot path bit-identical across two runs"""
    import satt_amd  # noqa: F401
    B, Td, Ti, U1, U2, lengths = SHAPES[shape]
    P = make_problem(B, Td, Ti, U1, U2, lengths, regime, seed=11 + 7 * REGIMES.index(regime) + 101 * sorted(SHAPES).index(shape))
    assert_regime(P, regime)
    q = encode_saf(np.concatenate([P["x1"], P["x2"]], axis=-1), U1)
    th, dth = decode_saf(q)
    arith = reference(P, th[..., :U1], dth[..., :U1], th[..., U1:], dth[..., U1:])
    ex = exact(P)
    if U2 == 0:
        for d in (arith, ex):
            del d["dkeys2"], d["dv2"]
    r = Run(P, q)
    t0 = Td // 3
    judge("%s/%s full" % (shape, regime), host(r.full()), arith, ex)
    for pad in (0, 96 * 1024):
        judge("%s/%s range pad %d" % (shape, regime, pad), host(r.ranged(t0, pad)), arith, ex)
        a = host(r.acc(t0, pad))
        judge("%s/%s acc pad %d" % (shape, regime, pad), a, arith, ex)
        b = host(r.acc(t0, pad))
        diff = [k for k in a if not np.array_equal(a[k], b[k])]
        assert not diff, ("float64-slot path not bit-repeatable", diff)


GENERIC = {         # B, Td, Ti, U1, U2, lengths, pass saved factors (a shape the saved-factor kernel refuses: it must not read them)
    "Ti160": (4, 20, 160, 224, 32, [160, 1, 131, 97], False),
    "refused_Ti97": (3, 17, 97, 128, 32, [97, 1, 50], True),
    "single": (3, 16, 160, 256, 0, [160, 1, 77], False),
}


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", sorted(GENERIC))
def test_recomputing_param_grads(shape, regime):
    """attn_param_grads_k: saf = NULL, or a shape the saved-factor kernel refuses (U1 + U2 != 256; saved factors present but
    poisoned with NaN: never read).  It recomputes tanh in fp32: both bars against the exact float64 sums (max-norm 1e-4)."""
    import satt_amd  # noqa: F401
    from satt_amd._lib import SattError
    B, Td, Ti, U1, U2, lengths, with_saf = GENERIC[shape]
    P = make_problem(B, Td, Ti, U1, U2, lengths, regime, seed=5 + 7 * REGIMES.index(regime) + 101 * sorted(GENERIC).index(shape))
    assert_regime(P, regime)
    ex = exact(P)
    if U2 == 0:
        del ex["dkeys2"], ex["dv2"]
    r = Run(P, np.full((B, Td, Ti, U1 + U2), np.nan, dtype=np.float16) if with_saf else None)
    t0 = Td // 3
    judge("%s/%s full" % (shape, regime), host(r.full()), None, ex, arith_bar=1e-4)
    for pad in (0, 96 * 1024):
        judge("%s/%s range pad %d" % (shape, regime, pad), host(r.ranged(t0, pad)), None, ex, arith_bar=1e-4)
    if with_saf:
        with pytest.raises(SattError, match=r"unsupported size.*\(-2\)"):      # the float64-slot entry point: saved-factor kernel only
            r.acc(t0, 0)
