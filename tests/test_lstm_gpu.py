"""The recurrent ZoneoutLSTM kernels of csrc/lstm.hip and csrc/lstm_cluster.hip, each launched directly (ops.lstm_fwd / lstm_bwd,
ops.lstm_cluster_fwd / _bwd / _fwd_x, ops.lstm_cluster_pack / _pack_in) and compared with the float64 loop of tests/lstm_common.py
(checked on its own by tests/test_lstm_cpu.py, which also says what the bars resolve).  Per case: hout, gates, cnew, cstate, hstate
and dxg, per tensor and direction, zeros beyond the length included.  Every output is NaN before the launch; pad columns of widened
buffers hold a finite sentinel and must keep it.  Every backward runs twice: on the kernel's own saved tensors (as the engine does)
and on the reference's saved tensors cast to fp32 (the backward judged alone).

Bars (tests/test_ops_gpu.py): 1e-5 on everything the forward writes, 5e-5 on dxg.

Kernel and branch pinned by each case group (tables in tests/lstm_common.py):
  lstm_fwd_mfma_k /      H = 8, 24, 40, 104, 128 (fewer units than one wave tile, ragged tiles, the limit MH), both directions:
  lstm_bwd_mfma_k        lengths (9, 1, 2, 3, 4, 5) at T = 9: every len % 4 of the loop unrolled by LPD = 4 - the masked tail steps, the
                         late store of the previous step (pv_on / pv_t) and the final store behind the loop - len = 1 and len = T;
                         (13, 8, 7, 6) at T = 13: several groups of four in either walk; (5, 0, 3): len = 0 behind lenc = max(len, 1),
                         all zeros written; without lengths T = 1, 3, 4, 5: below, at and above one group.
  lstm_fwd_k /           H = 136 (the first H of the streaming form: KS = 15 forward, 60 backward), 256, and 1024 (the launchers'
  lstm_bwd_k             limit: KS = 2 forward, KS = 8 backward, 52 KB of dynamic LDS); lengths (5, 1, 3), T = 1.
  zoneout branches       H = 24, 128, 136: training with rates (0, 0) and (0, 0.5) - the zct == 0 / zht == 0 short-cuts - and eval mode
                         with lengths (the streaming form's eval branch had never run with lengths).
  saturated gates        xg ~ N(0, 6) at H = 128 and 136: finite, same bars.
  leading dimensions     hout / dhout rows of ndir * H + 8 at H = 40 and 136.
  forward only           H = 12 (register-resident form) and 132 (streaming form, KS = 15, rows of 528 columns): accepted by the forward
                         launcher, declined by the backward launcher (H % 8).
  declines               H = 1032, H = 12 (backward), ndir = 3, B = 0: no launch, the code checked.
  lstm_cluster_fwd_k /   (H, C) = (16, 2), (48, 2), (128, 2), (64, 8), (192, 4), (256, 4), (256, 8): HU = 8 .. 64 (the limit), HU = 24
  lstm_cluster_bwd_k     and 48 (a wave's 32-column tile straddles gates), NL = 32 .. 256; B = 1 and 8 (B % 8 == 0 lets the members of a
                         sample share an XCD: plain-store exchange; B = 1, 3: agent scope - which one ran is printed, not asserted);
                         T = 1 (t == 0 exit of the backward, no exchange at all), T = 2 (t + 1 < t1 exit); the four zoneout modes;
                         hout / dhout rows of H + 8.
  chunked passes         (256, 4), T = 23 as [0,1) [1,2) [2,18) [18,23) on one workspace whose granules hold 0x5A: the restart from
                         cstate / hstate of step t0 - 1, bstate, the per-launch handshake tags; bit-equal to the full range in training
                         and eval mode, and within the bars of float64.
  lstm_cluster_pack_k    row stride 4H + 8.
  fused projection       lstm_cluster_pack_in_k + the prologue of lstm_cluster_fwd_k: Kin = 4, 36, 100 (K tail: min(k, Kin - 4) with
                         zeroing), 256, 544 (KT = 17: three batches of KB = 6 tiles, the last one clamped); passes of 1, 16 and 16 + 4
                         steps; bias and NULL bias; ldx = Kin and Kin + 12; a launch of the last chunk only.

Largest measured error per family (MI355X) next to its bar:
  register-resident form   forward tensors 3.6e-7 (1e-5), dxg 3.9e-7 (5e-5)
  streaming form           forward tensors 3.4e-7 (1e-5), dxg 5.4e-7 (5e-5)
  cluster form             forward tensors 3.7e-7 (1e-5), dxg 2.9e-7 (5e-5)
  fused projection         xg against float64 3.5e-7 (1e-3); bit-identical to ops.linear at every Kin, on the large-tile GEMM
                           (Kin = 256, 544) and on the generic one (Kin = 4, 36, 100: K % 8 != 0 keeps them off the tile kernel)
That is the floor of fp32 arithmetic (3e-7 with the same loop in numpy fp32, tests/test_lstm_cpu.py).  No case showed a defect."""
import pytest
import torch

import satt_amd  # noqa: F401
import lstm_common as lc
from test_gemm_tile_gpu import TOL, make_weight, paths

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
SENTINEL = 1234.5
E_BADARG, E_UNSUPPORTED = -1, -2


def dev(a, dtype=torch.float32):
    return torch.tensor(a, dtype=dtype).to(DEV).contiguous()


def nans(*shape):
    return torch.full(shape, NAN, device=DEV)


def widened(rows, width, pad, fill=NAN):
    """(buffer [rows, width + pad], its [rows, width] view): NaN (or `fill`) in the view, the sentinel in the pad columns"""
    full = torch.full((rows, width + pad), fill, device=DEV)
    full[:, width:] = SENTINEL
    return full, full[:, :width]


def pad_untouched(full, width):
    return bool((full[:, width:] == SENTINEL).all())


def code_of(err):
    return int(str(err.value).rsplit("(", 1)[1].rstrip(")"))


def raises_code(fn, code):
    from satt_amd import _lib
    with pytest.raises(_lib.SattError) as err:
        fn()
    assert code_of(err) == code, str(err.value)


def check_forward(case, ref, got, what):
    """got: name -> device tensor in the kernels' layouts"""
    worst = 0.0
    for n in lc.FWD_NAMES:
        worst = max(worst, lc.close(n, got[n], ref[n], lc.BAR_FWD, case.ndir, what))
    # exactly zero beyond the length, every tensor and direction
    B, T = case.B, case.T
    hout = got["hout"].view(B, T, -1)
    for b, L in enumerate(lc.inputs(case).lengths.tolist()):
        if L < T:
            assert float(hout[b, L:].abs().max()) == 0.0, (what, "hout", b)
            for n in lc.SAVED:
                assert float(got[n].view(case.ndir, B, T, -1)[:, b, L:].abs().max()) == 0.0, (what, n, b)
    return worst


def check_dxg(case, ref, dxg, what):
    worst = lc.close("dxg", dxg, ref["dxg"], lc.BAR_DXG, case.ndir, what)
    for b, L in enumerate(lc.inputs(case).lengths.tolist()):
        if L < case.T:
            assert float(dxg.view(case.ndir, case.B, case.T, -1)[:, b, L:].abs().max()) == 0.0, (what, "dxg", b)
    return worst


def ref_saved(ref, case):
    """the reference's saved tensors as the kernels lay them out, fp32"""
    return {n: ref[n].to(torch.float32).reshape(case.ndir, case.B * case.T, -1).to(DEV).contiguous() for n in lc.SAVED}


# ------------------------------------------------------------------------------------------------ single-workgroup kernels
def single_forward(case):
    from satt_amd import ops
    inp = lc.inputs(case)
    ndir, B, T, H = case.ndir, case.B, case.T, case.H
    training, zc, zh = case.mode
    sc, sh = lc.streams(case)
    Wh = dev(inp.Wh).to(torch.bfloat16).contiguous()
    assert torch.equal(Wh.float().cpu(), torch.tensor(inp.Wh))              # bf16-representable: the cast is exact
    lens = None if case.lengths is None else dev(inp.lengths, torch.int64)
    seed = torch.tensor([case.seed], dtype=torch.int32, device=DEV)
    full, hout = widened(B * T, ndir * H, case.pad)
    got = {"hout": hout, "gates": nans(ndir, B * T, 4 * H), "cnew": nans(ndir, B * T, H), "cstate": nans(ndir, B * T, H),
           "hstate": nans(ndir, B * T, H)}
    ops.lstm_fwd(dev(inp.xg), Wh, lens, ndir, B, T, H, training, zc, zh, seed, sc, sh, hout, got["gates"], got["cnew"], got["cstate"],
                 got["hstate"])
    torch.cuda.synchronize()
    assert pad_untouched(full, ndir * H)
    return got, (lens, seed)


def single_backward(case, saved, lens, seed):
    from satt_amd import ops
    inp = lc.inputs(case)
    ndir, B, T, H = case.ndir, case.B, case.T, case.H
    training, zc, zh = case.mode
    sc, sh = lc.streams(case)
    WhT = dev(inp.Wh).transpose(1, 2).contiguous().to(torch.bfloat16)
    dfull, dh = widened(B * T, ndir * H, case.pad, 0.0)
    dh.copy_(dev(inp.dh).view(B * T, ndir * H))
    dxg = nans(ndir, B * T, 4 * H)
    ops.lstm_bwd(dh, WhT, lens, ndir, B, T, H, training, zc, zh, seed, sc, sh, saved["gates"], saved["cnew"], saved["cstate"], dxg)
    torch.cuda.synchronize()
    assert pad_untouched(dfull, ndir * H)
    return dxg


@pytest.mark.parametrize("case", lc.SINGLE, ids=lc.case_id)
def test_lstm_single(case):
    ref = lc.reference(case)
    got, (lens, seed) = single_forward(case)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    check_forward(case, ref, got, "single")
    check_dxg(case, ref, single_backward(case, got, lens, seed), "single own saved")
    check_dxg(case, ref, single_backward(case, ref_saved(ref, case), lens, seed), "single ref saved")


@pytest.mark.parametrize("case", lc.SINGLE_FWD_ONLY, ids=lc.case_id)
def test_lstm_single_forward_only_widths(case):
    """H % 8 != 0: the forward launcher takes every even H, the backward launcher declines"""
    from satt_amd import ops
    ref = lc.reference(case)
    got, (lens, seed) = single_forward(case)
    check_forward(case, ref, got, "single fwd-only")
    ndir, B, T, H = case.ndir, case.B, case.T, case.H
    sc, sh = lc.streams(case)
    WhT = torch.zeros(ndir, 4 * H, H, dtype=torch.bfloat16, device=DEV)
    dxg = nans(ndir, B * T, 4 * H)
    raises_code(lambda: ops.lstm_bwd(torch.zeros(B * T, ndir * H, device=DEV), WhT, lens, ndir, B, T, H, False, 0.1, 0.15, seed, sc, sh,
                                     got["gates"], got["cnew"], got["cstate"], dxg), E_UNSUPPORTED)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dxg).all())


def test_lstm_single_declines():
    """no launch: every buffer is sized for the shape asked for and still NaN afterwards"""
    from satt_amd import ops
    seed = torch.tensor([1], dtype=torch.int32, device=DEV)

    def both(ndir, B, T, H, code_f, code_b, Bbuf=None):
        Bb = B if Bbuf is None else Bbuf
        nd = max(ndir, 1)
        sc, sh = tuple(range(3, 3 + nd)), tuple(range(13, 13 + nd))
        Wh = torch.zeros(nd, H, 4 * H, dtype=torch.bfloat16, device=DEV)
        xg = torch.zeros(nd, Bb * T, 4 * H, device=DEV)
        hout = nans(Bb * T, nd * H)
        sv = [nans(nd, Bb * T, 4 * H), nans(nd, Bb * T, H), nans(nd, Bb * T, H), nans(nd, Bb * T, H)]
        if code_f is not None:
            raises_code(lambda: ops.lstm_fwd(xg, Wh, None, ndir, B, T, H, True, 0.1, 0.15, seed, sc, sh, hout, *sv), code_f)
        dxg = nans(nd, Bb * T, 4 * H)
        raises_code(lambda: ops.lstm_bwd(torch.zeros(Bb * T, nd * H, device=DEV), Wh.view(nd, 4 * H, H), None, ndir, B, T, H, True, 0.1,
                                         0.15, seed, sc, sh, torch.zeros_like(sv[0]), torch.zeros_like(sv[1]), torch.zeros_like(sv[2]),
                                         dxg), code_b)
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in [hout, dxg] + sv)

    both(1, 1, 1, 1032, E_UNSUPPORTED, E_UNSUPPORTED)
    both(1, 2, 3, 12, None, E_UNSUPPORTED)
    both(3, 2, 3, 16, E_BADARG, E_BADARG)
    both(1, 0, 3, 16, E_BADARG, E_BADARG, Bbuf=1)


# ------------------------------------------------------------------------------------------------ cluster kernels
def cluster_ready(B, T, H, C):
    """the launchers' own conditions, asserted before every launch: accepted shape, every member resident"""
    from satt_amd import _lib, ops
    assert _lib.lib().satt_lstm_cluster_check(B, T, H, C) == 0
    for bw in (False, True):
        n, per_cu, cus = ops.lstm_cluster_residency(B, T, H, C, bw)
        assert n == B * C and n <= per_cu * cus, (n, per_cu, cus)


class ClusterRun:
    """one workspace and the launches made on it"""

    def __init__(self, case, garbage=False):
        from satt_amd import ops
        self.case = case
        self.ws = ops.lstm_cluster_ws(case.B, case.H, case.C, DEV)
        if garbage:
            self.ws[:-64] = 0x5A         # the first launch of a pass zeroes the granules; the 64-byte status tail is the owner's
        self.launches = 0
        inp = lc.inputs(case)
        self.xg = dev(inp.xg)
        self.pf, self.pb = ops.lstm_cluster_pack(dev(inp.Wh[0]), case.H, case.C)
        self.seed = torch.tensor([case.seed], dtype=torch.int32, device=DEV)

    def before(self):
        c = self.case
        cluster_ready(c.B, c.T, c.H, c.C)
        self.launches += 1

    def after(self, what):
        from satt_amd import ops
        c = self.case
        ops.lstm_cluster_status(self.ws, c.B, c.H, c.C)
        count, slow = ops.lstm_cluster_fastpath(self.ws, c.B, c.H, c.C)
        print("%-40s same-XCD workgroup-launches %d, others %d (B * C * launches = %d)" % (what, count, slow, c.B * c.C * self.launches))
        assert count + slow == c.B * c.C * self.launches

    def forward(self, chunks=None, xg=None):
        from satt_amd import ops
        c = self.case
        B, T, H = c.B, c.T, c.H
        training, zc, zh = c.mode
        (sc,), (sh,) = lc.streams(c)
        full, hout = widened(B * T, H, c.pad)
        got = {"hout": hout, "gates": nans(1, B * T, 4 * H), "cnew": nans(1, B * T, H), "cstate": nans(1, B * T, H), "hstate": nans(1, B * T, H)}
        for t0, t1 in chunks or ((0, T),):
            self.before()
            ops.lstm_cluster_fwd(self.xg if xg is None else xg, self.pf, B, T, H, c.C, training, zc, zh, self.seed, sc, sh, hout,
                                 got["gates"], got["cnew"], got["cstate"], got["hstate"], self.ws, t0, t1)
            self.after("fwd [%d, %d)" % (t0, t1))
        assert pad_untouched(full, H)
        return got

    def backward(self, saved, chunks=None):
        from satt_amd import ops
        c = self.case
        B, T, H = c.B, c.T, c.H
        training, zc, zh = c.mode
        (sc,), (sh,) = lc.streams(c)
        dfull, dh = widened(B * T, H, c.pad, 0.0)
        dh.copy_(dev(lc.inputs(c).dh).view(B * T, H))
        dxg, bstate = nans(1, B * T, 4 * H), nans(B, 2, H)
        for t0, t1 in reversed(chunks or ((0, T),)):
            self.before()
            ops.lstm_cluster_bwd(dh, self.pb, B, T, H, c.C, training, zc, zh, self.seed, sc, sh, saved["gates"], saved["cnew"],
                                 saved["cstate"], dxg, self.ws, t0, t1, bstate if chunks else None)
            self.after("bwd [%d, %d)" % (t0, t1))
        assert pad_untouched(dfull, H)
        return dxg


@pytest.mark.parametrize("case", lc.CLUSTER, ids=lc.case_id)
def test_lstm_cluster(case):
    ref = lc.reference(case)
    run = ClusterRun(case)
    got = run.forward()
    check_forward(case, ref, got, "cluster")
    check_dxg(case, ref, run.backward(got), "cluster own saved")
    check_dxg(case, ref, run.backward(ref_saved(ref, case)), "cluster ref saved")


@pytest.mark.parametrize("case", lc.CLUSTER_CHUNKED, ids=lc.case_id)
def test_lstm_cluster_chunked(case):
    """chunk launches on one workspace with garbage granules == the full-range launch bit for bit, and within the bars of float64"""
    ref = lc.reference(case)
    full = ClusterRun(case)
    got_f = full.forward()
    dxg_f = full.backward(got_f)
    chk = ClusterRun(case, garbage=True)
    got_c = chk.forward(lc.CHUNKS)
    dxg_c = chk.backward(got_c, lc.CHUNKS)
    for n in lc.FWD_NAMES:
        assert torch.equal(got_f[n], got_c[n]), n
    assert torch.equal(dxg_f, dxg_c)
    check_forward(case, ref, got_c, "cluster chunked")
    check_dxg(case, ref, dxg_c, "cluster chunked own saved")
    check_dxg(case, ref, chk.backward(ref_saved(ref, case), lc.CHUNKS), "cluster chunked ref saved")


@pytest.mark.parametrize("H,C", lc.PACK_STRIDE)
def test_lstm_cluster_pack_row_stride(H, C):
    from satt_amd import ops
    g = torch.Generator().manual_seed(H + C)
    wide = torch.full((H, 4 * H + 8), SENTINEL)
    wide[:, :4 * H] = torch.randn(H, 4 * H, generator=g) / H ** 0.5
    wide = wide.to(DEV)
    view = wide[:, :4 * H]
    assert view.stride(0) == 4 * H + 8
    pf, pb = ops.lstm_cluster_pack(view, H, C)
    qf, qb = ops.lstm_cluster_pack(view.contiguous(), H, C)
    torch.cuda.synchronize()
    assert torch.equal(pf.view(torch.int16), qf.view(torch.int16)) and torch.equal(pb.view(torch.int16), qb.view(torch.int16))
    assert float(pf.float().abs().max()) < 10.0 and float(pb.float().abs().max()) < 10.0        # no sentinel column went in
    assert float(pf.float().abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------ fused input projection
def fused_inputs(c):
    g = torch.Generator().manual_seed(c.seed)
    M, G = c.B * c.T, 4 * c.H
    x = torch.randn(M, c.Kin, generator=g)
    Win = torch.randn(c.Kin, G, generator=g) / c.Kin ** 0.5
    bias = torch.randn(G, generator=g) if c.bias else None
    Wh = torch.tensor(lc.bf16_round((torch.randn(c.H, G, generator=g) / c.H ** 0.5).numpy()))
    return x, Win, bias, Wh


@pytest.mark.parametrize("c", lc.FUSED, ids=lc.fused_id)
def test_lstm_cluster_fused_projection(c):
    from satt_amd import ops
    ops.set_precision("bf16")
    B, T, H, C, Kin = c.B, c.T, c.H, c.C, c.Kin
    M, G = B * T, 4 * H
    x, Win, bias, Wh = fused_inputs(c)
    xfull = torch.full((M, Kin + c.xpad), SENTINEL)
    xfull[:, :Kin] = x
    xfull = xfull.to(DEV)
    xd = xfull[:, :Kin]
    assert xd.stride(0) == Kin + c.xpad and xd.data_ptr() % 16 == 0
    Wind, bd = Win.to(DEV), None if bias is None else bias.to(DEV)
    pin = ops.lstm_cluster_pack_in(Wind, H, C)
    pf, _ = ops.lstm_cluster_pack(Wh.to(DEV), H, C)
    seed = torch.tensor([c.seed], dtype=torch.int32, device=DEV)
    training, zc, zh = lc.Z_TRAIN
    sc, sh = 12, 13
    cluster_ready(B, T, H, C)

    def outs():
        return {"hout": nans(M, H), "gates": nans(1, M, G), "cnew": nans(1, M, H), "cstate": nans(1, M, H), "hstate": nans(1, M, H)}

    def launch(o, ws, xg, t0, t1, fused):
        if fused:
            ops.lstm_cluster_fwd_x(xd, Kin, pin, bd, xg, pf, B, T, H, C, training, zc, zh, seed, sc, sh, o["hout"], o["gates"], o["cnew"],
                                   o["cstate"], o["hstate"], ws, t0, t1)
        else:
            ops.lstm_cluster_fwd(xg, pf, B, T, H, C, training, zc, zh, seed, sc, sh, o["hout"], o["gates"], o["cnew"], o["cstate"],
                                 o["hstate"], ws, t0, t1)

    def finish(ws, launches, what):
        ops.lstm_cluster_status(ws, B, H, C)
        count, slow = ops.lstm_cluster_fastpath(ws, B, H, C)
        print("%-40s same-XCD workgroup-launches %d, others %d" % (what, count, slow))
        assert count + slow == B * C * launches

    # 1. every chunk fused
    xg, o1, ws1 = nans(1, M, G), outs(), ops.lstm_cluster_ws(B, H, C, DEV)
    for t0, t1 in lc.FUSED_CHUNKS:
        launch(o1, ws1, xg, t0, t1, True)
    finish(ws1, len(lc.FUSED_CHUNKS), "fused")
    assert bool(torch.isfinite(xg).all())                                    # completely written
    assert bool((xfull[:, Kin:] == SENTINEL).all())
    want = x.bfloat16().double() @ Win.bfloat16().double() + (0.0 if bias is None else bias.double())
    e = lc.close("xg", xg.view(M, G), want, TOL, 1, "fused projection vs float64")
    # 2. the separate product
    xg_ref = nans(M, G)
    with paths() as log:
        ops.linear(xd, make_weight(Wind), bd, xg_ref)
    lc.close("xg", xg_ref, want, TOL, 1, "ops.linear vs float64")
    same = torch.equal(xg.view(M, G).view(torch.int32), xg_ref.view(torch.int32))
    diff = float((xg.view(M, G) - xg_ref).abs().max())
    print("%-40s gemm path %s, bit-identical %s, max |diff| %.3e, err vs float64 %.3e" % (lc.fused_id(c), log, same, diff, e))
    assert log == [1 if Kin % 8 == 0 else 0], log      # the large-tile kernel where it applies (K % 8 == 0), the generic one otherwise
    assert same, (log, diff)
    # 3. the recurrence on that xg, unfused, same chunks
    o2, ws2 = outs(), ops.lstm_cluster_ws(B, H, C, DEV)
    for t0, t1 in lc.FUSED_CHUNKS:
        launch(o2, ws2, xg_ref.view(1, M, G), t0, t1, False)
    finish(ws2, len(lc.FUSED_CHUNKS), "unfused")
    for n in lc.FWD_NAMES:
        assert torch.equal(o1[n].view(torch.int32), o2[n].view(torch.int32)), n
    # 4. only the last chunk fused, behind unfused chunks on the same workspace: rows below 17 of xg stay as they are
    t_last = lc.FUSED_CHUNKS[-1][0]
    xg3 = nans(1, B, T, G)
    xg3[0, :, :t_last] = xg_ref.view(B, T, G)[:, :t_last]
    before = xg3.clone()
    o3, ws3 = outs(), ops.lstm_cluster_ws(B, H, C, DEV)
    for t0, t1 in lc.FUSED_CHUNKS:
        launch(o3, ws3, xg3.view(1, M, G), t0, t1, t0 == t_last)
    finish(ws3, len(lc.FUSED_CHUNKS), "last chunk fused")
    assert torch.equal(xg3[0, :, :t_last].contiguous().view(torch.int32), before[0, :, :t_last].contiguous().view(torch.int32))
    assert torch.equal(xg3.view(1, M, G).view(torch.int32), xg.view(torch.int32))
    for n in lc.FWD_NAMES:
        assert torch.equal(o1[n].view(torch.int32), o3[n].view(torch.int32)), n


def test_lstm_cluster_fused_projection_declines():
    """no launch: buffers sized for the shapes asked for, outputs still NaN"""
    from satt_amd import ops
    B, T, H, C = 3, 37, 64, 8
    M, G = B * T, 4 * H
    seed = torch.tensor([1], dtype=torch.int32, device=DEV)
    pf, _ = ops.lstm_cluster_pack(torch.zeros(H, G, device=DEV), H, C)
    ws = ops.lstm_cluster_ws(B, H, C, DEV)
    xg, hout = nans(1, M, G), nans(M, H)
    sv = [nans(1, M, G), nans(1, M, H), nans(1, M, H), nans(1, M, H)]
    good = ops.lstm_cluster_pack_in(torch.zeros(36, G, device=DEV), H, C)
    big = torch.zeros(2 * good.numel() * 20, dtype=torch.bfloat16, device=DEV)       # larger than the pack of any Kin tried below

    def fwd_x(x, Kin):
        return lambda: ops.lstm_cluster_fwd_x(x, Kin, big, None, xg, pf, B, T, H, C, True, 0.1, 0.15, seed, 12, 13, hout, *sv, ws, 0, T)

    for Kin in (548, 6):
        raises_code(lambda: ops.lstm_cluster_pack_in(torch.zeros(Kin, G, device=DEV), H, C), E_UNSUPPORTED)
        raises_code(fwd_x(torch.zeros(M, Kin + (-Kin) % 4, device=DEV)[:, :Kin], Kin), E_BADARG)
    raises_code(fwd_x(torch.zeros(M, 38, device=DEV)[:, :36], 36), E_BADARG)                   # ldx = Kin + 2
    flat = torch.zeros(M * 36 + 4, device=DEV)
    off = flat[1:1 + M * 36].view(M, 36)                                                          # four bytes off a 16-byte boundary
    assert off.data_ptr() % 16 == 4
    raises_code(fwd_x(off, 36), E_BADARG)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in [xg, hout] + sv)
    ops.lstm_cluster_status(ws, B, H, C)
