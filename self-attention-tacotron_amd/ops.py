"""Tensor-level wrappers over the C-ABI (include/satt_hip.h).  torch is used only for device memory and the
current HIP stream; every arithmetic op below runs in libsatt_hip.so.  No fallback paths."""
import ctypes as C
import math

import torch

from . import _lib
from ._lib import ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID, ACT_SOFTSIGN, PREC_BF16, PREC_F32, GemmParams

_state = {"prec": PREC_BF16}


def set_precision(name):
    """'bf16' (MFMA bf16 operands, fp32 accumulate — the benchmark dtype) or 'f32' (exact fp32 MFMA; parity mode)."""
    _state["prec"] = {"bf16": PREC_BF16, "f32": PREC_F32}[name]


def get_precision():
    return "bf16" if _state["prec"] == PREC_BF16 else "f32"


def _p(t):
    return None if t is None else t.data_ptr()


def bind_device(device):
    """the device whose current stream the launches go to (one process drives one GPU: Engine / DecodeSession call this once).
    torch.cuda.current_stream() without an index resolves the device through five Python layers incl. an os.getenv per call -
    at ~380 calls per train step that was a third of the host's enqueue time."""
    idx = torch.device(device).index
    _state["dev"] = torch.cuda.current_device() if idx is None else idx


def _dev_index():
    d = _state.get("dev")
    if d is None:
        d = _state["dev"] = torch.cuda.current_device()
    return d


def current_stream():
    """torch's current stream object on the bound device (cheap form of torch.cuda.current_stream())"""
    return torch.cuda.current_stream(_dev_index())


def _s():
    return torch._C._cuda_getCurrentRawStream(_dev_index())


class on_stream:
    """`with ops.on_stream(s):` - torch.cuda.stream(s) without resolving the device on every entry and exit (the engine switches
    streams ~70 times per step; torch's context manager spent ~8 us per switch in Python)"""
    __slots__ = ("s", "prev")

    def __init__(self, s):
        self.s = s

    def __enter__(self):
        self.prev = torch._C._cuda_getCurrentStream(_dev_index())       # (stream id, device index, device type)
        s = self.s
        torch._C._cuda_setStream(stream_id=s.stream_id, device_index=s.device_index, device_type=s.device_type)
        return s

    def __exit__(self, *exc):
        p = self.prev
        torch._C._cuda_setStream(stream_id=p[0], device_index=p[1], device_type=p[2])
        return False


def _ld(t):
    assert t.dim() == 2 and (t.stride(1) == 1 or t.shape[1] == 1), "need a row-major 2-D view"
    return t.stride(0)


def rate_thresh(rate):
    """(uint32 threshold, scale) for a dropout / zoneout rate; (0, 1) disables."""
    if rate <= 0.0:
        return 0, 1.0
    return min(int(rate * 4294967296.0), 0xFFFFFFFF), 1.0 / (1.0 - rate)


class Drop:
    """Dropout descriptor for the GEMM epilogue / softmax: rate, stream id, device seed tensor (uint32 as int32)."""

    def __init__(self, rate, stream, seed):
        self.thresh, self.scale = rate_thresh(rate)
        self.stream = stream
        self.seed = seed


class Weight:
    """GEMM weight operand: the fp32 master view `w` ([K, N] or [taps, Cin, Cout]) plus its bf16 shadows (satt_shadow_pack):
    `t` = per-tap transpose ([N, K] / [taps, Cout, Cin]) consumed by forward products, `n` = plain cast consumed by input
    gradients.  Every op below also accepts a bare fp32 tensor (no shadows: generic kernel)."""
    __slots__ = ("w", "t", "n")

    def __init__(self, w, t=None, n=None):
        self.w, self.t, self.n = w, t, n

    @property
    def shape(self):
        return self.w.shape

    def rows(self, r0, r1):
        """the weight of the input features [r0, r1) of a Dense layer: W[r0:r1, :]"""
        return Weight(self.w[r0:r1], None if self.t is None else self.t[:, r0:r1],
                      None if self.n is None else self.n[r0:r1])


def _wsplit(W):
    return (W.w, W.t, W.n) if isinstance(W, Weight) else (W, None, None)


def gemm(M, N, K, A, lda, B, sb_k, sb_n, Cm, ldc, *, a_mode=0, conv=None, kin=0, sb_tap=0, batch=(1, 1),
         sA=(0, 0), sB=(0, 0), sC=(0, 0), bias=None, act=ACT_NONE, alpha=1.0, accumulate=False, splitk=1,
         residual=None, ldr=0, drop=None, prec=None, bank=None, Bs=None, sbs_tap=0, sbs_n=0, colsum=None,
         split_overwrite=False, only_path=None):
    """split_overwrite: a split-K product that REPLACES C (not +=): with a slab workspace the kernels write C directly,
    otherwise C is zeroed here and the splits add atomically.  only_path: launch only if satt_gemm_path says so (returns
    False otherwise, nothing launched)."""
    p = GemmParams()
    p.M, p.N, p.K = M, N, K
    p.nb_outer, p.nb_inner = batch
    p.A, p.lda, p.strideA_o, p.strideA_i, p.a_mode = _p(A), lda, sA[0], sA[1], a_mode
    if conv is not None:
        p.conv_T, p.conv_C, p.conv_sgn, p.conv_off = conv
    p.B, p.sb_tap, p.sb_k, p.sb_n, p.strideB_o, p.strideB_i, p.kin = _p(B), sb_tap, sb_k, sb_n, sB[0], sB[1], kin
    p.C, p.ldc, p.strideC_o, p.strideC_i = _p(Cm), ldc, sC[0], sC[1]
    p.bias = _p(bias)
    p.residual, p.ldr = _p(residual), ldr
    p.act, p.alpha, p.accumulate, p.splitk = act, alpha, int(accumulate), splitk
    if drop is not None and drop.thresh:
        p.drop_thresh, p.drop_scale, p.drop_stream, p.seed = drop.thresh, drop.scale, drop.stream, _p(drop.seed)
    p.precision = _state["prec"] if prec is None else prec
    if bank is not None:
        p.bank_ng, p.bank_a_col, p.bank_c_col, p.bank_b_unit = bank
    if Bs is not None:
        p.Bs, p.sbs_tap, p.sbs_n = _p(Bs), sbs_tap, sbs_n
    p.colsum = _p(colsum)
    l = _lib.lib()
    if only_path is not None and l.satt_gemm_path(C.byref(p)) != only_path:
        return False
    # split reductions: a slab workspace (caller-owned: here, torch's caching allocator on the current stream) replaces
    # the fp32 atomics; the tensor must stay referenced until the launch has been issued
    ws = None
    nws = l.satt_gemm_ws_floats(C.byref(p))
    if nws > 0:
        ws = _slab_ws(nws, Cm.device)
        p.ws = ws.data_ptr()
    if split_overwrite and splitk > 1:
        if ws is None:
            Cm.zero_()
            p.accumulate = 1
        else:
            p.accumulate = 0
    if gemm_path_log is not None:
        gemm_path_log.append(l.satt_gemm_path(C.byref(p)))
    _lib.check(l.satt_gemm(C.byref(p), _s()), "satt_gemm")
    return True


gemm_path_log = None    # tests: set to [] to record the kernel family (satt_gemm_path) of every GEMM call


_ws_cache = {}


def _slab_ws(n, device):
    """slab workspace of the CURRENT stream (grow-only, one per stream): a split GEMM and its slab reduction run back to
    back on one stream, so launches of the same stream can share the buffer - and no allocator traffic (a first-time
    (stream, size) request of the caching allocator is a synchronising hipMalloc in the middle of a step)"""
    key = (str(device), _s())
    t = _ws_cache.get(key)
    if t is None or t.numel() < n:
        t = torch.empty(max(n, 1 << 22), dtype=torch.float32, device=device)
        _ws_cache[key] = t
    return t


def _splitk(tiles, k, target=320):
    """number of reduction splits: generic 64x64 kernel - enough workgroups to fill the chip; large tiles (benchmark
    precision) - about `target` workgroups of at least 16 K steps each"""
    if _state["prec"] != PREC_BF16:
        want = max(1, 512 // max(tiles, 1))
        return max(1, min(want, (k + 255) // 256, 64))
    want = max(1, -(-target // max(tiles, 1)))
    # at least 10 K steps of 32 rows per workgroup, at most 32 slices: the small weight-gradient products (1 - 12 output tiles) are
    # bound by the per-step load latency of their workgroups, not by the slab traffic (tools/probes/dw_splitk_sweep.py:
    # 128 x 256 x 5120 takes 23.6 us in 8 slices, 18.7 in 16; 256 x 256 x 12800 27.9 in 24, 27.4 in 32, 32.7 in 64)
    sk = max(1, min(want, k // 320, 32))
    # multiples of 8 let the weight-gradient kernel give every XCD whole reduction slices (csrc/gemm_tile.hip, gemm_dw_k: the
    # operands of a slice then cross the fabric once instead of once per tile row / column)
    if sk >= 8:
        sk = (sk + 3) // 8 * 8 if (sk + 3) // 8 * 8 <= max(8, min(k // 320, 32)) else sk // 8 * 8
    return sk


def _tiles(m, n, bm=128, bn=128):
    """output tiles of an [m, n] product: bm x bn on the large-tile kernels (benchmark precision), 64 x 64 otherwise"""
    if _state["prec"] != PREC_BF16:
        bm = bn = 64
    return ((m + bm - 1) // bm) * ((n + bn - 1) // bn)


def linear(x, W, b, out, act=ACT_NONE, drop=None, residual=None, accumulate=False):
    """out[M,N] = act(x[M,K] @ W[K,N] + b) (dropout) (+residual).  All 2-D row-major views."""
    M, K = x.shape
    W, Wt, _ = _wsplit(W)
    N = W.shape[1]
    gemm(M, N, K, x, _ld(x), W, _ld(W), 1, out, _ld(out), bias=b, act=act, drop=drop, residual=residual,
         ldr=_ld(residual) if residual is not None else 0, accumulate=accumulate,
         Bs=Wt, sbs_n=Wt.stride(0) if Wt is not None else 0)


def linear_rows(x, W, b, out, B, T, t0, t1):
    """out[b, t0:t1, :] = x[b, t0:t1, :] @ W + b for every sample b (row subset of [B*T, *] matrices)."""
    W, Wt, _ = _wsplit(W)
    K, N = x.shape[1], W.shape[1]
    ldx, ldo = _ld(x), _ld(out)
    gemm(t1 - t0, N, K, x[t0:], ldx, W, _ld(W), 1, out[t0:], ldo, bias=b, batch=(B, 1), sA=(T * ldx, 0),
         sC=(T * ldo, 0), Bs=Wt, sbs_n=Wt.stride(0) if Wt is not None else 0)


def linear_dx_rows(dy, W, dx, B, T, t0, t1, accumulate=False):
    """dx[b, t0:t1, :] (+)= dy[b, t0:t1, :] @ W^T for every sample b."""
    W, _, Wn = _wsplit(W)
    N, K = dy.shape[1], W.shape[0]
    ldy, ldx = _ld(dy), _ld(dx)
    gemm(t1 - t0, K, N, dy[t0:], ldy, W, 1, _ld(W), dx[t0:], ldx, batch=(B, 1), sA=(T * ldy, 0), sC=(T * ldx, 0),
         accumulate=accumulate, Bs=Wn, sbs_n=Wn.stride(0) if Wn is not None else 0)


def linear_dx(dy, W, dx, accumulate=False, residual=None):
    """dx[M,K] (+)= dy[M,N] @ W[K,N]^T (+ residual[M,K])"""
    M, N = dy.shape
    W, _, Wn = _wsplit(W)
    K = W.shape[0]
    gemm(M, K, N, dy, _ld(dy), W, 1, _ld(W), dx, _ld(dx), accumulate=accumulate, residual=residual,
         ldr=_ld(residual) if residual is not None else 0, Bs=Wn, sbs_n=Wn.stride(0) if Wn is not None else 0)


def linear_dw(x, dy, dW, db=None):
    """dW[K,N] += x[M,K]^T @ dy[M,N]   (split-K, atomic accumulate); db[N] += column sums of dy (bias gradient)"""
    M, K = x.shape
    N = dy.shape[1]
    gemm(K, N, M, x, _ld(x), dy, _ld(dy), 1, dW, _ld(dW), a_mode=1, accumulate=True, splitk=_splitk(_tiles(K, N), M),
         colsum=db)


def conv1d(x, T, W, out):
    """SAME Conv1D over time: x [B*T, Cin] rows (b,t); W [k,Cin,Cout] contiguous; out [B*T, Cout] view.
    Few output tiles with a long reduction (the 2048-channel projection conv) are split along K."""
    M, Cin = x.shape
    W, Wt, _ = _wsplit(W)
    k, _, Cout = W.shape
    tiles = _tiles(M, Cout, 64, 128) if Wt is not None else ((M + 63) // 64) * ((Cout + 63) // 64)
    # (480 workgroups: the 2048-channel projection conv at 5120 rows, 80 tiles x 6144 - 4 slices 40.1 us, 6 slices 30.2, 8 33.8:
    # tools/probes/proj1_splitk_sweep.py)
    sk = _splitk(tiles, k * Cin, target=480) if (tiles < 256 and k * Cin >= 2048 and out.is_contiguous()) else 1
    gemm(M, Cout, k * Cin, x, _ld(x), W, Cout, 1, out, _ld(out), a_mode=2, conv=(T, Cin, 1, -((k - 1) // 2)),
         kin=Cin, sb_tap=Cin * Cout, splitk=sk, split_overwrite=True, Bs=Wt, sbs_tap=Cin * Cout, sbs_n=Cin)


def conv1d_dx(dy, T, W, dx, accumulate=False):
    """dx[B*T,Cin] (+)= conv-transpose of dy[B*T,Cout] with W[k,Cin,Cout]."""
    M, Cout = dy.shape
    W, _, Wn = _wsplit(W)
    k, Cin, _ = W.shape
    gemm(M, Cin, k * Cout, dy, _ld(dy), W, 1, Cout, dx, _ld(dx), a_mode=2, conv=(T, Cout, -1, (k - 1) // 2),
         kin=Cout, sb_tap=Cin * Cout, accumulate=accumulate, Bs=Wn, sbs_tap=Cin * Cout, sbs_n=Cout)


def conv_bank(x, T, Wall, ng, out):
    """out[:, g*Cout:(g+1)*Cout] = SAME conv of width g+1 over x, g = 0..ng-1, in ONE launch.  Wall: the weights
    [1,Cin,Cout], [2,Cin,Cout], ... [ng,Cin,Cout] contiguous in memory (a flat view); out [B*T, ng*Cout]."""
    M, Cin = x.shape
    Wall, Wt, _ = _wsplit(Wall)
    Cout = out.shape[1] // ng
    gemm(M, Cout, ng * Cin, x, _ld(x), Wall, Cout, 1, out, _ld(out), a_mode=2, conv=(T, Cin, 1, 0),
         kin=Cin, sb_tap=Cin * Cout, bank=(ng, 0, Cout, Cin * Cout), Bs=Wt, sbs_tap=Cin * Cout, sbs_n=Cin)


def conv_bank_dx(dy, T, Wall, ng, dx):
    """dx[B*T, Cin] += sum over the ng widths of the transposed convs of dy[:, g*Cout:(g+1)*Cout] (one launch)."""
    M = dy.shape[0]
    Wall, _, Wn = _wsplit(Wall)
    Cout = dy.shape[1] // ng
    Cin = dx.shape[1]
    gemm(M, Cin, ng * Cout, dy, _ld(dy), Wall, 1, Cout, dx, _ld(dx), a_mode=2, conv=(T, Cout, -1, 0), kin=Cout,
         sb_tap=Cin * Cout, accumulate=True, bank=(ng, Cout, 0, Cin * Cout), Bs=Wn, sbs_tap=Cin * Cout, sbs_n=Cout)


def conv1d_dw(x, T, dy, dW, splitk=None):
    """dW[k,Cin,Cout] += sum over rows of shifted x^T dy."""
    M, Cin = x.shape
    k, _, Cout = dW.shape
    gemm(k * Cin, Cout, M, x, _ld(x), dy, _ld(dy), 1, dW, Cout, a_mode=3, conv=(T, Cin, 1, -((k - 1) // 2)),
         accumulate=True, splitk=_splitk(_tiles(k * Cin, Cout), M) if splitk is None else splitk)


def conv_bank_dw(x, T, dy, dWall, ng):
    """dW of all widths 1..ng of the conv bank: dWall = the gradients [1,Cin,Cout], [2,Cin,Cout], ... contiguous (flat
    view); dy [B*T, ng*Cout].  One launch on the large-tile kernel; per-width calls otherwise."""
    M, Cin = x.shape
    Cout = dy.shape[1] // ng
    tiles = sum(-(-((g + 1) * Cin) // 128) for g in range(ng)) * -(-Cout // 128)
    if gemm(ng * Cin, Cout, M, x, _ld(x), dy, _ld(dy), 1, dWall, Cout, a_mode=3, conv=(T, Cin, 1, 0), accumulate=True,
            splitk=_splitk(tiles, M), bank=(ng, 0, Cout, Cin * Cout), only_path=2):
        return
    off = 0
    for k in range(1, ng + 1):
        n = k * Cin * Cout
        conv1d_dw(x, T, dy[:, (k - 1) * Cout:k * Cout], dWall.view(-1)[off:off + n].view(k, Cin, Cout))
        off += n


def shifted_dw(x, T, shift, dy, dW, db=None):
    """dW[Cx,N] += sum_(b,t) x[b,t+shift,:]^T dy[b,t,:]  (recurrent-weight gradient; zero outside [0,T));
    db[N] += column sums of dy."""
    M, Cx = x.shape
    N = dy.shape[1]
    gemm(Cx, N, M, x, _ld(x), dy, _ld(dy), 1, dW, _ld(dW), a_mode=3, conv=(T, Cx, 1, shift), accumulate=True,
         splitk=_splitk(_tiles(Cx, N), M), colsum=db)


def shadow_pack(flat, table, nweights, st, sn):
    """bf16 shadows (per-tap transpose `st`, plain cast `sn`) of the weights listed in the device table; one launch"""
    _lib.check(_lib.lib().satt_shadow_pack(_p(flat), _p(table), nweights, _p(st), _p(sn), _s()), "shadow_pack")


def embedding_fwd(ids, table, out, offset=0):
    _lib.check(_lib.lib().satt_embedding_fwd(_p(ids), _p(table), _p(out), ids.numel(), table.shape[1], offset, _s()))


def embedding_bwd(ids, dout, dtable, offset=0, atomic=True):
    """dtable[ids - offset] += dout.  atomic=False: deterministic form (one workgroup per table row adds its tokens in ascending
    order): bit-stable, but a padded batch sends a third of its tokens to ONE row (the padding symbol) and that workgroup then
    runs alone - measured 80 us against 37 us for the atomic form on the benchmark batch, so the engine keeps the atomics."""
    if atomic:
        _lib.check(_lib.lib().satt_embedding_bwd(_p(ids), _p(dout), _p(dtable), ids.numel(), dtable.shape[1], offset, _s()))
    else:
        _lib.check(_lib.lib().satt_embedding_bwd_rows(_p(ids), _p(dout), _p(dtable), ids.numel(), dtable.shape[1], offset,
                                                      dtable.shape[0], _s()))


def _accent_args(ids, table, offset, Ws, bs):
    l = len(Ws)
    W1, b1 = (Ws[1], bs[1]) if l == 2 else (None, None)
    return (_p(ids), _p(table), table.shape[0], offset, table.shape[1], l, _p(Ws[0]), _p(bs[0]), Ws[0].shape[1], _p(W1), _p(b1),
            W1.shape[1] if l == 2 else 0)


def accent_prenet_fwd(ids, table, offset, Ws, bs, out, drops):
    """out[:, :] = PreNet stack (Ws, bs: fp32 [in, out] / [out] per layer) over table[ids - offset] in ONE launch; `out` is a
    row-major view (normally the trailing columns of the shared pre-net buffer).  drops: one Drop per layer (same rate).
    False (nothing launched) when the shape is beyond the kernel's cap (> 2 layers, widths > 64, LDS): compose it from
    embedding_fwd + linear then."""
    if len(Ws) > 2:
        return False
    d0, d1 = drops[0], drops[-1]
    rc = _lib.lib().satt_accent_prenet_fwd(*_accent_args(ids, table, offset, Ws, bs), _p(out), _ld(out), ids.numel(), d0.thresh,
                                           d0.scale, d0.stream, d1.stream, _p(d0.seed), _s())
    if rc == -2:
        return False
    _lib.check(rc, "accent_prenet_fwd")
    return True


def accent_prenet_bwd(ids, table, offset, Ws, bs, dout, drops, dtable, dWs, dbs):
    """backward of accent_prenet_fwd in ONE launch: dWs / dbs / dtable += (float atomics).  False when beyond the cap."""
    if len(Ws) > 2:
        return False
    d0, d1 = drops[0], drops[-1]
    two = len(Ws) == 2
    rc = _lib.lib().satt_accent_prenet_bwd(*_accent_args(ids, table, offset, Ws, bs), _p(dout), _ld(dout), ids.numel(), d0.thresh,
                                           d0.scale, d0.stream, d1.stream, _p(d0.seed), _p(dtable), _p(dWs[0]), _p(dbs[0]),
                                           _p(dWs[1]) if two else None, _p(dbs[1]) if two else None, _s())
    if rc == -2:
        return False
    _lib.check(rc, "accent_prenet_bwd")
    return True


SPK_IDS, SPK_EMBED, SPK_SCALAR = 0, 1, 2      # csrc/speaker_cond.hip: where the speaker of a row comes from


def speaker_cond_supported(B, E, R, P0):
    """True when the one-launch speaker kernel takes the shape (caps and LDS footprint: include/satt_hip.h)"""
    return bool(_lib.lib().satt_speaker_cond_supported(B, E, R, P0))


def _speaker_src(speaker, B):
    """(mode, ids pointer, scalar id, embedding pointer) of `speaker`: an int (one id for every row), an int64 tensor [B] or
    a float32 tensor [B, E]"""
    if isinstance(speaker, int):
        return SPK_SCALAR, None, speaker, None
    if speaker.dtype == torch.int64:
        assert speaker.numel() == B and speaker.is_contiguous()
        return SPK_IDS, _p(speaker), 0, None
    assert speaker.dtype == torch.float32 and speaker.shape[0] == B and speaker.is_contiguous()
    return SPK_EMBED, None, 0, _p(speaker)


def speaker_cond_fwd(speaker, table, offset, Wr, br, Ws, bs, semb, rs, sproj):
    """semb = table[speaker - offset] (or `speaker` itself when it is a float [B, E] tensor, or row `speaker` for every sample when it
    is an int); rs = relu(semb Wr + br); sproj = softsign(rs Ws + bs): ONE launch.  False (nothing launched) beyond the cap."""
    B = semb.shape[0]
    mode, ids, sid, emb = _speaker_src(speaker, B)
    rc = _lib.lib().satt_speaker_cond_fwd(mode, ids, sid, emb, B, _p(table), 0 if table is None else table.shape[0], offset,
                                          Wr.shape[0], _p(Wr), _p(br), Wr.shape[1], _p(Ws), _p(bs), Ws.shape[1], _p(semb), _p(rs),
                                          _p(sproj), _s())
    if rc == -2:
        return False
    _lib.check(rc, "speaker_cond_fwd")
    return True


def rows_bcast_add(y, v, B, T, t0=0, t1=None):
    """y[b, t, :] += v[b, :] for t0 <= t < t1 (default T); y [B*T, N] and v [B, N] row-major 2-D views (leading dimensions taken
    from the views).  An empty range launches nothing.  csrc/speaker_cond.hip"""
    N = v.shape[1]
    assert y.shape == (B * T, N) and v.shape[0] == B
    _lib.check(_lib.lib().satt_rows_bcast_add(_p(y), _ld(y), _p(v), _ld(v), B, T, N, t0, T if t1 is None else t1, _s()),
               "rows_bcast_add")


def rows_time_sum(dy, lengths, dv, B, T, t0=0):
    """dv[b, :] = sum of dy[b, t, :] over t0 <= t < min(T, lengths[b]) (lengths int64 [B] or None = T); dy [B*T, N], dv [B, N]
    row-major 2-D views.  Deterministic (fixed summation order).  csrc/speaker_cond.hip"""
    N = dv.shape[1]
    assert dy.shape == (B * T, N) and dv.shape[0] == B and (lengths is None or (lengths.dtype == torch.int64 and lengths.numel() == B))
    _lib.check(_lib.lib().satt_rows_time_sum(_p(dy), _ld(dy), _p(lengths), _p(dv), _ld(dv), B, T, N, t0, _s()), "rows_time_sum")


def melspec_supported(n_fft, win, hop, num_mels):
    """True when satt_melspec takes these STFT parameters (host-only: needs the library, not a GPU)"""
    return bool(_lib.lib().satt_melspec_supported(int(n_fft), int(win), int(hop), int(num_mels)))


def melspec(signal, sample_offsets, frame_offsets, n_fft, win, hop, window, twiddle, band_start, band_offset, band_weight,
            ref_level_db, mel, mag=None):
    """log-mel spectrograms of a batch of utterances in one launch (csrc/melspec.hip).  signal: fp32 [total samples], utterance u
    at sample_offsets[u] .. sample_offsets[u + 1] (int64 [U + 1]), its rows of mel [total frames, num_mels] (and of the optional
    mag [total frames, n_fft / 2 + 1]) at frame_offsets[u] .. frame_offsets[u + 1] (int64 [U + 1], 1 + n // hop rows each).  The
    tables are those of utils/audio.py MelspecTables.  Parameters outside satt_melspec_supported raise."""
    assert signal.dtype == torch.float32 and signal.dim() == 1 and signal.is_contiguous()
    assert sample_offsets.dtype == torch.int64 and frame_offsets.dtype == torch.int64
    assert sample_offsets.numel() == frame_offsets.numel() >= 2
    assert window.dtype == torch.float32 and window.numel() == n_fft and twiddle.dtype == torch.float32 and twiddle.numel() == 2 * n_fft
    assert band_start.dtype == torch.int32 and band_offset.dtype == torch.int32 and band_weight.dtype == torch.float32
    num_mels = band_start.numel()
    assert band_offset.numel() == num_mels + 1
    assert mel.dtype == torch.float32 and mel.dim() == 2 and mel.is_contiguous() and mel.shape[1] == num_mels
    assert mag is None or (mag.dtype == torch.float32 and mag.is_contiguous() and mag.shape == (mel.shape[0], n_fft // 2 + 1))
    p = _lib.MelspecParams(
        n_fft=n_fft, win=win, hop=hop, num_mels=num_mels, n_utts=sample_offsets.numel() - 1, n_band_weights=band_weight.numel(),
        total_samples=signal.numel(), total_frames=mel.shape[0], signal=_p(signal), sample_offsets=_p(sample_offsets),
        frame_offsets=_p(frame_offsets), window=_p(window), twiddle=_p(twiddle), band_start=_p(band_start),
        band_offset=_p(band_offset), band_weight=_p(band_weight), ref_level_db=float(ref_level_db), mel=_p(mel), mag=_p(mag))
    _lib.check(_lib.lib().satt_melspec(C.byref(p), _s()), "melspec")


def resample_supported(up, down, taps):
    """True when satt_resample takes this ratio and filter length (host-only: needs the library, not a GPU)"""
    return bool(_lib.lib().satt_resample_supported(int(up), int(down), int(taps)))


def resample_run_length():
    """the outputs one workgroup of csrc/resample.hip takes: the launch's seams fall at its multiples, counted through the batch"""
    return int(_lib.lib().satt_resample_run_length())


def resample(signal_in, in_offsets, out_offsets, up, down, table, signal_out):
    """sample-rate conversion of a batch of utterances in one launch (csrc/resample.hip).  signal_in: fp32 [total in], utterance u
    at in_offsets[u] .. in_offsets[u + 1] (int64 [U + 1], n >= 1 samples), its ceil(n up / down) results in signal_out (fp32
    [total out]) at out_offsets[u] .. out_offsets[u + 1].  table: fp32 [up, taps], utils/audio.py ResampleTables.  Parameters outside
    satt_resample_supported raise."""
    assert signal_in.dtype == torch.float32 and signal_in.dim() == 1 and signal_in.is_contiguous()
    assert signal_out.dtype == torch.float32 and signal_out.dim() == 1 and signal_out.is_contiguous()
    assert in_offsets.dtype == torch.int64 and out_offsets.dtype == torch.int64 and in_offsets.numel() == out_offsets.numel() >= 2
    assert table.dtype == torch.float32 and table.dim() == 2 and table.is_contiguous() and table.shape[0] == up
    taps = table.shape[1]
    if not resample_supported(up, down, taps):
        raise ValueError("resample does not take up=%d down=%d taps=%d (coprime and not both 1, up <= 1024, down <= 4096, taps even "
                         "and <= 4096)" % (up, down, taps))
    p = _lib.ResampleParams(up=up, down=down, taps=taps, n_utts=in_offsets.numel() - 1, total_in=signal_in.numel(),
                            total_out=signal_out.numel(), signal_in=_p(signal_in), in_offsets=_p(in_offsets),
                            out_offsets=_p(out_offsets), table=_p(table), signal_out=_p(signal_out))
    _lib.check(_lib.lib().satt_resample(C.byref(p), _s()), "resample")


def dtw_supported(Ta, Tb, K):
    """True when satt_dtw takes pairs of these lengths and this feature width (host-only: needs the library, not a GPU)"""
    return bool(_lib.lib().satt_dtw_supported(int(Ta), int(Tb), int(K)))


def dtw_max_frames():
    """the longest sequence csrc/dtw.hip takes: three diagonals of D and L in 48 KiB of LDS"""
    return int(_lib.lib().satt_dtw_max_frames())


def dtw(a, b, a_offsets, b_offsets, max_ta, max_tb, cost, steps, dirs=None, dir_offsets=None, path=None, path_offsets=None):
    """dynamic time warping of a batch of pairs in one launch (csrc/dtw.hip).  a: fp32 [total a, K], b: fp32 [total b, K]; pair u is
    a[a_offsets[u] .. a_offsets[u + 1]) against b[b_offsets[u] .. b_offsets[u + 1]) (int64 [U + 1]); max_ta / max_tb: the longest
    of each side.  cost fp32 [U] and steps int32 [U] receive D and L of the corner.  With dirs (uint8, Ta * Tb bytes per pair at
    dir_offsets) and path (int32 [total, 2], Ta + Tb - 1 pairs of room per pair at path_offsets) the warping path is written too.
    Shapes outside satt_dtw_supported raise."""
    assert a.dtype == torch.float32 and a.dim() == 2 and a.is_contiguous()
    assert b.dtype == torch.float32 and b.dim() == 2 and b.is_contiguous() and b.shape[1] == a.shape[1]
    assert a_offsets.dtype == torch.int64 and b_offsets.dtype == torch.int64 and a_offsets.numel() == b_offsets.numel() >= 2
    n = a_offsets.numel() - 1
    assert cost.dtype == torch.float32 and cost.is_contiguous() and cost.numel() >= n
    assert steps.dtype == torch.int32 and steps.is_contiguous() and steps.numel() >= n
    want_path = dirs is not None
    if want_path:
        assert dirs.dtype == torch.uint8 and dirs.dim() == 1 and dirs.is_contiguous()
        assert path.dtype == torch.int32 and path.dim() == 2 and path.shape[1] == 2 and path.is_contiguous()
        assert dir_offsets.dtype == torch.int64 and path_offsets.dtype == torch.int64 and dir_offsets.numel() == path_offsets.numel() == n + 1
    else:
        assert dir_offsets is None and path is None and path_offsets is None
    K = a.shape[1]
    if not dtw_supported(max_ta, max_tb, K):
        raise ValueError("dtw does not take Ta=%d Tb=%d K=%d (1 <= Ta, Tb <= %d, 1 <= K <= 128)" % (max_ta, max_tb, K, dtw_max_frames()))
    p = _lib.DtwParams(n_pairs=n, K=K, max_ta=max_ta, max_tb=max_tb, total_a=a.shape[0], total_b=b.shape[0],
                       total_dirs=dirs.numel() if want_path else 0, total_path=path.shape[0] if want_path else 0, a=_p(a), b=_p(b),
                       a_offsets=_p(a_offsets), b_offsets=_p(b_offsets), cost=_p(cost), steps=_p(steps), dirs=_p(dirs),
                       dir_offsets=_p(dir_offsets), path=_p(path), path_offsets=_p(path_offsets))
    _lib.check(_lib.lib().satt_dtw(C.byref(p), _s()), "dtw")


def yin_supported(window, tau_max, hop):
    """True when satt_yin takes this window, longest lag and hop (host-only: needs the library, not a GPU)"""
    return bool(_lib.lib().satt_yin_supported(int(window), int(tau_max), int(hop)))


def yin_limits():
    """(longest window, longest lag, frames a workgroup takes) of csrc/yin.hip"""
    L = _lib.lib()
    return int(L.satt_yin_max_window()), int(L.satt_yin_max_lag()), int(L.satt_yin_run_length())


def yin(signal, in_offsets, frame_offsets, window, tau_min, tau_max, hop, sample_rate, threshold, f0, aperiodicity, power):
    """YIN pitch tracking of a batch of utterances in one launch (csrc/yin.hip).  signal: fp32 [total in], utterance u at
    in_offsets[u] .. in_offsets[u + 1] (int64 [U + 1], n >= 1 samples), its 1 + n // hop frames of f0, aperiodicity and power (fp32
    [total frames] each) at frame_offsets[u] .. frame_offsets[u + 1].  Parameters outside satt_yin_supported raise."""
    assert signal.dtype == torch.float32 and signal.dim() == 1 and signal.is_contiguous()
    assert in_offsets.dtype == torch.int64 and frame_offsets.dtype == torch.int64 and in_offsets.numel() == frame_offsets.numel() >= 2
    for o in (f0, aperiodicity, power):
        assert o.dtype == torch.float32 and o.dim() == 1 and o.is_contiguous() and o.numel() == f0.numel()
    if not yin_supported(window, tau_max, hop):
        raise ValueError("yin does not take window=%d tau_max=%d hop=%d (1 <= window <= %d, 3 <= tau_max <= %d, 1 <= hop <= 2^20)"
                         % ((window, tau_max, hop) + yin_limits()[:2]))
    p = _lib.YinParams(window=window, tau_min=tau_min, tau_max=tau_max, hop=hop, n_utts=in_offsets.numel() - 1,
                       sample_rate=float(sample_rate), threshold=float(threshold), total_in=signal.numel(), total_frames=f0.numel(),
                       signal=_p(signal), in_offsets=_p(in_offsets), frame_offsets=_p(frame_offsets), f0=_p(f0),
                       aperiodicity=_p(aperiodicity), power=_p(power))
    _lib.check(_lib.lib().satt_yin(C.byref(p), _s()), "yin")


def yin_candidates(signal, in_offsets, frame_offsets, window, tau_min, tau_max, hop, cand_period, cand_value, power):
    """the period candidates of every frame of a batch of utterances in one launch (csrc/yin.hip).  Signal and offsets as for `yin`;
    cand_period and cand_value: fp32 [total frames, 8], power: fp32 [total frames].  Parameters outside satt_yin_supported raise."""
    assert signal.dtype == torch.float32 and signal.dim() == 1 and signal.is_contiguous()
    assert in_offsets.dtype == torch.int64 and frame_offsets.dtype == torch.int64 and in_offsets.numel() == frame_offsets.numel() >= 2
    assert power.dtype == torch.float32 and power.dim() == 1 and power.is_contiguous()
    for o in (cand_period, cand_value):
        assert o.dtype == torch.float32 and o.is_contiguous() and tuple(o.shape) == (power.numel(), 8)
    if not yin_supported(window, tau_max, hop):
        raise ValueError("yin_candidates does not take window=%d tau_max=%d hop=%d (1 <= window <= %d, 3 <= tau_max <= %d, 1 <= hop <= 2^20)"
                         % ((window, tau_max, hop) + yin_limits()[:2]))
    p = _lib.YinCandidatesParams(window=window, tau_min=tau_min, tau_max=tau_max, hop=hop, n_utts=in_offsets.numel() - 1,
                                 total_in=signal.numel(), total_frames=power.numel(), signal=_p(signal), in_offsets=_p(in_offsets),
                                 frame_offsets=_p(frame_offsets), cand_period=_p(cand_period), cand_value=_p(cand_value), power=_p(power))
    _lib.check(_lib.lib().satt_yin_candidates(C.byref(p), _s()), "yin_candidates")


def mel_nnls_supported(num_bins, num_mels, iters):
    """True when satt_mel_nnls takes this many bins, bands and iterations (host-only: needs the library, not a GPU)"""
    return bool(_lib.lib().satt_mel_nnls_supported(int(num_bins), int(num_mels), int(iters)))


def mel_nnls(amp, start, beta, step, band_start, band_offset, band_weight, bin_first, bin_offset, bin_weight, out):
    """non-negative inversion of the mel basis for a batch of frames in one launch (csrc/mel_nnls.hip).  amp: fp32 [N, num_mels],
    start and out: fp32 [N, num_bins], beta: fp32 [iters]; the banded basis and its transposed table are those of utils/audio.py
    MelNnlsTables.  Sizes outside satt_mel_nnls_supported raise."""
    assert amp.dtype == torch.float32 and amp.dim() == 2 and amp.is_contiguous()
    N, M = amp.shape
    for o in (start, out):
        assert o.dtype == torch.float32 and o.dim() == 2 and o.is_contiguous() and o.shape[0] == N and o.shape[1] == start.shape[1]
    F = start.shape[1]
    assert beta.dtype == torch.float32 and beta.dim() == 1 and beta.is_contiguous()
    for o in (band_start, band_offset, bin_first, bin_offset):
        assert o.dtype == torch.int32 and o.dim() == 1 and o.is_contiguous()
    assert band_start.numel() == M and band_offset.numel() == M + 1 and bin_first.numel() == F and bin_offset.numel() == F + 1
    for o in (band_weight, bin_weight):
        assert o.dtype == torch.float32 and o.dim() == 1 and o.is_contiguous()
    iters = beta.numel()
    if not mel_nnls_supported(F, M, iters) or N < 1:
        raise ValueError("mel_nnls does not take num_bins=%d num_mels=%d iters=%d frames=%d (num_bins <= 2049, num_mels <= 128, "
                         "1 <= iters <= 1024, frames >= 1)" % (F, M, iters, N))
    p = _lib.MelNnlsParams(num_bins=F, num_mels=M, iters=iters, n_weights=band_weight.numel(), n_tweights=bin_weight.numel(),
                           step=float(step), n_frames=N, amp=_p(amp), start=_p(start), beta=_p(beta), band_start=_p(band_start),
                           band_offset=_p(band_offset), band_weight=_p(band_weight), bin_first=_p(bin_first),
                           bin_offset=_p(bin_offset), bin_weight=_p(bin_weight), out=_p(out))
    _lib.check(_lib.lib().satt_mel_nnls(C.byref(p), _s()), "mel_nnls")


def f0_viterbi_supported(max_frames):
    """True when satt_f0_viterbi takes utterances of up to this many frames (host-only: needs the library, not a GPU)"""
    return bool(_lib.lib().satt_f0_viterbi_supported(int(max_frames)))


def f0_viterbi_max_frames():
    """the longest utterance csrc/f0_viterbi.hip takes: a predecessor byte per frame and state in 18 KiB of LDS"""
    return int(_lib.lib().satt_f0_viterbi_max_frames())


def f0_viterbi(cand_period, cand_value, gate, frame_offsets, max_frames, tau_max, sample_rate, jump_cost, switch_cost, unvoiced_cost,
               lag_bias, f0, state, cost):
    """the cheapest path through the candidates of a batch of utterances in one launch (csrc/f0_viterbi.hip).  cand_period,
    cand_value: fp32 [total frames, 8]; gate: uint8 [total frames]; utterance u owns frames frame_offsets[u] .. frame_offsets[u + 1]
    (int64 [U + 1]) of f0 (fp32) and state (uint8) and entry u of cost (fp32 [U]).  max_frames: the longest utterance of the batch;
    one outside satt_f0_viterbi_supported raises."""
    n = frame_offsets.numel() - 1
    assert frame_offsets.dtype == torch.int64 and n >= 1
    assert gate.dtype == torch.uint8 and state.dtype == torch.uint8 and f0.dtype == torch.float32 and cost.dtype == torch.float32
    assert gate.dim() == state.dim() == f0.dim() == cost.dim() == 1 and gate.numel() == state.numel() == f0.numel() and cost.numel() == n
    for o in (cand_period, cand_value):
        assert o.dtype == torch.float32 and o.is_contiguous() and tuple(o.shape) == (f0.numel(), 8)
    assert all(o.is_contiguous() for o in (gate, state, f0, cost, frame_offsets))
    if not f0_viterbi_supported(max_frames):
        raise ValueError("f0_viterbi does not take an utterance of %d frames (1 <= frames <= %d)" % (max_frames, f0_viterbi_max_frames()))
    p = _lib.F0ViterbiParams(n_utts=n, max_frames=max_frames, tau_max=tau_max, sample_rate=float(sample_rate), jump_cost=float(jump_cost),
                             switch_cost=float(switch_cost), unvoiced_cost=float(unvoiced_cost), lag_bias=float(lag_bias),
                             total_frames=f0.numel(), cand_period=_p(cand_period), cand_value=_p(cand_value), gate=_p(gate),
                             frame_offsets=_p(frame_offsets), f0=_p(f0), state=_p(state), cost=_p(cost))
    _lib.check(_lib.lib().satt_f0_viterbi(C.byref(p), _s()), "f0_viterbi")


def griffin_lim_supported(n_fft, win, hop):
    """True when satt_griffin_lim takes these STFT parameters (host-only: needs the library, not a GPU)"""
    return bool(_lib.lib().satt_griffin_lim_supported(int(n_fft), int(win), int(hop)))


def griffin_lim_workspace_bytes(n_fft, total_frames):
    return int(_lib.lib().satt_griffin_lim_workspace_bytes(int(n_fft), int(total_frames)))


def griffin_lim(mag, ang, c_prev, signal, sample_offsets, frame_offsets, n_fft, win, hop, iters, alpha, window, twiddle, envelope,
                workspace, spec_out=None):
    """`iters` Griffin-Lim iterations and the inverse STFT behind them for a batch of utterances in one call (csrc/griffin_lim.hip).
    mag: fp32 [total frames, n_fft / 2 + 1]; ang: fp32 [total frames, n_fft / 2 + 1, 2] unit complex, in/out; c_prev: the same shape,
    in/out, or None with alpha == 0; signal: fp32 [total samples], out.  Utterance u owns rows frame_offsets[u] .. frame_offsets[u +
    1] (T frames) and samples sample_offsets[u] .. sample_offsets[u + 1] ((T - 1) hop of them; int64 [U + 1] each).  window / twiddle
    are those of utils/audio.py MelspecTables, envelope is overlap_envelope_tables (fp64 [hop + 2 n_fft]); spec_out (optional, ang's
    shape) receives the last re-analysis.  Parameters outside satt_griffin_lim_supported raise."""
    NF = n_fft // 2 + 1
    assert mag.dtype == torch.float32 and mag.dim() == 2 and mag.shape[1] == NF and mag.is_contiguous()
    for x in (ang, c_prev, spec_out):
        assert x is None or (x.dtype == torch.float32 and x.shape == (mag.shape[0], NF, 2) and x.is_contiguous())
    assert ang is not None and (c_prev is not None or alpha == 0)
    assert signal.dtype == torch.float32 and signal.dim() == 1 and signal.is_contiguous()
    assert sample_offsets.dtype == torch.int64 and frame_offsets.dtype == torch.int64
    assert sample_offsets.numel() == frame_offsets.numel() >= 2
    assert window.dtype == torch.float32 and window.numel() == n_fft and twiddle.dtype == torch.float32 and twiddle.numel() == 2 * n_fft
    assert envelope.dtype == torch.float64 and envelope.numel() == hop + 2 * n_fft
    assert workspace.dtype == torch.float32 and workspace.numel() * 4 >= griffin_lim_workspace_bytes(n_fft, mag.shape[0])
    if not griffin_lim_supported(n_fft, win, hop):
        raise ValueError("griffin_lim does not take n_fft=%d win=%d hop=%d (n_fft in 512 / 1024 / 2048 / 4096, 16 <= win <= n_fft, "
                         "1 <= hop <= win / 2)" % (n_fft, win, hop))
    p = _lib.GriffinLimParams(
        n_fft=n_fft, win=win, hop=hop, n_utts=sample_offsets.numel() - 1, iters=int(iters), alpha=float(alpha),
        total_samples=signal.numel(), total_frames=mag.shape[0], sample_offsets=_p(sample_offsets), frame_offsets=_p(frame_offsets),
        window=_p(window), twiddle=_p(twiddle), envelope=_p(envelope), mag=_p(mag), ang=_p(ang), c_prev=_p(c_prev), signal=_p(signal),
        workspace=_p(workspace), spec_out=_p(spec_out))
    _lib.check(_lib.lib().satt_griffin_lim(C.byref(p), _s()), "griffin_lim")


def act_bwd(dy, y, dx, act, scale=1.0):
    rows, cols = y.shape
    _lib.check(_lib.lib().satt_act_bwd(_p(dy), _ld(dy), _p(y), _ld(y), _p(dx), _ld(dx), rows, cols, act, scale, _s()))


def act_bwd_res(dy, z, res, dx, act, scale=1.0):
    """dx = dy * act'(.) with the activation output given as z - res (z = act(u) + res from a GEMM epilogue with a residual)"""
    rows, cols = z.shape
    _lib.check(_lib.lib().satt_act_bwd_res(_p(dy), _ld(dy), _p(z), _ld(z), _p(res), _ld(res), _p(dx), _ld(dx), rows, cols, act,
                                           scale, _s()))


def bn_maxpool_fwd(x, gamma, beta, mp, mean, rstd, mmean, mvar, ws, B, T, eps, momentum, act):
    """mp = maxpool(act(bn(x))) in one pass (x contiguous [B*T, C]); returns False (nothing launched) if the shape does not fit"""
    rc = _lib.lib().satt_bn_maxpool_fwd(_p(x), _p(gamma), _p(beta), _p(mp), _p(mean), _p(rstd), _p(mmean), _p(mvar), _p(ws), B, T,
                                        x.shape[1], eps, momentum, act, _s())
    if rc == -2:
        return False
    _lib.check(rc, "bn_maxpool_fwd")
    return True


def maxpool_bn_bwd(dmp, x, gamma, beta, mean, rstd, dx, dgamma, dbeta, ws, dbuf, B, T, act):
    _lib.check(_lib.lib().satt_maxpool_bn_bwd(_p(dmp), _p(x), _p(gamma), _p(beta), _p(mean), _p(rstd), _p(dx), _p(dgamma), _p(dbeta),
                                              _p(ws), _p(dbuf), B, T, x.shape[1], act, _s()), "maxpool_bn_bwd")


def bn_ws(rows, Cc, device):
    return torch.empty(_lib.lib().satt_bn_ws_floats(rows, Cc), dtype=torch.float32, device=device)


def bn_fwd(x, gamma, beta, y, mean, rstd, mmean, mvar, ws, eps, momentum, act):
    rows, Cc = x.shape
    _lib.check(_lib.lib().satt_bn_fwd(_p(x), _ld(x), _p(gamma), _p(beta), _p(y), _ld(y), _p(mean), _p(rstd),
                                      _p(mmean), _p(mvar), _p(ws), rows, Cc, eps, momentum, act, _s()), "bn_fwd")


def bn_fused_state(rows, Cc, device):
    """(ws, sync) of the one-launch BatchNorm pair for one call site: sync is zeroed here ONCE and returned to zero by every
    launch - keep the pair with the call site (engine: one per BatchNorm layer)"""
    l = _lib.lib()
    return (torch.empty(l.satt_bn_fused_ws_floats(rows, Cc), dtype=torch.float32, device=device),
            torch.zeros(l.satt_bn_fused_sync_words(Cc), dtype=torch.int32, device=device))


def bn_fwd_fused(x, gamma, beta, y, mean, rstd, mmean, mvar, state, eps, momentum, act):
    """BatchNorm forward (training statistics) in one launch; False (nothing launched) when the grid is too large for it"""
    rows, Cc = x.shape
    rc = _lib.lib().satt_bn_fwd_fused(_p(x), _ld(x), _p(gamma), _p(beta), _p(y), _ld(y), _p(mean), _p(rstd), _p(mmean), _p(mvar),
                                      _p(state[0]), _p(state[1]), rows, Cc, eps, momentum, act, _s())
    if rc == -2:
        return False
    _lib.check(rc, "bn_fwd_fused")
    return True


def bn_bwd_fused(dy, x, gamma, beta, mean, rstd, dx, dgamma, dbeta, state, act):
    rows, Cc = x.shape
    rc = _lib.lib().satt_bn_bwd_fused(_p(dy), _ld(dy), _p(x), _ld(x), _p(gamma), _p(beta), _p(mean), _p(rstd), _p(dx), _ld(dx),
                                      _p(dgamma), _p(dbeta), _p(state[0]), _p(state[1]), rows, Cc, act, _s())
    if rc == -2:
        return False
    _lib.check(rc, "bn_bwd_fused")
    return True


def bn_infer(x, gamma, beta, mmean, mvar, y, eps, act):
    rows, Cc = x.shape
    _lib.check(_lib.lib().satt_bn_infer(_p(x), _ld(x), _p(gamma), _p(beta), _p(mmean), _p(mvar), _p(y), _ld(y), rows,
                                        Cc, eps, act, _s()), "bn_infer")


def bn_bwd(dy, x, gamma, beta, mean, rstd, dx, dgamma, dbeta, ws, act):
    rows, Cc = x.shape
    _lib.check(_lib.lib().satt_bn_bwd(_p(dy), _ld(dy), _p(x), _ld(x), _p(gamma), _p(beta), _p(mean), _p(rstd),
                                      _p(dx), _ld(dx), _p(dgamma), _p(dbeta), _p(ws), rows, Cc, act, _s()), "bn_bwd")


def maxpool_fwd(x, y, B, T, Cc):
    _lib.check(_lib.lib().satt_maxpool_fwd(_p(x), _p(y), B, T, Cc, _s()))


def maxpool_bwd(dy, x, dx, B, T, Cc):
    _lib.check(_lib.lib().satt_maxpool_bwd(_p(dy), _p(x), _p(dx), B, T, Cc, _s()))


def highway_fwd(z, x, y):
    rows, H = x.shape
    _lib.check(_lib.lib().satt_highway_fwd(_p(z), _p(x), _p(y), rows, H, _s()))


def highway_bwd(dy, z, x, dz, dx):
    rows, H = x.shape
    _lib.check(_lib.lib().satt_highway_bwd(_p(dy), _p(z), _p(x), _p(dz), _p(dx), rows, H, _s()))


def _highway_layers(Ws, bs, zs, ys, dzs):
    arr = (_lib.HighwayLayer * len(Ws))()
    for n, W in enumerate(Ws):
        arr[n].Wt, arr[n].Wn = _p(W.t), _p(W.n)
        arr[n].b = _p(bs[n]) if bs is not None else None
        arr[n].z, arr[n].y = _p(zs[n]), _p(ys[n])
        arr[n].dz = _p(dzs[n]) if dzs is not None else None
    return arr


def highway_stack_ok(Ws, H):
    """the one-launch highway stack (csrc/highway.hip) applies: bf16 mode, 128 units, bf16 shadows of every layer"""
    return get_precision() == "bf16" and H == 128 and 0 < len(Ws) <= 8 and \
        all(isinstance(W, Weight) and W.t is not None and W.n is not None for W in Ws)


def highway_stack_fwd(x, Ws, bs, zs, ys):
    """all layers of the highway stack in one launch: zs[n] [rows, 2H] pre-activations, ys[n] [rows, H] outputs of layer n"""
    rows, H = x.shape
    _lib.check(_lib.lib().satt_highway_stack_fwd(_p(x), _highway_layers(Ws, bs, zs, ys, None), len(Ws), rows, H, _s()))


def highway_stack_bwd(dy, x, Ws, zs, ys, dzs, dx):
    """backward of highway_stack_fwd: dzs[n] [rows, 2H] = gradient wrt layer n's pre-activations (the operand of its weight-gradient
    GEMM), dx [rows, H] = gradient wrt the stack input"""
    rows, H = x.shape
    _lib.check(_lib.lib().satt_highway_stack_bwd(_p(dy), _p(x), _highway_layers(Ws, None, zs, ys, dzs), len(Ws), rows, H, _p(dx), _s()))


def colsum(x, out, accumulate=True):
    rows, cols = x.shape
    _lib.check(_lib.lib().satt_colsum(_p(x), _ld(x), _p(out), rows, cols, int(accumulate), _s()))


def loc_filter_dw(a1, dfl, dF, dbF, B, Td, Ti, kernel, filters):
    """location-filter gradients in one launch; False when the dedicated kernel does not serve this filter shape"""
    rc = _lib.lib().satt_loc_filter_dw(_p(a1), _p(dfl), _p(dF), _p(dbF), B, Td, Ti, kernel, filters, _s())
    if rc == -2:
        return False
    _lib.check(rc, "loc_filter_dw")
    return True


def axpby(x, y, a=1.0, b=1.0):
    rows, cols = x.shape
    _lib.check(_lib.lib().satt_axpby(_p(x), _ld(x), _p(y), _ld(y), rows, cols, a, b, _s()))


def seq_mask(x, lengths, y, B, T, Cc, round_bf16=False):
    _lib.check(_lib.lib().satt_seq_mask(_p(x), _p(lengths), _p(y), B, T, Cc, int(round_bf16), _s()))


def bcast_add(sv, y, B, T, Cc):
    _lib.check(_lib.lib().satt_bcast_add(_p(sv), _p(y), B, T, Cc, _s()))


def segment_colsum(x, ds, B, T, Cc, accumulate=False):
    _lib.check(_lib.lib().satt_segment_colsum(_p(x), _p(ds), B, T, Cc, int(accumulate), _s()))


def to_bf16(src, dst, transpose=False):
    rows, cols = src.shape
    _lib.check(_lib.lib().satt_to_bf16(_p(src), _ld(src), _p(dst), rows, cols, int(transpose), _s()))


def softmax_fwd(s, p, pd, nbh, T, scale, causal, drop):
    d = drop if drop is not None else Drop(0.0, 0, None)
    _lib.check(_lib.lib().satt_softmax_fwd(_p(s), _p(p), _p(pd), nbh, T, scale, int(causal), d.thresh, d.scale,
                                           d.stream, _p(d.seed), _s()), "softmax_fwd")


def small_attn_supported(head_dim, T):
    return bool(_lib.lib().satt_small_attn_supported(int(head_dim), int(T)))


def small_attn_fwd(kvq, D, p, o, B, T, heads, scale, drop):
    """fused attention of the encoder block (head depth 16): p [B*H,T,T] probabilities (returned alignments), o [B*T, D]"""
    d = drop if drop is not None else Drop(0.0, 0, None)
    _lib.check(_lib.lib().satt_small_attn_fwd(_p(kvq), _ld(kvq), _p(p), _p(o), _ld(o), B, T, D, heads, scale, d.thresh, d.scale,
                                              d.stream, _p(d.seed), _s()), "small_attn_fwd")


def small_attn_bwd(kvq, D, p, do, dkvq, rowsum, B, T, heads, scale, drop):
    d = drop if drop is not None else Drop(0.0, 0, None)
    _lib.check(_lib.lib().satt_small_attn_bwd(_p(kvq), _ld(kvq), _p(p), _p(do), _ld(do), _p(dkvq), _ld(dkvq), _p(rowsum), B, T, D,
                                              heads, scale, d.thresh, d.scale, d.stream, _p(d.seed), _s()), "small_attn_bwd")


def dropout(x, y, drop):
    """y = dropout(x) with the counter-based mask of `drop` (index = row-major position); also the backward on dy."""
    rows, cols = x.shape
    d = drop if drop is not None else Drop(0.0, 0, None)
    _lib.check(_lib.lib().satt_dropout(_p(x), _ld(x), _p(y), _ld(y), rows, cols, d.thresh, d.scale, d.stream, _p(d.seed),
                                       _s()), "dropout")


def softmax_rows(s, p, rows, cols, scale):
    """p[r, :cols] = softmax(scale * s[r, :cols]); s, p: 2-D views with arbitrary leading dimension."""
    _lib.check(_lib.lib().satt_softmax_rows(_p(s), _ld(s), _p(p), _ld(p), rows, cols, scale, _s()), "softmax_rows")


def softmax_bwd(dpd, p, ds, nbh, T, scale, causal, drop):
    d = drop if drop is not None else Drop(0.0, 0, None)
    _lib.check(_lib.lib().satt_softmax_bwd(_p(dpd), _p(p), _p(ds), nbh, T, scale, int(causal), d.thresh, d.scale,
                                           d.stream, _p(d.seed), _s()), "softmax_bwd")


def flash_attn_supported(hd):
    """the fused attention kernels serve head_dim 128 in the benchmark precision (csrc/flash.hip)"""
    return hd == 128 and _state["prec"] == PREC_BF16


def flash_attn_fwd(kvq, D, o, lse, B, T, H, scale, causal, drop, kvq_b=None):
    """kvq [B*T, 3D] = K | V | Q column blocks (heads of D/H = 128 inside each); o [B*T, D]; lse [B*H, T];
    kvq_b (optional, bf16 [B*T, 3D]): written with the bf16 copies of K | V | Q for the backward kernels"""
    d = drop if drop is not None else Drop(0.0, 0, None)
    if kvq_b is not None:
        _lib.check(_lib.lib().satt_flash_attn_fwd_b(_p(kvq), _p(kvq[:, D:]), _p(kvq[:, 2 * D:]), _ld(kvq), _p(o), _ld(o), _p(lse),
                                                    B, T, H, D // H, scale, int(causal), d.thresh, d.scale, d.stream, _p(d.seed),
                                                    _p(kvq_b), _p(kvq_b[:, D:]), _p(kvq_b[:, 2 * D:]), _ld(kvq_b), _s()), "flash_attn_fwd")
        return
    _lib.check(_lib.lib().satt_flash_attn_fwd(_p(kvq), _p(kvq[:, D:]), _p(kvq[:, 2 * D:]), _ld(kvq), _p(o), _ld(o), _p(lse),
                                              B, T, H, D // H, scale, int(causal), d.thresh, d.scale, d.stream, _p(d.seed),
                                              _s()), "flash_attn_fwd")


FLASH_TILE = 64     # rows per key / query tile of the fused attention kernels (csrc/flash.hip FT)


def flash_attn_bwd(kvq, D, o, do, lse, delta, dkvq, B, T, H, scale, causal, drop, tiles=None, with_delta=True, kvq_b=None, do_b=None):
    """dkvq [B*T, 3D] = dK | dV | dQ (written, not accumulated).  tiles = (lo, hi): only the 64-row tiles [lo, hi) (causal: any
    range leaves its own rows final; ranges run LAST TO FIRST, each with with_delta: a launch computes the row sums o . d o of its own
    query tiles and reads those of later tiles).  kvq_b (bf16 [B*T, 3D] written by
    flash_attn_fwd) + do_b (bf16 [B*T, D] scratch): the bf16-source kernels - bit-identical results, half the operand bytes."""
    d = drop if drop is not None else Drop(0.0, 0, None)
    nt = (T + FLASH_TILE - 1) // FLASH_TILE
    lo, hi = (0, nt) if tiles is None else tiles
    if kvq_b is not None:
        _lib.check(_lib.lib().satt_flash_attn_bwd_tiles_b(
            _p(kvq_b), _p(kvq_b[:, D:]), _p(kvq_b[:, 2 * D:]), _ld(kvq_b), _p(o), _p(do), _ld(o), _p(do_b), _ld(do_b), _p(lse),
            _p(delta), _p(dkvq), _p(dkvq[:, D:]), _p(dkvq[:, 2 * D:]), _ld(dkvq), B, T, H, D // H, scale, int(causal), d.thresh,
            d.scale, d.stream, _p(d.seed), lo, hi, int(with_delta), _s()), "flash_attn_bwd")
        return
    _lib.check(_lib.lib().satt_flash_attn_bwd_tiles(
        _p(kvq), _p(kvq[:, D:]), _p(kvq[:, 2 * D:]), _ld(kvq), _p(o), _p(do), _ld(o), _p(lse), _p(delta), _p(dkvq),
        _p(dkvq[:, D:]), _p(dkvq[:, 2 * D:]), _ld(dkvq), B, T, H, D // H, scale, int(causal), d.thresh, d.scale, d.stream,
        _p(d.seed), lo, hi, int(with_delta), _s()), "flash_attn_bwd")


def _u32arr(vals):
    return (C.c_uint32 * len(vals))(*vals)


def lstm_fwd(xg, Wh, lengths, ndir, B, T, H, training, zc, zh, seed, streams_c, streams_h, hout, gates, cnew,
             cstate, hstate):
    """satt_lstm_fwd: every even H <= 1024 (H <= 128: register-resident kernel, else streaming); SattError otherwise"""
    zct, _ = rate_thresh(zc if training else 0.0)
    zht, _ = rate_thresh(zh if training else 0.0)
    _lib.check(_lib.lib().satt_lstm_fwd(_p(xg), _p(Wh), _p(lengths), ndir, B, T, H, int(training), zc, zh, zct, zht,
                                        _p(seed), _u32arr(streams_c), _u32arr(streams_h), _p(hout), _ld(hout),
                                        _p(gates), _p(cnew), _p(cstate), _p(hstate), _s()), "lstm_fwd")


def lstm_bwd(dhout, WhT, lengths, ndir, B, T, H, training, zc, zh, seed, streams_c, streams_h, gates, cnew, cstate,
             dxg):
    """satt_lstm_bwd: H % 8 == 0, H <= 1024 (narrower than the forward, which takes every even H); SattError otherwise"""
    zct, _ = rate_thresh(zc if training else 0.0)
    zht, _ = rate_thresh(zh if training else 0.0)
    _lib.check(_lib.lib().satt_lstm_bwd(_p(dhout), _ld(dhout), _p(WhT), _p(lengths), ndir, B, T, H, int(training), zc,
                                        zh, zct, zht, _p(seed), _u32arr(streams_c), _u32arr(streams_h), _p(gates),
                                        _p(cnew), _p(cstate), _p(dxg), _s()), "lstm_bwd")


def lstm_cluster_size(B, H, T=1):
    """workgroups per sample for the register-resident cluster LSTM (0: not applicable -> single-workgroup kernel)."""
    l = _lib.lib()
    for Cn in (4, 8, 2):
        if l.satt_lstm_cluster_check(B, T, H, Cn) == 0:
            rs = [lstm_cluster_residency(B, T, H, Cn, bw) for bw in (False, True)]
            if all(r is None or r[0] <= r[1] * r[2] for r in rs):    # every workgroup of either launch can be resident (None: no device)
                return Cn
    return 0


def lstm_cluster_residency(B, T, H, Cn, backward=False):
    """(workgroups, workgroups per CU, CUs) of a cluster LSTM launch on the current device (satt_lstm_cluster_residency: the
    occupancy calculator's answer for the kernel), or None without a device"""
    n, per, cus = C.c_int(0), C.c_int(0), C.c_int(0)
    if _lib.lib().satt_lstm_cluster_residency(B, T, H, Cn, int(backward), C.byref(n), C.byref(per), C.byref(cus)) != 0:
        return None
    return n.value, per.value, cus.value


def lstm_cluster_ws(B, H, Cn, device):
    """exchange workspace, ZERO-filled: launches clear the granules only, the 64-byte tail (error word, exchange-path
    counters) is sticky until the owner zeroes it again"""
    return torch.zeros(_lib.lib().satt_lstm_cluster_ws_bytes(B, H, Cn), dtype=torch.uint8, device=device)


def cluster_err_word(ws):
    """device pointer of a cluster workspace's sticky error word (adam_step's err arguments)"""
    return ws.data_ptr() + ws.numel() - 64


def lstm_cluster_pack(Wh, H, Cn):
    """register-order bf16 packs (forward, backward) of the fp32 recurrent weights Wh [H, 4H] for cluster size Cn."""
    l = _lib.lib()
    n = l.satt_lstm_cluster_pack_elems(Cn)
    pf = torch.empty(n, dtype=torch.bfloat16, device=Wh.device)
    pb = torch.empty(n, dtype=torch.bfloat16, device=Wh.device)
    _lib.check(l.satt_lstm_cluster_pack(_p(Wh), _ld(Wh), H, Cn, _p(pf), _p(pb), _s()), "lstm_cluster_pack")
    return pf, pb


def lstm_cluster_fwd(xg, Wh, B, T, H, Cn, training, zc, zh, seed, stream_c, stream_h, hout, gates, cnew, cstate, hstate,
                     ws, t0=0, t1=None):
    zct, _ = rate_thresh(zc if training else 0.0)
    zht, _ = rate_thresh(zh if training else 0.0)
    _lib.check(_lib.lib().satt_lstm_cluster_fwd(_p(xg), _p(Wh), B, T, H, Cn, int(training), zc, zh, zct, zht, _p(seed),
                                                stream_c, stream_h, _p(hout), _ld(hout), _p(gates), _p(cnew),
                                                _p(cstate), _p(hstate), _p(ws), t0, T if t1 is None else t1, _s()),
               "lstm_cluster_fwd")


LSTM_CLUSTER_FUSED_KMAX = 544     # input width up to which satt_lstm_cluster_fwd_x forms the input projection itself


def lstm_cluster_pack_in(Win, H, Cn):
    """register-order bf16 pack of the fp32 INPUT weights Win [K, 4H] (a row view of the layer's weight matrix) for the fused input
    projection of lstm_cluster_fwd(x=...), cluster size Cn"""
    l = _lib.lib()
    K = Win.shape[0]
    pk = torch.empty(l.satt_lstm_cluster_pack_in_elems(K, Cn), dtype=torch.bfloat16, device=Win.device)
    _lib.check(l.satt_lstm_cluster_pack_in(_p(Win), _ld(Win), K, H, Cn, _p(pk), _s()), "lstm_cluster_pack_in")
    return pk


def lstm_cluster_fwd_x(x, Kin, Win_pack, bias, xg, Wh, B, T, H, Cn, training, zc, zh, seed, stream_c, stream_h, hout, gates, cnew,
                       cstate, hstate, ws, t0=0, t1=None):
    """lstm_cluster_fwd whose launch first forms xg[:, t0:t1] = x[:, t0:t1, :Kin] Win + bias itself (bit-identical to ops.linear on
    the bf16 shadow; x: fp32 rows [B*T, ldx]) - for the short chunks at the end of the forward pipeline, where a GEMM launch of
    its own costs more than the product"""
    zct, _ = rate_thresh(zc if training else 0.0)
    zht, _ = rate_thresh(zh if training else 0.0)
    _lib.check(_lib.lib().satt_lstm_cluster_fwd_x(_p(xg), _p(Wh), B, T, H, Cn, int(training), zc, zh, zct, zht, _p(seed),
                                                  stream_c, stream_h, _p(hout), _ld(hout), _p(gates), _p(cnew),
                                                  _p(cstate), _p(hstate), _p(ws), t0, T if t1 is None else t1, _p(x), _ld(x),
                                                  int(Kin), _p(Win_pack), _p(bias), _s()),
               "lstm_cluster_fwd_x")


def lstm_cluster_bwd(dhout, WhT, B, T, H, Cn, training, zc, zh, seed, stream_c, stream_h, gates, cnew, cstate, dxg, ws,
                     t0=0, t1=None, bstate=None):
    zct, _ = rate_thresh(zc if training else 0.0)
    zht, _ = rate_thresh(zh if training else 0.0)
    _lib.check(_lib.lib().satt_lstm_cluster_bwd(_p(dhout), _ld(dhout), _p(WhT), B, T, H, Cn, int(training), zc, zh, zct,
                                                zht, _p(seed), stream_c, stream_h, _p(gates), _p(cnew), _p(cstate),
                                                _p(dxg), _p(ws), t0, T if t1 is None else t1, _p(bstate), _s()),
               "lstm_cluster_bwd")


def lstm_cluster_status(ws, B, H, Cn):
    _lib.check(_lib.lib().satt_lstm_cluster_status(_p(ws), B, H, Cn, _s()), "lstm cluster hand-off timeout")


def attn_rnn_params(**kw):
    p = _lib.AttnRnnParams()
    for k, v in kw.items():
        if isinstance(v, torch.Tensor):
            v = v.data_ptr()
        setattr(p, k, v)
    return p


def attn_rnn_fwd(p):
    _lib.check(_lib.lib().satt_attn_rnn_fwd(C.byref(p), _s()), "attn_rnn_fwd")


def attn_rnn_bwd(fwd_params, **kw):
    pb = _lib.AttnRnnBwdParams()
    pb.f = fwd_params
    for k, v in kw.items():
        if isinstance(v, torch.Tensor):
            v = v.data_ptr()
        setattr(pb, k, v)
    _lib.check(_lib.lib().satt_attn_rnn_bwd(C.byref(pb), _s()), "attn_rnn_bwd")


def attn_rnn_accepts(fwd_params):
    """True if the single-workgroup attention kernels take this problem (satt_attn_rnn_check: host-only, no launch)"""
    return _lib.lib().satt_attn_rnn_check(C.byref(fwd_params)) == 0


ATTN_CLUSTER_SIZES = (4, 8, 2)  # candidate workgroups per sample in order of preference (B * C <= 256; 4 leaves
                                # half of the CUs to the LSTM kernels that run concurrently on the other streams)


def attn_cluster_size(fwd_params):
    """workgroups per sample for the cluster attention kernels (0 -> single-workgroup kernels): the largest candidate
    the library accepts for this problem (satt_attn_cluster_check: sizes, register-resident slice, LDS, residency)."""
    l = _lib.lib()
    for Cn in ATTN_CLUSTER_SIZES:
        if l.satt_attn_cluster_check(C.byref(fwd_params), Cn) == 0:
            rs = [attn_cluster_residency(fwd_params, Cn, bw) for bw in (False, True)]
            if all(r is None or r[0] <= r[1] * r[2] for r in rs):    # every workgroup of either launch can be resident (None: no device)
                return Cn
    return 0


def attn_cluster_residency(fwd_params, Cn, backward=False, vw1=None, **kw):
    """(workgroups, workgroups per CU, CUs) of the launch attn_cluster_fwd / attn_cluster_bwd would make (same kernel selection,
    same LDS size: satt_attn_cluster_residency / _bwd_residency), or None without a device.  kw: fields of the backward
    parameter block that select the kernel (saf comes with fwd_params)."""
    n, per, cus = C.c_int(0), C.c_int(0), C.c_int(0)
    if backward:
        cb = _lib.AttnClusterBwdParams()
        cb.b.f = fwd_params; cb.C = Cn
        rc = _lib.lib().satt_attn_cluster_bwd_residency(C.byref(cb), C.byref(n), C.byref(per), C.byref(cus))
    else:
        cp = _lib.AttnClusterParams()
        cp.f = fwd_params; cp.C = Cn; cp.vw1 = _p(vw1)
        rc = _lib.lib().satt_attn_cluster_residency(C.byref(cp), C.byref(n), C.byref(per), C.byref(cus))
    if rc != 0:
        return None
    return n.value, per.value, cus.value


def attn_cluster_pack(Wrec, A, Cn):
    """per-member bf16 slices of Wrec [K, 4A] (fp32 view): (WrecP in MFMA operand order, WrecTP [C,4A,nwp])."""
    K = Wrec.shape[0]
    l = _lib.lib()
    wp = torch.empty(l.satt_attn_cluster_pack_elems(K, A, Cn, 0), dtype=torch.bfloat16, device=Wrec.device)
    wtp = torch.empty(l.satt_attn_cluster_pack_elems(K, A, Cn, 1), dtype=torch.bfloat16, device=Wrec.device)
    _lib.check(l.satt_attn_cluster_pack(_p(Wrec), _ld(Wrec), _p(wp), _p(wtp), K, A, Cn, _s()), "attn_cluster_pack")
    return wp, wtp


def attn_cluster_ws(fwd_params, Cn, device):
    """exchange workspace, zero-filled (see lstm_cluster_ws)"""
    return torch.zeros(_lib.lib().satt_attn_cluster_ws_bytes(C.byref(fwd_params), Cn), dtype=torch.uint8,
                       device=device)


def attn_cluster_state(fwd_params, Cn, device):
    return torch.empty(_lib.lib().satt_attn_cluster_state_floats(C.byref(fwd_params), Cn), dtype=torch.float32,
                       device=device)


def attn_cluster_fold(fwd_params, Cn):
    """True if the folded form of the forward attention kernel exists for this problem (csrc/attn_cluster.hip, FOLD)"""
    return bool(_lib.lib().satt_attn_cluster_fold(C.byref(fwd_params), Cn))


def attn_cluster_fwd(fwd_params, Cn, WrecP, ws, t0=0, t1=None, progress=None, bounds=(), vw1=None):
    """progress (int32 device tensor, zeroed by the caller) + bounds (chunk end steps): the launch spans several pipeline
    chunks and signals the end of each one - consumers wait with stream_wait_value(progress, (k+1) * B * Cn)"""
    cp = _lib.AttnClusterParams()
    cp.f = fwd_params; cp.C = Cn; cp.WrecP = _p(WrecP); cp.ws = _p(ws)
    cp.t0 = t0; cp.t1 = fwd_params.Td if t1 is None else t1
    cp.vw1 = _p(vw1)
    cp.progress = _p(progress); cp.nbound = len(bounds) if progress is not None else 0
    for i, bnd in enumerate(bounds):
        cp.bound[i] = bnd
    _lib.check(_lib.lib().satt_attn_cluster_fwd(C.byref(cp), _s()), "attn_cluster_fwd")


_hip = None


def _hiprt():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipStreamWaitValue32.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint, C.c_uint32]
        _hip.hipStreamWaitValue32.restype = C.c_int
        _hip.hipStreamWriteValue32.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint]
        _hip.hipStreamWriteValue32.restype = C.c_int
    return _hip


def stream_wait_value(counter, value, stream=None):
    """the stream (default: current) does not run later work until *counter >= value (hipStreamWaitValue32, GTE): the
    producer/consumer edge between a RUNNING persistent kernel that counts its finished chunks and the next layer"""
    st = stream.cuda_stream if stream is not None else _s()
    rc = _hiprt().hipStreamWaitValue32(st, counter.data_ptr(), int(value), 0, 0xFFFFFFFF)
    if rc:
        raise _lib.SattError("hipStreamWaitValue32 failed (%d)" % rc)


def stream_write_value(counter, value, stream=None):
    st = stream.cuda_stream if stream is not None else _s()
    rc = _hiprt().hipStreamWriteValue32(st, counter.data_ptr(), int(value), 0)
    if rc:
        raise _lib.SattError("hipStreamWriteValue32 failed (%d)" % rc)


def attn_cluster_bwd(fwd_params, Cn, WrecTP, ws, t0=0, t1=None, state=None, ready=None, done=None, bounds=(), **kw):
    """ready / done (int32 device words, zeroed by the caller) + bounds (first step of every chunk in processing order,
    i.e. descending): one launch over several pipeline chunks, see satt_attn_cluster_bwd_params"""
    cb = _lib.AttnClusterBwdParams()
    cb.b.f = fwd_params
    cb.t0 = t0; cb.t1 = fwd_params.Td if t1 is None else t1; cb.state = _p(state)
    cb.ready = _p(ready); cb.done = _p(done); cb.nbound = len(bounds) if ready is not None else 0
    for i, bnd in enumerate(bounds):
        cb.bound[i] = bnd
    for k, v in kw.items():
        if isinstance(v, torch.Tensor):
            v = v.data_ptr()
        setattr(cb.b, k, v)
    cb.C = Cn; cb.WrecTP = _p(WrecTP); cb.ws = _p(ws)
    _lib.check(_lib.lib().satt_attn_cluster_bwd(C.byref(cb), _s()), "attn_cluster_bwd")


def attn_cluster_status(fwd_params, Cn, ws):
    _lib.check(_lib.lib().satt_attn_cluster_status(C.byref(fwd_params), Cn, _p(ws), _s()),
               "attention cluster hand-off timeout")


def attn_cluster_fastpath(fwd_params, Cn, ws):
    """(fast, slow): workgroup-launches on ws since it was zeroed that exchanged through same-XCD plain stores / through
    write-through stores (host-synchronous; tests)"""
    n, m = C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().satt_attn_cluster_fastpath(C.byref(fwd_params), Cn, _p(ws), _s(), C.byref(n), C.byref(m)), "fastpath")
    return n.value, m.value


def lstm_cluster_fastpath(ws, B, H, Cn):
    n, m = C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().satt_lstm_cluster_fastpath(_p(ws), B, H, Cn, _s(), C.byref(n), C.byref(m)), "fastpath")
    return n.value, m.value


def attn_param_grads(fwd_params, de1, de2, dkeys1, dkeys2, dv1, db1, dlocU, dv2, t0=None, t1=None, accumulate=False,
                     lds_pad=0):
    """deferred attention gradients of the steps [t0, t1) (default: all); accumulate adds into dkeys1/2."""
    t0 = 0 if t0 is None else t0
    t1 = fwd_params.Td if t1 is None else t1
    _lib.check(_lib.lib().satt_attn_param_grads_range(C.byref(fwd_params), _p(de1), _p(de2), _p(dkeys1), _p(dkeys2),
                                                      _p(dv1), _p(db1), _p(dlocU), _p(dv2), t0, t1, int(accumulate),
                                                      int(lds_pad), _s()), "attn_param_grads")


def attn_param_grads_acc_doubles(fwd_params):
    """float64 elements satt_attn_param_grads_acc needs for this problem (one slot per workgroup of its fixed grid)"""
    return int(_lib.lib().satt_attn_param_grads_acc_doubles(C.byref(fwd_params)))


def attn_param_grads_acc_buffer(fwd_params, device):
    """float64 workgroup slots of the deferred attention gradients (saved-factor path) for THIS problem size (B, Ti)"""
    return torch.zeros(_lib.lib().satt_attn_param_grads_acc_doubles(C.byref(fwd_params)), dtype=torch.float64, device=device)


def attn_param_grads_acc(fwd_params, de1, de2, dkeys1, dkeys2, acc, t0=None, t1=None, accumulate=False, lds_pad=0):
    t0 = 0 if t0 is None else t0
    t1 = fwd_params.Td if t1 is None else t1
    _lib.check(_lib.lib().satt_attn_param_grads_acc(C.byref(fwd_params), _p(de1), _p(de2), _p(dkeys1), _p(dkeys2), _p(acc), t0, t1,
                                                    int(accumulate), int(lds_pad), _s()), "attn_param_grads_acc")


def attn_param_grads_finish(fwd_params, acc, dv1, db1, dlocU, dv2):
    _lib.check(_lib.lib().satt_attn_param_grads_finish(C.byref(fwd_params), _p(acc), _p(dv1), _p(db1), _p(dlocU), _p(dv2), _s()),
               "attn_param_grads_finish")


def loss_fwd_bwd(mel, mel_ld, target, spec_mask, stop, stop_ld, done, bin_mask, B, Tm, nm, Td, l2, losses, dmel,
                 dmel_ld, dstop, dstop_ld, ws):
    _lib.check(_lib.lib().satt_loss_fwd_bwd(_p(mel), mel_ld, _p(target), _p(spec_mask), _p(stop), stop_ld, _p(done),
                                            _p(bin_mask), B, Tm, nm, Td, int(l2), _p(losses), _p(dmel), dmel_ld,
                                            _p(dstop), dstop_ld, _p(ws), _s()), "loss_fwd_bwd")


def loss_mask_sums(spec_mask, bin_mask, B, Tm, Td, ws):
    """mask sums of the batch into ws (8 floats) + reset of its accumulators: call any time before loss_fwd_bwd_presummed"""
    _lib.check(_lib.lib().satt_loss_mask_sums(_p(spec_mask), _p(bin_mask), B, Tm, Td, _p(ws), _s()), "loss_mask_sums")


def loss_fwd_bwd_presummed(mel, mel_ld, target, spec_mask, stop, stop_ld, done, bin_mask, B, Tm, nm, Td, l2, losses, dmel,
                           dmel_ld, dstop, dstop_ld, ws):
    _lib.check(_lib.lib().satt_loss_fwd_bwd_presummed(_p(mel), mel_ld, _p(target), _p(spec_mask), _p(stop), stop_ld, _p(done),
                                                      _p(bin_mask), B, Tm, nm, Td, int(l2), _p(losses), _p(dmel), dmel_ld,
                                                      _p(dstop), dstop_ld, _p(ws), _s()), "loss_fwd_bwd_presummed")


def opt_state(device):
    """optimiser scratch {sumsq, norm, lr_t, scale, per-block partials} for sumsq / adam_step"""
    return torch.zeros(_lib.lib().satt_sumsq_state_floats(), dtype=torch.float32, device=device)


def sumsq(g, state):
    _lib.check(_lib.lib().satt_sumsq(_p(g), g.numel(), _p(state), _s()))


def adam_step(p, g, m, v, state, step_dev, seed_dev, lr0, decay, step_factor, b1, b2, eps, clip, grad_scale, err_words=()):
    """err_words: up to three device pointers (cluster_err_word) - the update is skipped on the device if any is set"""
    e = (list(err_words) + [None, None, None])[:3]
    _lib.check(_lib.lib().satt_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(state), _p(step_dev),
                                         _p(seed_dev), lr0, int(decay), step_factor, b1, b2, eps, clip, grad_scale,
                                         e[0], e[1], e[2], _s()), "adam_step")


def poison_on_error(g, err_words=()):
    """data-parallel guard: g[0] = NaN if any cluster error word is set (call on a bucket's first element before its all-reduce)"""
    e = (list(err_words) + [None, None, None])[:3]
    _lib.check(_lib.lib().satt_poison_on_error(_p(g), e[0], e[1], e[2], _s()), "poison_on_error")


_probe_cache = {}


def streams_run_concurrently(main, other, spins=40000):
    """True if a kernel launched on `other` AFTER a kernel was launched on `main` runs while that kernel is still
    running (the two streams do not share a hardware queue and nothing - e.g. a counter-collecting profiler -
    serialises kernels).  One-off probe per stream pair, ~0.1 ms (60 ms when it fails)."""
    key = (main.cuda_stream, other.cuda_stream)
    if key[0] == key[1]:
        return False
    if key not in _probe_cache:
        buf = torch.zeros(2, dtype=torch.int32, device=main.device)
        torch.cuda.synchronize(main.device)
        _lib.check(_lib.lib().satt_stream_probe(buf[0:1].data_ptr(), buf[1:2].data_ptr(), int(spins), main.cuda_stream,
                                                other.cuda_stream), "stream_probe")
        torch.cuda.synchronize(main.device)
        _probe_cache[key] = bool(int(buf[1]) == 1)
    return _probe_cache[key]


# ---------------------------------------------------------------------- autoregressive decode step (csrc/decode.hip)
def dec_linear_params(xs, W, y, *, bias=None, act=ACT_NONE, res=None, step=None, B=None, lstm=None, step_out=None,
                      stop=None, drop=None, drop_T=0):
    """y = act([x0 | x1 | x2] W + bias) + res.  xs: list of (tensor, features, batch_stride, step_stride[, parity_stride]);
    y / res: (tensor, batch_stride, step_stride); W: fp32 [K, N] view or ops.Weight (bf16 plain-cast shadow in bf16 mode).
    lstm=(H, c_state, h_state, zc, zh): LSTM form - W yields the gates and the ZoneoutLSTMCell runs in the epilogue on the
    [2, B, H] states (double-buffered by step parity); y receives the pre-zoneout cell output.
    step_out=(counter, add): workgroup (0,0) publishes *step + add into `counter` (a word this launch does not read);
    stop=(logits, batch_stride, step_stride, flag, threshold, min_steps): it also evaluates the previous step's stop rule.
    drop (a Drop) / drop_T: dropout that stays on while synthesising (apply_dropout_on_inference) - the training kernels' mask
    over a [B, drop_T, N] activation, row (b, *step).
    Returns the filled parameter block (kept by the caller: the tensors it points to must stay alive)."""
    p = _lib.DecLinearParams()
    w, _, wn = _wsplit(W)
    p.B = int(B)
    p.N = int(w.shape[1])
    p.nseg = len(xs)
    for s, xd in enumerate(xs):
        t, k, bs, ss = xd[:4]
        p.x[s] = t.data_ptr(); p.k[s] = int(k); p.x_bs[s] = int(bs); p.x_ss[s] = int(ss)
        p.x_ps[s] = int(xd[4]) if len(xd) > 4 else 0
    if sum(int(xd[1]) for xd in xs) != w.shape[0]:
        raise _lib.SattError("dec_linear: input segments do not add up to the rows of W")
    if w.dtype == torch.bfloat16:                      # a caller-built bf16 matrix
        p.Wb = w.data_ptr(); p.ldw = int(w.stride(0))
    elif _state["prec"] == PREC_BF16 and wn is not None:
        p.Wb = wn.data_ptr(); p.ldw = int(wn.stride(0))
    else:
        p.W = w.data_ptr(); p.ldw = int(w.stride(0))
    p.bias = _p(bias)
    p.act = int(act)
    if res is not None:
        p.res = res[0].data_ptr(); p.res_bs = int(res[1]); p.res_ss = int(res[2])
    p.y = y[0].data_ptr(); p.y_bs = int(y[1]); p.y_ss = int(y[2])
    p.step = _p(step)
    if step_out is not None:
        p.step_out = step_out[0].data_ptr(); p.step_add = int(step_out[1])
    if stop is not None:
        p.stop = stop[0].data_ptr(); p.stop_bs = int(stop[1]); p.stop_ss = int(stop[2]); p.flag = stop[3].data_ptr()
        p.stop_threshold = float(stop[4]); p.min_steps = int(stop[5])
    if lstm is not None:
        p.lstm_H = int(lstm[0]); p.c_state = lstm[1].data_ptr(); p.h_state = lstm[2].data_ptr()
        p.zc = float(lstm[3]); p.zh = float(lstm[4])
    if drop is not None and drop.thresh:
        p.drop_thresh, p.drop_scale, p.drop_stream, p.drop_seed, p.drop_T = drop.thresh, drop.scale, drop.stream, _p(drop.seed), int(drop_T)
    return p


def dec_linear(p):
    _lib.check(_lib.lib().satt_dec_linear(C.byref(p), _s()), "dec_linear")


def dec_linear2(pa, pb):
    """two plain Dense layers in one launch; returns False (nothing launched) if the pair does not fit the fused kernel"""
    rc = _lib.lib().satt_dec_linear2(C.byref(pa), C.byref(pb), _s())
    if rc == -2:        # SATT_E_UNSUPPORTED
        return False
    _lib.check(rc, "dec_linear2")
    return True


def dec_linear_chain(pre, main):
    """pre (1 or 2 DecLinearParams) -> main in one launch; returns False (nothing launched) if the chain does not fit"""
    arr = (_lib.DecLinearParams * len(pre))(*pre)
    rc = _lib.lib().satt_dec_linear_chain(arr, len(pre), C.byref(main), _s())
    if rc == -2:        # SATT_E_UNSUPPORTED
        return False
    _lib.check(rc, "dec_linear_chain")
    return True


def dec_attention_params(**kw):
    p = _lib.DecAttentionParams()
    for k, v in kw.items():
        if isinstance(v, torch.Tensor):
            v = v.data_ptr()
        setattr(p, k, v)
    return p


def dec_attention(p):
    _lib.check(_lib.lib().satt_dec_attention(C.byref(p), _s()), "dec_attention")


def dec_mega_params(**kw):
    """parameter block of the persistent decode step (satt_dec_mega_params); tensors are passed as their device pointers"""
    p = _lib.DecMegaParams()
    for k, v in kw.items():
        if isinstance(v, torch.Tensor):
            v = v.data_ptr()
        setattr(p, k, v)
    return p


def dec_mega_supported(p):
    return bool(_lib.lib().satt_dec_mega_supported(C.byref(p)))


MEGA_VAR_TABLES_LDS, MEGA_VAR_LJ, MEGA_VAR_SPEAKER, MEGA_VAR_TWO_SAMPLES = 1, 2, 4, 8      # include/satt_hip.h: SATT_MEGA_VAR_*


def dec_mega_variant(p):
    """the instantiation of the persistent kernel a launch of `p` takes: an OR of MEGA_VAR_*, -1 where the kernel does not take it"""
    return int(_lib.lib().satt_dec_mega_variant(C.byref(p)))


def dec_mega_scratch_floats(B, heads, hd):
    return int(_lib.lib().satt_dec_mega_scratch_floats(B, heads, hd))


def dec_mega(p, nsteps):
    """`nsteps` whole decoder steps in ONE launch (csrc/decode_mega2.hip)"""
    p.nsteps = int(nsteps)
    _lib.check(_lib.lib().satt_dec_mega(C.byref(p), _s()), "dec_mega")


MEGA_VAR_AGENT, MEGA_VAR_DROPOUT = 16, 32      # include/satt_hip.h: SATT_MEGA_VAR_* of the option block
MEGA_VAR_SINGLE = 64                           # the single-source form (the baseline model)


def dec_mega_opt_params(agentW=None, agentb=None, agent_tab=None, u_state=None, drop=None, drop_T=0, drop_streams=(0, 0)):
    """option block of the persistent decode step (satt_dec_mega_opt_params).  agentW .. u_state: the transition agent (None: off);
    drop (a Drop: rate and the session's seed word; its stream is not used) / drop_T / drop_streams: pre-net dropout that stays on -
    dec_linear_params' mask, per pre-net layer its own stream."""
    o = _lib.DecMegaOptParams()
    ptr = lambda v: v.data_ptr() if isinstance(v, torch.Tensor) else v          # (tensors, or addresses as dec_mega_params takes them)
    o.agentW, o.agentb, o.agent_tab, o.u_state = ptr(agentW), ptr(agentb), ptr(agent_tab), ptr(u_state)
    if drop is not None and drop.thresh:
        o.drop_thresh, o.drop_scale, o.drop_seed, o.drop_T = drop.thresh, drop.scale, ptr(drop.seed), int(drop_T)
        o.drop_stream[0], o.drop_stream[1] = int(drop_streams[0]), int(drop_streams[1])
    return o


def dec_mega_opt_variant(p, opt):
    """dec_mega_variant of a launch with the option block `opt` (None: without): plus MEGA_VAR_AGENT / MEGA_VAR_DROPOUT"""
    return int(_lib.lib().satt_dec_mega_opt_variant(C.byref(p), None if opt is None else C.byref(opt)))


def dec_mega_opt(p, opt, nsteps):
    """dec_mega with the option block `opt`"""
    p.nsteps = int(nsteps)
    _lib.check(_lib.lib().satt_dec_mega_opt(C.byref(p), None if opt is None else C.byref(opt), _s()), "dec_mega_opt")


MEGA_VAR_FORCED = 256                          # forced alignments (satt_dec_mega_forced): the generic-width instantiations only


def dec_mega_forced_params(teach1, teach2=None):
    """teacher alignments of a forced launch (satt_dec_mega_forced_params): [B][Td][Ti] fp32 with the Td of the main block; teach2
    None in the single-source form"""
    f = _lib.DecMegaForcedParams()
    ptr = lambda v: v.data_ptr() if isinstance(v, torch.Tensor) else v
    f.teach1, f.teach2 = ptr(teach1), ptr(teach2)
    return f


def dec_mega_forced_variant(p, opt, f):
    """dec_mega_opt_variant of a launch with the teacher alignments `f` (None: without): plus MEGA_VAR_FORCED, without MEGA_VAR_LJ"""
    return int(_lib.lib().satt_dec_mega_forced_variant(C.byref(p), None if opt is None else C.byref(opt), None if f is None else C.byref(f)))


def dec_mega_forced(p, opt, f, nsteps):
    """dec_mega_opt with forced alignments: the mechanisms are bypassed, row t of `f` is the alignment of step t"""
    p.nsteps = int(nsteps)
    _lib.check(_lib.lib().satt_dec_mega_forced(C.byref(p), None if opt is None else C.byref(opt), None if f is None else C.byref(f), _s()),
               "dec_mega_forced")


MEGA_VAR_GROUPS = 128                          # group mode: one pair of samples per XCD (satt_dec_mega_groups)
MEGA_GROUPS_MAX = 8


def dec_mega_groups_blocks(blocks):
    """host array of satt_dec_mega_group from (params, option block or None, b0) triples - copies: the array is self-contained"""
    arr = (_lib.DecMegaGroup * len(blocks))()
    for g, (p, o, b0) in zip(arr, blocks):
        C.memmove(C.byref(g.p), C.byref(p), C.sizeof(p))
        if o is not None:
            C.memmove(C.byref(g.o), C.byref(o), C.sizeof(o))
        g.has_opt, g.b0 = int(o is not None), int(b0)
    return arr


def dec_mega_groups_supported(arr):
    return bool(_lib.lib().satt_dec_mega_groups_supported(arr, len(arr)))


def dec_mega_groups_variant(arr):
    """the instantiation a group launch of `arr` takes: the blocks' MEGA_VAR_* bits | MEGA_VAR_GROUPS, -1 where it is not taken"""
    return int(_lib.lib().satt_dec_mega_groups_variant(arr, len(arr)))


def dec_mega_groups_scratch_floats(ngroups, heads, hd):
    return int(_lib.lib().satt_dec_mega_groups_scratch_floats(ngroups, heads, hd))


def dec_mega_groups_device(arr, device):
    """the device copy of a host array of group blocks (the kernel reads its blocks from device memory)"""
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return raw.to(device)


def dec_mega_groups(arr, dev_blocks):
    """the blocks' nsteps decoder steps of up to eight pairs of samples in ONE launch (csrc/decode_mega2.hip, group mode)"""
    _lib.check(_lib.lib().satt_dec_mega_groups(arr, _p(dev_blocks), len(arr), _s()), "dec_mega_groups")


def dec_mega_groups_forced_variant(arr, f):
    """dec_mega_groups_variant of a launch with the batch's teacher alignments `f` (None: without): plus MEGA_VAR_FORCED, without
    MEGA_VAR_LJ"""
    return int(_lib.lib().satt_dec_mega_groups_forced_variant(arr, len(arr), None if f is None else C.byref(f)))


def dec_mega_groups_forced(arr, dev_blocks, f):
    """dec_mega_groups with forced alignments: `f` holds the teacher rows of the whole (padded) batch, [2 len(arr)][Td][Ti]; group g
    reads batch rows b0, b0 + 1"""
    _lib.check(_lib.lib().satt_dec_mega_groups_forced(arr, _p(dev_blocks), len(arr), None if f is None else C.byref(f), _s()),
               "dec_mega_groups_forced")


def dec_stop_scan(yout, B, rows, NO, t0, nsteps, min_steps, stop_threshold, flag):
    """stop rule of the batch over the steps t0 .. t0 + nsteps - 1 of yout [B][rows][NO] (row t + 1 = step t): *flag = t + 1"""
    _lib.check(_lib.lib().satt_dec_stop_scan(_p(yout), int(B), int(rows), int(NO), int(t0), int(nsteps), int(min_steps),
                                             float(stop_threshold), _p(flag), _s()), "dec_stop_scan")


def dec_ends_scan(yout, B, rows, NO, t0, nsteps, min_steps, stop_threshold, ends, flag):
    """per-utterance stop over the steps t0 .. t0 + nsteps - 1 of yout [B][rows][NO]: ends[b] = t_b + 1 at sample b's first
    qualifying step (sticky, int32 [B]); *flag = max(ends) once every sample has ended"""
    _lib.check(_lib.lib().satt_dec_ends_scan(_p(yout), int(B), int(rows), int(NO), int(t0), int(nsteps), int(min_steps),
                                             float(stop_threshold), _p(ends), _p(flag), _s()), "dec_ends_scan")


def dec_self_attn(kvq, out, step, B, Td, D, heads, scale):
    _lib.check(_lib.lib().satt_dec_self_attn(_p(kvq), _p(out), _p(step), B, Td, D, heads, float(scale), _s()), "dec_self_attn")


def l2_reg(w, g, table, nseg, scale, reg, total=None):
    """g += scale * w and reg (+ total) += scale * sum(w^2) / 2 over the (offset, count) segments of `table`"""
    _lib.check(_lib.lib().satt_l2_reg(_p(w), _p(g), _p(table), int(nseg), float(scale), _p(reg), _p(total), _s()), "l2_reg")
