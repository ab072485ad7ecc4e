"""csrc/yin.hip satt_yin_candidates and csrc/f0_viterbi.hip against the float32 NumPy backend of utils/pitch.py (every output equal
bit for bit), their batching guarantees, what they leave untouched (poisoned outputs, bad offset tables), non-finite samples, LDS
poison, the trap signal end to end and evaluate_f0.py --tracker viterbi on the hip backend."""
import os

import numpy as np
import pytest
import torch

import audio_common as ac
import f0_viterbi_common as fc
import satt_amd  # noqa: F401
from satt_amd import _lib, ops
from satt_amd.utils import audio, pitch

pytestmark = pytest.mark.gpu

DEV = "cuda"
K = fc.K
POISON = -77.25
POISON_BYTE = 0xA5
# (sr, hop, keyword arguments): 1 chunk of lags (tau_max 134), 2 (267 and 368), 4 (800 and 1022, the longest but one)
CONFIGS = [(8000, 100, {}), (16000, 200, {}), (22050, 275, {}), (48000, 600, dict(fmin=60.0)), (48000, 600, dict(fmin=47.0))]
COSTS = (0.3, 0.1, 0.15, 0.1)


def signal(sr, n, seed):
    """as test_yin_gpu.signal: a gliding harmonic tone behind a tenth of noise; every sample its own value"""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    f = (90.0 + 15.0 * seed) * (1.0 + 0.5 * k / sr)
    ph = 2.0 * np.pi * np.cumsum(f) / sr
    y = sum(0.4 / h * np.sin(h * ph + h) for h in (1, 2, 3)) + 2e-3 * rng.standard_normal(n)
    y[:n // 10] = 3e-3 * rng.standard_normal(n // 10)
    return y.astype(np.float32)


_REF = {}


def cand_reference(y, sr, hop, **kw):
    """the NumPy candidates of a signal, computed once"""
    key = (y.tobytes(), sr, hop, tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = pitch.yin_candidates_numpy(y, sr, hop, **kw)
    return _REF[key]


def dev(v, dt):
    return torch.as_tensor(np.ascontiguousarray(v), dtype=dt).to(DEV)


def cand_raw(x, io, fo, sr, hop, total_frames=None, tail=0, **kw):
    """one launch on poisoned outputs, the offset tables as given: cand_period, cand_value [total + tail, 8], power [total + tail]"""
    W, tau_min, tau_max = pitch.yin_sizes(sr, **kw)
    total = int(fo[-1]) if total_frames is None else total_frames
    per, val = (torch.full((total + tail, K), POISON, dtype=torch.float32, device=DEV) for _ in range(2))
    pw = torch.full((total + tail,), POISON, dtype=torch.float32, device=DEV)
    ops.yin_candidates(dev(x, torch.float32), dev(io, torch.int64), dev(fo, torch.int64), W, tau_min, tau_max, hop, per[:total], val[:total], pw[:total])
    torch.cuda.synchronize()
    return [b.cpu().numpy() for b in (per, val, pw)]


def cand_launch(signals, sr, hop, tail=0, **kw):
    lens = np.asarray([len(s) for s in signals], np.int64)
    io = np.concatenate([[0], np.cumsum(lens)])
    fo = np.concatenate([[0], np.cumsum(1 + lens // hop)])
    raw = cand_raw(np.concatenate(signals), io, fo, sr, hop, tail=tail, **kw)
    return [tuple(b[fo[u]:fo[u + 1]] for b in raw) for u in range(len(signals))], raw, fo


def same(got, want, nan_ok=False):
    if nan_ok:
        return all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want))
    return all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def dip_counts(y, sr, hop, **kw):
    _, tau_min, tau_max = pitch.yin_sizes(sr, **kw)
    dp, _ = pitch.yin_dprime_numpy(y, sr, hop, **kw)
    mid = dp[:, tau_min:tau_max]
    return ((mid < dp[:, tau_min - 1:tau_max - 1]) & (mid <= dp[:, tau_min + 1:tau_max + 1])).sum(axis=1)


# ---- the candidates kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,hop,kw", CONFIGS, ids=lambda v: str(v) if not isinstance(v, dict) else "_".join("%s%g" % i for i in v.items()))
def test_candidates_equal_the_numpy_backend(sr, hop, kw):
    assert (pitch.yin_sizes(sr, **kw)[2] + 256) // 256 == {134: 1, 267: 2, 368: 2, 800: 4, 1022: 4}[pitch.yin_sizes(sr, **kw)[2]]
    ns = [1, hop - 1, hop, 16 * hop - 1, 16 * hop + 1]                                   # 1, 1, 2, 16 and 17 frames: the workgroup seam
    ys = [signal(sr, n, i) for i, n in enumerate(ns)]
    refs = [cand_reference(y, sr, hop, **kw) for y in ys]
    res, _, _ = cand_launch(ys, sr, hop, **kw)                                          # the mixed batch of 5
    for n, y, got, want in zip(ns, ys, res, refs):
        assert got[0].shape == (1 + n // hop, K) and same(got, want), (sr, n)
    alone, _, _ = cand_launch([ys[4]], sr, hop, **kw)
    assert same(alone[0], refs[4])
    assert sum(int((w[0] > 0).sum()) for w in refs) >= 20


def test_frames_with_no_one_eight_and_more_dips():
    sr, hop = 16000, 200
    k = np.arange(4000)
    ys = [np.zeros(1000, np.float32), np.sin(2 * np.pi * k / 200.0).astype(np.float32), np.sin(2 * np.pi * k / 33.0).astype(np.float32),
          np.random.default_rng(1).standard_normal(4000).astype(np.float32)]
    counts = [dip_counts(y, sr, hop) for y in ys]
    assert np.all(counts[0] == 0) and (counts[1] == 1).sum() >= 5 and (counts[2] == 8).sum() >= 5 and (counts[3] > 8).sum() >= 5
    res, _, _ = cand_launch(ys, sr, hop)
    for y, got, c in zip(ys, res, counts):
        assert same(got, cand_reference(y, sr, hop)) and np.array_equal((got[0] > 0).sum(axis=1), np.minimum(c, K))


def test_nan_and_inf_samples():
    sr, hop = 16000, 200
    good = signal(sr, 3333, 3)
    bad = good.copy()
    bad[700], bad[1500], bad[2500] = np.nan, np.inf, -np.inf
    res, _, _ = cand_launch([bad, good, np.full(1000, np.nan, np.float32)], sr, hop)
    assert same(res[0], cand_reference(bad, sr, hop), nan_ok=True) and same(res[1], cand_reference(good, sr, hop))
    assert np.all(res[2][0] == 0) and np.all(res[2][1] == np.inf)                       # a frame of NaN samples has no dip
    touched = ~np.isfinite(res[0][2])                                                   # a NaN or Inf sample in the frame's window
    assert touched.sum() >= 3 and np.all(res[0][0][touched] == 0)
    out = pitch.track_f0([bad, good], sr, hop, tracker="viterbi", backend="hip", device=DEV)
    want = pitch.track_f0([bad, good], sr, hop, tracker="viterbi")
    assert all(same(o, w, nan_ok=True) for o, w in zip(out, want)) and not out[0][3][touched].any()


# ---- the Viterbi kernel --------------------------------------------------------------------------------------------------------------------
def vit_reference(seed, T, costs=COSTS):
    key = ("v", seed, T, costs)
    if key not in _REF:
        tab = fc.grid_table(seed, T)
        _REF[key] = (tab, pitch.f0_viterbi_numpy(*tab, 16000, 267, *costs))
    return _REF[key]


def vit_raw(tables, fo, total_frames=None, tail=0, costs=COSTS, max_frames=None):
    """one launch on poisoned outputs, the offset table as given: f0, state [total + tail], cost [U]"""
    per, val, gate = (np.concatenate([t[i] for t in tables]) for i in range(3))
    total = len(per) if total_frames is None else total_frames
    f0 = torch.full((total + tail,), POISON, dtype=torch.float32, device=DEV)
    state = torch.full((total + tail,), POISON_BYTE, dtype=torch.uint8, device=DEV)
    cost = torch.full((len(fo) - 1,), POISON, dtype=torch.float32, device=DEV)
    longest = max(len(t[0]) for t in tables) if max_frames is None else max_frames
    ops.f0_viterbi(dev(per[:total], torch.float32), dev(val[:total], torch.float32), dev(gate[:total], torch.uint8), dev(fo, torch.int64), longest,
                   267, 16000, *costs, f0[:total], state[:total], cost)
    torch.cuda.synchronize()
    return f0.cpu().numpy(), state.cpu().numpy(), cost.cpu().numpy()


def vit_launch(tables, tail=0, costs=COSTS):
    fo = np.concatenate([[0], np.cumsum([len(t[0]) for t in tables])])
    f0, state, cost = vit_raw(tables, fo, tail=tail, costs=costs)
    return [(f0[fo[u]:fo[u + 1]], state[fo[u]:fo[u + 1]], cost[u]) for u in range(len(tables))], (f0, state, cost), fo


def vit_same(got, want):
    return same(got[:2], want[:2]) and np.float32(got[2]).tobytes() == np.float32(want[2]).tobytes()


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 2047, 2048])
def test_viterbi_equals_the_numpy_backend(T):
    tab, want = vit_reference(T, T)
    res, _, _ = vit_launch([tab])
    assert len(res[0][0]) == T and vit_same(res[0], want)
    if T >= 63:
        assert len(set(want[1])) >= 4 and (want[1] < K).sum() >= 10 and (want[1] == K).sum() >= 3    # between slots, and unvoiced


def test_viterbi_mixed_batch_and_other_costs():
    Ts = [65, 1, 700, 32, 33, 2, 2048, 31]
    refs = [vit_reference(T, T) for T in Ts]
    res, raw, _ = vit_launch([tab for tab, _ in refs])
    again, raw2, _ = vit_launch([tab for tab, _ in refs])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(raw, raw2))                    # two launches: identical bits
    back, _, _ = vit_launch([tab for tab, _ in refs][::-1])
    for u, (_, want) in enumerate(refs):
        assert vit_same(res[u], want) and vit_same(back[len(Ts) - 1 - u], want), Ts[u]
    for costs in ((0.0, 0.0, 0.15, 0.1), (0.5, 0.25, 0.125, 0.0), (1.0, 0.0, 1.0, 0.5)):   # free jumps; a grid of 1/8: ties everywhere
        refs = [vit_reference(T, T, costs) for T in (65, 700)]
        res, _, _ = vit_launch([tab for tab, _ in refs], costs=costs)
        assert all(vit_same(r, want) for r, (_, want) in zip(res, refs)), costs


def test_viterbi_empty_slots_and_gated_frames():
    T = 130
    per, val, gate = fc.grid_table(9, T)
    empty = (np.zeros((T, K), np.float32), np.full((T, K), np.inf, np.float32), np.ones(T, np.uint8))
    closed = (per, val, np.zeros(T, np.uint8))
    half = (per, val, (np.arange(T) < 70).astype(np.uint8))
    one = (np.where(np.arange(K) == 0, per, 0).astype(np.float32), np.where(np.arange(K) == 0, val, np.inf).astype(np.float32), gate)
    tabs = [empty, closed, half, one]
    res, _, _ = vit_launch(tabs)
    for tab, got in zip(tabs, res):
        assert vit_same(got, pitch.f0_viterbi_numpy(*tab, 16000, 267, *COSTS))
    assert np.all(res[0][1] == K) and np.all(res[1][1] == K) and np.all(res[2][1][70:] == K) and (res[2][1][:70] < K).sum() >= 20
    assert np.all(res[0][0] == 0) and set(res[3][1]) <= {0, K}


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
def test_the_trap_signal_end_to_end():
    y, truth, judged, voiced_truth = fc.trap()
    want = pitch.track_f0([y], fc.SR, fc.HOP, tracker="viterbi", with_state=True)[0]
    got = pitch.track_f0([y], fc.SR, fc.HOP, tracker="viterbi", with_state=True, backend="hip", device=DEV)[0]
    assert same(got, want)
    assert fc.gpe(got[0], truth, judged) == 0.0 and np.all(fc.edge_distance(np.nonzero(got[3] != voiced_truth)[0]) <= 2)
    plain = pitch.track_f0([y], fc.SR, fc.HOP, backend="hip", device=DEV)[0]
    assert fc.gpe(plain[0], truth, judged) > 0.2 and same(plain, pitch.track_f0([y], fc.SR, fc.HOP)[0])


def test_results_do_not_depend_on_batching_or_on_the_launch_budget():
    sr, hop = 22050, 275
    ns = [1, 274, 275, 16 * 275 - 1, 3000, 16 * 275, 9000, 550]
    ys = [signal(sr, n, i) for i, n in enumerate(ns)]
    refs = [cand_reference(y, sr, hop) for y in ys]
    whole, raw, _ = cand_launch(ys, sr, hop)
    again, raw2, _ = cand_launch(ys, sr, hop)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(raw, raw2))
    back, _, _ = cand_launch(ys[::-1], sr, hop)
    for u, want in enumerate(refs):
        assert same(whole[u], want) and same(back[len(ys) - 1 - u], want), ns[u]
    cut = pitch.yin_candidates_hip(ys, sr, hop, device=DEV, max_launch_samples=5000)
    assert all(same(c, want) for c, want in zip(cut, refs))
    full = pitch.track_f0(ys, sr, hop, tracker="viterbi", with_state=True, backend="hip", device=DEV)
    small = pitch.track_f0(ys, sr, hop, tracker="viterbi", with_state=True, backend="hip", device=DEV, max_launch_samples=20)
    want = pitch.track_f0(ys, sr, hop, tracker="viterbi", with_state=True)
    assert all(same(a, w) and same(b, w) for a, b, w in zip(full, small, want))
    assert sum(int(w[3].sum()) for w in want) >= 20
    tabs = [vit_reference(T, T)[0] for T in (65, 700, 33)]
    a = pitch.f0_viterbi_hip(tabs, 16000, 267, device=DEV)
    b = pitch.f0_viterbi_hip(tabs, 16000, 267, device=DEV, max_launch_samples=100)
    assert all(vit_same(x, y) and vit_same(x, vit_reference(T, T)[1]) for x, y, T in zip(a, b, (65, 700, 33)))


# ---- outputs -------------------------------------------------------------------------------------------------------------------------------
def test_poisoned_outputs_are_overwritten_where_valid_and_nowhere_else():
    sr, hop = 16000, 200
    ys = [signal(sr, n, i) for i, n in enumerate((1, 199, 1400, 3333))]
    res, raw, fo = cand_launch(ys, sr, hop, tail=50)
    assert all(same(got, cand_reference(y, sr, hop)) for got, y in zip(res, ys))
    for b in raw:
        assert len(b) == fo[-1] + 50 and np.all(b[fo[-1]:] == POISON) and not np.any(b[:fo[-1]] == POISON)
    Ts = (1, 65, 300)
    res, (f0, state, cost), fo = vit_launch([vit_reference(T, T)[0] for T in Ts], tail=50)
    assert all(vit_same(got, vit_reference(T, T)[1]) for got, T in zip(res, Ts))
    assert np.all(f0[fo[-1]:] == POISON) and np.all(state[fo[-1]:] == POISON_BYTE)
    assert not np.any(f0[:fo[-1]] == POISON) and np.all(state[:fo[-1]] <= K) and not np.any(cost == POISON)


def check_bad_cand_tables(x, io, fo, untouched, total_in=None, total_frames=None):
    sr, hop = 16000, 200
    raw = cand_raw(x[:total_in], io, fo, sr, hop, total_frames=total_frames, tail=10)
    total = int(fo[-1]) if total_frames is None else total_frames
    for u in range(len(io) - 1):
        lo, hi = max(0, min(int(fo[u]), total)), max(0, min(int(fo[u + 1]), total))
        if u in untouched:
            assert all(np.all(b[lo:hi] == POISON) for b in raw), u
        else:
            assert same([b[lo:hi] for b in raw], cand_reference(x[io[u]:io[u + 1]], sr, hop)), u
    assert all(np.all(b[total:] == POISON) for b in raw)


def test_bad_offset_tables_leave_the_candidates_untouched():
    x = np.concatenate([signal(16000, n, i) for i, n in enumerate((1000, 777, 1500))])
    io, fo = [0, 1000, 1777, 3277], [0, 6, 10, 18]
    check_bad_cand_tables(x, io, fo, set())                                              # the good tables first
    check_bad_cand_tables(x, io, [0, 6, 11, 19], {1})                                    # 5 frames claimed, 1 + 777 // 200 = 4
    check_bad_cand_tables(x, [0, 1000, 900, 2400], [0, 6, 7, 15], {1})                   # n < 0
    check_bad_cand_tables(x, [-1, 1000, 1777, 3277], fo, {0})                            # a range in front of the buffer
    check_bad_cand_tables(x, io, fo, {2}, total_in=3276)                                 # a range past total_in
    check_bad_cand_tables(x, io, fo, {2}, total_frames=17)                               # a range past total_frames
    check_bad_cand_tables(x, io, [-2, 4, 8, 16], {0})                                    # frames in front of the buffer


def check_bad_vit_table(tabs, fo, untouched, total_frames=None):
    """utterance u is read at fo[u] .. fo[u + 1] of the concatenated tables, whatever they were built from"""
    f0, state, cost = vit_raw(tabs, fo, total_frames=total_frames, tail=10, max_frames=2048)
    per, val, gate = (np.concatenate([t[i] for t in tabs]) for i in range(3))
    total = len(per) if total_frames is None else total_frames
    for u in range(len(fo) - 1):
        lo, hi = int(fo[u]), int(fo[u + 1])
        if u in untouched:
            lo, hi = max(0, min(lo, total)), max(0, min(hi, total))
            assert np.all(f0[lo:hi] == POISON) and np.all(state[lo:hi] == POISON_BYTE) and cost[u] == POISON, u
        else:
            want = pitch.f0_viterbi_numpy(per[lo:hi], val[lo:hi], gate[lo:hi], 16000, 267, *COSTS)
            assert vit_same((f0[lo:hi], state[lo:hi], cost[u]), want), u
    assert np.all(f0[total:] == POISON) and np.all(state[total:] == POISON_BYTE)


def test_bad_offset_tables_leave_the_paths_untouched():
    tabs = [fc.grid_table(s, T) for s, T in ((1, 40), (2, 2100), (3, 70))]
    check_bad_vit_table(tabs, [0, 40, 2140, 2210], {1})                                  # 2100 frames: more than the kernel takes
    check_bad_vit_table(tabs, [0, 40, 40, 110], {1})                                     # no frame
    check_bad_vit_table(tabs, [0, 40, 110, 100], {2})                                    # fewer than none
    check_bad_vit_table(tabs, [-3, 40, 100, 170], {0})                                   # frames in front of the buffer
    check_bad_vit_table(tabs, [0, 40, 100, 2211], {2})                                   # frames past the buffer
    check_bad_vit_table(tabs, [0, 40, 100, 170], {2}, total_frames=169)                  # frames past total_frames
    check_bad_vit_table(tabs, [0, 40, 100, 170], set())                                  # the good table


def test_refusals_come_before_any_launch():
    T = 2049
    per, val = torch.zeros(T, K, device=DEV), torch.zeros(T, K, device=DEV)
    f0, state, cost = torch.full((T,), POISON, device=DEV), torch.full((T,), POISON_BYTE, dtype=torch.uint8, device=DEV), torch.full((1,), POISON, device=DEV)
    with pytest.raises(ValueError, match="2048"):
        ops.f0_viterbi(per, val, torch.ones(T, dtype=torch.uint8, device=DEV), torch.tensor([0, T], device=DEV), T, 267, 16000, *COSTS, f0, state, cost)
    with pytest.raises(_lib.SattError):
        ops.f0_viterbi(per, val, torch.ones(T, dtype=torch.uint8, device=DEV), torch.tensor([0, T], device=DEV), 2048, 267, 16000, -1.0, 0.1, 0.15, 0.1,
                       f0, state, cost)
    with pytest.raises(ValueError, match="2048"):
        pitch.track_f0([np.zeros(2048 * 200, np.float32)], 16000, 200, tracker="viterbi", backend="hip", device=DEV)
    torch.cuda.synchronize()
    assert bool((f0 == POISON).all()) and bool((state == POISON_BYTE).all()) and bool((cost == POISON).all())


# ---- LDS poison ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", [0x7FC00000, 0xFF800000, 0x00000000, 0x3F800000], ids=["nan", "minus_inf", "zero", "one"])
def test_bits_do_not_depend_on_what_lds_held(pattern):
    """satt_debug_poison_lds leaves the pattern in every LDS word of every CU in front of the launch: a d', a cost, a predecessor
    or a path byte read before it was written changes the candidates or the path"""
    poison = lambda: _lib.check(_lib.lib().satt_debug_poison_lds(pattern, 100, ops.current_stream().cuda_stream), "poison_lds")
    for sr, hop in ((22050, 275), (48000, 600)):
        ys = [signal(sr, n, i) for i, n in enumerate((1, hop + 1, 7 * hop - 1, 5000))]
        poison()
        res, _, _ = cand_launch(ys, sr, hop)
        assert all(same(got, cand_reference(y, sr, hop)) for got, y in zip(res, ys))
    Ts = (1, 2, 33, 65, 700)
    poison()
    res, _, _ = vit_launch([vit_reference(T, T)[0] for T in Ts])
    assert all(vit_same(got, vit_reference(T, T)[1]) for got, T in zip(res, Ts))


# ---- the public surface --------------------------------------------------------------------------------------------------------------------
def test_f0_batch_viterbi_hip_equals_numpy():
    from test_yin_cpu import toy_hparams
    hp = toy_hparams()
    ys = [signal(16000, n, i) for i, n in enumerate((3333, 1, 16000, 799))]
    h = audio.Audio(hp, backend="hip", device=DEV).f0_batch(ys, tracker="viterbi")
    n = audio.Audio(hp, backend="numpy").f0_batch(ys, tracker="viterbi")
    for x, y in zip(h, n):
        assert sorted(x) == ["aperiodicity", "f0", "power", "state", "voiced"]
        assert all(x[k].tobytes() == y[k].tobytes() and x[k].dtype == y[k].dtype for k in x)
    assert h[2]["voiced"].sum() >= 20 and h[2]["voiced"].dtype == bool and h[2]["state"].dtype == np.uint8
    assert audio.Audio(hp, backend="hip", device=DEV).f0_batch([], tracker="viterbi") == []
    kw = dict(fmin=80.0, fmax=400.0, window_ms=20.0, threshold=0.1, silence_db=40.0, jump_cost=0.5, switch_cost=0.2, lag_bias=0.0)
    h2 = audio.Audio(hp, backend="hip", device=DEV).f0_batch(ys, tracker="viterbi", **kw)
    n2 = audio.Audio(hp, backend="numpy").f0_batch(ys, tracker="viterbi", **kw)
    assert all(x[k].tobytes() == y[k].tobytes() for x, y in zip(h2, n2) for k in x)


def test_evaluate_f0_viterbi_hip_gives_the_numpy_csv_byte_for_byte(tmp_path):
    import test_yin_cpu as tc
    stats = tc.write_stats(str(tmp_path / "hparams.json"))
    pred_dir, ref_dir = str(tmp_path / "pw"), str(tmp_path / "rw")
    tc.write_toy_wavs(pred_dir, ref_dir)
    outs = {}
    for backend in ("hip", "numpy"):
        outs[backend] = str(tmp_path / ("out_" + backend))
        ac.run_driver("evaluate_f0.py", "--hparam-json-file", stats, "--backend", backend, "--tracker", "viterbi", "--pred-wav-dir", pred_dir,
                      "--ref-wav-dir", ref_dir, str(tmp_path / "unused"), outs[backend])
    csvs = [open(os.path.join(outs[b], "f0_distance.csv"), "rb").read() for b in ("hip", "numpy")]
    assert csvs[0] == csvs[1] and csvs[0].count(b"\n") == 3
    rows = tc.read_csv(os.path.join(outs["hip"], "f0_distance.csv"))
    assert abs(rows["utt000"]["f0_rmse_cents"] - 100.0) <= 3.0
