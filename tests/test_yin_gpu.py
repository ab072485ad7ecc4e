"""csrc/yin.hip against the float32 NumPy backend (f0, aperiodicity and power equal bit for bit), its batching guarantees, what it
leaves untouched (poisoned outputs, bad offset tables), refusals, non-finite samples, LDS poison, the float64 bounds of
tests/pitch_common.py, and the Python surface over it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import audio_common as ac
import pitch_common as pc
import satt_amd  # noqa: F401
from satt_amd import _lib, ops
from satt_amd.utils import audio, pitch

pytestmark = pytest.mark.gpu

DEV = "cuda"
POISON = -77.25
# (sr, hop, keyword arguments): the three corpora's rates (2, 2 and 4 chunks of lags; W % 4 = 0, 3, 0), three chunks at 32 kHz, one
# chunk with a window shorter than one 16-byte read and one with W % 4 = 2
EXTRA = [(32000, 400, {}), (100, 5, dict(fmin=10.0, fmax=50.0, window_ms=40.0)), (8000, 100, dict(fmin=40.0, window_ms=6.25))]


def lengths(sr, hop, kw):
    W = pitch.yin_sizes(sr, **{k: v for k, v in kw.items()})[0]
    return sorted({n for n in (1, W - 1, W, hop - 1, hop, hop + 1, 7 * hop - 1, 7 * hop, sr + 3) if n >= 1})


def signal(sr, n, seed):
    """a harmonic tone whose pitch glides through the lag range, behind a tenth of noise: voiced and unvoiced frames, every sample
    its own value"""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    f = (90.0 + 15.0 * seed) * (1.0 + 0.5 * k / sr)
    ph = 2.0 * np.pi * np.cumsum(f) / sr
    y = sum(0.4 / h * np.sin(h * ph + h) for h in (1, 2, 3)) + 2e-3 * rng.standard_normal(n)
    y[:n // 10] = 3e-3 * rng.standard_normal(n // 10)
    return y.astype(np.float32)


_REF = {}


def reference(sr, hop, n, seed, **kw):
    """the signal and its NumPy result, computed once"""
    key = (sr, hop, n, seed, tuple(sorted(kw.items())))
    if key not in _REF:
        y = signal(sr, n, seed)
        _REF[key] = (y, pitch.yin_numpy(y, sr, hop, **kw))
    return _REF[key]


def raw_launch(x, io, fo, sr, hop, total_frames=None, tail=0, threshold=pitch.THRESHOLD, **kw):
    """one launch on poisoned outputs; the offset tables as given (int64 lists).  Returns f0, aperiodicity, power [total + tail]"""
    W, tau_min, tau_max = pitch.yin_sizes(sr, **kw)
    total = int(fo[-1]) if total_frames is None else total_frames
    t = lambda v, dt=torch.int64: torch.as_tensor(np.asarray(v), dtype=dt).to(DEV)
    bufs = [torch.full((total + tail,), POISON, dtype=torch.float32, device=DEV) for _ in range(3)]
    views = [b[:total] for b in bufs]
    ops.yin(t(x, torch.float32), t(io), t(fo), W, tau_min, tau_max, hop, sr, threshold, *views)
    torch.cuda.synchronize()
    return [b.cpu().numpy() for b in bufs]


def launch(signals, sr, hop, tail=0, **kw):
    """the batch in one launch: (list of (f0, aperiodicity, power), raw buffers, frame offsets)"""
    lens = np.asarray([len(s) for s in signals], np.int64)
    io = np.concatenate([[0], np.cumsum(lens)])
    fo = np.concatenate([[0], np.cumsum(1 + lens // hop)])
    raw = raw_launch(np.concatenate(signals), io, fo, sr, hop, tail=tail, **kw)
    return [tuple(b[fo[u]:fo[u + 1]] for b in raw) for u in range(len(signals))], raw, fo


def same(got, want, nan_ok=False):
    if nan_ok:
        return all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want))
    return all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


# ---- the kernel against the NumPy backend --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,hop,kw", [(sr, hop, {}) for sr, hop in pc.CONFIGS] + EXTRA, ids=lambda v: str(v) if not isinstance(v, dict) else "")
def test_kernel_equals_the_numpy_backend(sr, hop, kw):
    ns = lengths(sr, hop, kw)
    refs = [reference(sr, hop, n, i, **kw) for i, n in enumerate(ns)]
    res, _, _ = launch([y for y, _ in refs], sr, hop, **kw)
    voiced = 0
    for n, got, (y, want) in zip(ns, res, refs):
        assert len(got[0]) == 1 + n // hop and same(got, want), (sr, n)
        alone, _, _ = launch([y], sr, hop, **kw)
        assert same(alone[0], want), (sr, n, "alone")
        voiced += int((want[0] > 0).sum())
    assert voiced >= 10                                                                  # both ways through the pick were taken


def test_the_threshold_is_strict():
    """the threshold set to the very float32 value of a voiced frame's lowest d': that lag no longer passes (d' < threshold, not <=),
    so the frame turns unvoiced - in the kernel as in the NumPy backend"""
    sr, hop = 16000, 200
    y, (f0, _, _) = reference(sr, hop, 3333, 3)
    _, tau_min, tau_max = pitch.yin_sizes(sr)
    dp, _ = pitch.yin_dprime_numpy(y, sr, hop)
    t = int(np.nonzero(f0 > 0)[0][-1])
    thr = float(dp[t, tau_min:tau_max].min())
    want = pitch.yin_numpy(y, sr, hop, threshold=thr)
    assert want[0][t] == 0 and want[1][t] <= np.float32(thr) and (want[0] > 0).sum() >= 1
    res, _, _ = launch([y], sr, hop, threshold=thr)
    assert same(res[0], want)
    assert np.nextafter(np.float32(thr), np.float32(1)) > np.float32(thr) and pitch.yin_numpy(y, sr, hop, threshold=float(np.nextafter(np.float32(thr), np.float32(1))))[0][t] > 0


# ---- batching ------------------------------------------------------------------------------------------------------------------------
def test_a_signal_does_not_depend_on_its_batch_or_its_place():
    sr, hop = 22050, 275
    ns = [1, 274, 275, 551, 7 * 275 - 1, 3000, 16 * 275, 15 * 275 - 1, 9000, 550]       # frame counts around the 16 a workgroup takes
    refs = [reference(sr, hop, n, i) for i, n in enumerate(ns)]
    ys = [y for y, _ in refs]
    whole, raw, _ = launch(ys, sr, hop)
    again, raw2, _ = launch(ys, sr, hop)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(raw, raw2))                  # two launches: identical bits
    back, _, _ = launch(ys[::-1], sr, hop)
    part, _, _ = launch(ys[3:7], sr, hop)
    for u, (_, want) in enumerate(refs):
        assert same(whole[u], want) and same(back[len(ys) - 1 - u], want), ns[u]
    for u in range(3, 7):
        assert same(part[u - 3], refs[u][1])


# ---- outputs -------------------------------------------------------------------------------------------------------------------------
def test_nothing_outside_the_batchs_own_frames_is_written():
    sr, hop = 16000, 200
    ns = [1, 199, 1400, 3333]
    refs = [reference(sr, hop, n, i) for i, n in enumerate(ns)]
    res, raw, fo = launch([y for y, _ in refs], sr, hop, tail=100)
    for got, (_, want) in zip(res, refs):
        assert same(got, want)
    for b in raw:
        assert len(b) == fo[-1] + 100 and np.all(b[fo[-1]:] == POISON) and not np.any(b[:fo[-1]] == POISON)


def check_bad_tables(x, io, fo, untouched, sr=16000, hop=200, total_in=None, total_frames=None):
    """launch with the tables as given; the utterances of `untouched` keep their poison, the others equal NumPy on their own slices"""
    raw = raw_launch(x[:total_in], io, fo, sr, hop, total_frames=total_frames, tail=10)
    total = int(fo[-1]) if total_frames is None else total_frames
    for u in range(len(io) - 1):
        lo, hi = max(0, min(int(fo[u]), total)), max(0, min(int(fo[u + 1]), total))
        if u in untouched:
            assert all(np.all(b[lo:hi] == POISON) for b in raw), u
        else:
            want = pitch.yin_numpy(x[io[u]:io[u + 1]], sr, hop)
            assert same([b[lo:hi] for b in raw], want), u
    assert all(np.all(b[total:] == POISON) for b in raw)


def test_bad_offset_tables_leave_their_utterances_untouched():
    x = np.concatenate([signal(16000, n, i) for i, n in enumerate((1000, 777, 1500))])
    io, fo = [0, 1000, 1777, 3277], [0, 6, 10, 18]
    check_bad_tables(x, io, fo, set())                                                   # the good tables first
    check_bad_tables(x, io, [0, 6, 11, 19], {1})                                         # 5 frames claimed, 1 + 777 // 200 = 4
    check_bad_tables(x, io, [0, 6, 9, 17], {1})                                          # 3 frames claimed
    check_bad_tables(x, [0, 1000, 1000, 2500], [0, 6, 7, 15], {1})                       # n = 0
    check_bad_tables(x, [0, 1000, 900, 2400], [0, 6, 7, 15], {1})                        # n < 0
    check_bad_tables(x, [-1, 1000, 1777, 3277], fo, {0})                                 # a range in front of the buffer
    check_bad_tables(x, io, fo, {2}, total_in=3276)                                      # a range past total_in
    check_bad_tables(x, io, fo, {2}, total_frames=17)                                    # a range past total_frames
    check_bad_tables(x, io, [-2, 4, 8, 16], {0})                                         # frames in front of the buffer


def test_refusals_come_before_any_launch():
    x = torch.zeros(1000, device=DEV)
    io, fo = torch.tensor([0, 1000], device=DEV), torch.tensor([0, 6], device=DEV)
    out = [torch.full((6,), POISON, device=DEV) for _ in range(3)]
    for W, tau_min, tau_max, hop in ((1537, 32, 267, 200), (400, 32, 1024, 200), (0, 32, 267, 200), (400, 32, 267, 0), (400, 2, 2, 200)):
        with pytest.raises(ValueError):
            ops.yin(x, io, fo, W, tau_min, tau_max, hop, 16000, 0.15, *out)
    for kw in (dict(tau_min=1), dict(tau_min=267), dict(signal=None), dict(power=None), dict(n_utts=0)):
        f = dict(window=400, tau_min=32, tau_max=267, hop=200, n_utts=1, sample_rate=16000.0, threshold=0.15, total_in=1000, total_frames=6,
                 signal=x.data_ptr(), in_offsets=io.data_ptr(), frame_offsets=fo.data_ptr(), f0=out[0].data_ptr(),
                 aperiodicity=out[1].data_ptr(), power=out[2].data_ptr())
        f.update(kw)
        with pytest.raises(_lib.SattError):
            _lib.check(_lib.lib().satt_yin(_lib.C.byref(_lib.YinParams(**f)), ops._s()), "yin")
    torch.cuda.synchronize()
    assert all(bool((o == POISON).all()) for o in out)


NAN_SCRIPT = r"""
import sys
import numpy as np
sys.path[:0] = [%r, %r]
import satt_amd
from satt_amd.utils import pitch
z = np.load(sys.argv[1])
res = pitch.yin_hip([z["bad"], z["good"]], 16000, 200)
np.savez(sys.argv[2], **{"%%s%%d" %% (k, u): r[i] for u, r in enumerate(res) for i, k in enumerate(("f0", "ap", "pw"))})
"""


def test_nan_and_inf_samples_neither_hang_nor_fault(tmp_path):
    """the launch runs in a child process under a time limit: no loop bound of the kernel depends on a sample"""
    good, want = reference(16000, 200, 3333, 3)
    bad = good.copy()
    bad[700] = np.nan
    bad[1500] = np.inf
    bad[2500] = -np.inf
    np.savez(str(tmp_path / "in.npz"), bad=bad, good=good)
    (tmp_path / "run.py").write_text(NAN_SCRIPT % (ac.ROOT, os.path.join(ac.ROOT, "tests")))
    r = subprocess.run([sys.executable, str(tmp_path / "run.py"), str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(str(tmp_path / "out.npz"))
    assert same([z["f01"], z["ap1"], z["pw1"]], want)                                   # the other utterance is unaffected
    twin = pitch.yin_numpy(bad, 16000, 200)
    assert same([z["f00"], z["ap0"], z["pw0"]], twin, nan_ok=True)
    assert np.isnan(z["pw0"]).any() and not pitch.voicing(z["f00"], z["pw0"]).any()
    clean = ~np.isnan(z["pw0"]) & ~np.isinf(z["pw0"])
    assert clean.sum() >= 3


# ---- LDS poison ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", [0x7FC00000, 0xFF800000, 0x00000000, 0x3F800000], ids=["nan", "minus_inf", "zero", "one"])
def test_bits_do_not_depend_on_what_lds_held(pattern):
    """satt_debug_poison_lds leaves the pattern in every LDS word of every CU in front of the launch: a sample, a d or a d' read
    before it was written changes the sums, the minimum or the pick"""
    for sr, hop in ((22050, 275), (48000, 600)):
        ns = [1, hop + 1, 7 * hop - 1, 5000]
        refs = [reference(sr, hop, n, i) for i, n in enumerate(ns)]
        _lib.check(_lib.lib().satt_debug_poison_lds(pattern, 100, ops.current_stream().cuda_stream), "poison_lds")
        res, _, _ = launch([y for y, _ in refs], sr, hop)
        for got, (_, want) in zip(res, refs):
            assert same(got, want)


# ---- float64 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,hop", pc.CONFIGS)
def test_kernel_meets_the_float64_bounds(sr, hop):
    tones = pc.tone_set(sr, hop)
    res, _, _ = launch([y for _, y, _ in tones], sr, hop)
    for (period, y, ref), (f0, ap, power) in zip(tones, res):
        pc.check_against_float64(f0, ap, power, None, ref, "%d period %.2f:" % (sr, period))
        _, inside = pc.frame_sets(sr, hop, len(y))
        assert np.abs(pc.cents(f0[inside], period, sr)).max() <= pc.CENTS_BOUND


# ---- the public surface --------------------------------------------------------------------------------------------------------------
def test_f0_batch_hip_equals_numpy():
    from test_yin_cpu import toy_hparams
    hp = toy_hparams()
    ys = [signal(16000, n, i) for i, n in enumerate((3333, 1, 16000, 799))]
    h = audio.Audio(hp, backend="hip", device=DEV).f0_batch(ys)
    n = audio.Audio(hp, backend="numpy").f0_batch(ys)
    for x, y in zip(h, n):
        assert sorted(x) == ["aperiodicity", "f0", "power", "voiced"]
        assert all(x[k].tobytes() == y[k].tobytes() and x[k].dtype == y[k].dtype for k in x)
    assert h[2]["voiced"].sum() >= 20 and h[2]["voiced"].dtype == bool
    assert audio.Audio(hp, backend="hip", device=DEV).f0_batch([]) == []
    # a sample budget that cuts the batch into several launches, and other arguments: the same results
    cut = pitch.yin_hip(ys, 16000, 200, device=DEV, max_launch_samples=4000)
    assert all(same(c, (x["f0"], x["aperiodicity"], x["power"])) for c, x in zip(cut, h))
    kw = dict(fmin=80.0, fmax=400.0, window_ms=20.0, threshold=0.1)
    h2 = audio.Audio(hp, backend="hip", device=DEV).f0_batch(ys, silence_db=40.0, **kw)
    n2 = audio.Audio(hp, backend="numpy").f0_batch(ys, silence_db=40.0, **kw)
    assert all(x[k].tobytes() == y[k].tobytes() for x, y in zip(h2, n2) for k in x)


def test_evaluate_f0_driver_on_the_hip_backend(tmp_path):
    import test_yin_cpu as tc
    stats = tc.write_stats(str(tmp_path / "hparams.json"))
    au = audio.Audio(tc.toy_hparams(), backend="hip", device=DEV)
    # wav mode
    pred_dir, ref_dir, out = str(tmp_path / "pw"), str(tmp_path / "rw"), str(tmp_path / "out_wav")
    keys, skipped = tc.write_toy_wavs(pred_dir, ref_dir)
    ac.run_driver("evaluate_f0.py", "--hparam-json-file", stats, "--backend", "hip", "--pred-wav-dir", pred_dir, "--ref-wav-dir", ref_dir,
                  str(tmp_path / "unused"), out)
    sp = [au.load_wav(os.path.join(pred_dir, k + ".wav")) for k in keys]
    sr_ = [au.load_wav(os.path.join(ref_dir, k + ".wav")) for k in keys]
    mels = [au.normalize_mel(S).astype(np.float32) for S in au.melspectrogram_batch(sp + sr_)]
    want, _, _ = tc.expected(au, keys, sp, sr_, mels[:2], mels[2:])
    assert tc.read_csv(os.path.join(out, "f0_distance.csv")) == want
    assert abs(want["utt000"]["f0_rmse_cents"] - 100.0) <= 3.0
    tc.check_summary(json.load(open(os.path.join(out, "summary.json"))), want, "wav", skipped)
    # prediction records, both sides through Griffin-Lim
    pred, out = str(tmp_path / "pred"), str(tmp_path / "out_rec")
    records = tc.write_toy_records(pred)
    ac.run_driver("evaluate_f0.py", "--hparam-json-file", stats, "--backend", "hip", "--iters", "4", "--seed", "3", pred, out)
    keys = [k for k in sorted(records) if records[k][1] is not None]
    mp, mr = [records[k][0] for k in keys], [records[k][1] for k in keys]
    wavs = au.inv_melspectrogram_batch([au.denormalize_mel(S.astype(np.float64)) for S in mp + mr], iters=4, seed=3)
    want, _, _ = tc.expected(au, keys, wavs[:3], wavs[3:], mp, mr)
    assert tc.read_csv(os.path.join(out, "f0_distance.csv")) == want
    tc.check_summary(json.load(open(os.path.join(out, "summary.json"))), want, "griffin_lim", ["utt002"])
