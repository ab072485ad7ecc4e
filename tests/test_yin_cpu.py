"""The float32 NumPy backend of the YIN tracker (utils/pitch.py) against the float64 programme of tests/pitch_common.py and against
known pitches, a scalar float32 restatement of the definition on a tiny configuration, the host-side voicing and metrics, the C ABI
of satt_yin without a GPU, and evaluate_f0.py on the numpy backend in both of its modes."""
import csv
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import audio_common as ac
import pitch_common as pc
import satt_amd  # noqa: F401
from satt_amd.hparams import hparams
from satt_amd.utils import audio, pitch, tfrecord

ROOT = ac.ROOT
TINY = dict(sr=100, hop=5, fmin=10.0, fmax=50.0, window_ms=40.0)          # W = 4, lags 2 .. 10: small enough for a scalar loop


def test_sizes_and_defaults():
    assert (pitch.FMIN, pitch.FMAX, pitch.WINDOW_MS, pitch.THRESHOLD, pitch.SILENCE_DB) == (60.0, 500.0, 25.0, 0.15, 50.0)
    assert pitch.yin_sizes(16000) == (400, 32, 267) and pitch.yin_sizes(22050) == (551, 44, 368) and pitch.yin_sizes(48000) == (1200, 96, 800)
    for sr, _ in pc.CONFIGS:
        assert pitch.yin_sizes(sr) == pc.sizes(sr)
    assert pitch.yin_sizes(**{k: v for k, v in TINY.items() if k != "hop"}) == (4, 2, 10)
    assert not any(k in hparams.values() for k in ("fmin", "fmax", "f0_threshold", "window_ms", "silence_db"))


# ---- the twin against float64 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,hop", pc.CONFIGS)
def test_numpy_backend_against_float64(sr, hop):
    _, tau_min, tau_max = pc.sizes(sr)
    robust = []
    for period, y, ref in pc.tone_set(sr, hop):
        dp, power = pitch.yin_dprime_numpy(y, sr, hop)
        f0, ap = pitch.yin_pick_numpy(dp, sr, tau_min, tau_max)
        pc.check_against_float64(f0, ap, power, dp, ref, "%d period %.2f:" % (sr, period))
        whole = pitch.yin_numpy(y, sr, hop)
        assert all(x.dtype == np.float32 and x.tobytes() == w.tobytes() for x, w in zip((f0, ap, power), whole))
        robust.append(ref["robust"])
    robust = np.concatenate(robust)
    assert 1.0 - robust.mean() <= pc.SKIP_MAX, (int((~robust).sum()), len(robust))      # a condition on the inputs, float64 alone


@pytest.mark.parametrize("sr,hop", pc.CONFIGS)
def test_known_pitch(sr, hop):
    W, tau_min, tau_max = pc.sizes(sr)
    for period, y, ref in pc.tone_set(sr, hop):
        assert tau_min < period < tau_max - 1
        lead, inside = pc.frame_sets(sr, hop, len(y))
        assert len(lead) >= 3 and len(inside) >= 10
        assert np.abs(pc.cents(ref["f0"][inside], period, sr)).max() <= pc.CENTS_64           # the yardstick's own error, as recorded
        f0, ap, power = pitch.yin_numpy(y, sr, hop)
        v = pitch.voicing(f0, power)
        assert v[inside].all() and np.abs(pc.cents(f0[inside], period, sr)).max() <= pc.CENTS_BOUND, period
        assert not v[lead].any() and np.all(f0[lead] == 0) and np.all(ap[lead] >= pitch.THRESHOLD), period
    below, above = pc.outside(sr)
    assert below < tau_min - 2 and above > tau_max + 2 and tau_min < 2 * below < tau_max - 1
    y = pc.tone(sr, below, 7)
    f0, _, _ = pitch.yin_numpy(y, sr, hop)
    _, inside = pc.frame_sets(sr, hop, len(y))
    assert np.all(f0[inside] > 0) and np.abs(pc.cents(f0[inside], 2 * below, sr)).max() <= pc.CENTS_BOUND     # the sub-octave
    y = pc.tone(sr, above, 7)
    f0, ap, _ = pitch.yin_numpy(y, sr, hop)
    _, inside = pc.frame_sets(sr, hop, len(y))
    assert np.all(f0[inside] == 0) and np.all(ap[inside] >= pitch.THRESHOLD)


def scalar32(y, sr, hop, fmin, fmax, window_ms, threshold=0.15):
    """the definition of DESIGN.md 3.6 one float32 operation at a time"""
    F = np.float32
    W, tau_min, tau_max = pitch.yin_sizes(sr, fmin, fmax, window_ms)
    n = len(y)
    x = lambda k: F(y[k]) if 0 <= k < n else F(0)
    out = []
    for t in range(1 + n // hop):
        s = t * hop - (W + tau_max) // 2
        d, pw = [], F(0)
        for j in range(W):
            pw = F(pw + F(x(s + j) * x(s + j)))
        for tau in range(tau_max + 1):
            acc = F(0)
            for j in range(W):
                df = F(x(s + j) - x(s + j + tau))
                acc = F(acc + F(df * df))
            d.append(acc)
        dp, c = [F(1)], F(0)
        for tau in range(1, tau_max + 1):
            c = F(c + d[tau])
            dp.append(F(F(d[tau] * F(tau)) / c) if c > 0 else F(1))
        tau0 = next((k for k in range(tau_min, tau_max) if dp[k] < F(threshold)), None)
        if tau0 is None:
            out.append((F(0), min(dp[tau_min:tau_max + 1]), F(pw / F(W))))
            continue
        k = tau0
        while k + 1 <= tau_max - 1 and dp[k + 1] < dp[k]:
            k += 1
        a, b, c3 = dp[k - 1], dp[k], dp[k + 1]
        num, den = F(a - c3), F(F(a - b) + F(c3 - b))
        shift = F(0)
        if den > 0:
            shift = F(F(F(0.5) * num) / den)
            shift = F(1) if shift > 1 else (F(-1) if shift < -1 else shift)
        out.append((F(F(sr) / F(F(k) + shift)), b, F(pw / F(W))))
    return [np.asarray(col, np.float32) for col in zip(*out)]


def tiny_signals():
    rng = np.random.default_rng(3)
    k = np.arange(83)
    return [(np.sin(2 * np.pi * k / 5.3) + 0.3 * np.sin(4 * np.pi * k / 5.3 + 1) + 0.01 * rng.standard_normal(83)).astype(np.float32),
            (np.sin(2 * np.pi * k[:37] / 7.7) + 0.05 * rng.standard_normal(37)).astype(np.float32),
            rng.standard_normal(21).astype(np.float32), np.float32([0.5]), np.float32([0.25, -0.5, 0.25, 1.0])]


def test_numpy_backend_equals_the_scalar_definition_bit_for_bit():
    voiced = 0
    for y in tiny_signals():
        got = pitch.yin_numpy(y, **TINY)
        want = scalar32(y, **TINY)
        assert len(got[0]) == 1 + len(y) // TINY["hop"]
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes(), (len(y), g, w)
        voiced += int((got[0] > 0).sum())
    assert voiced >= 10                                                                   # the parabola's branch was taken
    # the threshold at the very float32 value of a voiced frame's lowest d': d' < threshold is strict, the frame turns unvoiced
    y = tiny_signals()[0]
    dp, _ = pitch.yin_dprime_numpy(y, **TINY)
    t = int(np.nonzero(pitch.yin_numpy(y, **TINY)[0] > 0)[0][-1])
    thr = float(dp[t, 2:10].min())
    got, want = pitch.yin_numpy(y, threshold=thr, **TINY), scalar32(y, threshold=thr, **TINY)
    assert got[0][t] == 0 and all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


def test_zeros_and_a_constant_are_unvoiced_and_finite():
    for sr, hop in pc.CONFIGS:
        for level in (0.0, 0.37):
            y = np.full(3 * hop + 17, level, np.float32)
            f0, ap, power = pitch.yin_numpy(y, sr, hop)
            assert len(f0) == 4 and np.all(f0 == 0) and np.all(np.isfinite(ap)) and np.all(np.isfinite(power))
            assert not pitch.voicing(f0, power).any()
            if level == 0.0:
                assert np.all(ap == 1) and np.all(power == 0)
    # inside a constant signal (no edge in the span) d = 0 everywhere: d' = 1
    sr, hop = pc.CONFIGS[0]
    f0, ap, power = pitch.yin_numpy(np.full(4000, 0.37, np.float32), sr, hop)
    assert np.all(f0 == 0) and ap[10] == 1 and abs(power[10] - 0.37 ** 2) < 1e-6


def test_refusals():
    y = np.zeros(100, np.float32)
    for kw in (dict(sr=900, hop=10), dict(sr=16000, hop=0), dict(sr=16000, hop=200, fmin=10.0), dict(sr=16000, hop=200, window_ms=100.0),
               dict(sr=16000, hop=200, fmin=600.0), dict(sr=96000, hop=1200)):
        with pytest.raises(ValueError):
            pitch.yin_numpy(y, **kw)
    for bad in (np.zeros(0, np.float32), np.zeros((3, 3), np.float32)):
        with pytest.raises(ValueError):
            pitch.yin_numpy(bad, 16000, 200)


# ---- voicing and metrics ---------------------------------------------------------------------------------------------------------------
def test_voicing():
    f0 = np.float32([100, 0, 100, 100, np.nan])
    power = np.float32([1.0, 1.0, 1e-5, 0.99e-5, 1.0])
    assert list(pitch.voicing(f0, power)) == [True, False, False, False, False]        # (1e-5 is the bar itself: not above it)
    assert list(pitch.voicing(f0, power, silence_db=60.0)) == [True, False, True, True, False]
    assert not pitch.voicing(f0, np.zeros(5, np.float32)).any()
    assert len(pitch.voicing([], [])) == 0


def test_f0_metrics():
    f = np.asarray([100.0, 110.0, 0.0, 130.0, 150.0, 0.0])
    v = f > 0
    diag = np.stack([np.arange(6), np.arange(6)], axis=1)
    m = pitch.f0_metrics(f, v, f, v, diag)
    assert (m["steps"], m["voiced_both"], m["vuv_error"], m["f0_rmse_cents"], m["f0_rmse_hz"], m["gpe"]) == (6, 4, 0.0, 0.0, 0.0, 0.0)
    assert abs(m["log_f0_corr"] - 1.0) <= 1e-12
    m = pitch.f0_metrics(f * 2.0 ** (1.0 / 12.0), v, f, v, diag)                         # a semitone up
    assert abs(m["f0_rmse_cents"] - 100.0) <= 1e-9 and abs(m["log_f0_corr"] - 1.0) <= 1e-12 and m["gpe"] == 0.0
    assert abs(m["f0_rmse_hz"] - np.sqrt(np.mean((f[v] * (2.0 ** (1.0 / 12.0) - 1.0)) ** 2))) <= 1e-9
    # hand-built voicing: predicted V V U U V V, reference V U V U V V over the diagonal: 2 of 6 differ, 3 voiced on both sides;
    # of those, 100 -> 121 (+21 %) and 150 -> 119 (-20.67 %) are gross, 140 -> 150 is not
    fp, fr = np.asarray([121.0, 100.0, 0.0, 0.0, 119.0, 150.0]), np.asarray([100.0, 0.0, 90.0, 0.0, 150.0, 140.0])
    m = pitch.f0_metrics(fp, fp > 0, fr, fr > 0, diag)
    assert (m["steps"], m["voiced_both"]) == (6, 3) and abs(m["vuv_error"] - 2.0 / 6.0) <= 1e-15 and abs(m["gpe"] - 2.0 / 3.0) <= 1e-15
    assert abs(m["f0_rmse_hz"] - np.sqrt((21.0 ** 2 + 31.0 ** 2 + 10.0 ** 2) / 3.0)) <= 1e-9
    # a path that repeats frames counts steps, not frames
    warp = np.asarray([[0, 0], [0, 1], [1, 1], [2, 2], [3, 3], [4, 4], [4, 5], [5, 5]])
    m = pitch.f0_metrics(fp, fp > 0, fr, fr > 0, warp)
    assert (m["steps"], m["voiced_both"]) == (8, 4) and abs(m["vuv_error"] - 3.0 / 8.0) <= 1e-15
    # the None cases: nothing voiced on both sides; one such step; zero variance
    m = pitch.f0_metrics(fp, fp > 0, fr, np.zeros(6, bool), diag)
    assert m["voiced_both"] == 0 and all(m[k] is None for k in ("f0_rmse_cents", "f0_rmse_hz", "log_f0_corr", "gpe")) and m["vuv_error"] == 4.0 / 6.0
    m = pitch.f0_metrics(fp, fp > 0, fr, fr > 0, diag[:2])
    assert m["voiced_both"] == 1 and m["log_f0_corr"] is None and m["f0_rmse_hz"] == 21.0
    flat = np.full(6, 120.0)
    m = pitch.f0_metrics(flat, flat > 0, f + 1.0, f > -1, diag)
    assert m["voiced_both"] == 6 and m["log_f0_corr"] is None and m["f0_rmse_cents"] > 0


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_yin_struct_layout_matches_c(tmp_path):
    from satt_amd import _lib
    names = [n for n, _ in _lib.YinParams._fields_]
    assert names == ["window", "tau_min", "tau_max", "hop", "n_utts", "sample_rate", "threshold", "total_in", "total_frames", "signal",
                     "in_offsets", "frame_offsets", "f0", "aperiodicity", "power"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "satt_hip.h"\nint main() {\n  printf("%zu", sizeof(satt_yin_params));\n'
    src += "".join('  printf(" %%zu", offsetof(satt_yin_params, %s));\n' % n for n in names) + "  return 0; }\n"
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    vals = list(map(int, subprocess.check_output([str(tmp_path / "t")]).split()))
    P = _lib.YinParams
    assert vals == [ctypes.sizeof(P)] + [getattr(P, n).offset for n in names]
    header = open(os.path.join(ROOT, "include", "satt_hip.h")).read()
    for sym in ("satt_yin_supported", "satt_yin_max_window", "satt_yin_max_lag", "satt_yin_run_length", "satt_yin"):
        assert sym + "(" in header and sym in _lib.SIGNATURES
    assert _lib.SIGNATURES["satt_yin"][1][-1] is ctypes.c_void_p


def test_yin_supported_agrees_with_the_python_predicate():
    from satt_amd import ops
    assert ops.yin_limits() == (pitch.YIN_MAX_WINDOW, pitch.YIN_MAX_LAG, pitch.YIN_RUN) == (1536, 1023, 16)
    for W in (-1, 0, 1, 4, 400, 1200, 1535, 1536, 1537, 1 << 20):
        for tau_max in (-1, 0, 2, 3, 10, 267, 800, 1022, 1023, 1024, 1 << 20):
            for hop in (-1, 0, 1, 200, 600, (1 << 20) - 1, 1 << 20, (1 << 20) + 1):
                assert ops.yin_supported(W, tau_max, hop) == pitch.yin_supported(W, tau_max, hop), (W, tau_max, hop)
    for sr in (16000, 22050, 24000, 32000, 44100, 48000):                                 # the defaults at the common rates
        W, tau_min, tau_max = pitch.yin_sizes(sr)
        assert tau_min >= 2 and ops.yin_supported(W, tau_max, sr // 80)


def test_bad_arguments_return_before_any_launch():
    """there is no GPU here: every one of these calls has to come back with its code before the library touches the runtime"""
    from satt_amd import _lib
    lib = _lib.lib()
    BADARG, UNSUPPORTED = -1, -2
    assert b"bad argument" in lib.satt_strerror(BADARG) and b"unsupported" in lib.satt_strerror(UNSUPPORTED)
    keep = [(ctypes.c_int64 * 4)() for _ in range(6)]                                   # host memory: never dereferenced by the entry point
    ptr = [ctypes.addressof(k) for k in keep]

    def params(**kw):
        f = dict(window=400, tau_min=32, tau_max=267, hop=200, n_utts=1, sample_rate=16000.0, threshold=0.15, total_in=1000, total_frames=6,
                 signal=ptr[0], in_offsets=ptr[1], frame_offsets=ptr[2], f0=ptr[3], aperiodicity=ptr[4], power=ptr[5])
        f.update(kw)
        return _lib.YinParams(**f)
    assert lib.satt_yin(None, None) == BADARG
    for kw in (dict(signal=None), dict(in_offsets=None), dict(frame_offsets=None), dict(f0=None), dict(aperiodicity=None), dict(power=None),
               dict(n_utts=0), dict(total_in=0), dict(total_frames=-1), dict(tau_min=1), dict(tau_min=267), dict(tau_min=300),
               dict(sample_rate=0.0), dict(sample_rate=float("nan")), dict(threshold=float("nan"))):
        assert lib.satt_yin(ctypes.byref(params(**kw)), None) == BADARG, kw
    for kw in (dict(window=0), dict(window=1537), dict(tau_max=2, tau_min=2), dict(tau_max=1024), dict(hop=0), dict(hop=(1 << 20) + 1)):
        assert lib.satt_yin(ctypes.byref(params(**kw)), None) == UNSUPPORTED, kw


# ---- evaluate_f0.py --------------------------------------------------------------------------------------------------------------------
SR, HOP = 16000, 200
PERIODS = {"utt000": (80.0, 80.0 * 2.0 ** (1.0 / 12.0), 0.30, 0.32), "utt001": (123.4, 123.4, 0.26, 0.25),
           "utt002": (100.0, 100.0, 0.25, 0.25), "utt003": (61.7, 55.0, 0.28, 0.27)}


def toy_hparams():
    hp = hparams.copy()
    hp.parse("num_freq=513,sample_rate=16000,frame_length_ms=50.0,frame_shift_ms=12.5,num_mels=80")
    hp.set("average_mel_level_db", [-40.0 - 0.1 * m for m in range(80)])
    hp.set("stddev_mel_level_db", [10.0 + 0.05 * m for m in range(80)])
    return hp


def toy_signals():
    """{key: (predicted signal, reference signal)}: tones of PERIODS behind a short noise lead-in; utt000 is a semitone apart"""
    return {key: (pc.tone(SR, pp, 40 + i, 0.05, tp), pc.tone(SR, pr, 50 + i, 0.05, tr)) for i, (key, (pp, pr, tp, tr)) in enumerate(sorted(PERIODS.items()))}


def write_toy_records(root, without_truth=("utt002",)):
    """prediction records whose mels are the normalised mels of toy_signals(); returns {key: (mel, ground truth or None)}"""
    os.makedirs(root, exist_ok=True)
    au = audio.Audio(toy_hparams(), backend="numpy")
    out = {}
    for u, (key, (yp, yr)) in enumerate(sorted(toy_signals().items())):
        mel, gt = (au.normalize_mel(S).astype(np.float32) for S in au.melspectrogram_batch([yp, yr]))
        gt = None if key in without_truth else gt
        tfrecord.write_prediction_result(u, key, [np.zeros((4, len(mel)), np.float32)], mel, gt, "text %d" % u, np.arange(4), None,
                                         os.path.join(root, key + ".tfrecord"))
        out[key] = (mel, gt)
    return out


def write_toy_wavs(pred_dir, ref_dir):
    os.makedirs(pred_dir)
    os.makedirs(ref_dir)
    for key, (yp, yr) in toy_signals().items():
        if key != "utt001":
            ac.write_wav(os.path.join(pred_dir, key + ".wav"), yp, SR)
        if key != "utt003":
            ac.write_wav(os.path.join(ref_dir, key + ".wav"), yr, SR)
    return ["utt000", "utt002"], ["utt001", "utt003"]


def write_stats(path):
    hp = toy_hparams()
    with open(path, "w") as f:
        json.dump(dict(num_mels=80, num_freq=513, sample_rate=16000, average_mel_level_db=list(hp.average_mel_level_db),
                       stddev_mel_level_db=list(hp.stddev_mel_level_db)), f)
    return path


def read_csv(path):
    rows = list(csv.reader(open(path)))
    assert rows[0] == ["key", "frames_pred", "frames_ref", "steps", "voiced_both", "vuv_error", "f0_rmse_cents", "f0_rmse_hz", "log_f0_corr", "gpe"]
    num = lambda s: None if s == "" else float(s)
    return {r[0]: dict(frames_pred=int(r[1]), frames_ref=int(r[2]), steps=int(r[3]), voiced_both=int(r[4]), vuv_error=num(r[5]),
                       f0_rmse_cents=num(r[6]), f0_rmse_hz=num(r[7]), log_f0_corr=num(r[8]), gpe=num(r[9])) for r in rows[1:]}


def expected(au, keys, sig_pred, sig_ref, mel_pred, mel_ref, **par):
    dist = au.mel_distance_batch(mel_pred, mel_ref, want_paths=True)
    tracks = au.f0_batch(sig_pred + sig_ref, **par)
    out = {}
    for u, key in enumerate(keys):
        tp, tr = tracks[u], tracks[len(keys) + u]
        m = pitch.f0_metrics(tp["f0"], tp["voiced"], tr["f0"], tr["voiced"], dist[u]["path"])
        out[key] = dict(frames_pred=dist[u]["frames_pred"], frames_ref=dist[u]["frames_ref"], **m)
    return out, tracks, dist


def check_summary(s, want, mode, skipped):
    assert s["count"] == len(want) and s["mode"] == mode and s["skipped"] == skipped
    assert s["steps"] == sum(w["steps"] for w in want.values()) and s["voiced_both"] == sum(w["voiced_both"] for w in want.values())
    for k in ("vuv_error", "f0_rmse_cents", "f0_rmse_hz", "log_f0_corr", "gpe"):
        v = [w[k] for w in want.values() if w[k] is not None]
        assert (s["mean"][k] is None and not v) or abs(s["mean"][k] - np.mean(v)) <= 1e-12, k
    nb = s["voiced_both"]
    for k in ("f0_rmse_cents", "f0_rmse_hz"):
        ww = np.sqrt(sum(w["voiced_both"] * w[k] ** 2 for w in want.values() if w[k] is not None) / nb) if nb else None
        assert (ww is None and s["weighted_" + k] is None) or abs(s["weighted_" + k] - ww) <= 1e-9
    assert (s["sample_rate"], s["hop"]) == (SR, HOP)


def test_evaluate_f0_driver_on_wav_directories(tmp_path):
    pred_dir, ref_dir, out = str(tmp_path / "pw"), str(tmp_path / "rw"), str(tmp_path / "out")
    keys, skipped = write_toy_wavs(pred_dir, ref_dir)
    stats = write_stats(str(tmp_path / "hparams.json"))
    r = ac.run_driver("evaluate_f0.py", "--hparam-json-file", stats, "--backend", "numpy", "--pred-wav-dir", pred_dir, "--ref-wav-dir", ref_dir,
                      "--write-tracks", str(tmp_path / "unused"), out)
    assert "utt001: in %s only, skipped" % ref_dir in r.stdout and "utt003: in %s only, skipped" % pred_dir in r.stdout
    au = audio.Audio(toy_hparams(), backend="numpy")
    sp = [au.load_wav(os.path.join(pred_dir, k + ".wav")) for k in keys]
    sr_ = [au.load_wav(os.path.join(ref_dir, k + ".wav")) for k in keys]
    mels = [au.normalize_mel(S).astype(np.float32) for S in au.melspectrogram_batch(sp + sr_)]
    want, tracks, dist = expected(au, keys, sp, sr_, mels[:2], mels[2:])
    got = read_csv(os.path.join(out, "f0_distance.csv"))
    assert got == want and list(got) == keys
    # the semitone pair: about 100 cents, every voiced frame within a few cents of it; the equal pair: about none
    assert want["utt000"]["voiced_both"] >= 15 and abs(want["utt000"]["f0_rmse_cents"] - 100.0) <= 3.0 and want["utt000"]["gpe"] == 0.0
    assert want["utt002"]["voiced_both"] >= 15 and want["utt002"]["f0_rmse_cents"] <= 2.0 and want["utt002"]["vuv_error"] <= 0.15
    s = json.load(open(os.path.join(out, "summary.json")))
    check_summary(s, want, "wav", skipped)
    assert (s["fmin"], s["fmax"], s["window_ms"], s["threshold"], s["silence_db"], s["iters"], s["seed"]) == (60.0, 500.0, 25.0, 0.15, 50.0, None, None)
    z = np.load(os.path.join(out, "utt000.f0.npz"))
    assert np.array_equal(z["path"], dist[0]["path"]) and z["f0_pred"].tobytes() == tracks[0]["f0"].tobytes()
    assert z["f0_ref"].tobytes() == tracks[2]["f0"].tobytes() and np.array_equal(z["voiced_ref"], tracks[2]["voiced"])
    assert sorted(os.listdir(out)) == ["f0_distance.csv", "summary.json", "utt000.f0.npz", "utt002.f0.npz"]
    # the tracker's arguments reach it
    ac.run_driver("evaluate_f0.py", "--hparam-json-file", stats, "--backend", "numpy", "--pred-wav-dir", pred_dir, "--ref-wav-dir", ref_dir,
                  "--fmin", "80", "--fmax", "400", "--window-ms", "20", "--threshold", "0.1", "--silence-db", "40", out)
    par = dict(fmin=80.0, fmax=400.0, window_ms=20.0, threshold=0.1, silence_db=40.0)
    want2, _, _ = expected(au, keys, sp, sr_, mels[:2], mels[2:], **par)
    assert read_csv(os.path.join(out, "f0_distance.csv")) == want2
    s = json.load(open(os.path.join(out, "summary.json")))
    assert {k: s[k] for k in par} == par


def test_evaluate_f0_driver_on_prediction_records(tmp_path):
    pred, out = str(tmp_path / "pred"), str(tmp_path / "out")
    records = write_toy_records(pred)
    stats = write_stats(str(tmp_path / "hparams.json"))
    r = ac.run_driver("evaluate_f0.py", "--hparam-json-file", stats, "--backend", "numpy", "--iters", "4", "--seed", "3", pred, out)
    assert "utt002: no ground-truth mel, skipped" in r.stdout
    keys = [k for k in sorted(records) if records[k][1] is not None]
    au = audio.Audio(toy_hparams(), backend="numpy")
    mp, mr = [records[k][0] for k in keys], [records[k][1] for k in keys]
    wavs = au.inv_melspectrogram_batch([au.denormalize_mel(S.astype(np.float64)) for S in mp + mr], iters=4, seed=3)
    want, _, _ = expected(au, keys, wavs[:3], wavs[3:], mp, mr)
    assert read_csv(os.path.join(out, "f0_distance.csv")) == want
    s = json.load(open(os.path.join(out, "summary.json")))
    check_summary(s, want, "griffin_lim", ["utt002"])
    assert (s["iters"], s["seed"]) == (4, 3) and not [f for f in os.listdir(out) if f.endswith(".npz")]
    for key in keys:
        assert want[key]["frames_pred"] == len(records[key][0]) and want[key]["frames_ref"] == len(records[key][1])


def test_evaluate_f0_driver_refusals(tmp_path):
    stats = write_stats(str(tmp_path / "hparams.json"))
    pred = str(tmp_path / "pred")
    write_toy_records(pred, without_truth=tuple(PERIODS))
    r = ac.run_driver("evaluate_f0.py", "--hparam-json-file", stats, "--backend", "numpy", pred, check=False)
    assert r.returncode != 0 and "holds a ground-truth mel" in r.stderr
    r = ac.run_driver("evaluate_f0.py", "--hparam-json-file", stats, "--backend", "numpy", "--pred-wav-dir", pred, pred, check=False)
    assert r.returncode != 0 and "go together" in r.stderr
    r = ac.run_driver("evaluate_f0.py", "--hparam-json-file", stats, "--backend", "numpy", str(tmp_path), check=False)
    assert r.returncode != 0 and "no *.tfrecord" in r.stderr
    bare = str(tmp_path / "bare.json")
    with open(bare, "w") as f:
        json.dump(dict(num_mels=80, num_freq=513, sample_rate=16000), f)
    r = ac.run_driver("evaluate_f0.py", "--hparam-json-file", bare, "--backend", "numpy", pred, check=False)
    assert r.returncode != 0 and "average_mel_level_db" in r.stderr
