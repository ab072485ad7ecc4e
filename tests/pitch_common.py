"""Shared yardstick of the pitch tests (test_yin_cpu / test_yin_gpu): a float64 programme of the YIN formulas of DESIGN.md 3.6,
written frame by frame from the definition (it shares no code with utils/pitch.py), the seeded tone set, and the bounds both
backends are held to.

The bounds are 8 x the float32 NumPy backend's own measured deviation from the float64 programme over tone_set() (the rule
profiles/melspec_tolerances.txt states); profiles/yin_tolerances.txt holds the measured values (tools/yin_tolerances.py):
    E_DPRIME  max |d' - d'64| / max(1, d'64) over all frames and lags
    E_POWER   max |power - power64| / max_t(power64) over the frames of a signal
    E_F0      max |f0 / f064 - 1| over the frames whose float64 decision is robust (both backends voiced there)
A frame's float64 decision is robust when tau0 (or its absence) and tau* are the same at threshold - 1e-4, threshold and
threshold + 1e-4; on a robust frame the backends must agree with the float64 programme on voiced / unvoiced.  At most SKIP_MAX of
the frames may fail to be robust: tone_set() is chosen so that the float64 programme alone keeps that condition.

CENTS_BOUND is 2 x the float64 programme's own worst error against the known periods of tone_set(), in cents."""
import math

import numpy as np

CONFIGS = [(16000, 200), (22050, 275), (48000, 600)]          # (sample rate, hop)
FMIN, FMAX, WINDOW_MS, THRESHOLD = 60.0, 500.0, 25.0, 0.15
E_DPRIME_NUMPY, E_POWER_NUMPY, E_F0_NUMPY = 3.3e-6, 1.4e-6, 1.7e-6    # measured, rounded up (profiles/yin_tolerances.txt)
C_DPRIME, C_POWER, C_F0 = 8 * E_DPRIME_NUMPY, 8 * E_POWER_NUMPY, 8 * E_F0_NUMPY
CENTS_64 = 0.6                                                # the float64 programme's worst error on tone_set(), rounded up
CENTS_BOUND = 2 * CENTS_64
SKIP_MAX = 0.05
LEAD_S, TONE_S = 0.12, 0.30                                   # seconds of noise lead-in and of tone


def sizes(sr):
    """(W, tau_min, tau_max) by the definition"""
    return int(math.floor(sr * WINDOW_MS / 1000.0 + 0.5)), int(sr // FMAX), int(-(-sr // FMIN))


def pick64(dp, sr, tau_min, tau_max, threshold):
    """(tau0 or None, tau* or None, f0, aperiodicity) of one row of d'"""
    tau0 = next((t for t in range(tau_min, tau_max) if dp[t] < threshold), None)
    if tau0 is None:
        return None, None, 0.0, float(min(dp[tau_min:tau_max + 1]))
    t = tau0
    while t + 1 <= tau_max - 1 and dp[t + 1] < dp[t]:
        t += 1
    a, b, c = dp[t - 1], dp[t], dp[t + 1]
    curv = a - 2.0 * b + c
    shift = min(1.0, max(-1.0, 0.5 * (a - c) / curv)) if curv > 0 else 0.0
    return tau0, t, sr / (t + shift), float(b)


def yin64(y, sr, hop, threshold=THRESHOLD):
    """dict of float64 arrays dprime [T, tau_max + 1], power, f0, aperiodicity [T] and robust (bool [T]) of one signal"""
    x = np.asarray(y, np.float64)
    n = len(x)
    W, tau_min, tau_max = sizes(sr)
    T = 1 + n // hop
    dprime, power, f0, ap, robust = np.ones((T, tau_max + 1)), np.zeros(T), np.zeros(T), np.zeros(T), np.zeros(T, bool)
    for t in range(T):
        s = t * hop - (W + tau_max) // 2
        seg = np.zeros(W + tau_max)
        lo, hi = max(s, 0), min(s + W + tau_max, n)
        if hi > lo:
            seg[lo - s:hi - s] = x[lo:hi]
        head = seg[:W]
        d = np.asarray([np.sum((head - seg[tau:tau + W]) ** 2) for tau in range(tau_max + 1)])
        power[t] = np.sum(head * head) / W
        run = np.cumsum(d[1:])
        for tau in range(1, tau_max + 1):
            dprime[t, tau] = d[tau] * tau / run[tau - 1] if run[tau - 1] > 0 else 1.0
        picks = [pick64(dprime[t], sr, tau_min, tau_max, thr) for thr in (threshold, threshold - 1e-4, threshold + 1e-4)]
        _, _, f0[t], ap[t] = picks[0]
        robust[t] = all(p[:2] == picks[0][:2] for p in picks[1:])
    return dict(dprime=dprime, power=power, f0=f0, aperiodicity=ap, robust=robust)


def tone(sr, period, seed, lead_s=LEAD_S, tone_s=TONE_S):
    """float32: lead_s of Gaussian noise (sigma 3e-3), then tone_s of five harmonics (1 / k) of sr / period Hz at 0.4 with noise of
    sigma 1e-3 on top"""
    rng = np.random.default_rng(seed)
    n0, n1 = int(lead_s * sr), int(tone_s * sr)
    k = np.arange(n1)
    y = sum(0.4 / h * np.sin(2.0 * np.pi * h * k / period + 0.9 * h) for h in range(1, 6))
    return np.concatenate([3e-3 * rng.standard_normal(n0), y + 1e-3 * rng.standard_normal(n1)]).astype(np.float32)


def periods(sr):
    """non-integer periods in samples across the lag range: one just inside tau_min, one just inside tau_max - 1 (the longest lag
    the pick may return), four between"""
    _, tau_min, tau_max = sizes(sr)
    inner = [tau_min + (tau_max - tau_min) * f + 0.37 for f in (0.08, 0.22, 0.45, 0.7)]
    return [tau_min + 0.6] + inner + [tau_max - 2.4]


def outside(sr):
    """(a period below tau_min, a period above tau_max).  The first is found at twice the period (the sub-octave: the first lag in
    range at which the signal repeats), the second not at all.  Both lie a fifth of the range's end away: a few samples outside,
    d' still passes the threshold at the end lag itself."""
    _, tau_min, tau_max = sizes(sr)
    return 0.8 * tau_min + 0.3, 1.15 * tau_max + 0.6


def frame_sets(sr, hop, n, lead_s=LEAD_S):
    """(frames whose whole span lies in the lead-in, frames whose whole span lies in the tone) of a tone() signal of n samples"""
    W, _, tau_max = sizes(sr)
    n0 = int(lead_s * sr)
    t = np.arange(1 + n // hop)
    s = t * hop - (W + tau_max) // 2
    return t[(s >= 0) & (s + W + tau_max <= n0)], t[(s >= n0) & (s + W + tau_max <= n)]


_TONES = {}


def tone_set(sr, hop):
    """[(period, signal, float64 result)] of periods(sr), computed once"""
    if (sr, hop) not in _TONES:
        _TONES[sr, hop] = [(p, y, yin64(y, sr, hop)) for p, y in ((p, tone(sr, p, 100 + i)) for i, p in enumerate(periods(sr)))]
    return _TONES[sr, hop]


def cents(f, period, sr):
    return 1200.0 * np.log2(np.asarray(f, np.float64) * period / sr)


def deviations(f0, ap, power, dprime, ref):
    """(E_DPRIME or None without dprime, E_POWER, E_F0, share of frames that are not robust) of one backend result against yin64's;
    asserts the voicing agreement on the robust frames"""
    r = ref["robust"]
    f0 = np.asarray(f0, np.float64)
    assert np.array_equal(f0[r] > 0, ref["f0"][r] > 0), "voiced / unvoiced differs on a frame whose float64 decision is robust"
    both = r & (ref["f0"] > 0)
    e_f0 = float(np.abs(f0[both] / ref["f0"][both] - 1.0).max()) if both.any() else 0.0
    e_ap = float((np.abs(np.asarray(ap, np.float64)[r] - ref["aperiodicity"][r]) / np.maximum(1.0, ref["aperiodicity"][r])).max()) if r.any() else 0.0
    top = ref["power"].max()
    e_pw = float(np.abs(np.asarray(power, np.float64) - ref["power"]).max() / top) if top > 0 else float(np.abs(power).max())
    e_dp = None
    if dprime is not None:
        e_dp = float((np.abs(np.asarray(dprime, np.float64) - ref["dprime"]) / np.maximum(1.0, ref["dprime"])).max())
    return e_dp, max(e_pw, 0.0), e_f0, e_ap, 1.0 - float(r.mean())


def check_against_float64(f0, ap, power, dprime, ref, what=""):
    """the bounds of the module docstring for one backend result; aperiodicity is d' at tau*, held to the d' bound on robust frames"""
    e_dp, e_pw, e_f0, e_ap, skipped = deviations(f0, ap, power, dprime, ref)
    print("%s d' %s  power %.3e  f0 %.3e  aperiodicity %.3e  not robust %.3f" % (what, "%.3e" % e_dp if e_dp is not None else "-", e_pw, e_f0, e_ap, skipped))
    assert e_dp is None or e_dp <= C_DPRIME, (e_dp, C_DPRIME)
    assert e_ap <= C_DPRIME, (e_ap, C_DPRIME)
    assert e_pw <= C_POWER, (e_pw, C_POWER)
    assert e_f0 <= C_F0, (e_f0, C_F0)
    return e_dp, e_pw, e_f0, e_ap, skipped
