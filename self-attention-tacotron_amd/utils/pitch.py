"""Fundamental frequency on the mel frame grid: YIN (de Cheveigne & Kawahara 2002), and the pitch metrics of two tracks along a DTW
path (DESIGN.md 3.6 holds the definition).  The tracker runs in csrc/yin.hip (backend "hip", a batch of utterances in one launch) or
in `yin_numpy`, a float32 restatement with the kernel's operations in the kernel's order: both agree bit for bit on f0, aperiodicity
and power.  The voicing decision and the metrics are host code, the same for both.

This is plain YIN: no octave-error smoothing, no pYIN / Viterbi, not WORLD.  Its values compare between runs of this tool only.
fmin, fmax, window_ms, threshold and silence_db are arguments, not hparams."""
import math

import numpy as np

FMIN, FMAX, WINDOW_MS, THRESHOLD, SILENCE_DB = 60.0, 500.0, 25.0, 0.15, 50.0
YIN_MAX_WINDOW = 1536                 # satt_yin_max_window(): with the span and the lags of four frames in at most 57 KiB of LDS
YIN_MAX_LAG = 1023                    # satt_yin_max_lag(): four chunks of 256 lags, four lags a lane
YIN_MAX_HOP = 1 << 20
YIN_RUN = 16                          # satt_yin_run_length(): frames per workgroup, counted through the batch


def yin_supported(window, tau_max, hop):
    """the predicate of satt_yin_supported, evaluated here so that both backends refuse the same sizes"""
    return 1 <= window <= YIN_MAX_WINDOW and 3 <= tau_max <= YIN_MAX_LAG and 1 <= hop <= YIN_MAX_HOP


def yin_sizes(sr, fmin=FMIN, fmax=FMAX, window_ms=WINDOW_MS):
    """(W, tau_min, tau_max) = (round(sr window_ms / 1000), floor(sr / fmax), ceil(sr / fmin))"""
    return int(math.floor(sr * window_ms / 1000.0 + 0.5)), int(math.floor(sr / fmax)), int(math.ceil(sr / fmin))


def yin_check(sr, hop, fmin=FMIN, fmax=FMAX, window_ms=WINDOW_MS):
    """(W, tau_min, tau_max), or ValueError naming the sizes when neither backend takes them"""
    if not (sr > 0 and fmin > 0 and fmax > fmin and window_ms > 0):
        raise ValueError("yin: need sr > 0, 0 < fmin < fmax and window_ms > 0, got sr=%r fmin=%r fmax=%r window_ms=%r" % (sr, fmin, fmax, window_ms))
    W, tau_min, tau_max = yin_sizes(sr, fmin, fmax, window_ms)
    if tau_min < 2 or tau_min >= tau_max:
        raise ValueError("yin: sr=%d fmin=%g fmax=%g give lags %d .. %d; need 2 <= floor(sr / fmax) < ceil(sr / fmin)" % (sr, fmin, fmax, tau_min, tau_max))
    if not yin_supported(W, tau_max, hop):
        raise ValueError("yin: sr=%d fmin=%g window_ms=%g hop=%d give window=%d tau_max=%d; supported are 1 <= window <= %d, "
                         "3 <= tau_max <= %d, 1 <= hop <= %d" % (sr, fmin, window_ms, hop, W, tau_max, YIN_MAX_WINDOW, YIN_MAX_LAG, YIN_MAX_HOP))
    return W, tau_min, tau_max


def _signal(y):
    y = np.ascontiguousarray(y, np.float32)
    if y.ndim != 1 or len(y) < 1:
        raise ValueError("yin: need a one-dimensional signal of at least one sample, got shape %r" % (y.shape,))
    return y


def yin_dprime_numpy(y, sr, hop, fmin=FMIN, fmax=FMAX, window_ms=WINDOW_MS):
    """(d' float32 [T, tau_max + 1], power float32 [T]) of one signal with the kernel's operations in the kernel's order: the sums
    over j ascending, whole [T, lags] arrays at a time; difference, product and sum each rounded to float32"""
    W, tau_min, tau_max = yin_check(sr, hop, fmin, fmax, window_ms)
    y = _signal(y)
    n, L = len(y), tau_max + 1
    T, off = 1 + n // hop, (W + tau_max) // 2
    xp = np.zeros(off + n + W + tau_max, np.float32)             # x[k] at k + off, zeros around it
    xp[off:off + n] = y
    V = np.lib.stride_tricks.as_strided(xp, (T, W + tau_max), (hop * xp.itemsize, xp.itemsize), writeable=False)   # V[t, e] = x[s_t + e]
    D, P = np.zeros((T, L), np.float32), np.zeros(T, np.float32)
    df, sq = np.empty((T, L), np.float32), np.empty(T, np.float32)
    with np.errstate(all="ignore"):
        for j in range(W):
            np.subtract(V[:, j:j + 1], V[:, j:j + L], out=df)
            np.multiply(df, df, out=df)
            np.add(D, df, out=D)
            np.multiply(V[:, j], V[:, j], out=sq)
            np.add(P, sq, out=P)
        c = np.add.accumulate(D[:, 1:], axis=1, dtype=np.float32)       # c(tau) = c(tau - 1) + d(tau): one ascending chain
        q = (D[:, 1:] * np.arange(1, L, dtype=np.float32)) / c
        dp = np.ones((T, L), np.float32)
        dp[:, 1:] = np.where(c > 0, q, np.float32(1.0))
        return dp, P / np.float32(W)


def yin_pick_numpy(dp, sr, tau_min, tau_max, threshold=THRESHOLD):
    """(f0, aperiodicity) float32 [T] from d' [T, tau_max + 1]: the pick and the parabola of DESIGN.md 3.6 in float32"""
    T = len(dp)
    thr = np.float32(threshold)
    f0, ap = np.zeros(T, np.float32), np.empty(T, np.float32)
    with np.errstate(all="ignore"):
        below = dp[:, tau_min:tau_max] < thr
        has = below.any(axis=1)
        low = np.fmin.reduce(dp[:, tau_min:tau_max + 1], axis=1, initial=np.float32(np.inf))
        for t in range(T):
            if not has[t]:
                ap[t] = low[t]
                continue
            row = dp[t]
            k = tau_min + int(np.argmax(below[t]))
            while k + 1 <= tau_max - 1 and row[k + 1] < row[k]:
                k += 1
            a, b, c = row[k - 1], row[k], row[k + 1]
            num, den = a - c, (a - b) + (c - b)
            shift = np.float32(0.0)
            if den > 0:
                shift = (np.float32(0.5) * num) / den
                if shift > 1:
                    shift = np.float32(1.0)
                if shift < -1:
                    shift = np.float32(-1.0)
            ap[t] = b
            f0[t] = np.float32(sr) / (np.float32(k) + shift)
    return f0, ap


def yin_numpy(y, sr, hop, fmin=FMIN, fmax=FMAX, window_ms=WINDOW_MS, threshold=THRESHOLD):
    """(f0, aperiodicity, power), float32 [1 + n // hop] each, of one signal: the bits of csrc/yin.hip"""
    _, tau_min, tau_max = yin_check(sr, hop, fmin, fmax, window_ms)
    dp, power = yin_dprime_numpy(y, sr, hop, fmin, fmax, window_ms)
    f0, ap = yin_pick_numpy(dp, sr, tau_min, tau_max, threshold)
    return f0, ap, power


def _yin_launch(signals, sr, hop, W, tau_min, tau_max, threshold, device):
    import torch
    from .. import ops
    lens = np.asarray([len(s) for s in signals], np.int64)
    io = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    fo = np.concatenate([[0], np.cumsum(1 + lens // hop)]).astype(np.int64)
    x = torch.from_numpy(np.concatenate(signals)).to(device)
    out = [torch.empty(int(fo[-1]), dtype=torch.float32, device=device) for _ in range(3)]
    ops.yin(x, torch.from_numpy(io).to(device), torch.from_numpy(fo).to(device), W, tau_min, tau_max, hop, sr, threshold, *out)
    f0, ap, power = (o.cpu().numpy() for o in out)
    return [(f0[fo[u]:fo[u + 1]], ap[fo[u]:fo[u + 1]], power[fo[u]:fo[u + 1]]) for u in range(len(signals))]


def yin_hip(signals, sr, hop, fmin=FMIN, fmax=FMAX, window_ms=WINDOW_MS, threshold=THRESHOLD, device="cuda", max_launch_samples=None):
    """csrc/yin.hip over `signals` (float32 arrays of >= 1 sample at rate sr): the list of (f0, aperiodicity, power), in input
    order.  One launch for the batch, cut only where it would exceed `max_launch_samples` (default audio.MAX_LAUNCH_SAMPLES; one
    signal always goes out)."""
    from .audio import MAX_LAUNCH_SAMPLES
    W, tau_min, tau_max = yin_check(sr, hop, fmin, fmax, window_ms)
    signals = [_signal(s) for s in signals]
    budget = MAX_LAUNCH_SAMPLES if max_launch_samples is None else int(max_launch_samples)
    out, group, count = [], [], 0
    for s in signals:
        if group and count + len(s) > budget:
            out += _yin_launch(group, sr, hop, W, tau_min, tau_max, threshold, device)
            group, count = [], 0
        group.append(s)
        count += len(s)
    if group:
        out += _yin_launch(group, sr, hop, W, tau_min, tau_max, threshold, device)
    return out


def voicing(f0, power, silence_db=SILENCE_DB):
    """bool [T]: f0 > 0 and power > max_t(power) 10^(-silence_db / 10), in float64.  A signal whose largest power is 0 (or NaN) is
    all unvoiced; a NaN f0 is unvoiced."""
    f0, power = np.asarray(f0, np.float64), np.asarray(power, np.float64)
    if len(power) == 0:
        return np.zeros(0, bool)
    with np.errstate(invalid="ignore"):
        return (f0 > 0) & (power > power.max() * 10.0 ** (-silence_db / 10.0))


def f0_metrics(f0_pred, v_pred, f0_ref, v_ref, path):
    """the pitch metrics of a predicted and a reference track along a DTW path [steps, 2] of (predicted frame, reference frame), in
    float64: steps; vuv_error, the share of steps whose voicing differs; voiced_both, the steps voiced on both sides, and over
    those f0_rmse_cents (of 1200 log2(fp / fr)), f0_rmse_hz, log_f0_corr (Pearson on ln f0; None below 2 steps or at zero
    variance) and gpe (the share with |fp / fr - 1| > 0.2).  Without a step voiced on both sides the four are None."""
    path = np.asarray(path, np.int64).reshape(-1, 2)
    i, j = path[:, 0], path[:, 1]
    vp, vr = np.asarray(v_pred, bool)[i], np.asarray(v_ref, bool)[j]
    both = vp & vr
    steps, nb = len(path), int(both.sum())
    out = dict(steps=steps, voiced_both=nb, vuv_error=float(np.mean(vp != vr)) if steps else None,
               f0_rmse_cents=None, f0_rmse_hz=None, log_f0_corr=None, gpe=None)
    if nb == 0:
        return out
    fp, fr = np.asarray(f0_pred, np.float64)[i][both], np.asarray(f0_ref, np.float64)[j][both]
    cents = 1200.0 * np.log2(fp / fr)
    out["f0_rmse_cents"] = float(np.sqrt(np.mean(cents * cents)))
    out["f0_rmse_hz"] = float(np.sqrt(np.mean((fp - fr) ** 2)))
    out["gpe"] = float(np.mean(np.abs(fp / fr - 1.0) > 0.2))
    if nb >= 2:
        lp, lr = np.log(fp), np.log(fr)
        lp, lr = lp - lp.mean(), lr - lr.mean()
        den = math.sqrt(float(lp @ lp) * float(lr @ lr))
        if den > 0.0:
            out["log_f0_corr"] = float(lp @ lr) / den
    return out
