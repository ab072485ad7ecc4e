"""Fundamental frequency on the mel frame grid: YIN (de Cheveigne & Kawahara 2002), and the pitch metrics of two tracks along a DTW
path (DESIGN.md 3.6 holds the definition).  The tracker runs in csrc/yin.hip (backend "hip", a batch of utterances in one launch) or
in `yin_numpy`, a float32 restatement with the kernel's operations in the kernel's order: both agree bit for bit on f0, aperiodicity
and power.  The voicing decision and the metrics are host code, the same for both.

`track_f0` is the front of two trackers.  "yin" is plain YIN: every frame is decided alone, by the first dip of d' below the
threshold, which reports the octave above wherever the fundamental is weak.  "viterbi" keeps the K = 8 deepest dips of d' of every
frame as period candidates (csrc/yin.hip satt_yin_candidates / `yin_candidates_numpy`) and chooses among them and an "unvoiced"
state along the utterance by dynamic programming (csrc/f0_viterbi.hip / `f0_viterbi_numpy`): octave jumps between neighbouring
frames cost jump_cost.  Both stages are float32 without transcendental functions, and the two backends agree bit for bit on them as
well.  This is neither pYIN (no probabilities, no threshold prior) nor WORLD: values compare between runs of this tool only.
fmin, fmax, window_ms, threshold, silence_db and the four costs are arguments, not hparams."""
import math

import numpy as np

FMIN, FMAX, WINDOW_MS, THRESHOLD, SILENCE_DB = 60.0, 500.0, 25.0, 0.15, 50.0
YIN_MAX_WINDOW = 1536                 # satt_yin_max_window(): with the span and the lags of four frames in at most 57 KiB of LDS
YIN_MAX_LAG = 1023                    # satt_yin_max_lag(): four chunks of 256 lags, four lags a lane
YIN_MAX_HOP = 1 << 20
YIN_RUN = 16                          # satt_yin_run_length(): frames per workgroup, counted through the batch
F0_CANDIDATES = 8                     # SATT_F0_CANDIDATES: candidate slots of a frame; state 8 of the Viterbi tracker is "unvoiced"
F0_VITERBI_MAX_FRAMES = 2048          # satt_f0_viterbi_max_frames(): a predecessor byte per frame and state in 18 KiB of LDS
JUMP_COST, SWITCH_COST, LAG_BIAS = 0.3, 0.1, 0.1     # unvoiced_cost defaults to the threshold (profiles/f0_viterbi_defaults.txt)
TRACKERS = ("yin", "viterbi")


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


def silence_gate(power, silence_db=SILENCE_DB):
    """bool [T]: power > max_t(power) 10^(-silence_db / 10), in float64: the frames that may be voiced.  A signal whose largest
    power is 0 (or NaN) has none."""
    power = np.asarray(power, np.float64)
    if len(power) == 0:
        return np.zeros(0, bool)
    with np.errstate(invalid="ignore"):
        return power > power.max() * 10.0 ** (-silence_db / 10.0)


def voicing(f0, power, silence_db=SILENCE_DB):
    """bool [T]: f0 > 0 and silence_gate(power).  A signal whose largest power is 0 (or NaN) is all unvoiced; a NaN f0 is
    unvoiced."""
    f0 = np.asarray(f0, np.float64)
    if len(f0) == 0:
        return np.zeros(0, bool)
    with np.errstate(invalid="ignore"):
        return (f0 > 0) & silence_gate(power, silence_db)


# ---- the Viterbi tracker: candidates, path, front ----------------------------------------------------------------------------------------
def yin_candidates_pick_numpy(dp, tau_min, tau_max):
    """(cand_period, cand_value) float32 [T, 8] from d' [T, tau_max + 1]: the dips of [tau_min, tau_max - 1], the 8 with the smallest
    d' (ties to the smaller lag) in ascending lag order, each with the parabola and clamp of the YIN pick; unused slots 0 and +inf"""
    T, K = len(dp), F0_CANDIDATES
    per, val = np.zeros((T, K), np.float32), np.full((T, K), np.inf, np.float32)
    with np.errstate(all="ignore"):
        mid = dp[:, tau_min:tau_max]
        dips = (mid < dp[:, tau_min - 1:tau_max - 1]) & (mid <= dp[:, tau_min + 1:tau_max + 1])
        for t in np.nonzero(dips.any(axis=1))[0]:
            row = dp[t]
            k = tau_min + np.nonzero(dips[t])[0]
            k = np.sort(k[np.lexsort((k, row[k]))[:K]])                # by (d', lag), the first 8, then by lag
            a, b, c = row[k - 1], row[k], row[k + 1]
            num, den = a - c, (a - b) + (c - b)
            shift = (np.float32(0.5) * num) / den
            shift = np.where(shift > 1, np.float32(1.0), shift)
            shift = np.where(shift < -1, np.float32(-1.0), shift)
            shift = np.where(den > 0, shift, np.float32(0.0)).astype(np.float32)
            per[t, :len(k)] = k.astype(np.float32) + shift
            val[t, :len(k)] = b
    return per, val


def yin_candidates_numpy(y, sr, hop, fmin=FMIN, fmax=FMAX, window_ms=WINDOW_MS):
    """(cand_period [T, 8], cand_value [T, 8], power [T]), float32, T = 1 + n // hop, of one signal: the bits of csrc/yin.hip
    satt_yin_candidates"""
    _, tau_min, tau_max = yin_check(sr, hop, fmin, fmax, window_ms)
    dp, power = yin_dprime_numpy(y, sr, hop, fmin, fmax, window_ms)
    per, val = yin_candidates_pick_numpy(dp, tau_min, tau_max)
    return per, val, power


def f0_viterbi_check(frames, jump_cost, switch_cost, unvoiced_cost, lag_bias):
    """ValueError when neither backend takes an utterance of `frames` frames or these costs"""
    if not 1 <= frames <= F0_VITERBI_MAX_FRAMES:
        raise ValueError("f0_viterbi: an utterance of %d frames; supported are 1 <= frames <= %d" % (frames, F0_VITERBI_MAX_FRAMES))
    for name, c in (("jump_cost", jump_cost), ("switch_cost", switch_cost), ("unvoiced_cost", unvoiced_cost), ("lag_bias", lag_bias)):
        if not (0.0 <= np.float32(c) < np.inf):
            raise ValueError("f0_viterbi: %s=%r must be finite and >= 0" % (name, c))


def _table(cand_period, cand_value, gate):
    per, val = np.ascontiguousarray(cand_period, np.float32), np.ascontiguousarray(cand_value, np.float32)
    gate = np.ascontiguousarray(np.asarray(gate) != 0, np.uint8)
    if per.ndim != 2 or per.shape[1] != F0_CANDIDATES or val.shape != per.shape or gate.shape != per.shape[:1]:
        raise ValueError("f0_viterbi: need cand_period and cand_value [T, %d] and gate [T], got shapes %r, %r and %r"
                         % (F0_CANDIDATES, per.shape, val.shape, gate.shape))
    return per, val, gate


def f0_viterbi_numpy(cand_period, cand_value, gate, sr, tau_max, jump_cost=JUMP_COST, switch_cost=SWITCH_COST, unvoiced_cost=THRESHOLD,
                     lag_bias=LAG_BIAS):
    """(f0 float32 [T], state uint8 [T], cost float32) of one utterance's candidate tables: the bits of csrc/f0_viterbi.hip.  The
    costs of all steps at once, then the chain one frame at a time."""
    per, val, gate = _table(cand_period, cand_value, gate)
    T, K, F = len(per), F0_CANDIDATES, np.float32
    f0_viterbi_check(T, jump_cost, switch_cost, unvoiced_cost, lag_bias)
    inf = F(np.inf)
    with np.errstate(all="ignore"):
        obs = np.full((T, K + 1), F(unvoiced_cost), np.float32)
        used = (gate[:, None] != 0) & (per > 0)
        obs[:, :K] = np.where(used, val + F(lag_bias) * (per / F(tau_max)), inf)
        trans = np.full((max(T - 1, 0), K + 1, K + 1), F(switch_cost), np.float32)     # [t - 1, q, j]: from q of t - 1 to j of t
        trans[:, K, K] = 0
        pq, pj = per[:-1, :, None], per[1:, None, :]
        up = pq > pj
        trans[:, :K, :K] = F(jump_cost) * (np.where(up, pq, pj) / np.where(up, pj, pq) - F(1.0))
        pred = np.full((T, K + 1), K, np.uint8)
        delta, cols = obs[0].copy(), np.arange(K + 1)
        for t in range(1, T):
            v = delta[:, None] + trans[t - 1]
            v[np.isnan(v)] = inf                                        # a strict < from +inf passes NaN and +inf over
            arg = np.argmin(v, axis=0)                                  # the first minimum: the smaller q
            best = v[arg, cols]
            pred[t] = np.where(best < inf, arg, K)
            delta = best + obs[t]
        v = np.where(np.isnan(delta), inf, delta)
        end = int(np.argmin(v)) if v.min() < inf else K
        state = np.empty(T, np.uint8)
        s = end
        for t in range(T - 1, -1, -1):
            state[t] = s
            s = int(pred[t, s])
        cand = state < K
        f0 = np.zeros(T, np.float32)
        f0[cand] = F(sr) / per[cand, state[cand]]
        return f0, state, F(v[end])


def _groups(items, sizes, budget):
    """`items` cut into consecutive groups whose sizes add up to at most `budget` (one item always goes out)"""
    group, count = [], 0
    for it, n in zip(items, sizes):
        if group and count + n > budget:
            yield group
            group, count = [], 0
        group.append(it)
        count += n
    if group:
        yield group


def _budget(max_launch_samples):
    from .audio import MAX_LAUNCH_SAMPLES
    return MAX_LAUNCH_SAMPLES if max_launch_samples is None else int(max_launch_samples)


def _candidates_launch(signals, hop, W, tau_min, tau_max, device):
    import torch
    from .. import ops
    lens = np.asarray([len(s) for s in signals], np.int64)
    io = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    fo = np.concatenate([[0], np.cumsum(1 + lens // hop)]).astype(np.int64)
    x = torch.from_numpy(np.concatenate(signals)).to(device)
    total = int(fo[-1])
    per, val = (torch.empty((total, F0_CANDIDATES), dtype=torch.float32, device=device) for _ in range(2))
    power = torch.empty(total, dtype=torch.float32, device=device)
    ops.yin_candidates(x, torch.from_numpy(io).to(device), torch.from_numpy(fo).to(device), W, tau_min, tau_max, hop, per, val, power)
    per, val, power = (o.cpu().numpy() for o in (per, val, power))
    return [(per[fo[u]:fo[u + 1]], val[fo[u]:fo[u + 1]], power[fo[u]:fo[u + 1]]) for u in range(len(signals))]


def yin_candidates_hip(signals, sr, hop, fmin=FMIN, fmax=FMAX, window_ms=WINDOW_MS, device="cuda", max_launch_samples=None):
    """csrc/yin.hip satt_yin_candidates over `signals`: the list of (cand_period, cand_value, power), in input order.  One launch for
    the batch, cut only where it would exceed `max_launch_samples` (default audio.MAX_LAUNCH_SAMPLES; one signal always goes out)."""
    W, tau_min, tau_max = yin_check(sr, hop, fmin, fmax, window_ms)
    signals = [_signal(s) for s in signals]
    out = []
    for group in _groups(signals, [len(s) for s in signals], _budget(max_launch_samples)):
        out += _candidates_launch(group, hop, W, tau_min, tau_max, device)
    return out


def _viterbi_launch(tables, sr, tau_max, costs, device):
    import torch
    from .. import ops
    lens = np.asarray([len(t[0]) for t in tables], np.int64)
    fo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    per, val, gate = (torch.from_numpy(np.concatenate([t[i] for t in tables])).to(device) for i in range(3))
    f0 = torch.empty(int(fo[-1]), dtype=torch.float32, device=device)
    state = torch.empty(int(fo[-1]), dtype=torch.uint8, device=device)
    cost = torch.empty(len(tables), dtype=torch.float32, device=device)
    ops.f0_viterbi(per, val, gate, torch.from_numpy(fo).to(device), int(lens.max()), tau_max, sr, *costs, f0, state, cost)
    f0, state, cost = (o.cpu().numpy() for o in (f0, state, cost))
    return [(f0[fo[u]:fo[u + 1]], state[fo[u]:fo[u + 1]], cost[u]) for u in range(len(tables))]


def f0_viterbi_hip(tables, sr, tau_max, jump_cost=JUMP_COST, switch_cost=SWITCH_COST, unvoiced_cost=THRESHOLD, lag_bias=LAG_BIAS,
                   device="cuda", max_launch_samples=None):
    """csrc/f0_viterbi.hip over `tables`, a list of (cand_period [T, 8], cand_value [T, 8], gate [T]): the list of (f0, state, cost),
    in input order.  One launch for the batch, cut only where its frames would exceed `max_launch_samples` (default
    audio.MAX_LAUNCH_SAMPLES; one utterance always goes out)."""
    tables = [_table(*t) for t in tables]
    for t in tables:
        f0_viterbi_check(len(t[0]), jump_cost, switch_cost, unvoiced_cost, lag_bias)
    out = []
    for group in _groups(tables, [len(t[0]) for t in tables], _budget(max_launch_samples)):
        out += _viterbi_launch(group, sr, tau_max, (jump_cost, switch_cost, unvoiced_cost, lag_bias), device)
    return out


def track_f0(signals, sr, hop, fmin=FMIN, fmax=FMAX, window_ms=WINDOW_MS, threshold=THRESHOLD, silence_db=SILENCE_DB, tracker="yin",
             jump_cost=JUMP_COST, switch_cost=SWITCH_COST, unvoiced_cost=None, lag_bias=LAG_BIAS, backend="numpy", device="cuda",
             max_launch_samples=None, with_state=False):
    """the list of (f0, aperiodicity, power, voiced) of `signals` (with_state: and the state track, uint8, under "viterbi").
    tracker "yin": the YIN pick and voicing().  tracker "viterbi": the candidates of every frame, gate = silence_gate(power), the
    cheapest path; voiced is state != 8 and aperiodicity the chosen slot's value, in state 8 the frame's smallest candidate value
    (+inf without a candidate).  unvoiced_cost defaults to the threshold, which plain YIN alone uses otherwise.  backend "hip"
    runs the kernels, "numpy" their float32 restatements: the same bits."""
    if tracker not in TRACKERS:
        raise ValueError("track_f0: tracker=%r is none of %r" % (tracker, TRACKERS))
    if backend not in ("hip", "numpy"):
        raise ValueError("track_f0: backend=%r is neither 'hip' nor 'numpy'" % (backend,))
    _, _, tau_max = yin_check(sr, hop, fmin, fmax, window_ms)
    signals = [_signal(s) for s in signals]
    if not signals:
        return []
    par = dict(fmin=fmin, fmax=fmax, window_ms=window_ms)
    if tracker == "yin":
        if backend == "numpy":
            res = [yin_numpy(y, sr, hop, threshold=threshold, **par) for y in signals]
        else:
            res = yin_hip(signals, sr, hop, threshold=threshold, device=device, max_launch_samples=max_launch_samples, **par)
        return [(f0, ap, power, voicing(f0, power, silence_db)) for f0, ap, power in res]
    costs = dict(jump_cost=jump_cost, switch_cost=switch_cost, unvoiced_cost=threshold if unvoiced_cost is None else unvoiced_cost,
                 lag_bias=lag_bias)
    for y in signals:
        f0_viterbi_check(1 + len(y) // hop, **costs)
    if backend == "numpy":
        cands = [yin_candidates_numpy(y, sr, hop, **par) for y in signals]
    else:
        cands = yin_candidates_hip(signals, sr, hop, device=device, max_launch_samples=max_launch_samples, **par)
    tables = [(per, val, silence_gate(power, silence_db)) for per, val, power in cands]
    if backend == "numpy":
        paths = [f0_viterbi_numpy(*t, sr, tau_max, **costs) for t in tables]
    else:
        paths = f0_viterbi_hip(tables, sr, tau_max, device=device, max_launch_samples=max_launch_samples, **costs)
    out = []
    for (per, val, power), (f0, state, _) in zip(cands, paths):
        voiced = state != F0_CANDIDATES
        ap = val.min(axis=1)                                            # unused slots hold +inf
        ap[voiced] = val[voiced, state[voiced]]
        out.append((f0, ap, power, voiced) + ((state,) if with_state else ()))
    return out


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
