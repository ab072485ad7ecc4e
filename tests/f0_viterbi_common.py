"""Shared yardsticks of the Viterbi pitch tracker's tests (test_f0_viterbi_cpu / test_f0_viterbi_gpu): the trap signal whose
fundamental is weak for 0.3 s, a scalar float32 programme of the candidate rule of DESIGN.md 3.6 (one operation at a time from d';
it shares no code with utils/pitch.py's pick), a float64 enumeration of ALL paths through a small table, and seeded candidate
tables on a coarse grid.  Nothing here is measured from the code under test."""
import itertools

import numpy as np

K = 8                                                          # candidate slots; state K is "unvoiced"
SR, HOP, N = 16000, 200, 16000


# ---- the trap signal ---------------------------------------------------------------------------------------------------------------------
def trap():
    """(y float32 [16000], truth f0 [81], judged frames (61), frames voiced in truth): a glide between 118 and 166 Hz whose
    fundamental lies 22 dB below its second harmonic from 0.3 s to 0.6 s, silent for its first and last 0.1 s"""
    t = np.arange(N) / SR
    f = 140.0 * 2.0 ** (0.25 * np.sin(2.0 * np.pi * 1.5 * t))
    ph = 2.0 * np.pi * np.cumsum(f) / SR
    mid = (0.3 < t) & (t < 0.6)
    y = (np.where(mid, 0.08, 0.6) * np.sin(ph) + np.sin(2.0 * ph + 0.7) + np.where(mid, 0.0, 0.3) * np.sin(3.0 * ph + 1.1)
         + 0.02 * np.random.default_rng(0).standard_normal(N))
    y[:SR // 10] = 0.0
    y[-(SR // 10):] = 0.0
    i = np.arange(1 + N // HOP)
    at = i * HOP / SR
    truth = f[np.minimum(i * HOP, N - 1)]
    return y.astype(np.float32), truth, (0.12 < at) & (at < 0.88), (0.1 <= at) & (at < 0.9)


def gpe(f0, truth, judged):
    """the share of the judged frames whose f0 is off by more than 20 % (an unvoiced frame, f0 = 0, is off by 100 %)"""
    return float(np.mean(np.abs(np.asarray(f0, np.float64)[judged] / truth[judged] - 1.0) > 0.2))


def edge_distance(frames):
    """frames from 0.1 s or 0.9 s, whichever is nearer"""
    return np.minimum(np.abs(frames - 0.1 * SR / HOP), np.abs(frames - 0.9 * SR / HOP))


# ---- the candidate rule, one float32 operation at a time ---------------------------------------------------------------------------------
def candidates32(dp, tau_min, tau_max):
    """(period, value) float32 [T, 8] from d' [T, tau_max + 1]"""
    F = np.float32
    per, val = np.zeros((len(dp), K), np.float32), np.full((len(dp), K), np.inf, np.float32)
    with np.errstate(all="ignore"):
        for t, row in enumerate(dp):
            dips = [k for k in range(tau_min, tau_max) if row[k] < row[k - 1] and row[k] <= row[k + 1]]
            dips.sort(key=lambda k: (float(row[k]), k))
            for c, k in enumerate(sorted(dips[:K])):
                a, b, c3 = F(row[k - 1]), F(row[k]), F(row[k + 1])
                num, den = F(a - c3), F(F(a - b) + F(c3 - b))
                off = F(0)
                if den > 0:
                    off = F(F(F(0.5) * num) / den)
                    off = F(1) if off > 1 else (F(-1) if off < -1 else off)
                per[t, c], val[t, c] = F(F(k) + off), b
    return per, val


# ---- every path, in float64 --------------------------------------------------------------------------------------------------------------
def enumerate_paths(per, val, gate, tau_max, jump, switch, unvoiced, bias):
    """[(cost, path)] of all 9^T paths with a finite cost, cheapest first (ties by path): the definition in float64.  With costs on
    a grid of 1/64 and the periods of exact_table() every sum is exact in float32 as well."""
    T = len(per)
    per, val = np.asarray(per, np.float64), np.asarray(val, np.float64)

    def obs(t, j):
        if j == K:
            return unvoiced
        return val[t, j] + bias * (per[t, j] / tau_max) if gate[t] and per[t, j] > 0 else np.inf

    def trans(t, q, j):
        if q == K or j == K:
            return 0.0 if q == j else switch
        hi, lo = max(per[t - 1, q], per[t, j]), min(per[t - 1, q], per[t, j])
        return jump * (hi / lo - 1.0)
    states = [[j for j in range(K + 1) if np.isfinite(obs(t, j))] for t in range(T)]
    out = []
    for path in itertools.product(*states):
        c = obs(0, path[0])
        for t in range(1, T):
            c = (c + trans(t, path[t - 1], path[t])) + obs(t, path[t])
        out.append((c, path))
    return sorted(out)


def exact_table(rng, T, used_max=3):
    """a table whose path costs are exact in float32 and float64 alike: periods from {32, 64, 128} (ratios 1, 2, 4; tau_max 128, so
    period / tau_max is 1/4, 1/2 or 1), values multiples of 1/64 below 1, at most used_max used slots a frame, now and then a frame
    gated out or without a candidate"""
    per, val = np.zeros((T, K), np.float32), np.full((T, K), np.inf, np.float32)
    gate = rng.random(T) > 0.15
    for t in range(T):
        n = int(rng.integers(0, used_max + 1))
        p = np.sort(rng.choice([32.0, 64.0, 128.0], size=n, replace=False))
        per[t, :n], val[t, :n] = p, rng.integers(0, 64, n) / 64.0
    return per, val, gate


def exact_costs(rng):
    """(jump, switch, unvoiced, bias): multiples of 1/64"""
    return tuple(float(v) / 64.0 for v in (rng.integers(0, 65), rng.integers(0, 33), rng.integers(1, 33), rng.integers(0, 17)))


# ---- tables for the kernel ---------------------------------------------------------------------------------------------------------------
def grid_table(seed, T, tau_min=32, tau_max=267):
    """(period, value, gate) of T frames: 0 .. 8 used slots a frame in ascending order of period.  The periods are multiples (1/2, 1,
    3/2, 2, 3) of a base that holds for a run of frames, and a few stray ones, on a grid of 1/4 sample; the values lie on a grid of
    1/32 up to 1/4, so equal costs meet on most steps.  Runs of frames are gated out, others hold no candidate."""
    rng = np.random.default_rng(seed)
    per, val = np.zeros((T, K), np.float32), np.full((T, K), np.inf, np.float32)
    n = rng.integers(1, K + 1, T)
    n[rng.random(T) < 0.1] = 0
    n[rng.random(T) < 0.2] = K
    base = 0.0
    for t in range(T):
        if t % 16 == 0:
            base = 60.0 + 0.25 * rng.integers(0, 160)
        pool = np.concatenate([base * np.float64([0.5, 1.0, 1.5, 2.0, 3.0]), rng.integers(4 * tau_min, 4 * tau_max, 3) / 4.0])
        p = np.unique(np.clip(np.round(4.0 * rng.permutation(pool)[:n[t]]) / 4.0, tau_min, tau_max - 1))
        per[t, :len(p)] = p
        val[t, :len(p)] = rng.integers(0, 9, len(p)) / 32.0
    gate = np.ones(T, bool)
    for start in rng.integers(0, T, 1 + T // 40):
        gate[start:start + int(rng.integers(1, 6))] = False
    return per, val, gate.astype(np.uint8)
