"""Shared yardstick of the non-negative mel inversion tests (test_mel_nnls_cpu / test_mel_nnls_gpu / tools/mel_nnls_quality.py).

The yardstick is the iteration of DESIGN.md 3.6 written densely in float64 from the formulas: a dense [M, F] matrix filled here from
the float32 band weights, L = numpy.linalg.norm(B, 2) ** 2, step = 1 / L, FISTA's beta in float64.  It uses neither the banded
tables' gathers, nor the transposed table, nor the library's step, and starts from the same float32 amplitudes a and start x_0 as
the backends.

Inputs: the five configurations of audio_common.CONFIGS; the frames of kernel_cases(name)[1:] (five signals of 5 to 9 frames) through
melspec_numpy; hand-made tables (HAND) with an empty band, a band of one bin, a bin under three bands, a band with a zero inside its
run, and a dense one whose weights do not fit the kernel's LDS.

Tolerance (profiles/mel_nnls_tolerances.txt holds the measurements): per frame max_f |x - x64| <= C * max_f x64 at K = 1, 3, 64.
C is 8 x the worst figure of the float32 NumPy backend over exactly these inputs; the same C is the kernel's bar (the kernel has the
NumPy backend's bits, so the factor covers nothing of its own).  The worst figure has to stay at or below 1e-4: above that something
other than rounding is at work."""
import functools
import math

import numpy as np

import audio_common as ac

NAMES = list(ac.CONFIGS)
KS = (1, 3, 64)
REF_LEVEL_DB = ac.REF_LEVEL_DB

# measured worst deviation of the float32 NumPy backend from the yardstick over inputs(name), K in KS: profiles/mel_nnls_tolerances.txt
WORST_NUMPY = 1.54e-5          # 1.535e-5 of the frame maximum (fft512_hop_beyond_window, K = 64); at K = 1 and 3 at most 1.8e-7
C = 8 * WORST_NUMPY
WORST_ALLOWED = 1e-4

RESIDUAL_BOUND = 1e-3          # relative residual of every frame at K = 64 (worst measured 5.7e-5)
DEFECT_BOUND = 0.02            # the floored pseudo-inverse's worst frame on every configuration is at least this (0.027 - 0.106)


@functools.lru_cache(maxsize=None)
def tables(name):
    from satt_amd.utils import audio
    return audio.MelspecTables(*ac.CONFIGS[name])


@functools.lru_cache(maxsize=None)
def mels(name):
    """the dB mel spectrograms [T, M] of kernel_cases(name)[1:]: 5 - 9 frames each (4 - 7 where hop exceeds the window)"""
    from satt_amd.utils import audio
    out = [audio.melspec_numpy(tables(name), y, REF_LEVEL_DB) for y in ac.kernel_cases(name)[1:]]
    assert all(4 <= len(S) <= 9 for S in out), [len(S) for S in out]
    return out


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(a float32 [N, M], x_0 float32 [N, F]) of all frames of mels(name), made as mel_to_linear makes them:
    a = float32(10 ** ((S + ref) / 20)), x_0 = float32(max(1e-10, amp64 @ pinv(basis).T))"""
    t = tables(name)
    S = np.concatenate(mels(name)).astype(np.float64)
    amp = 10.0 ** ((S + REF_LEVEL_DB) / 20.0)
    x0 = np.maximum(1e-10, amp @ np.linalg.pinv(t.basis).T)
    a, x0 = amp.astype(np.float32), x0.astype(np.float32)
    a.setflags(write=False)
    x0.setflags(write=False)
    return a, x0


def dense(band_start, band_offset, band_weight, num_bins):
    """float64 [M, F] filled from the float32 band weights, entry by entry"""
    B = np.zeros((len(band_start), num_bins))
    for m in range(len(band_start)):
        for i in range(int(band_offset[m + 1]) - int(band_offset[m])):
            B[m, int(band_start[m]) + i] = float(np.float32(band_weight[int(band_offset[m]) + i]))
    return B


@functools.lru_cache(maxsize=None)
def dense_of(name):
    t = tables(name)
    return dense(t.band_start, t.band_offset, t.band_weight, t.n_fft // 2 + 1)


def yardstick(B, a, x0, iters):
    """float64 [N, F]: x_K of the dense iteration from float32 a [N, M] and x_0 [N, F]"""
    B = np.asarray(B, np.float64)
    a, x = np.asarray(a, np.float64), np.asarray(x0, np.float64)
    step = 1.0 / np.linalg.norm(B, 2) ** 2
    y, t = x, 1.0
    with np.errstate(all="ignore"):
        for _ in range(iters):
            g = (y @ B.T - a) @ B
            v = y - step * g
            xn = np.where(v > 0, v, 0.0)
            t_next = (1.0 + math.sqrt(1.0 + 4.0 * t * t)) / 2.0
            y = xn + ((t - 1.0) / t_next) * (xn - x)
            x, t = xn, t_next
    return x


@functools.lru_cache(maxsize=None)
def yardstick_of(name, iters):
    """computed once and shared; read-only"""
    a, x0 = inputs(name)
    x = yardstick(dense_of(name), a, x0, iters)
    x.setflags(write=False)
    return x


def frame_errors(x, x64):
    """per frame max_f |x - x64| / max_f x64"""
    return np.abs(np.asarray(x, np.float64) - x64).max(axis=1) / x64.max(axis=1)


def residuals(B, x, a):
    """per frame |B x - a| / |a| in float64 against the float32 a"""
    a = np.asarray(a, np.float64)
    return np.linalg.norm(np.asarray(x, np.float64) @ B.T - a, axis=1) / np.linalg.norm(a, axis=1)


# ---- hand-made tables ------------------------------------------------------------------------------------------------------------------
def hand_basis(kind):
    """float64 [M, F] of a hand-made basis"""
    rng = np.random.default_rng(7)
    if kind == "odd":
        # 9 bins, 5 bands: band 1 is empty, band 2 has one bin, bin 4 lies under bands 2, 3 and 4, bands 0 and 3 have zeros inside
        # their runs, bin 6 lies under bands 0 and 4 but not under those between, bins 0 and 8 lie under none
        B = np.zeros((5, 9))
        B[0, 1:7] = [0.5, 0.25, 0.125, 0.0, 0.0, 0.3]
        B[2, 4] = 0.75
        B[3, 3:8] = [0.2, 0.4, 0.0, 0.0, 0.15]
        B[4, 4:7] = [0.1, 0.6, 0.2]
        return B
    if kind == "wide":
        # 300 bins (two bins a thread at most), 21 bands (two rounds of 16 teams, the second with 5): overlapping runs of 1 .. 77
        # bins (up to 5 terms a lane), up to 6 bands over a bin
        B = np.zeros((21, 300))
        for m in range(21):
            lo = 1 + 13 * m
            n = 1 + (m * 19) % 77
            B[m, lo:min(299, lo + n)] = 0.05 + rng.random(min(299, lo + n) - lo)
        return B
    if kind == "dense":
        # every band over every bin of n_fft = 4096: 2 x 16 x 2049 weights = 256 KiB, which the kernel reads from global memory
        return 0.01 + rng.random((16, 2049)) / 2049.0
    raise KeyError(kind)


HAND = ("odd", "wide", "dense")


@functools.lru_cache(maxsize=None)
def hand(kind):
    """(MelNnlsTables, dense float64 [M, F] of the float32 weights, a float32 [N, M], x_0 float32 [N, F]) of a hand-made basis: the
    amplitudes of random non-negative spectra with holes, x_0 the floored pseudo-inverse (halved for "dense")"""
    from satt_amd.utils import audio
    basis = hand_basis(kind)
    start, offset, weight = audio.banded(basis)
    nt = audio.MelNnlsTables(start, offset, weight, basis.shape[1])
    B = dense(start, offset, weight, basis.shape[1])
    rng = np.random.default_rng(11)
    N = 3 if kind == "dense" else 7
    spec = rng.random((N, basis.shape[1])) * (rng.random((N, basis.shape[1])) < 0.4)
    amp = spec @ B.T
    x0 = np.maximum(1e-10, amp @ np.linalg.pinv(B).T)
    if kind == "dense":
        x0 = 0.5 * x0              # (the pseudo-inverse of a dense positive basis is the solution already: start away from it)
    a, x0 = amp.astype(np.float32), x0.astype(np.float32)
    a.setflags(write=False)
    x0.setflags(write=False)
    return nt, B, a, x0


# ---- edge frames -----------------------------------------------------------------------------------------------------------------------
def level_frames(name, level_db):
    """(a, x_0) of two frames whose every mel is level_db (ref_level_db REF_LEVEL_DB)"""
    t = tables(name)
    amp = np.full((2, t.num_mels), 10.0 ** ((level_db + REF_LEVEL_DB) / 20.0))
    return amp.astype(np.float32), np.maximum(1e-10, amp @ np.linalg.pinv(t.basis).T).astype(np.float32)


def nonfinite_frames(name):
    """three frames of inputs(name); the middle one with a NaN and a +Inf amplitude.  Returns (a_bad, a_good, x_0)"""
    a, x0 = inputs(name)
    good = a[3:6].copy()
    bad = good.copy()
    bad[1, 2] = np.nan
    bad[1, tables(name).num_mels - 3] = np.inf
    return bad, good, x0[3:6].copy()


# ---- the definition as a scalar float32 loop ------------------------------------------------------------------------------------------
def scalar32(band_start, band_offset, band_weight, num_bins, a, x0, iters, step, beta):
    """x_K of ONE frame: Python floats rounded through np.float32 after every operation, in the stated summation order.  The
    transposed product walks the bands that hold a non-zero weight for the bin, ascending (read from the banded table itself)."""
    f32 = np.float32
    M, F = len(band_start), num_bins
    w = [[f32(band_weight[int(band_offset[m]) + i]) for i in range(int(band_offset[m + 1]) - int(band_offset[m]))] for m in range(M)]
    x = [f32(v) for v in x0]
    y = list(x)
    step = f32(step)
    for k in range(iters):
        r = []
        for m in range(M):
            s = []
            for j in range(16):                                   # lane j: the terms j, j + 16, .. ascending, one chain from +0
                acc = f32(0.0)
                for i in range(j, len(w[m]), 16):
                    acc = f32(acc + f32(w[m][i] * y[int(band_start[m]) + i]))
                s.append(acc)
            while len(s) > 1:                                     # the adjacent pairwise tree
                s = [f32(s[2 * i] + s[2 * i + 1]) for i in range(len(s) // 2)]
            r.append(f32(s[0] - f32(a[m])))
        xn = []
        for f in range(F):
            over = [m for m in range(M) if 0 <= f - int(band_start[m]) < len(w[m]) and w[m][f - int(band_start[m])] != 0]
            g = f32(0.0)
            if over:
                for m in range(over[0], over[-1] + 1):            # bands ascending; one between them without the bin has weight 0
                    inside = 0 <= f - int(band_start[m]) < len(w[m])
                    g = f32(g + f32((w[m][f - int(band_start[m])] if inside else f32(0.0)) * r[m]))
            v = f32(y[f] - f32(step * g))
            xn.append(v if v > 0 else f32(0.0))
        y = [f32(xn[f] + f32(f32(beta[k]) * f32(xn[f] - x[f]))) for f in range(F)]
        x = xn
    return np.asarray(x, np.float32)


def round_trip(audio_obj, seed, iters=30, **kw):
    """mean |dB| difference over frames 2 .. T-2 of mel -> inversion -> Griffin-Lim -> mel on harmonic(3308, 22050, seed)"""
    y = ac.harmonic(3308, 22050, seed=seed)
    S = audio_obj.melspectrogram(y)
    T = S.shape[1]
    w = audio_obj.inv_melspectrogram(S, iters=iters, **kw)
    assert w.dtype == np.float32 and w.shape == ((T - 1) * 275,) and np.isfinite(w).all()
    return float(np.abs(audio_obj.melspectrogram(w) - S)[:, 2:T - 2].mean())
