"""What the non-negative mel inversion (utils/audio.py, inversion="nnls") buys over the floored pseudo-inverse, on the CPU with the
NumPy backend:
  residual:    per configuration of tests/audio_common.CONFIGS and signal (harmonic() and a gliding-F0 formant signal, 0.5 s), the
               relative residual |B x - a| / |a| of the worst frame, for the floored pseudo-inverse and behind K = 16, 32, 64, 128
               iterations (float64, against the float32 amplitudes; B dense from the float32 weights) - the choice of K;
  round trip:  mel -> inversion -> Griffin-Lim -> mel, the mean |dB| difference over frames 2 .. T-2 (the figure of
               griffin_lim_common.check_end_to_end), with "pinv" and with "nnls" (K = 64): the four configurations Griffin-Lim takes
               x the two signals at 60 iterations, and check_end_to_end's own signal (harmonic(3308, 22050, seed = 3 .. 5)) at 30.
    python tools/mel_nnls_quality.py          (profiles/mel_nnls_quality.txt holds a recorded run)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import audio_common as ac  # noqa: E402
import griffin_lim_common as gc  # noqa: E402
import mel_nnls_common as mc  # noqa: E402
import satt_amd  # noqa: E402,F401
from satt_amd.hparams import hparams  # noqa: E402
from satt_amd.utils import audio  # noqa: E402

KS = (16, 32, 64, 128)


def glide(n, sample_rate, seed=0):
    """harmonics of an F0 gliding from 110 to 220 Hz under three formants (700, 1200, 2600 Hz), plus a little noise"""
    t = np.arange(n) / sample_rate
    f0 = 110.0 * 2.0 ** (t / t[-1])
    ph = 2.0 * np.pi * np.cumsum(f0) / sample_rate
    y = np.zeros(n)
    for k in range(1, int(0.45 * sample_rate / 220.0)):
        f = k * f0
        env = sum(g / (1.0 + ((f - c) / w) ** 2) for c, w, g in ((700.0, 130.0, 1.0), (1200.0, 150.0, 0.6), (2600.0, 250.0, 0.3)))
        y += env * np.sin(k * ph + 0.3 * k)
    y *= 0.4 / np.abs(y).max()
    return (y + 1e-3 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


SIGNALS = (("harmonic", ac.harmonic), ("glide", glide))


def audio_of(name):
    sr, n_fft, win, hop, num_mels = ac.CONFIGS[name]
    hp = hparams.copy()
    hp.parse("num_freq=%d,sample_rate=%d,frame_length_ms=%r,frame_shift_ms=%r,num_mels=%d,ref_level_db=20"
             % (n_fft // 2 + 1, sr, 1000.0 * win / sr, 1000.0 * hop / sr, num_mels))
    au = audio.Audio(hp, backend="numpy")
    assert (au.tables.n_fft, au.tables.win, au.tables.hop) == (n_fft, win, hop), (name, au.tables.win, au.tables.hop)
    return au


def round_trip(au, y, iters, **kw):
    S = au.melspectrogram(y)
    T = S.shape[1]
    w = au.inv_melspectrogram(S, iters=iters, **kw)
    return float(np.abs(au.melspectrogram(w) - S)[:, 2:T - 2].mean())


def main():
    print("relative residual |B x - a| / |a|, worst frame")
    print("%-26s %-9s %6s %10s" % ("configuration", "signal", "frames", "pinv+floor") + "".join("  K = %-6d" % k for k in KS))
    for name in mc.NAMES:
        sr = ac.CONFIGS[name][0]
        t = mc.tables(name)
        nt = audio.mel_nnls_tables(t)
        B = mc.dense_of(name)
        for label, make in SIGNALS:
            S = audio.melspec_numpy(t, make(sr // 2, sr, seed=1), 20.0).astype(np.float64)
            amp = 10.0 ** ((S + 20.0) / 20.0)
            a = amp.astype(np.float32)
            x0 = np.maximum(1e-10, amp @ np.linalg.pinv(t.basis).T).astype(np.float32)
            row = [mc.residuals(B, x0, a).max()] + [mc.residuals(B, audio.mel_nnls_numpy(nt, a, x0, k), a).max() for k in KS]
            print("%-26s %-9s %6d %10.4f" % (name, label, len(a), row[0]) + "".join("  %-10.2e" % v for v in row[1:]))
    print()
    print("round trip mel -> inversion -> Griffin-Lim -> mel, mean |dB| over frames 2 .. T-2 (nnls: K = 64)")
    print("%-26s %-16s %5s %8s %8s %7s" % ("configuration", "signal", "iters", "pinv", "nnls", "ratio"))
    for name in gc.NAMES:
        sr = ac.CONFIGS[name][0]
        au = audio_of(name)
        for label, make in SIGNALS:
            y = make(sr // 2, sr, seed=1)
            p, n = round_trip(au, y, 60), round_trip(au, y, 60, inversion="nnls")
            print("%-26s %-16s %5d %8.3f %8.3f %7.3f" % (name, label, 60, p, n, n / p))
    au = gc.lj_audio("numpy")
    for seed in (3, 4, 5):
        p, n = mc.round_trip(au, seed), mc.round_trip(au, seed, inversion="nnls")
        print("%-26s %-16s %5d %8.3f %8.3f %7.3f" % ("ljspeech", "harmonic seed %d" % seed, 30, p, n, n / p))


if __name__ == "__main__":
    main()
