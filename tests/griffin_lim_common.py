"""Shared yardstick of the Griffin-Lim tests (test_griffin_lim_cpu / test_griffin_lim_gpu / tools/griffin_lim_tolerances.py).

The float64 yardstick is torch.stft / torch.istft on the CPU (center=True, reflect padding, periodic Hann window) - framing, padding,
transforms and the overlap-add envelope are code this project did not write.  One float64 iteration is written out in step64:
    y = istft(mag ang);  c = stft(y);  u = c + alpha (c - c_prev);  ang' = u / max(|u|, 1e-30)
The kernel and the float32 NumPy backend are both measured against it ON THE SAME float32 INPUTS (mag and ang are rounded to
float32 / complex64 first and the yardstick starts from the rounded values).

Inputs: the four configurations of audio_common.CONFIGS with hop <= win / 2, and for each the spectra X = stft64(y) of
kernel_cases(name)[1:] - five signals of 5 to 9 frames, frame counts 4 j +- 1.  Case 0 of every configuration (3 or 4 frames) has
(T - 1) hop < n_fft / 2 + 1 and is the refusal case.

Tolerances (profiles/griffin_lim_tolerances.txt holds the measurements):
  C_ISTFT: |y - y64|.max() <= C_ISTFT * |y64|.max();
  C_ITER:  per frame max_k |c - c64| <= C_ITER * max_k |c64|, and per bin |ang' - ang64'| |u64| <= C_ITER * max_k |c64| * (1 + 2 alpha).
Both are 8 x the worst deviation of the float32 NumPy backend (pocketfft) over exactly these inputs - for C_ITER over one iteration
from the seeded random phase and over each of the first six iterations taken one step at a time from the backend's own state, at
alpha = 0 and 0.99.  The factor has the mel kernel's reason (float32 twiddle tables, another stage count and order); it is not
derived from the kernel's results."""
import functools

import numpy as np
import torch

import audio_common as ac

NAMES = ["fft512_full_window", "fft1024", "ljspeech", "vctk"]
ALPHAS = (0.0, 0.99)
STEPS = 6

# measured worst deviations of the float32 NumPy backend: profiles/griffin_lim_tolerances.txt; the kernel gets 8 x
C_ISTFT = 8 * 2.3e-7       # 2.289e-7 of the signal maximum (ljspeech)
C_ITER = 8 * 2.4e-7        # 2.376e-7 of the frame maximum (ljspeech, one of the six single steps); 2.059e-7 for the first iteration


def _window(win):
    return torch.hann_window(win, periodic=True, dtype=torch.float64)


def stft64(y, n_fft, hop, win):
    """complex128 [T, n_fft // 2 + 1]"""
    s = torch.stft(torch.as_tensor(np.asarray(y, np.float64)), n_fft, hop_length=hop, win_length=win, window=_window(win), center=True,
                   pad_mode="reflect", return_complex=True)
    return s.numpy().T.copy()


def istft64(X, n_fft, hop, win):
    """float64 [(T - 1) hop] of a complex [T, n_fft // 2 + 1] spectrogram"""
    X = torch.as_tensor(np.ascontiguousarray(np.asarray(X, np.complex128).T))
    return torch.istft(X, n_fft, hop_length=hop, win_length=win, window=_window(win), center=True,
                       length=(X.shape[1] - 1) * hop).numpy()


def step64(mag, ang, c_prev, alpha, n_fft, hop, win):
    """one float64 iteration from (float32 / complex64) state: (y64, c64, u64, ang64')"""
    mag, ang = np.asarray(mag, np.float64), np.asarray(ang, np.complex128)
    y = istft64(mag * ang, n_fft, hop, win)
    c = stft64(y, n_fft, hop, win)
    u = c + alpha * (c - np.asarray(c_prev, np.complex128)) if alpha != 0 else c
    return y, c, u, u / np.maximum(np.abs(u), 1e-30)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """[(y0 float32, mag float32 [T, NF], ang complex64 = X / |X|, random complex64 unit phases)] of kernel_cases(name)[1:]"""
    _, n_fft, win, hop, _ = ac.CONFIGS[name]
    out = []
    for i, y in enumerate(ac.kernel_cases(name)[1:]):
        X = stft64(y, n_fft, hop, win)
        mag = np.abs(X).astype(np.float32)
        ang = (X / np.maximum(np.abs(X), 1e-300)).astype(np.complex64)
        rnd = np.exp(2j * np.pi * np.random.default_rng(100 + i).random(X.shape)).astype(np.complex64)
        out.append((y, mag, ang, rnd))
    return out


def refused_input(name):
    """case 0: too few frames for the re-analysis to reflect-pad"""
    _, n_fft, win, hop, _ = ac.CONFIGS[name]
    y = ac.kernel_cases(name)[0]
    X = stft64(y, n_fft, hop, win)
    assert (X.shape[0] - 1) * hop < n_fft // 2 + 1
    return np.abs(X).astype(np.float32), (X / np.maximum(np.abs(X), 1e-300)).astype(np.complex64)


def frame_err(c, c64):
    """per frame max_k |c - c64| / max_k |c64|"""
    return np.abs(c.astype(np.complex128) - c64).max(axis=1) / np.abs(c64).max(axis=1)


def ang_err(ang, ang64, u64, c64, alpha):
    """per frame max_k |ang' - ang64'| |u64| / (max_k |c64| (1 + 2 alpha))"""
    return (np.abs(ang.astype(np.complex128) - ang64) * np.abs(u64)).max(axis=1) / (np.abs(c64).max(axis=1) * (1.0 + 2.0 * alpha))


def convergence(c, mag):
    return float(np.linalg.norm(np.abs(c.astype(np.complex128)) - mag) / np.linalg.norm(mag.astype(np.float64)))


def lj_audio(backend):
    from satt_amd.hparams import hparams
    from satt_amd.utils import audio
    hp = hparams.copy()
    hp.parse("num_freq=1025,sample_rate=22050,frame_length_ms=50.0,frame_shift_ms=12.5,num_mels=80,ref_level_db=20")
    hp.set("average_mel_level_db", [-30.0] * 80)
    hp.set("stddev_mel_level_db", [12.0] * 80)
    return audio.Audio(hp, backend=backend)


def check_end_to_end(a):
    """Audio at the LJSpeech hparams on 0.15 s of harmonic(): 30 iterations bring the mel spectrogram of the result closer to the
    one inverted than the inverse STFT of the random phase is"""
    y = ac.harmonic(3308, 22050, seed=3)
    S = a.melspectrogram(y)
    T = S.shape[1]
    assert S.shape == (80, T) and T == 1 + 3308 // 275
    dist = []
    for iters in (0, 30):
        w = a.inv_melspectrogram(S, iters=iters)
        assert w.dtype == np.float32 and w.shape == ((T - 1) * 275,) and np.isfinite(w).all()
        dist.append(float(np.abs(a.melspectrogram(w) - S)[:, 2:T - 2].mean()))
    print("mean |dB| difference: %.3f at iters = 0, %.3f at iters = 30" % tuple(dist))
    assert dist[1] < dist[0], dist
    return dist


MEL_DIR_SAMPLES = (3308, 2800, 4000)          # 13, 11 and 15 frames at the LJSpeech hop


def write_mel_dir(root, stats=True):
    """<root>/hparams.json (the LJSpeech example + corpus statistics, unless stats is False) and <root>/mels/utt<i>.mfbsp: three
    normalised log-mel spectrograms of different lengths, as predict_mel.py writes them.  Returns (json path, mel dir, [dB mel])"""
    import json
    import os
    from satt_amd.utils import audio
    d = json.load(open(ac.LJ_JSON))
    d.pop("_comment", None)
    if stats:
        d.update(average_mel_level_db=[-30.0] * 80, stddev_mel_level_db=[12.0] * 80)
    cfg = os.path.join(str(root), "hparams.json")
    json.dump(d, open(cfg, "w"))
    mel_dir = os.path.join(str(root), "mels")
    os.makedirs(mel_dir)
    t = audio.MelspecTables(*ac.CONFIGS["ljspeech"])
    mels = []
    for i, n in enumerate(MEL_DIR_SAMPLES):
        S = audio.melspec_numpy(t, ac.harmonic(n, 22050, seed=20 + i), 20.0)
        ((S + 30.0) / 12.0).astype("<f4").tofile(os.path.join(mel_dir, "utt%d.mfbsp" % i))
        mels.append(S)
    return cfg, mel_dir, mels


def read_wav(path):
    """(rate, int16 samples) through the standard `wave` module"""
    import wave
    with wave.open(path, "rb") as w:
        assert w.getnchannels() == 1 and w.getsampwidth() == 2
        return w.getframerate(), np.frombuffer(w.readframes(w.getnframes()), "<i2")


def check_wav_dir(out_dir):
    import os
    assert sorted(os.listdir(out_dir)) == ["utt%d.wav" % i for i in range(len(MEL_DIR_SAMPLES))]
    wavs = []
    for i, n in enumerate(MEL_DIR_SAMPLES):
        rate, pcm = read_wav(os.path.join(out_dir, "utt%d.wav" % i))
        assert rate == 22050 and pcm.dtype == np.int16 and len(pcm) == (n // 275) * 275          # (T - 1) hop, T = 1 + n // hop
        assert np.abs(pcm.astype(np.int32)).max() == round(0.95 * 32767)
        wavs.append(pcm)
    return wavs


def numpy_run(tables):
    """run(mags, angs, iters, alpha, c_prevs) -> (ys, angs, c_prevs, cs) on the float32 NumPy backend"""
    from satt_amd.utils import audio

    def run(mags, angs, iters, alpha, c_prevs=None):
        res = [audio.griffin_lim_numpy(tables, m, a, iters, alpha, None if c_prevs is None else c_prevs[i], want_state=True)
               for i, (m, a) in enumerate(zip(mags, angs))]
        return tuple([r[j] for r in res] for j in range(4))
    return run


def hip_run(tables):
    from satt_amd.utils import audio

    def run(mags, angs, iters, alpha, c_prevs=None):
        return audio.griffin_lim_hip(tables, mags, angs, iters, alpha, c_prevs=c_prevs, want_state=True)
    return run


def measure(name, run):
    """worst figures of one backend over inputs(name): dict with
    istft (iters = 0 against istft64), roundtrip (the same signal against y0[:n]), iter_c / iter_ang (one iteration from the random
    phase, worst over ALPHAS), step_c (iterations 1 .. STEPS one at a time from the backend's own state, worst over ALPHAS)"""
    _, n_fft, win, hop, _ = ac.CONFIGS[name]
    cases = inputs(name)
    mags = [c[1] for c in cases]
    out = dict(istft=0.0, roundtrip=0.0, iter_c=0.0, iter_ang=0.0, step_c=0.0)
    ys, _, _, _ = run(mags, [c[2] for c in cases], 0, 0.0)
    for (y0, mag, ang, _), y in zip(cases, ys):
        y64 = istft64(mag.astype(np.float64) * ang, n_fft, hop, win)
        assert y.shape == y64.shape
        out["istft"] = max(out["istft"], np.abs(y - y64).max() / np.abs(y64).max())
        out["roundtrip"] = max(out["roundtrip"], np.abs(y - y0[:len(y)].astype(np.float64)).max() / np.abs(y0).max())
    for alpha in ALPHAS:
        angs, prevs = [c[3] for c in cases], [np.zeros_like(c[3]) for c in cases]
        for k in range(1, STEPS + 1):
            _, angs1, prevs1, cs = run(mags, angs, 1, alpha, prevs)
            for mag, a0, p0, a1, c in zip(mags, angs, prevs, angs1, cs):
                _, c64, u64, a64 = step64(mag, a0, p0, alpha, n_fft, hop, win)
                e_c, e_a = frame_err(c, c64).max(), ang_err(a1, a64, u64, c64, alpha).max()
                if k == 1:
                    out["iter_c"], out["iter_ang"] = max(out["iter_c"], e_c), max(out["iter_ang"], e_a)
                out["step_c"] = max(out["step_c"], e_c)
            angs, prevs = angs1, prevs1
    return out
