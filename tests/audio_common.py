"""Shared yardstick of the audio front-end tests (test_melspec_cpu / test_melspec_gpu / test_preprocess_*).

The float64 yardstick is torch.stft on the CPU - framing, reflect padding and transform that this project did not write - followed
by a Slaney mel basis written here from the formulas (scalar loops, independent of satt_amd.utils.audio.mel_basis).  The kernel
and the float32 NumPy backend are both measured against it.

Tolerances (profiles/melspec_tolerances.txt holds the measurements):
  C_MAG: per frame, max_k |mag - mag64| <= C_MAG * max_k mag64;   C_DB: |dB - dB64| <= C_DB elementwise, no element left out.
Both are 8 x the worst deviation of the float32 NumPy backend (pocketfft) from the yardstick over exactly the inputs of
test_melspec_gpu.py (kernel_cases below).  The factor is for the kernel's float32 twiddle tables and its different stage count
and order, one more bit per stage group; it is not derived from the kernel's own results."""
import math

import numpy as np
import torch

# name: (sample_rate, n_fft, win, hop, num_mels)
CONFIGS = {
    "fft512_full_window": (16000, 512, 512, 128, 80),
    "fft512_hop_beyond_window": (16000, 512, 200, 256, 13),
    "fft1024": (16000, 1024, 800, 200, 40),                      # log2(n_fft / 2) odd: the kernel's radix-2 tail stage
    "ljspeech": (22050, 2048, 1102, 275, 80),                    # (2048 - 1102) / 2 = 473 leading zeros
    "vctk": (48000, 4096, 2400, 600, 80),
}
FRAMES_PER_WORKGROUP = 4
REF_LEVEL_DB = 20.0

# measured worst deviations of the float32 NumPy backend over kernel_cases: 1.598e-7 of the frame maximum (vctk), 2.353e-4 dB
# (fft512_full_window, whose smallest mel amplitude is 1.5e-4; 1.3e-4 dB at the two example configurations) -
# profiles/melspec_tolerances.txt; the kernel gets 8 x
C_MAG = 8 * 1.6e-7
C_DB = 8 * 2.4e-4


def yardstick_mag(y, n_fft, hop, win):
    """float64 [T, n_fft // 2 + 1]"""
    s = torch.stft(torch.as_tensor(np.asarray(y, np.float64)), n_fft, hop_length=hop, win_length=win,
                   window=torch.hann_window(win, periodic=True, dtype=torch.float64), center=True, pad_mode="reflect",
                   return_complex=True)
    return s.abs().numpy().T.copy()


def _hz(m):
    return m * 200.0 / 3.0 if m < 15.0 else 1000.0 * math.exp((m - 15.0) * math.log(6.4) / 27.0)


def _mel(f):
    return f * 3.0 / 200.0 if f < 1000.0 else 15.0 + math.log(f / 1000.0) * 27.0 / math.log(6.4)


def slaney_basis(sample_rate, n_fft, num_mels):
    """float64 [num_mels, n_fft // 2 + 1] from the formulas: num_mels + 2 points equally spaced in mel over 0 .. sample_rate / 2,
    triangles normalised by 2 / (f[m + 2] - f[m])"""
    top = _mel(sample_rate / 2.0)
    f = [_hz(top * i / (num_mels + 1)) for i in range(num_mels + 2)]
    B = np.zeros((num_mels, n_fft // 2 + 1))
    for m in range(num_mels):
        for k in range(n_fft // 2 + 1):
            x = k * sample_rate / n_fft
            B[m, k] = max(0.0, min((x - f[m]) / (f[m + 1] - f[m]), (f[m + 2] - x) / (f[m + 2] - f[m + 1]))) * 2.0 / (f[m + 2] - f[m])
    return B


def yardstick_db(mag64, basis64, ref_level_db=REF_LEVEL_DB):
    amp = mag64 @ basis64.T
    return 20.0 * np.log10(np.maximum(1e-5, amp)) - ref_level_db, amp


def harmonic(n, sample_rate, seed=0):
    """29 harmonics of 140 Hz at 0.3 / k plus Gaussian noise of sigma 1e-3: every float64 mel amplitude stays >= 1e-4"""
    t = np.arange(n) / sample_rate
    y = sum(0.3 / k * np.sin(2 * np.pi * 140.0 * k * t + 0.7 * k) for k in range(1, 30))
    return (y + 1e-3 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def cosine(n, n_fft, bin_, amplitude=0.5):
    return (amplitude * np.cos(2 * np.pi * bin_ * np.arange(n) / n_fft)).astype(np.float32)


def impulse(n, pos):
    y = np.zeros(n, np.float32)
    y[pos] = 1.0
    return y


def lengths(n_fft, hop):
    """the shortest accepted length; k hop - 1, k hop, k hop + 1 (the frame count steps at k hop); frame counts one more and one
    less than a multiple of the frames a workgroup takes.  All <= 0.5 s at the configurations above."""
    short = n_fft // 2 + 1
    k = -(-short // hop) + 2
    j = (k + FRAMES_PER_WORKGROUP) // FRAMES_PER_WORKGROUP
    more = FRAMES_PER_WORKGROUP * j * hop + min(3, hop - 1)                        # T = 4 j + 1
    less = (FRAMES_PER_WORKGROUP * j - 2) * hop + hop // 2                        # T = 4 j - 1
    out = [short, k * hop - 1, k * hop, k * hop + 1, more, less]
    assert 1 + more // hop == FRAMES_PER_WORKGROUP * j + 1 and 1 + less // hop == FRAMES_PER_WORKGROUP * j - 1
    return out


def kernel_cases(name):
    """the harmonic inputs of one configuration, one per length of lengths() (seeded by position)"""
    sr, n_fft, win, hop, _ = CONFIGS[name]
    return [harmonic(n, sr, seed=i) for i, n in enumerate(lengths(n_fft, hop))]


def frame_errors(mag, mag64):
    """per frame: max_k |mag - mag64| / max_k mag64"""
    return np.abs(mag.astype(np.float64) - mag64).max(axis=1) / mag64.max(axis=1)


# ---- toy corpora for the driver tests (written with the standard `wave` module) --------------------------------------------------
import os  # noqa: E402
import subprocess  # noqa: E402
import sys  # noqa: E402
import wave  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LJ_JSON = os.path.join(ROOT, "examples", "ljspeech", "self-attention-tacotron.json")
LJ_RATE, LJ_HOP = 22050, 275
LJ_LINES = [("LJ001-0001", "Mr. Smith paid $3.50 in 1999."), ("LJ001-0002", "The 22nd   of May, 2005"),
            ("LJ001-0003", "Printing, in the only sense"), ("LJ001-0004", "10,000 people; 3.14 and 21"),
            ("LJ001-0005", "Dr. Jones: “naïve”?")]
LJ_SAMPLES = [3000, 4125, 2750, 5003, 3571]


def write_wav(path, samples, rate, channels=1):
    """float signal in [-1, 1) as 16-bit PCM"""
    pcm = np.round(np.asarray(samples, np.float64) * 32767.0).astype("<i2")
    if channels > 1:
        pcm = np.repeat(pcm[:, None], channels, axis=1)
    with wave.open(path, "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.tobytes())


def write_toy_ljspeech(root):
    """five short wavs and a metadata.csv under root; returns [(key, text, samples)]"""
    os.makedirs(os.path.join(root, "wavs"), exist_ok=True)
    with open(os.path.join(root, "metadata.csv"), "w", encoding="utf-8") as f:
        for (key, text), n in zip(LJ_LINES, LJ_SAMPLES):
            f.write("%s|%s|%s\n" % (key, text, text))
    for i, ((key, _), n) in enumerate(zip(LJ_LINES, LJ_SAMPLES)):
        write_wav(os.path.join(root, "wavs", key + ".wav"), harmonic(n, LJ_RATE, seed=10 + i), LJ_RATE)
    return [(k, t, n) for (k, t), n in zip(LJ_LINES, LJ_SAMPLES)]


VCTK_RATE, VCTK_HOP = 48000, 600
VCTK_SILENCE, VCTK_TONE = 9600, 7680         # samples of silence on either side of the tone: 0.2 s | 0.16 s | 0.2 s


def write_toy_vctk(root):
    """speaker-info.txt with a header, speakers 225 (F), 226 (M) and 315 (whose directories do not exist), two utterances each of
    silence - tone - silence; returns [(key, speaker, age, gender, samples)]"""
    with open(os.path.join(root, "speaker-info.txt"), "w", encoding="utf8") as f:
        f.write("ID  AGE  GENDER  ACCENTS  REGION\n225  23  F    English    Southern  England\n226  22  M    English    Surrey\n"
                "315  18  M    American  New  England\n")
    out = []
    n = 2 * VCTK_SILENCE + VCTK_TONE
    for spk, age, gender in ((225, 23, 0), (226, 22, 1)):
        os.makedirs(os.path.join(root, "txt", "p%d" % spk))
        os.makedirs(os.path.join(root, "wav48", "p%d" % spk))
        for u in (1, 2):
            key = "p%d_%03d" % (spk, u)
            with open(os.path.join(root, "txt", "p%d" % spk, key + ".txt"), "w", encoding="utf8") as f:
                f.write("Please  call Stella.\n" if u == 1 else "Ask her to bring these things.\n")
            y = np.zeros(n)
            y[VCTK_SILENCE:VCTK_SILENCE + VCTK_TONE] = 0.4 * np.sin(2 * np.pi * 220.0 * u * np.arange(VCTK_TONE) / VCTK_RATE)
            write_wav(os.path.join(root, "wav48", "p%d" % spk, key + ".wav"), y, VCTK_RATE)
            out.append((key, spk, age, gender, n))
    return out


def run_driver(script, *args, check=True):
    """a preprocessing driver as a subprocess; returns the CompletedProcess"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + list(args), capture_output=True, text=True, timeout=300)
    if check:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r
