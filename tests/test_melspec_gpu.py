"""csrc/melspec.hip against the float64 yardstick of tests/audio_common.py (torch.stft on the CPU + a Slaney basis written from the
formulas): magnitudes per frame within C_MAG of the frame maximum, every dB value within C_DB, batches bit-equal to single launches,
repeat launches bit-equal, and the analytic cases (bin-centred cosine, unit impulse, digital silence)."""
import functools

import numpy as np
import pytest
import torch

import audio_common as ac
import satt_amd  # noqa: F401
from satt_amd.utils import audio

pytestmark = pytest.mark.gpu
NAMES = sorted(ac.CONFIGS)


@functools.lru_cache(maxsize=None)
def tables(name):
    sr, n_fft, win, hop, mels = ac.CONFIGS[name]
    return audio.MelspecTables(sr, n_fft, win, hop, mels)


@functools.lru_cache(maxsize=None)
def reference(name):
    """[(signal, mag64, dB64, amplitude64)] of kernel_cases(name), computed once"""
    sr, n_fft, win, hop, mels = ac.CONFIGS[name]
    basis64 = ac.slaney_basis(sr, n_fft, mels)
    out = []
    for y in ac.kernel_cases(name):
        mag64 = ac.yardstick_mag(y, n_fft, hop, win)
        db64, amp = ac.yardstick_db(mag64, basis64)
        out.append((y, mag64, db64, amp))
    return out


@functools.lru_cache(maxsize=None)
def singles(name):
    """every signal of kernel_cases(name) in a launch of its own: [(mel, mag)]"""
    res = []
    for y, _, _, _ in reference(name):
        m, g = audio.melspec_hip(tables(name), [y], ac.REF_LEVEL_DB, want_mag=True)
        res.append((m[0], g[0]))
    return res


@pytest.mark.parametrize("name", NAMES)
def test_kernel_matches_the_float64_yardstick_at_every_length(name):
    _, n_fft, _, hop, mels = ac.CONFIGS[name]
    for (y, mag64, db64, amp), (mel, mag) in zip(reference(name), singles(name)):
        T = 1 + len(y) // hop
        assert mel.shape == (T, mels) and mag.shape == (T, n_fft // 2 + 1) and mag64.shape == mag.shape
        assert amp.min() >= 1e-4                      # the condition under which no dB element is left out
        e_mag, e_db = ac.frame_errors(mag, mag64).max(), np.abs(mel - db64).max()
        print("%s n=%d T=%d: mag %.3e (bound %.3e)  dB %.3e (bound %.3e)" % (name, len(y), T, e_mag, ac.C_MAG, e_db, ac.C_DB))
        assert e_mag <= ac.C_MAG, (name, len(y), e_mag)
        assert e_db <= ac.C_DB, (name, len(y), e_db)


@pytest.mark.parametrize("name", NAMES)
def test_a_mixed_batch_equals_the_single_launches_bit_for_bit(name):
    """five utterances of mixed lengths in one launch, the shortest accepted first and last"""
    ref, one = reference(name), singles(name)
    order = [0, 4, 2, 5, 0]
    mels, mags = audio.melspec_hip(tables(name), [ref[i][0] for i in order], ac.REF_LEVEL_DB, want_mag=True)
    for i, m, g in zip(order, mels, mags):
        assert m.tobytes() == one[i][0].tobytes() and g.tobytes() == one[i][1].tobytes(), (name, i)


@pytest.mark.parametrize("name", NAMES)
def test_repeat_launch_and_the_mag_output_leave_the_mel_bits_alone(name):
    ys = [r[0] for r in reference(name)]
    a, _ = audio.melspec_hip(tables(name), ys, ac.REF_LEVEL_DB, want_mag=True)
    b, _ = audio.melspec_hip(tables(name), ys, ac.REF_LEVEL_DB, want_mag=True)
    c = audio.melspec_hip(tables(name), ys, ac.REF_LEVEL_DB)               # mag = NULL: the magnitudes stay on chip
    for x, y, z, (o, _) in zip(a, b, c, singles(name)):
        assert x.tobytes() == y.tobytes() == z.tobytes() == o.tobytes()


def _inner(n, n_fft, hop):
    """the frames that lie inside the signal (no reflected sample), for a signal of n_fft + 6 hop samples"""
    inner = [t for t in range(1 + n // hop) if t * hop - n_fft // 2 >= 0 and t * hop + n_fft // 2 <= n]
    assert len(inner) >= 4
    return inner


@pytest.mark.parametrize("name", NAMES)
def test_bin_centred_cosine_peaks_at_a_win_over_four(name):
    sr, n_fft, win, hop, _ = ac.CONFIGS[name]
    amp, b, n = 0.5, n_fft // 8 + 3, n_fft + 6 * hop
    y = ac.cosine(n, n_fft, b, amp)
    _, (mag,) = audio.melspec_hip(tables(name), [y], ac.REF_LEVEL_DB, want_mag=True)
    mag64 = ac.yardstick_mag(y, n_fft, hop, win)
    assert ac.frame_errors(mag, mag64).max() <= ac.C_MAG
    inner = _inner(n, n_fft, hop)
    peak = amp * win / 4
    # the image at -b lies x = 2 b win / n_fft window bins away, where Hann's spectrum has fallen to |sinc(x) / (1 - x^2)| <
    # 1 / (pi x^3) of its peak (x >= 50 here); 1e-7 on top for the float32 rounding of the samples themselves
    leak = 1.0 / (np.pi * (2.0 * b * win / n_fft) ** 3) + 1e-7
    assert np.abs(mag64[inner, b] - peak).max() <= leak * peak
    assert np.abs(mag[inner, b] - peak).max() <= (leak + ac.C_MAG) * peak
    assert (mag[inner].argmax(axis=1) == b).all()


@pytest.mark.parametrize("name", NAMES)
def test_unit_impulse_has_a_flat_spectrum_equal_to_the_window_value(name):
    _, n_fft, win, hop, _ = ac.CONFIGS[name]
    n = n_fft + 6 * hop
    pos = n // 2
    _, (mag,) = audio.melspec_hip(tables(name), [ac.impulse(n, pos)], ac.REF_LEVEL_DB, want_mag=True)
    w = audio.padded_window(n_fft, win)
    seen = []
    for t in _inner(n, n_fft, hop):
        i = pos - (t * hop - n_fft // 2)                 # the impulse's place in frame t
        expect = w[i] if 0 <= i < n_fft else 0.0
        seen.append(expect)
        assert np.abs(mag[t] - expect).max() <= ac.C_MAG * w.max(), (name, t)
    assert max(seen) > 0.5                               # the window's body is among them


@pytest.mark.parametrize("name", NAMES)
def test_digital_silence_gives_the_floor_everywhere(name):
    _, n_fft, _, hop, mels = ac.CONFIGS[name]
    n = ac.lengths(n_fft, hop)[3]
    (mel,) = audio.melspec_hip(tables(name), [np.zeros(n, np.float32)], ac.REF_LEVEL_DB)
    assert mel.shape == (1 + n // hop, mels)
    assert np.abs(mel - (-100.0 - ac.REF_LEVEL_DB)).max() <= 1e-4


def test_audio_class_on_the_hip_backend_matches_the_yardstick():
    """Audio(hparams) at the LJSpeech hparams: melspectrogram is [num_mels, T]; melspectrogram_batch splits into several launches
    at the sample cap without changing a bit; a signal one sample too short is refused on the host"""
    from satt_amd.hparams import hparams
    hp = hparams.copy()
    hp.parse("num_freq=1025,sample_rate=22050,frame_length_ms=50.0,frame_shift_ms=12.5,num_mels=80,ref_level_db=20")
    a = audio.Audio(hp, backend="hip")
    assert (a.tables.n_fft, a.tables.hop, a.tables.win) == (2048, 275, 1102)
    ref = reference("ljspeech")
    S = a.melspectrogram(ref[2][0])
    assert S.shape == ref[2][2].T.shape and np.abs(S.T - ref[2][2]).max() <= ac.C_DB
    whole = a.melspectrogram_batch([r[0] for r in ref])
    cap, audio.MAX_LAUNCH_SAMPLES = audio.MAX_LAUNCH_SAMPLES, 5000
    try:
        split = a.melspectrogram_batch([r[0] for r in ref])
    finally:
        audio.MAX_LAUNCH_SAMPLES = cap
    assert all(x.tobytes() == y.tobytes() for x, y in zip(whole, split))
    with pytest.raises(ValueError):
        a.melspectrogram(np.zeros(1024, np.float32))
    assert torch.cuda.is_available() and audio.Audio(hp).backend == "hip"
