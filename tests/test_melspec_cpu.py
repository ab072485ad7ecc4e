"""Host side of the audio front end (no GPU): the C-ABI declaration of satt_melspec, the mel basis, the float32 NumPy backend against
the float64 yardstick (tests/audio_common.py) and the frozen fixture, trim, and the shortest accepted signal."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import audio_common as ac
import satt_amd  # noqa: F401
from satt_amd.hparams import hparams
from satt_amd.utils import audio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "melspec_small.npz")
EXAMPLES = [ac.CONFIGS["ljspeech"], ac.CONFIGS["vctk"]]


def lj_hparams(**kw):
    hp = hparams.copy()
    hp.parse("num_freq=1025,sample_rate=22050,frame_length_ms=50.0,frame_shift_ms=12.5,num_mels=80,ref_level_db=20")
    for k, v in kw.items():
        hp.set(k, v)
    return hp


def test_melspec_struct_layout_matches_c(tmp_path):
    """sizeof / offsetof of the ctypes mirror == the C struct (host compiler), and both entry points are declared on both sides"""
    from satt_amd import _lib
    names = [n for n, _ in _lib.MelspecParams._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "satt_hip.h"\nint main() {\n  printf("%zu", sizeof(satt_melspec_params));\n'
    src += "".join('  printf(" %%zu", offsetof(satt_melspec_params, %s));\n' % n for n in names) + "  return 0; }\n"
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    vals = list(map(int, subprocess.check_output([str(tmp_path / "t")]).split()))
    M = _lib.MelspecParams
    assert vals == [ctypes.sizeof(M)] + [getattr(M, n).offset for n in names]
    header = open(os.path.join(ROOT, "include", "satt_hip.h")).read()
    for sym in ("satt_melspec_supported", "satt_melspec"):
        assert sym + "(" in header and sym in _lib.SIGNATURES
    assert _lib.SIGNATURES["satt_melspec"][1][-1] is ctypes.c_void_p           # the stream comes last, as everywhere


def test_melspec_supported_set_and_each_single_violation():
    from satt_amd import ops
    for n_fft in (512, 1024, 2048, 4096):
        for win, hop, mels in ((16, 1, 1), (n_fft, n_fft, 128), (200 if n_fft == 512 else n_fft // 2, 256, 80)):
            assert ops.melspec_supported(n_fft, win, hop, mels), (n_fft, win, hop, mels)
    assert ops.melspec_supported(2048, 1102, 275, 80) and ops.melspec_supported(4096, 2400, 600, 80)
    for bad in ((256, 200, 64, 80), (8192, 2400, 600, 80), (1000, 800, 200, 80), (2048, 15, 275, 80), (2048, 2049, 275, 80),
                (2048, 1102, 0, 80), (2048, 1102, 2049, 80), (2048, 1102, 275, 0), (2048, 1102, 275, 129)):
        assert not ops.melspec_supported(*bad), bad
    hp = lj_hparams(num_mels=129)
    with pytest.raises(ValueError):
        audio.Audio(hp, backend="hip")
    assert audio.Audio(hp, backend="numpy").tables.num_mels == 129               # the restatement has no such cap


def test_stft_parameters_keep_the_reference_expressions():
    assert audio.stft_parameters(lj_hparams()) == (2048, 275, 1102)
    assert audio.stft_parameters(hparams.copy()) == (4096, 600, 2400)


@pytest.mark.parametrize("sr,n_fft,win,hop,mels", EXAMPLES)
def test_mel_basis(sr, n_fft, win, hop, mels):
    B = audio.mel_basis(sr, n_fft, mels)
    assert B.shape == (mels, n_fft // 2 + 1) and B.dtype == np.float64
    assert np.abs(B - ac.slaney_basis(sr, n_fft, mels)).max() <= 1e-15 * B.max() * 100     # the two independent statements agree
    assert (B.max(axis=1) > 0).all()                                     # no empty band
    assert ((B > 0).sum(axis=0) <= 2).all()                              # a bin feeds at most 2 bands
    area = B.sum(axis=1) * sr / n_fft
    assert area.min() >= 0.99 and area.max() <= 1.02, (area.min(), area.max())
    start, offset, weight = audio.banded(B)
    assert start.dtype == np.int32 and offset.dtype == np.int32 and weight.dtype == np.float32
    dense = np.zeros_like(B)
    for m in range(mels):
        dense[m, start[m]:start[m] + offset[m + 1] - offset[m]] = weight[offset[m]:offset[m + 1]]
    assert np.array_equal(dense, B.astype(np.float32).astype(np.float64))


def test_mel_scale_anchors():
    assert abs(float(audio.mel_to_hz(15.0)) - 1000.0) < 1e-9 and abs(float(audio.hz_to_mel(1000.0)) - 15.0) < 1e-12
    assert abs(float(audio.hz_to_mel(22050 / 2.0)) - 49.9106) < 1e-4
    assert abs(float(audio.hz_to_mel(48000 / 2.0)) - 61.2250) < 1e-4
    assert abs(float(audio.hz_to_mel(500.0)) - 7.5) < 1e-12
    for m in (0.0, 3.3, 15.0, 20.0, 61.0):
        assert abs(float(audio.hz_to_mel(audio.mel_to_hz(m))) - m) < 1e-9


def test_window_and_twiddle_tables():
    w = audio.padded_window(2048, 1102)
    assert w[:473].max() == 0.0 and w[473 + 1102:].max() == 0.0 and w[473] == 0.0 and w[474] > 0.0
    assert abs(w[473 + 551] - 1.0) < 1e-15 and abs(w.sum() - 551.0) < 1e-9          # periodic Hann: peak at win / 2, sum win / 2
    t = audio.twiddles(512)
    assert t.shape == (512, 2) and t.dtype == np.float32
    assert t[0].tolist() == [1.0, 0.0] and abs(t[128, 0]) < 1e-7 and t[128, 1] == -1.0


@pytest.mark.parametrize("name", sorted(ac.CONFIGS))
def test_numpy_backend_matches_the_yardstick(name):
    """the float32 restatement over the kernel's inputs: inside the constants measured from it (C = 8 x its worst case)"""
    sr, n_fft, win, hop, mels = ac.CONFIGS[name]
    tables = audio.MelspecTables(sr, n_fft, win, hop, mels)
    basis64 = ac.slaney_basis(sr, n_fft, mels)
    for y in ac.kernel_cases(name):
        db, mag = audio.melspec_numpy(tables, y, ac.REF_LEVEL_DB, want_mag=True)
        mag64 = ac.yardstick_mag(y, n_fft, hop, win)
        db64, amp = ac.yardstick_db(mag64, basis64)
        assert db.dtype == np.float32 and db.shape == (1 + len(y) // hop, mels) and amp.min() >= 1e-4
        assert ac.frame_errors(mag, mag64).max() <= ac.C_MAG / 8 and np.abs(db - db64).max() <= ac.C_DB / 8


def test_frozen_fixture_holds_the_yardstick_and_the_numpy_backend():
    g = np.load(GOLDEN)
    sr, n_fft, win, hop, mels, ref = (int(v) for v in g["params"])
    assert (sr, n_fft, win, hop, mels) == ac.CONFIGS["ljspeech"] and ref == ac.REF_LEVEL_DB
    y, frames = g["signal"], g["mag_frames"]
    assert y.dtype == np.float32 and 0.2 < len(y) / sr < 0.3 and os.path.getsize(GOLDEN) < 100 * 1024
    mag64 = ac.yardstick_mag(y, n_fft, hop, win)
    db64, _ = ac.yardstick_db(mag64, ac.slaney_basis(sr, n_fft, mels))
    assert np.abs(mag64[frames] - g["mag"]).max() <= 1e-12 * g["mag"].max()         # the yardstick has not moved
    assert np.abs(db64 - g["db"]).max() <= 1e-9
    a = audio.Audio(lj_hparams(), backend="numpy")
    S = a.melspectrogram(y)
    assert S.shape == (mels, 1 + len(y) // hop) and S.dtype == np.float32
    assert np.abs(S.T - g["db"]).max() <= ac.C_DB / 8
    _, mag = audio.melspec_numpy(a.tables, y, ref, want_mag=True)
    assert ac.frame_errors(mag[frames], g["mag"]).max() <= ac.C_MAG / 8
    assert np.array_equal(a.melspectrogram_batch([y, y[:3000]])[1], a.melspectrogram(y[:3000]).T)


def test_reflect_padding_at_the_shortest_length_and_the_refusal_below_it():
    a = audio.Audio(lj_hparams(), backend="numpy")
    y = ac.harmonic(1025, 22050, seed=5)
    S = a.melspectrogram(y)
    assert S.shape == (80, 4)
    mag64 = ac.yardstick_mag(y, 2048, 275, 1102)
    db64, _ = ac.yardstick_db(mag64, ac.slaney_basis(22050, 2048, 80))
    assert np.abs(S.T - db64).max() <= ac.C_DB / 8
    # frame 0 by hand: positions 0 .. 2047 are samples 1024, 1023, .., 1, 0, 1, .., 1023 - the edge sample is not repeated
    frame0 = np.concatenate([y[1024:0:-1], y[:1024]]).astype(np.float64) * audio.padded_window(2048, 1102)
    assert np.abs(np.abs(np.fft.rfft(frame0)) - mag64[0]).max() <= 1e-12 * mag64[0].max()
    with pytest.raises(ValueError):
        a.melspectrogram(y[:1024])
    with pytest.raises(ValueError):
        a.melspectrogram_batch([y, y[:1024]])


def test_trim_on_known_frame_boundaries():
    """silence - tone - silence: with frames of 1024 samples every 256, centred, frame t sees the tone when (t - 2) 256 .. (t + 2) 256
    overlaps it.  Tone at [9600, 17280): first frame 36 (9216 + 512 > 9600), last frame 69 (17664 - 512 < 17280)."""
    hp = hparams.copy()                                             # 48 kHz, trim_top_db 30, 1024 / 256, 4 silent frames of 600
    a = audio.Audio(hp, backend="numpy")
    y = np.zeros(26880, np.float32)
    y[9600:17280] = 0.4 * np.sin(2 * np.pi * 220.0 * np.arange(7680) / 48000.0)
    widen = int(4 * 12.5 * 48000 / 1000)
    assert widen == 2400
    out = a.trim(y)
    assert len(out) == (70 * 256 + widen) - (36 * 256 - widen) and np.array_equal(out, y[36 * 256 - widen:70 * 256 + widen])
    hp.set("num_silent_frames", 0)
    assert np.array_equal(audio.Audio(hp, backend="numpy").trim(y), y[36 * 256:70 * 256])
    # clamped to the signal on both sides; a tone up to the end ends at n
    hp.set("num_silent_frames", 100)
    assert np.array_equal(audio.Audio(hp, backend="numpy").trim(y), y)
    hp.set("num_silent_frames", 0)
    tail = y[:17000]
    assert np.array_equal(audio.Audio(hp, backend="numpy").trim(tail), tail[36 * 256:])
    # -30 dB: a second tone 40 dB down is silence, one 20 dB down is not
    for gain, kept in ((0.01, False), (0.1, True)):
        z = y.copy()
        z[20480:24576] = gain * 0.4 * np.sin(2 * np.pi * 220.0 * np.arange(4096) / 48000.0)
        assert (len(audio.Audio(hp, backend="numpy").trim(z)) > 70 * 256 - 36 * 256) == kept


def test_trim_of_silence_is_empty():
    a = audio.Audio(hparams.copy(), backend="numpy")
    assert len(a.trim(np.zeros(20000, np.float32))) == 0
    assert len(a.trim(np.full(20000, 1e-6, np.float32))) == 0                 # mean square 1e-12: below the 1e-10 floor
    assert len(a.trim(np.zeros(0, np.float32))) == 0


def test_wav_round_trip_and_refusals(tmp_path):
    a = audio.Audio(lj_hparams(), backend="numpy")
    y = ac.harmonic(3000, 22050, seed=1) * 0.5
    p = str(tmp_path / "a.wav")
    ac.write_wav(p, y, 22050)
    back = a.load_wav(p)
    assert back.dtype == np.float32 and len(back) == 3000 and np.abs(back - y).max() <= 1.0 / 32768 + 1e-7
    assert np.array_equal(back * 32768, np.round(back * 32768))             # int16 / 32768 exactly
    a.save_wav(back, str(tmp_path / "b.wav"))
    assert np.array_equal(a.load_wav(str(tmp_path / "b.wav")), back)
    wrong = str(tmp_path / "wrong.wav")
    ac.write_wav(wrong, y, 16000)
    with pytest.raises(ValueError) as e:
        a.load_wav(wrong)
    assert "wrong.wav" in str(e.value) and "16000" in str(e.value) and "22050" in str(e.value)
    stereo = str(tmp_path / "stereo.wav")
    ac.write_wav(stereo, y, 22050, channels=2)
    with pytest.raises(ValueError) as e:
        a.load_wav(stereo)
    assert "stereo.wav" in str(e.value) and "mono" in str(e.value)


def test_normalize_mel_and_backend_choice():
    hp = lj_hparams(average_mel_level_db=[-40.0] * 80, stddev_mel_level_db=[2.0] * 80)
    a = audio.Audio(hp, backend="numpy")
    assert np.allclose(a.normalize_mel(np.full((3, 80), -36.0, np.float32)), 2.0)
    with pytest.raises(ValueError):
        audio.Audio(hp, backend="librosa")
