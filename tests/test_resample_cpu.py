"""Host side of the resampler (no GPU): the ratio and length arithmetic, the float32 filter table, the float32 NumPy backend against
the float64 yardstick of tests/resample_common.py, tones through the pass band and the stop band, Audio(resample=...), the C-ABI
declaration of satt_resample, and the three preprocessing drivers with --resample on toy corpora."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
from scipy.io import wavfile

import audio_common as ac
import resample_common as rc
import satt_amd  # noqa: F401
from satt_amd.datasets.dataset_factory import create_from_tfrecord_files
from satt_amd.datasets.ljspeech import decode_target_record
from satt_amd.hparams import hparams
from satt_amd.utils import audio, tfrecord

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = rc.cases()


def hp_at(rate, **kw):
    hp = hparams.copy()
    hp.parse("num_freq=%d,sample_rate=%d,frame_length_ms=50.0,frame_shift_ms=12.5,num_mels=80,ref_level_db=20"
             % ({16000: 513, 22050: 1025, 24000: 1025, 48000: 2049}[rate], rate))
    for k, v in kw.items():
        hp.set(k, v)
    return hp


# ---- ratio, length, table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", sorted(rc.RATIOS))
def test_ratio_taps_and_output_length(pair):
    up, down, taps = rc.RATIOS[pair]
    assert audio.resample_ratio(*pair) == (up, down)
    t = audio.resample_tables(*pair)
    assert (t.up, t.down, t.taps, t.half) == (up, down, taps, taps // 2) and t.table.shape == (up, taps) and t.table.dtype == np.float32
    assert audio.resample_tables(*pair) is t                                          # cached per (a, b)
    for n in (1, 2, down - 1, down, down + 1, 3001, 132300, 7000000):
        n_out = t.length(n)
        assert (n_out - 1) * down < n * up <= n_out * down                             # n_out = ceil(n up / down), in integers
        assert n_out == rc.out_length(n, up, down)
    assert t.length(down) == up and t.length(down + 1) == up + -(-up // down)


@pytest.mark.parametrize("pair", sorted(rc.RATIOS) + [(48000, 24000), (44100, 48000)])
def test_table_matches_float64_h_sums_to_one_and_is_symmetric(pair):
    t = audio.resample_tables(*pair)
    s, half = rc.scale_half(t.up, t.down)
    assert half == t.half
    j = np.arange(-half + 1, half + 1)
    h64 = np.stack([rc.h(p / t.up - j, s) for p in range(t.up)])
    # rounding to float32: half an ulp of the value.  The exact-rational argument differs from phase / up - j by an ulp of the
    # ARGUMENT (<= 128 * 2^-53), which moves h by far less than float32 resolution of the largest tap
    assert np.all(np.abs(t.table - h64) <= np.abs(h64) * 2.0 ** -24 + h64.max() * 1e-12)
    assert np.abs(t.table.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6
    assert np.array_equal(t.table[1:], t.table[:0:-1, ::-1])                           # table[p][j] == table[up - p][taps - 1 - j]
    assert t.table[0, half - 1] == np.float32(s)                                       # phase 0, j = 0: h(0) = s


def test_check_refuses_by_the_kernels_predicate():
    for a, b in ((22050, 16001), (16000, 16000), (48000, 1000), (4097, 4096)):
        with pytest.raises(ValueError) as e:
            audio.resample_check(a, b)
        assert str(a) in str(e.value) and str(b) in str(e.value)
    assert audio.resample_check(22050, 16000) == (320, 441, 188)
    assert audio.resample_check(4096, 1024 * 3)[:2] == (3, 4)


# ---- the NumPy backend against the yardstick -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0].replace(" ", "_") for c in CASES])
def test_numpy_backend_against_the_yardstick(i):
    name, a, b, x = CASES[i]
    y = audio.resample_numpy(audio.resample_tables(a, b), x)
    y64 = rc.reference(name, a, b, x)
    assert y.dtype == np.float32 and y.shape == y64.shape
    e = rc.deviation(y, y64)
    print("%s: %.3e of the output maximum (bar %.3e)" % (name, e, rc.C_NUMPY))
    assert e <= rc.C_NUMPY


def test_numpy_backend_does_not_depend_on_its_blocks(monkeypatch):
    _, a, b, x = CASES[0]
    t = audio.resample_tables(a, b)
    whole = audio.resample_numpy(t, x)
    monkeypatch.setattr(audio, "RESAMPLE_NUMPY_BLOCK", 129)
    assert audio.resample_numpy(t, x).tobytes() == whole.tobytes()
    with pytest.raises(ValueError):
        audio.resample_numpy(t, np.zeros(0, np.float32))


# ---- tones: half a second at amplitude 0.5, the middle half of the output judged -------------------------------------------------------
def tone_through(a, b, hz):
    y = audio.resample_numpy(audio.resample_tables(a, b), rc.tone(a // 2, a, hz)).astype(np.float64)
    mid = slice(len(y) // 4, 3 * len(y) // 4)
    want = 0.5 * np.sin(2.0 * np.pi * hz * np.arange(len(y)) / b)
    return rc.db(np.abs(y - want)[mid].max() / 0.5), rc.db(np.abs(y)[mid].max() / 0.5)


@pytest.mark.parametrize("a,b,hz", [(22050, 16000, 1000.0), (22050, 16000, 7000.0), (48000, 16000, 7000.0), (16000, 22050, 7000.0)])
def test_pass_band_tone_comes_out_as_the_same_sine_at_the_new_rate(a, b, hz):
    err, level = tone_through(a, b, hz)
    print("%d -> %d %.0f Hz: error %.1f dB, level %.2f dB re the amplitude" % (a, b, hz, err, level))
    assert err < -100.0


@pytest.mark.parametrize("a,b,hz", [(22050, 16000, 8500.0), (22050, 16000, 10500.0), (48000, 16000, 9000.0)])
def test_stop_band_tone_is_removed(a, b, hz):
    _, level = tone_through(a, b, hz)
    print("%d -> %d %.0f Hz: output %.1f dB re the amplitude" % (a, b, hz, level))
    assert level < -100.0


# ---- Audio ---------------------------------------------------------------------------------------------------------------------------
def test_audio_refuses_by_default_and_resamples_on_request(tmp_path):
    n = 3210
    path = str(tmp_path / "sixteen.wav")
    ac.write_wav(path, ac.harmonic(n, 16000), 16000)
    hp = hp_at(22050)
    with pytest.raises(ValueError) as e:
        audio.Audio(hp, backend="numpy").load_wav(path)
    assert "sixteen.wav" in str(e.value) and "16000" in str(e.value) and "22050" in str(e.value)
    assert "resampling is not built" in str(e.value)
    a = audio.Audio(hp, backend="numpy", resample=True)
    rate, native = a.read_wav(path)
    assert rate == 16000 and native.dtype == np.float32 and len(native) == n
    y = a.load_wav(path)
    assert y.dtype == np.float32 and len(y) == -(-n * 441 // 320)
    assert y.tobytes() == audio.resample_numpy(audio.resample_tables(16000, 22050), native).tobytes()
    # a file at the target rate comes back untouched, from either kind of Audio
    same = str(tmp_path / "same.wav")
    ac.write_wav(same, ac.harmonic(n, 22050, seed=1), 22050)
    assert a.load_wav(same).tobytes() == audio.Audio(hp, backend="numpy").load_wav(same).tobytes() == a.read_wav(same)[1].tobytes()
    stereo = str(tmp_path / "stereo.wav")
    ac.write_wav(stereo, ac.harmonic(n, 16000), 16000, channels=2)
    with pytest.raises(ValueError) as e:
        a.load_wav(stereo)
    assert "mono" in str(e.value)


def test_resample_batch_keeps_input_order_with_mixed_rates():
    a = audio.Audio(hp_at(16000), backend="numpy", resample=True)
    rates = [22050, 16000, 48000, 22050, 16000, 48000]
    ys = [rc.noise(700 + 37 * i, 40 + i) for i in range(len(rates))]
    out = a.resample_batch(ys, rates)
    assert len(out) == len(ys)
    for y, rate, got in zip(ys, rates, out):
        if rate == 16000:
            assert got is y                                                            # passes through as the same array
        else:
            assert got.tobytes() == audio.resample_numpy(audio.resample_tables(rate, 16000), y).tobytes()
    with pytest.raises(ValueError) as e:
        a.resample_batch([ys[0]], [16001])
    assert "16001" in str(e.value) and "16000" in str(e.value)
    with pytest.raises(ValueError):
        a.resample_batch(ys, rates[:-1])


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_resample_supported_on_both_sides_of_every_bound():
    from satt_amd import ops
    for good in ((320, 441, 188), (1, 3, 406), (441, 320, 136), (1, 2, 2), (2, 1, 4096), (1024, 4095, 2), (1023, 4096, 4096), (1, 4096, 4096)):
        assert ops.resample_supported(*good), good
    for bad in ((1, 1, 136), (2, 4, 136), (320, 440, 188), (0, 441, 188), (1025, 4096, 188), (1025, 1, 188), (320, 0, 188),
                (1, 4097, 188), (3, 4097, 188), (320, 441, 0), (320, 441, 187), (320, 441, 4097), (320, 441, 4098), (-320, 441, 188)):
        assert not ops.resample_supported(*bad), bad
    # resample_check evaluates the same predicate: whatever it accepts, the library accepts
    for a, b in list(rc.RATIOS) + [(48000, 24000), (44100, 48000), (8000, 48000), (4096, 3072)]:
        assert ops.resample_supported(*audio.resample_check(a, b))
    assert (audio.RESAMPLE_MAX_UP, audio.RESAMPLE_MAX_DOWN, audio.RESAMPLE_MAX_TAPS) == (1024, 4096, 4096)
    assert ops.resample_run_length() >= 64


def test_resample_struct_layout_matches_c(tmp_path):
    """sizeof / offsetof of the ctypes mirror == the C struct (host compiler), and the entry points are declared on both sides"""
    from satt_amd import _lib
    names = [n for n, _ in _lib.ResampleParams._fields_]
    assert names == ["up", "down", "taps", "n_utts", "total_in", "total_out", "signal_in", "in_offsets", "out_offsets", "table", "signal_out"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "satt_hip.h"\nint main() {\n  printf("%zu", sizeof(satt_resample_params));\n'
    src += "".join('  printf(" %%zu", offsetof(satt_resample_params, %s));\n' % n for n in names) + "  return 0; }\n"
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    vals = list(map(int, subprocess.check_output([str(tmp_path / "t")]).split()))
    R = _lib.ResampleParams
    assert vals == [ctypes.sizeof(R)] + [getattr(R, n).offset for n in names]
    header = open(os.path.join(ROOT, "include", "satt_hip.h")).read()
    for sym in ("satt_resample_supported", "satt_resample_run_length", "satt_resample"):
        assert sym + "(" in header and sym in _lib.SIGNATURES
    assert _lib.SIGNATURES["satt_resample"][1][-1] is ctypes.c_void_p                  # the stream comes last, as everywhere


# ---- the drivers ---------------------------------------------------------------------------------------------------------------------
AT_16K = "sample_rate=16000,num_freq=513"          # n_fft 1024, hop 200, win 800
HOP_16K = 200


def target_mel(out, key):
    return decode_target_record(next(tfrecord.read_records(os.path.join(out, key + ".target.tfrecord"))))


@pytest.fixture(scope="module")
def lj16(tmp_path_factory):
    root = tmp_path_factory.mktemp("lj16")
    in_dir, out = str(root / "in"), str(root / "out")
    os.makedirs(in_dir)
    corpus = ac.write_toy_ljspeech(in_dir)
    ac.run_driver("preprocess_ljspeech.py", "--hparam-json-file", ac.LJ_JSON, "--hparams", AT_16K, "--backend", "numpy", "--resample",
                  in_dir, out)
    return in_dir, out, corpus


def test_ljspeech_driver_with_resample(lj16, tmp_path):
    in_dir, out, corpus = lj16
    h = json.load(open(os.path.join(out, "hparams.json")))
    assert (h["sample_rate"], h["num_freq"]) == (16000, 513) and len(h["average_mel_level_db"]) == 80
    assert set(os.listdir(out)) == {"list.csv", "hparams.json"} | {"%s.%s.tfrecord" % (k, s) for k, _, _ in corpus for s in ("source", "target")}
    a = audio.Audio(hp_at(16000), backend="numpy", resample=True)
    for i, (key, _, n) in enumerate(corpus):
        t = target_mel(out, key)
        n16 = -(-n * 320 // 441)
        assert t["target_length"] == 1 + n16 // HOP_16K and t["mel"].shape == (1 + n16 // HOP_16K, 80)
        if i == 0:                                                                       # and the record holds the mel of the resampled file
            y = a.load_wav(os.path.join(in_dir, "wavs", key + ".wav"))
            assert len(y) == n16 and np.array_equal(t["mel"], a.melspectrogram(y).T)
    # the emitted corpus loads through the training input pipeline with the emitted hparams.json
    hp = hparams.copy()
    hp.parse_json(open(ac.LJ_JSON).read())
    hp.parse_json(open(os.path.join(out, "hparams.json")).read())
    hp.parse("batch_size=5")
    keys = [k for k, _, _ in corpus]
    batch = next(create_from_tfrecord_files([os.path.join(out, k + ".source.tfrecord") for k in keys],
                                            [os.path.join(out, k + ".target.tfrecord") for k in keys], hp,
                                            cycle_length=2).prepare_and_zip().group_by_batch())
    assert sorted(batch["key"]) == keys and np.isfinite(np.asarray(batch["mel"])).all()
    # without --resample the same command fails by name, as it always did
    r = ac.run_driver("preprocess_ljspeech.py", "--hparam-json-file", ac.LJ_JSON, "--hparams", AT_16K, "--backend", "numpy", in_dir,
                      str(tmp_path / "refused"), check=False)
    assert r.returncode != 0 and "ValueError" in r.stderr and "LJ001-000" in r.stderr and "22050" in r.stderr and "16000" in r.stderr
    assert "resampling is not built" in r.stderr


def test_wavenet_driver(lj16, tmp_path):
    in_dir, out, corpus = lj16
    mel_dir, wav_dir = str(tmp_path / "mel"), str(tmp_path / "wav")
    stats = os.path.join(out, "hparams.json")
    ac.run_driver("preprocess_ljspeech_wavenet.py", "--hparam-json-file", stats, "--backend", "numpy", "--resample", in_dir, mel_dir, wav_dir)
    assert sorted(os.listdir(mel_dir)) == sorted(k + ".mfbsp" for k, _, _ in corpus)
    assert sorted(os.listdir(wav_dir)) == sorted(k + ".wav" for k, _, _ in corpus)
    h = json.load(open(stats))
    for key, _, n in corpus:
        rate, wav = wavfile.read(os.path.join(wav_dir, key + ".wav"))
        mel = np.fromfile(os.path.join(mel_dir, key + ".mfbsp"), "<f4").reshape(-1, 80)
        assert rate == 16000 and wav.dtype == np.float32 and len(wav) == -(-n * 320 // 441)
        assert mel.shape[0] == 1 + len(wav) // HOP_16K
        want = (target_mel(out, key)["mel"] - np.asarray(h["average_mel_level_db"], np.float32)) / np.asarray(h["stddev_mel_level_db"], np.float32)
        assert np.array_equal(mel, want)                                                 # the normalised mel of the LJSpeech driver's record
    # hparams without the per-bin statistics are refused by name
    r = ac.run_driver("preprocess_ljspeech_wavenet.py", "--hparam-json-file", ac.LJ_JSON, "--hparams", AT_16K, "--backend", "numpy",
                      "--resample", in_dir, str(tmp_path / "m2"), str(tmp_path / "w2"), check=False)
    assert r.returncode != 0 and "average_mel_level_db" in r.stderr and "num_mels" in r.stderr
    # and without --resample the wavs are refused by name
    r = ac.run_driver("preprocess_ljspeech_wavenet.py", "--hparam-json-file", stats, "--backend", "numpy", in_dir, str(tmp_path / "m3"),
                      str(tmp_path / "w3"), check=False)
    assert r.returncode != 0 and "ValueError" in r.stderr and "LJ001-000" in r.stderr and "resampling is not built" in r.stderr


def test_vctk_driver_with_resample(tmp_path):
    in_dir, out = str(tmp_path / "in"), str(tmp_path / "out")
    os.makedirs(in_dir)
    corpus = ac.write_toy_vctk(in_dir)
    ac.run_driver("preprocess_vctk.py", "--hparams", AT_16K, "--backend", "numpy", "--resample", in_dir, out)
    keys = [c[0] for c in corpus]
    assert set(os.listdir(out)) == {"list.csv", "hparams.json"} | {"%s.%s.tfrecord" % (k, s) for k in keys for s in ("source", "target")}
    assert json.load(open(os.path.join(out, "hparams.json")))["sample_rate"] == 16000
    a = audio.Audio(hp_at(16000), backend="numpy", resample=True)
    for key, spk, _, _, n in corpus:
        y = a.load_wav(os.path.join(in_dir, "wav48", "p%d" % spk, key + ".wav"))
        assert len(y) == n // 3
        trimmed = a.trim(y)                                                              # the trim runs on the resampled signal
        t = target_mel(out, key)
        # the tone is 0.16 s = 2560 samples at 16 kHz, widened by 4 frame shifts of 200 on either side and by the trim's frame grid
        assert ac.VCTK_TONE // 3 + 8 * HOP_16K <= len(trimmed) <= ac.VCTK_TONE // 3 + 8 * HOP_16K + 4 * 256 < len(y)
        assert t["target_length"] == 1 + len(trimmed) // HOP_16K and t["mel"].shape == (t["target_length"], 80)
    r = ac.run_driver("preprocess_vctk.py", "--hparams", AT_16K, "--backend", "numpy", in_dir, str(tmp_path / "refused"), check=False)
    assert r.returncode != 0 and "ValueError" in r.stderr and "48000" in r.stderr and "16000" in r.stderr and "p225_001.wav" in r.stderr
