"""mel_to_wav.py on the NumPy backend: a directory of three .mfbsp files of different lengths becomes three wavs; an hparams.json
without the corpus statistics is refused by name."""
import os

import numpy as np

import audio_common as ac
import griffin_lim_common as gc
import satt_amd  # noqa: F401


def test_mel_to_wav_on_the_numpy_backend(tmp_path):
    cfg, mel_dir, mels = gc.write_mel_dir(tmp_path)
    out = str(tmp_path / "wavs")
    r = ac.run_driver("mel_to_wav.py", "--hparam-json-file", cfg, "--backend", "numpy", "--iters", "3", mel_dir, out)
    assert "utt2: %d samples" % (14 * 275) in r.stdout
    wavs = gc.check_wav_dir(out)
    # the driver's numbers are those of the Audio class on the de-normalised file contents
    a = gc.lj_audio("numpy")
    S = np.fromfile(os.path.join(mel_dir, "utt1.mfbsp"), dtype="<f4").reshape(-1, 80) * np.float32(12.0) + np.float32(-30.0)
    assert np.abs(S - mels[1]).max() <= 1e-4
    a.save_wav_pcm16(a.inv_melspectrogram(S.T, iters=3), str(tmp_path / "one.wav"))
    assert gc.read_wav(str(tmp_path / "one.wav"))[1].tobytes() == wavs[1].tobytes()


def test_mel_to_wav_refuses_an_hparams_file_without_the_corpus_statistics(tmp_path):
    cfg, mel_dir, _ = gc.write_mel_dir(tmp_path, stats=False)
    r = ac.run_driver("mel_to_wav.py", "--hparam-json-file", cfg, "--backend", "numpy", mel_dir, str(tmp_path / "wavs"), check=False)
    assert r.returncode != 0 and "average_mel_level_db" in r.stderr and "stddev_mel_level_db" in r.stderr
    assert not os.path.exists(str(tmp_path / "wavs"))


def test_pcm16_scales_the_peak_and_keeps_silence_silent(tmp_path):
    a = gc.lj_audio("numpy")
    a.save_wav_pcm16(np.asarray([0.0, 0.001, -0.004, 0.002], np.float32), str(tmp_path / "a.wav"))
    rate, pcm = gc.read_wav(str(tmp_path / "a.wav"))
    assert rate == 22050 and pcm.tolist() == [0, 7782, -31129, 15564]
    a.save_wav_pcm16(np.zeros(5, np.float32), str(tmp_path / "z.wav"))
    assert gc.read_wav(str(tmp_path / "z.wav"))[1].tolist() == [0] * 5
