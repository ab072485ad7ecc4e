"""mel_to_wav.py on the HIP backend (a batch in one entry call equals one-by-one conversion bit for bit) and predict_mel.py --wav on
a freshly initialised LJSpeech-configuration checkpoint."""
import json
import os

import numpy as np
import pytest

import audio_common as ac
import griffin_lim_common as gc
import satt_amd  # noqa: F401

pytestmark = pytest.mark.gpu


def test_mel_to_wav_on_the_hip_backend_equals_one_by_one_conversion(tmp_path):
    cfg, mel_dir, _ = gc.write_mel_dir(tmp_path)
    out = str(tmp_path / "wavs")
    ac.run_driver("mel_to_wav.py", "--hparam-json-file", cfg, "--backend", "hip", "--iters", "5", mel_dir, out)
    wavs = gc.check_wav_dir(out)
    a = gc.lj_audio("hip")
    for i, pcm in enumerate(wavs):
        S = np.fromfile(os.path.join(mel_dir, "utt%d.mfbsp" % i), dtype="<f4").reshape(-1, 80) * np.float32(12.0) + np.float32(-30.0)
        a.save_wav_pcm16(a.inv_melspectrogram(S.T, iters=5), str(tmp_path / "one.wav"))           # a call of its own
        assert gc.read_wav(str(tmp_path / "one.wav"))[1].tobytes() == pcm.tobytes(), i


def test_predict_mel_writes_wavs_only_when_asked(tmp_path):
    from satt_amd.hparams import hparams
    from satt_amd.models.models import tacotron_model_factory
    from satt_amd.utils import tfrecord
    data, lists, ckpt = tmp_path / "data", tmp_path / "lists", tmp_path / "ckpt"
    for d in (data, lists, ckpt):
        d.mkdir()
    g = np.random.default_rng(0)
    s = np.concatenate([[0], g.integers(1, 60, 9), [0]]).astype("<i8")
    tfrecord.write_records(str(data / "LJ000.source.tfrecord"), [tfrecord.make_example(
        {"id": 0, "key": b"LJ000", "source": s.tobytes(), "source_length": len(s), "text": b"abc"})])
    (lists / "test.csv").write_text("LJ000\n")
    d = json.load(open(ac.LJ_JSON))
    d.pop("_comment", None)
    d.update(average_mel_level_db=[-40.0], stddev_mel_level_db=[10.0])
    cfg = str(tmp_path / "hparams.json")
    json.dump(d, open(cfg, "w"))
    hp = hparams.copy()
    hp.parse_json(json.dumps(d))
    tacotron_model_factory(hp, str(ckpt), device="cuda").save()                    # model-0.pt: the initial parameters
    common = ["--source-data-root", str(data), "--checkpoint-dir", str(ckpt), "--selected-list-dir", str(lists), "--hparam-json-file", cfg,
              "--hparams", "max_iters=12"]
    plain, wav = tmp_path / "plain", tmp_path / "wav"
    ac.run_driver("predict_mel.py", "--output-dir", str(plain), *common)
    ac.run_driver("predict_mel.py", "--output-dir", str(wav), "--wav", "--griffin-lim-iters", "4", *common)
    names = ["LJ000.alignment.npz", "LJ000.mfbsp", "LJ000.png", "LJ000.tfrecord"]
    assert sorted(os.listdir(plain)) == names and sorted(os.listdir(wav)) == sorted(names + ["LJ000.wav"])
    assert open(plain / "LJ000.mfbsp", "rb").read() == open(wav / "LJ000.mfbsp", "rb").read()
    rate, pcm = gc.read_wav(str(wav / "LJ000.wav"))
    assert rate == 22050 and len(pcm) == (24 - 1) * 275 and np.abs(pcm.astype(np.int32)).max() == round(0.95 * 32767)
