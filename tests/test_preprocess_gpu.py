"""The LJSpeech driver with the HIP mel kernel (--backend hip) against its --backend numpy run on the same toy corpus, and the emitted
corpus through the training input pipeline."""
import json
import os

import numpy as np
import pytest

import audio_common as ac
import satt_amd  # noqa: F401
from satt_amd.datasets.dataset_factory import create_from_tfrecord_files
from satt_amd.datasets.ljspeech import decode_target_record
from satt_amd.hparams import hparams
from satt_amd.utils import tfrecord

pytestmark = pytest.mark.gpu


def test_ljspeech_driver_on_the_hip_backend(tmp_path):
    in_dir = str(tmp_path / "in")
    os.makedirs(in_dir)
    corpus = ac.write_toy_ljspeech(in_dir)
    outs = {}
    for backend in ("hip", "numpy"):
        outs[backend] = str(tmp_path / backend)
        ac.run_driver("preprocess_ljspeech.py", "--hparam-json-file", ac.LJ_JSON, "--backend", backend, in_dir, outs[backend])
    assert sorted(os.listdir(outs["hip"])) == sorted(os.listdir(outs["numpy"]))
    keys = [k for k, _, _ in corpus]
    for key, _, n in corpus:
        mel = {b: decode_target_record(next(tfrecord.read_records(os.path.join(outs[b], key + ".target.tfrecord"))))["mel"] for b in outs}
        assert mel["hip"].shape == mel["numpy"].shape == (1 + n // ac.LJ_HOP, 80)
        assert np.abs(mel["hip"] - mel["numpy"]).max() <= ac.C_DB
        src = [open(os.path.join(outs[b], key + ".source.tfrecord"), "rb").read() for b in ("hip", "numpy")]
        assert src[0] == src[1]
    h = {b: json.load(open(os.path.join(outs[b], "hparams.json"))) for b in outs}
    for k in ("average_mel_level_db", "stddev_mel_level_db", "min_mel_level_db"):
        assert np.abs(np.asarray(h["hip"][k]) - np.asarray(h["numpy"][k])).max() <= ac.C_DB, k
    # the emitted corpus loads through the training input pipeline with the emitted hparams.json
    hp = hparams.copy()
    hp.parse_json(open(ac.LJ_JSON).read())
    hp.parse_json(open(os.path.join(outs["hip"], "hparams.json")).read())
    hp.parse("batch_size=5")
    src = [os.path.join(outs["hip"], k + ".source.tfrecord") for k in keys]
    tgt = [os.path.join(outs["hip"], k + ".target.tfrecord") for k in keys]
    b = next(create_from_tfrecord_files(src, tgt, hp, cycle_length=2).prepare_and_zip().group_by_batch())
    assert sorted(b["key"]) == keys
    assert np.isfinite(np.asarray(b["mel"])).all()
