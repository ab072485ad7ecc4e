"""train.py / predict_mel.py with the reference's command lines on a tiny on-disk corpus that carries `accent_type`
(examples/ljspeech/self-attention-tacotron-accent.json): training with checkpoints and the EVAL double pass, then synthesis whose
prediction records hold the accent ids of the utterance."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_accent_train_evaluate_predict(tmp_path):
    sys.path.insert(0, ROOT)
    import satt_amd  # noqa: F401
    from satt_amd.utils import tfrecord
    g = np.random.default_rng(0)
    data, lists, ckpt, out = tmp_path / "data", tmp_path / "lists", tmp_path / "ckpt", tmp_path / "out"
    for d in (data, lists, ckpt, out):
        d.mkdir()
    keys = ["JP%03d" % i for i in range(6)]
    accents = {}
    for i, k in enumerate(keys):
        L, T = int(g.integers(8, 16)), int(g.integers(20, 40))
        s = np.concatenate([[0], g.integers(1, 60, L - 2), [0]]).astype("<i8")
        accents[k] = (g.integers(0, 129, L) + 0x3100).astype(np.int64)
        tfrecord.write_records(str(data / (k + ".source.tfrecord")), [tfrecord.make_source_example(i, k, s, "abc", accents[k])])
        mel = g.normal(-40, 10, (T, 80)).astype("<f4")
        tfrecord.write_records(str(data / (k + ".target.tfrecord")), [tfrecord.make_example(
            {"id": i, "key": k.encode(), "mel": mel.tobytes(), "mel_width": 80, "target_length": T})])
    (lists / "train.csv").write_text("\n".join(keys[:4]) + "\n")
    (lists / "test.csv").write_text("\n".join(keys[4:]) + "\n")
    (lists / "validation.csv").write_text("\n".join(keys[2:4]) + "\n")
    d = json.load(open(os.path.join(ROOT, "examples", "ljspeech", "self-attention-tacotron-accent.json")))
    d.pop("_comment", None)
    d.update(average_mel_level_db=[-40.0], stddev_mel_level_db=[10.0])
    cfg = str(tmp_path / "hparams.json")
    json.dump(d, open(cfg, "w"))
    hp = "batch_size=2,save_checkpoints_steps=2,logfile=%s" % (tmp_path / "log.txt")
    common = ["--source-data-root", str(data), "--target-data-root", str(data), "--checkpoint-dir", str(ckpt),
              "--selected-list-dir", str(lists), "--hparam-json-file", cfg]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--max-steps", "4", "--hparams", hp] + common,
                       capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stderr[-2000:]
    log = open(tmp_path / "log.txt").read()
    assert os.path.exists(ckpt / "model-4.pt") and "step 4 loss" in log and "eval step 4" in log
    import torch
    a, b = torch.load(str(ckpt / "model-2.pt"), map_location="cpu"), torch.load(str(ckpt / "model-4.pt"), map_location="cpu")
    from satt_amd.hparams import hparams
    from satt_amd.params import ModelConfig, layout
    h = hparams.copy(); h.parse_json(open(cfg).read())
    lay, n = layout(ModelConfig.from_hparams(h))
    assert a["params"].numel() == n
    for k in ("accent_embedding", "enc.accent_prenet0.W", "enc.accent_prenet1.b"):       # checkpointed by name, and trained
        o, shp = lay[k]
        m = int(np.prod(shp))
        assert not torch.equal(a["params"][o:o + m], b["params"][o:o + m]), k
    r = subprocess.run([sys.executable, os.path.join(ROOT, "predict_mel.py"), "--output-dir", str(out), "--hparams",
                        "max_iters=12"] + common, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stderr[-2000:]
    for k in keys[4:]:
        mel = np.fromfile(out / (k + ".mfbsp"), dtype="<f4").reshape(-1, 80)
        assert mel.shape[0] == 24 and np.isfinite(mel).all()
        p = tfrecord.parse_prediction_result(next(tfrecord.read_records(str(out / (k + ".tfrecord")))))
        assert p["key"] == k and np.array_equal(p["accent_type"], accents[k]) and len(p["source"]) == len(accents[k])
    # synthesis from the source records alone (no --target-data-root: what a TTS user runs) carries the accent ids too
    out2 = tmp_path / "out2"; out2.mkdir()
    nc = list(common)
    i = nc.index("--target-data-root"); del nc[i:i + 2]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "predict_mel.py"), "--output-dir", str(out2), "--hparams",
                        "max_iters=12"] + nc, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stderr[-2000:]
    for k in keys[4:]:
        a = np.fromfile(out / (k + ".mfbsp"), dtype="<f4"); b = np.fromfile(out2 / (k + ".mfbsp"), dtype="<f4")
        assert a.shape == b.shape and np.allclose(a, b, atol=1e-3)           # the same utterance, the same ids: the same mel
        p = tfrecord.parse_prediction_result(next(tfrecord.read_records(str(out2 / (k + ".tfrecord")))))
        assert p["key"] == k and np.array_equal(p["accent_type"], accents[k])
    # a source record without the field is refused by name on this path as well
    bad = tmp_path / "bad"; bad.mkdir()
    for k in keys[4:]:
        s = np.frombuffer(tfrecord.parse_example(next(tfrecord.read_records(str(data / (k + ".source.tfrecord")))))["source"][0], "<i8")
        tfrecord.write_records(str(bad / (k + ".source.tfrecord")), [tfrecord.make_source_example(0, k, s, "abc")])
    nb = list(nc); nb[nb.index("--source-data-root") + 1] = str(bad)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "predict_mel.py"), "--output-dir", str(out2), "--hparams",
                        "max_iters=12"] + nb, capture_output=True, text=True, timeout=200)
    assert r.returncode != 0 and "JP004 has no accent_type" in r.stderr
