"""predict_mel.py --stop-per-utterance and Model.predict(stop_each=True): free-running synthesis of several utterances per decode,
every prediction cut at its utterance's own stop token.

The corpus is five utterances of different lengths (the pattern of tests/test_decode_forced_groups_gpu.py) and a freshly initialised
LJSpeech model with PostNetV2.  Such a model never crosses the default stop threshold, so the fixture prepares the checkpoint: it
decodes the driver's own batches once at full length, scales the stop column of the output projection (the stop logit is not fed
back: the frames stay what they are) and shifts the stop bias so that logit 0 - the default threshold 0.5 - falls into a gap of the
logits at which the utterances of the batch of four end at different steps within max_iters, no logit within 1e-3 of it.  What the
driver must then write follows from those full-length logits on the host (decode_ends_common.ends_of_logits)."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

from decode_common import recording
from decode_ends_common import ends_of_logits, logit, margin_ok, pick_threshold, write_corpus

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [(9, 21), (14, 30), (11, 17), (8, 26), (12, 23)]          # five utterances of different lengths (symbols, raw frames)
MAX_ITERS, MIN_STEPS, SCALE = 40, 10, 16.0


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """corpus, list, hparams file and the prepared checkpoint; yields (tmp, keys, the driver's common arguments, the expected number
    of decoder steps per key, the hparams file).  The global hparams object predict_mel.main parses into is restored afterwards."""
    sys.path.insert(0, ROOT)
    import satt_amd  # noqa: F401
    from satt_amd import ops
    from satt_amd.datasets.ljspeech import source_batches
    from satt_amd.hparams import hparams
    from satt_amd.inference import infer
    from satt_amd.models.models import tacotron_model_factory
    saved = copy.deepcopy(hparams.values())
    tmp = tmp_path_factory.mktemp("stop_each_driver")
    data, lists, ckpt = tmp / "data", tmp / "lists", tmp / "ckpt"
    for d in (data, lists, ckpt):
        d.mkdir()
    keys = write_corpus(str(data), LENGTHS)
    (lists / "test.csv").write_text("\n".join(keys) + "\n")
    d = json.load(open(os.path.join(ROOT, "examples", "ljspeech", "self-attention-tacotron.json")))
    d.pop("_comment", None)
    d.update(average_mel_level_db=[-40.0], stddev_mel_level_db=[10.0], use_postnet_v2=True, max_iters=MAX_ITERS)
    cfg = str(tmp / "hparams.json")
    json.dump(d, open(cfg, "w"))
    hp = hparams.copy()
    hp.parse_json(open(cfg).read())
    try:
        model = tacotron_model_factory(hp, str(ckpt), device="cuda")
        eng = model.engine
        src = [os.path.join(str(data), "%s.%s" % (k, hp.source_file_extension)) for k in keys]

        def full_logits():
            rows = []
            for b in source_batches(src, hp, 4):
                out = infer(eng, b["source"], b["source_length"], max_steps=MAX_ITERS, min_steps=10 ** 6, stop="each")
                rows.append(out["stop"][:, :, 0].cpu().numpy().astype(np.float64))
            return rows
        eng.P["dec.out.W"][:, -1] *= SCALE
        first, last = full_logits()
        bias = float(eng.P["dec.out.b"][-1])
        # either sign of the scale: x -> 2 bias - x mirrors the logits about the bias
        shift = None
        for sign in (1.0, -1.0):
            a, b = ((first, last) if sign > 0 else (2 * bias - first, 2 * bias - last))
            thr = pick_threshold(a, MIN_STEPS, 0, others=b)
            if thr is not None:
                want4 = ends_of_logits(a, MIN_STEPS, thr, MAX_ITERS)
                if (want4 < MAX_ITERS).all():
                    shift, flip = -logit(thr), sign < 0
                    break
        assert shift is not None, "no gap of the stop logits ends the four utterances at different steps"
        if flip:
            eng.P["dec.out.W"][:, -1] *= -1.0
        eng.P["dec.out.b"][-1] += shift
        ops.set_precision("bf16")
        first, last = full_logits()          # the logits of the prepared model, as the driver will see them
        assert margin_ok(first, 0.5) and margin_ok(last, 0.5)
        want = dict(zip(keys, ends_of_logits(first, MIN_STEPS, 0.5, MAX_ITERS).tolist() + ends_of_logits(last, MIN_STEPS, 0.5, MAX_ITERS).tolist()))
        four = [want[k] for k in keys[:4]]
        assert len(set(four)) >= 2 and max(four) < MAX_ITERS, four
        model.save()
        del model, eng
        common = ["--source-data-root", str(data), "--checkpoint-dir", str(ckpt), "--selected-list-dir", str(lists), "--hparam-json-file", cfg]
        yield tmp, keys, common, want, cfg
    finally:
        hparams._v.clear(); hparams._v.update(saved)
        ops.set_precision("bf16")


def predict(corpus, name, extra=(), forced=False):
    """predict_mel.main in process; returns (output directory, the names of the recorded launches of the persistent kernel).  The
    mode is given every time: main parses into the global hparams object, which keeps what an earlier call set"""
    import predict_mel
    tmp, keys, common = corpus[:3]
    out = tmp / name
    out.mkdir()
    with recording() as launches:
        predict_mel.main(["--output-dir", str(out), "--hparams", "use_forced_alignment_mode=%s" % forced] + common + list(extra))
    return out, [l.name for l in launches]


def test_stop_per_utterance_cuts_every_prediction_at_its_own_end(corpus):
    tmp, keys, _, want, _ = corpus
    one, launched1 = predict(corpus, "bs1")
    new, launched = predict(corpus, "bs4", ("--batch-size", "4", "--stop-per-utterance"))
    assert "dec_mega_groups" in launched and "dec_mega_groups" not in launched1          # the batch of four ran in group mode: FAILS ON THE PARENT
    files = sorted(os.listdir(new))
    assert files == sorted(k + e for k in keys for e in (".mfbsp", ".alignment.npz", ".png", ".tfrecord")) == sorted(os.listdir(one))
    for k, (L, _) in zip(keys, LENGTHS):
        n = want[k]
        mel = np.fromfile(new / (k + ".mfbsp"), dtype="<f4").reshape(-1, 80)
        print(k, "steps", n, "frames", mel.shape[0])
        assert mel.shape == (n * 2, 80) and np.isfinite(mel).all(), (k, mel.shape, n)
        z = np.load(new / (k + ".alignment.npz"))
        for name in ("alignment", "alignment2"):
            assert z[name].shape == (L, n), (k, name, z[name].shape)          # [T_memory, T_query], cut to the utterance
            assert np.allclose(z[name].sum(0), 1.0, atol=1e-4), (k, name)
    # the fifth utterance is a batch of one in both runs: the same rule, the same number of frames
    a, b = (np.fromfile(d / (keys[4] + ".mfbsp"), dtype="<f4") for d in (new, one))
    assert a.shape == b.shape


def test_the_switch_is_free_running_only(corpus):
    tmp = corpus[0]
    with pytest.raises(SystemExit) as e:
        predict(corpus, "forced", ("--batch-size", "4", "--stop-per-utterance", "--target-data-root", str(tmp / "data")),
                forced=True)
    assert "--stop-per-utterance" in str(e.value)
    assert not os.listdir(tmp / "forced")


def test_a_free_running_batch_without_the_switch_is_still_refused(corpus):
    with pytest.raises(SystemExit) as e:
        predict(corpus, "refused", ("--batch-size", "4"))
    assert "use_forced_alignment_mode" in str(e.value) and "a free-running batch has no per-utterance end" in str(e.value)
    assert not os.listdir(corpus[0] / "refused")


def test_postnet_sees_each_utterance_alone(corpus):
    """Model.predict(stop_each=True): mel_postnet of an utterance is postnet_infer of ITS cut mel, batch 1 - not a slice of the
    post-net over the padded batch, whose `same` convolutions would see the frames decoded after the utterance's stop token.
    Two postnet_infer calls on one input are not bit-equal as the library stands: its convolutions (K = 5 x 512 products per output,
    a few output tiles) run split along K and the slices are added by atomics in the order they arrive (measured here with the
    split on: 0, 0, 7.5e-7 and 4.8e-4 of the largest element for the four utterances - a reordered fp32 sum that flips the bf16
    rounding of an activation of the next layer).  That is the reference's own noise and no property of predict(), so the test
    takes it out: inside postnet_infer - there only, the decode is untouched - ops._splitk returns 1, every product is one
    ordered sum, and "equals" is held to bits."""
    from common import rel_err
    from satt_amd.datasets.ljspeech import source_batches
    from satt_amd.hparams import hparams
    from satt_amd.models.models import tacotron_model_factory
    tmp, keys, _, want, cfg = corpus
    hp = hparams.copy()
    hp.parse_json(open(cfg).read())
    hp.parse("use_forced_alignment_mode=False")
    model = tacotron_model_factory(hp, None, device="cuda")
    model.restore(str(max((tmp / "ckpt").glob("model-*.pt"))))
    src = [os.path.join(str(tmp / "data"), "%s.%s" % (k, hp.source_file_extension)) for k in keys[:4]]
    from satt_amd import inference, ops
    real = inference.postnet_infer

    def postnet_infer(eng, mel):
        splitk = ops._splitk
        ops._splitk = lambda tiles, k, target=320: 1
        try:
            return real(eng, mel)
        finally:
            ops._splitk = splitk
    inference.postnet_infer = postnet_infer          # (predict() looks the function up per call)
    try:
        preds = list(model.predict(lambda: source_batches(src, hp, 4), stop_each=True))
        assert [p["key"] for p in preds] == keys[:4]
        whole = []
        for p, (L, _) in zip(preds, LENGTHS):
            n = want[p["key"]]
            assert p["mel"].shape == p["mel_postnet"].shape == (2 * n, 80) and p["source"].shape == (L,)
            alone = postnet_infer(model.engine, torch.as_tensor(p["mel"]).cuda()[None])[0].cpu().numpy()
            print("%s mel_postnet against postnet_infer of the cut mel alone: rel_err=%.3e" % (p["key"], rel_err(p["mel_postnet"], alone)))
            assert np.array_equal(p["mel_postnet"], alone), p["key"]
            whole.append(p)
        # without the switch predict() is what it was: the batch rule (all four above the threshold at one step), nothing cut
        plain = list(model.predict(lambda: source_batches(src, hp, 4)))
    finally:
        inference.postnet_infer = real
    T = plain[0]["mel"].shape[0] // 2
    assert max(want[k] for k in keys[:4]) <= T <= MAX_ITERS
    assert all(p["mel"].shape == (2 * T, 80) and p["source"].shape == (max(L for L, _ in LENGTHS[:4]),) for p in plain)
    short = min(range(4), key=lambda i: want[keys[i]])
    n = want[keys[short]]
    assert np.array_equal(plain[short]["mel"][:2 * n], whole[short]["mel"])          # the same frames, cut
    far = rel_err(plain[short]["mel_postnet"][:2 * n], whole[short]["mel_postnet"])          # the padded post-net differs at the end
    print("slice of the padded batch's post-net against the utterance's own: rel_err=%.3e" % far)
    assert far > 1e-2, far          # (measured: 0.53 of the largest element)
