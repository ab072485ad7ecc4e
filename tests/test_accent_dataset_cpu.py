"""The accent_type field of the corpus records (this project's definition: an optional bytes feature of `<key>.source.tfrecord`,
raw little-endian int64, source_length entries): round trip, padding value, the error cases, the C-indexed and the pure-Python
record decoders side by side, and the prediction record."""
import os

import numpy as np
import pytest

import satt_amd  # noqa: F401
from satt_amd.datasets import ljspeech
from satt_amd.hparams import hparams
from satt_amd.utils import tfrecord


def hp_accent(**kw):
    hp = hparams.copy()
    hp.parse_json(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "ljspeech",
                                    "self-attention-tacotron-accent.json")).read())
    hp.batch_size = 3
    hp.average_mel_level_db = [0.0] * 80; hp.stddev_mel_level_db = [1.0] * 80
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


def write_corpus(d, n=5, accent=True, seed=0, tamper=None):
    g = np.random.default_rng(seed)
    files, truth = [], []
    for i in range(n):
        L = int(g.integers(3, 9))
        src = g.integers(1, 40, L).astype(np.int64)
        acc = (g.integers(0, 129, L) + 0x3100).astype(np.int64)
        key = "utt%d" % i
        ex = tfrecord.make_source_example(i, key, src, "hello", acc if accent else None)
        if tamper is not None and i == 1:
            ex = tamper(i, key, src, acc)
        ps, pt = os.path.join(d, key + ".source.tfrecord"), os.path.join(d, key + ".target.tfrecord")
        tfrecord.write_records(ps, [ex])
        T = int(g.integers(4, 9))
        mel = g.normal(0, 1, (T, 80)).astype("<f4")
        tfrecord.write_records(pt, [tfrecord.make_example({"id": i, "key": key.encode(), "mel": mel.tobytes(), "mel_width": 80,
                                                           "target_length": T})])
        files.append((ps, pt)); truth.append((src, acc))
    return files, truth


def batches(files, hp, native=True, workers=None):
    ds = ljspeech.Dataset([f[0] for f in files], [f[1] for f in files], hp, cycle_length=None,
                          **({} if workers is None else dict(num_workers=workers)))
    ds.native_reader = native
    return list(ds.prepare_and_zip().group_by_batch(hp.batch_size))


READERS = [(True, 3), (True, 1), (False, 3), (False, 1)]      # native reader threads / Python thread pool, several and one worker


def test_round_trip_and_padding(tmp_path):
    hp = hp_accent()
    files, truth = write_corpus(str(tmp_path))
    out = batches(files, hp)
    assert sum(b["source"].shape[0] for b in out) == 5
    n = 0
    for b in out:
        assert b["accent_type"].dtype == np.int64 and b["accent_type"].shape == b["source"].shape
        for r in range(b["source"].shape[0]):
            src, acc = truth[n]; n += 1
            L = int(b["source_length"][r])
            assert L == len(src) and (b["source"][r, :L] == src).all() and (b["accent_type"][r, :L] == acc).all()
            assert (b["source"][r, L:] == 0).all() and (b["accent_type"][r, L:] == hp.accent_type_offset).all()
    # a model without accent types ignores the field
    hp2 = hp_accent(use_accent_type=False, encoder="SelfAttentionCBHGEncoder")
    assert all("accent_type" not in b for b in batches(files, hp2))


def test_native_utterance_decoder_agrees_with_python(tmp_path):
    """satt_utterance_load (csrc/host_io.c) against decode_source_record, with and without the field; then the native reader
    threads, the Python thread pool and the sequential path give the same accent batches in the same order"""
    from satt_amd import _io
    files, truth = write_corpus(str(tmp_path), n=7)
    for (ps, pt), (src, acc) in zip(files, truth):
        arena, u = _io.utterance_load(ps, pt, 2)
        py = ljspeech.decode_source_record(next(tfrecord.read_records(ps)))
        assert u.accent_count == u.source_length == py.source_length == len(acc)
        got = np.frombuffer(arena[u.accent_off:u.accent_off + 8 * u.accent_count], "<i8")
        assert np.array_equal(got, py.accent_type) and np.array_equal(got, acc)
        assert np.array_equal(np.frombuffer(arena[u.source_off:u.source_off + 8 * u.source_count], "<i8"), py.source)
    os.makedirs(str(tmp_path / "plain"))
    plain, _ = write_corpus(str(tmp_path / "plain"), accent=False)
    _, u = _io.utterance_load(plain[0][0], plain[0][1], 2)
    assert u.accent_count == -1
    hp = hp_accent()
    ref = batches(files, hp, native=False, workers=1)
    assert len(ref) == 3
    for native, workers in READERS:
        got = batches(files, hp, native=native, workers=workers)
        assert len(got) == len(ref)
        for a, b in zip(ref, got):
            assert a["key"] == b["key"]
            for k in ("source", "source_length", "accent_type", "mel"):
                assert np.array_equal(a[k], b[k]), (k, native, workers)


def test_c_indexed_and_python_decoders_agree(tmp_path):
    files, truth = write_corpus(str(tmp_path))
    for (ps, _), (src, acc) in zip(files, truth):
        a = ljspeech.decode_source_view(tfrecord.read_record_views(ps)[0])          # include/satt_io.h index
        b = ljspeech.decode_source_record(next(tfrecord.read_records(ps)))          # pure-Python protobuf walk
        assert a.key == b.key and a.source_length == b.source_length == len(src)
        assert (a.source == b.source).all() and (a.accent_type == acc).all() and (b.accent_type == acc).all()
    os.makedirs(str(tmp_path / "plain"))
    files, _ = write_corpus(str(tmp_path / "plain"), accent=False)
    a = ljspeech.decode_source_view(tfrecord.read_record_views(files[0][0])[0])
    b = ljspeech.decode_source_record(next(tfrecord.read_records(files[0][0])))
    assert a.accent_type is None and b.accent_type is None


def test_missing_field_names_the_key(tmp_path):
    files, _ = write_corpus(str(tmp_path), accent=False)
    for native, workers in READERS:
        with pytest.raises(ValueError, match="utt0 has no accent_type"):
            batches(files, hp_accent(), native=native, workers=workers)


def test_wrong_length_names_the_key(tmp_path):
    def short(i, key, src, acc):
        ex = tfrecord.make_source_example(i, key, src, "hello")
        f = tfrecord.parse_example(ex)
        return tfrecord.make_example({"id": i, "key": key.encode(), "source": f["source"][0], "source_length": len(src),
                                      "text": b"hello", "accent_type": acc[:-1].astype("<i8").tobytes()})
    files, _ = write_corpus(str(tmp_path), tamper=short)
    with pytest.raises(ValueError, match="utt1: accent_type holds"):
        ljspeech.decode_source_record(next(tfrecord.read_records(files[1][0])))
    for native, workers in READERS:       # the native decoder refuses it with its own code; both messages name the utterance
        with pytest.raises(ValueError, match=r"utt1.*accent_type.*source_length"):
            batches(files, hp_accent(), native=native, workers=workers)
    from satt_amd import _io
    with pytest.raises(ValueError, match=r"utt1.*accent_type feature does not hold source_length"):
        _io.utterance_load(files[1][0], files[1][1], 2)
    with pytest.raises(ValueError, match="one id per source symbol"):
        tfrecord.make_source_example(0, "k", np.arange(4), "", np.arange(3))


def test_out_of_range_ids(tmp_path):
    def stray(i, key, src, acc):
        acc = acc.copy(); acc[0] = 5
        return tfrecord.make_source_example(i, key, src, "hello", acc)
    files, truth = write_corpus(str(tmp_path), tamper=stray)
    hp = hp_accent()                                   # accent_type_unknown = 0x3180 lies in [0x3100, 0x3100 + 129)
    for native, workers in READERS:
        out = batches(files, hp, native=native, workers=workers)
        assert out[0]["accent_type"][1, 0] == hp.accent_type_unknown
        assert (out[0]["accent_type"][1, 1:len(truth[1][1])] == truth[1][1][1:]).all()
        with pytest.raises(ValueError, match=r"utt1: accent_type 5 outside \[12544, 12673\) and accent_type_unknown = 7"):
            batches(files, hp_accent(accent_type_unknown=7), native=native, workers=workers)


def test_prediction_record_round_trips_accent_type(tmp_path):
    acc = (np.arange(6) + 0x3100).astype(np.int64)
    p = str(tmp_path / "p.tfrecord")
    tfrecord.write_prediction_result(3, "k", [np.zeros((6, 4), np.float32)], np.zeros((8, 80), np.float32),
                                     np.zeros((8, 80), np.float32), "text", np.arange(6, dtype=np.int64), acc, p)
    back = tfrecord.parse_prediction_result(next(tfrecord.read_records(p)))
    assert (back["accent_type"] == acc).all() and (back["source"] == np.arange(6)).all()
