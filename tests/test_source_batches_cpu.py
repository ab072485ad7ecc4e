"""Batches of utterances that have no targets (synthesis from the source records alone, predict_mel.py without --target-data-root):
ljspeech.source_batches / pad_sources state the source padding ONCE - they give, key by key and bit by bit, the source side of what
group_by_batch builds from the same records with targets (pad value 0 for `source`, accent_type_offset for `accent_type`, the
unknown-id mapping, the missing-field error, speaker ids), at batch size 1 the batch the driver used to build by hand, and the last
batch of a list is the ragged rest."""
import numpy as np
import pytest

import satt_amd  # noqa: F401
from satt_amd.datasets import ljspeech
from satt_amd.utils import tfrecord
from test_accent_dataset_cpu import batches, hp_accent, write_corpus

SOURCE_KEYS = ("source", "source_length", "id", "key", "text", "accent_type", "speaker_id")


def same_source_side(got, want):
    assert [k for k in SOURCE_KEYS if k in got] == [k for k in SOURCE_KEYS if k in want]
    assert set(got) <= set(SOURCE_KEYS), set(got)          # nothing of a target
    for k in got:
        if isinstance(want[k], np.ndarray):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
        else:
            assert list(got[k]) == list(want[k]), k


@pytest.mark.parametrize("accent", [True, False])
@pytest.mark.parametrize("bs", [1, 2, 3, 5, 8])
def test_source_batches_are_the_source_side_of_group_by_batch(tmp_path, accent, bs):
    hp = hp_accent(batch_size=bs) if accent else hp_accent(batch_size=bs, use_accent_type=False, encoder="SelfAttentionCBHGEncoder")
    files, truth = write_corpus(str(tmp_path), n=5)
    want = batches(files, hp)
    got = list(ljspeech.source_batches([f[0] for f in files], hp, bs))
    assert [len(b["key"]) for b in got] == [len(b["key"]) for b in want] == [bs] * (5 // bs) + ([5 % bs] if 5 % bs else [])
    for g, w in zip(got, want):
        same_source_side(g, w)
        assert ("accent_type" in g) == accent
    # the pad values, looked at directly
    for b in got:
        for r, L in enumerate(b["source_length"]):
            assert (b["source"][r, L:] == 0).all()
            if accent:
                assert (b["accent_type"][r, L:] == hp.accent_type_offset).all()


def test_a_batch_of_one_is_the_batch_the_driver_built_by_hand(tmp_path):
    """source [1, L] as stored, source_length / id [1], key / text lists of one, accent ids resolved over the symbols"""
    hp = hp_accent()
    files, truth = write_corpus(str(tmp_path), n=3)
    for i, (b, (src, acc)) in enumerate(zip(ljspeech.source_batches([f[0] for f in files], hp), truth)):
        assert b["source"].shape == (1, len(src)) and b["source"].dtype == np.int64 and (b["source"][0] == src).all()
        assert b["source_length"].tolist() == [len(src)] and b["id"].tolist() == [i] and b["id"].dtype == np.int64
        assert b["key"] == ["utt%d" % i] and b["text"] == ["hello"] and "speaker_id" not in b
        assert b["accent_type"].shape == (1, len(src)) and (b["accent_type"][0] == acc).all()


def test_unknown_accent_ids_and_missing_fields_are_handled_as_in_the_batched_reader(tmp_path):
    hp = hp_accent()
    files, _ = write_corpus(str(tmp_path), n=3, accent=False)
    with pytest.raises(ValueError, match="utt0.*accent_type"):
        next(ljspeech.source_batches([f[0] for f in files], hp, 2))
    (tmp_path / "b").mkdir()
    lo, hi = hp.accent_type_offset, hp.accent_type_offset + hp.num_accent_type

    def outside(i, key, src, acc):
        acc = acc.copy(); acc[0] = hi + 5
        return tfrecord.make_source_example(i, key, src, "hello", acc)
    files, truth = write_corpus(str(tmp_path / "b"), n=3, tamper=outside)
    hp_unk = hp_accent(accent_type_unknown=lo + 1)
    b = next(ljspeech.source_batches([f[0] for f in files], hp_unk, 3))
    assert b["accent_type"][1, 0] == lo + 1 and (b["accent_type"][1, 1:len(truth[1][1])] == truth[1][1][1:]).all()
    same_source_side(b, batches(files, hp_unk)[0])
    with pytest.raises(ValueError, match="utt1"):
        next(ljspeech.source_batches([f[0] for f in files], hp_accent(accent_type_unknown=hi + 1), 3))


def test_speaker_ids_travel_with_the_batch(tmp_path):
    hp = hp_accent(use_accent_type=False, encoder="SelfAttentionCBHGEncoder")
    paths = []
    for i, L in enumerate((4, 7, 5)):
        p = str(tmp_path / ("s%d.source.tfrecord" % i))
        tfrecord.write_records(p, [tfrecord.make_example({"id": i, "key": b"s%d" % i, "source": np.arange(1, L + 1, dtype="<i8").tobytes(),
                                                          "source_length": L, "text": b"t", "speaker_id": 225 + i})])
        paths.append(p)
    b, = ljspeech.source_batches(paths, hp, 4)
    assert b["speaker_id"].tolist() == [225, 226, 227] and b["speaker_id"].dtype == np.int64
    assert b["source"].shape == (3, 7) and b["source"][0].tolist() == [1, 2, 3, 4, 0, 0, 0] and b["source_length"].tolist() == [4, 7, 5]


def test_pad_sources_writes_into_the_arrays_it_is_given():
    """pad_batch hands its allocator on (page-locked ring slots): pad_sources asks it for `source` and `accent_type`, in that order"""
    hp = hp_accent()
    S = ljspeech.decode_source_record
    asked = []

    def new(name, shape, dtype):
        asked.append((name, shape, dtype))
        return np.full(shape, -7, dtype)
    ex = [tfrecord.make_source_example(i, "k%d" % i, np.arange(1, L + 1).astype(np.int64), "x", np.full(L, 0x3100 + i, np.int64))
          for i, L in enumerate((3, 6))]
    b = ljspeech.pad_sources([S(e) for e in ex], hp, new)
    assert asked == [("source", (2, 6), np.int64), ("accent_type", (2, 6), np.int64)]
    assert b["source"].tolist() == [[1, 2, 3, 0, 0, 0], [1, 2, 3, 4, 5, 6]]
    assert b["accent_type"][0].tolist() == [0x3100] * 3 + [hp.accent_type_offset] * 3 and b["accent_type"][1].tolist() == [0x3101] * 6
