"""Text front end and the two preprocessing drivers on toy corpora (no GPU: --backend numpy)."""
import csv
import json
import os

import numpy as np
import pytest

import audio_common as ac
import satt_amd  # noqa: F401
from satt_amd.datasets.ljspeech import decode_source_record, decode_target_record, read_pair
from satt_amd.hparams import hparams
from satt_amd.preprocess.cleaners import basic_cleaners, english_cleaners
from satt_amd.preprocess.text import sequence_to_text, symbols, text_to_sequence
from satt_amd.utils import tfrecord

EIGHT_KEYS = ["num_mels", "num_freq", "sample_rate", "frame_length_ms", "frame_shift_ms", "average_mel_level_db",
              "stddev_mel_level_db", "min_mel_level_db"]


def test_symbol_table():
    """reference preprocess/text.py:21 spells 67 characters (A-Z, a-z, 13 punctuation marks, backquote, space); with the silence id 0
    that makes 68 ids, 0 .. 67"""
    assert len(symbols) == 67 and len(set(symbols)) == 67
    assert "".join(symbols) == "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz!'\"()[],-.:;?` "
    seq, clean = text_to_sequence("A z", lambda t: t)
    assert seq == [0, 1, 67, 52, 0] and clean == "A z"
    every, _ = text_to_sequence("".join(symbols), lambda t: t)
    assert every == [0] + list(range(1, 68)) + [0] and len(set(every)) == 68
    assert sequence_to_text(every) == "".join(symbols)


CLEANED = [
    ("Mr. Smith", "mister smith"), ("1800", "eighteen hundred"), ("2000", "two thousand"), ("2005", "two thousand five"),
    ("1999", "nineteen ninety-nine"), ("21", "twenty-one"), ("3000", "three thousand"), ("10,000", "ten thousand"),
    ("$1", "one dollar"), ("$3.50", "three dollars, fifty cents"), ("£5", "five pounds"), ("1st", "first"),
    ("22nd", "twenty-second"), ("3.14", "three point fourteen"), ("a \t b\n\n c", "a b c"),
    ("MRS. Jones and dr. Who", "misess jones and doctor who"), ("St. John, Ft. Knox Co. Ltd.", "saint john, fort knox company limited"),
    ("$0.01", "one cent"), ("$2", "two dollars"), ("$1.01", "one dollar, one cent"), ("1000", "one thousand"), ("1001", "ten oh one"),
    ("2100", "twenty-one hundred"), ("100", "one hundred"), ("115", "one hundred fifteen"), ("0", "zero"), ("3rd", "third"),
    ("12th", "twelfth"), ("20th", "twentieth"), ("1,234,567", "one million, two hundred thirty-four thousand, five hundred sixty-seven"),
    ("“Café” – naïve…", "\"cafe\" - naive..."), ("It’s", "it's"),
]


@pytest.mark.parametrize("raw,clean", CLEANED)
def test_english_cleaners(raw, clean):
    assert english_cleaners(raw) == clean
    text_to_sequence(raw, english_cleaners)                      # and every cleaned character is in the table


def test_basic_cleaners_and_a_character_outside_the_table():
    assert basic_cleaners("Please  CALL\tStella. 21") == "please call stella. 21"
    with pytest.raises(ValueError) as e:
        text_to_sequence("call 21", basic_cleaners, key="p225_001")          # the basic cleaners leave digits in place
    assert "p225_001" in str(e.value) and "'2'" in str(e.value)
    with pytest.raises(ValueError) as e:
        text_to_sequence("a 中 b", english_cleaners, key="LJ9")
    assert "LJ9" in str(e.value) and ("中" in str(e.value) or "4E2D" in str(e.value))


# ---- the LJSpeech driver ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lj(tmp_path_factory):
    root = tmp_path_factory.mktemp("lj")
    in_dir, out = str(root / "in"), str(root / "out")
    os.makedirs(in_dir)
    corpus = ac.write_toy_ljspeech(in_dir)
    ac.run_driver("preprocess_ljspeech.py", "--hparam-json-file", ac.LJ_JSON, "--backend", "numpy", in_dir, out)
    return in_dir, out, corpus


def test_ljspeech_driver_files(lj):
    _, out, corpus = lj
    keys = [k for k, _, _ in corpus]
    expect = {"list.csv", "hparams.json"} | {"%s.%s.tfrecord" % (k, s) for k in keys for s in ("source", "target")}
    assert set(os.listdir(out)) == expect
    assert [r for r in csv.reader(open(os.path.join(out, "list.csv"), newline=""))] == [[k] for k in keys]
    h = json.load(open(os.path.join(out, "hparams.json")))
    assert list(h) == EIGHT_KEYS
    assert (h["num_mels"], h["num_freq"], h["sample_rate"], h["frame_length_ms"], h["frame_shift_ms"]) == (80, 1025, 22050, 50.0, 12.5)
    assert all(len(h[k]) == 80 for k in EIGHT_KEYS[5:])


def test_ljspeech_driver_records(lj):
    _, out, corpus = lj
    hp = hparams.copy()
    hp.parse_json(open(ac.LJ_JSON).read())
    hp.parse_json(open(os.path.join(out, "hparams.json")).read())
    frames = []
    for i, (key, text, n) in enumerate(corpus):
        sf, tf = os.path.join(out, key + ".source.tfrecord"), os.path.join(out, key + ".target.tfrecord")
        s = decode_source_record(next(tfrecord.read_records(sf)))
        t = decode_target_record(next(tfrecord.read_records(tf)))
        seq, clean = text_to_sequence(text, english_cleaners)
        assert (s.id, s.key, s.text, s.source_length) == (i, key, clean, len(seq)) and s.source.tolist() == seq
        assert s.source[0] == 0 and s.source[-1] == 0 and s.speaker_id == -1
        assert (t["id"], t["key"], t["mel_width"], t["target_length"]) == (i, key, 80, 1 + n // ac.LJ_HOP)
        assert t["mel"].shape == (1 + n // ac.LJ_HOP, 80)
        frames.append(t["mel"])
        s2, m2, raw_len = read_pair(sf, tf, hp)
        assert s2.key == key and raw_len == t["target_length"] and m2.mel.shape[1] == 80
    assert corpus[0][1].startswith("Mr.") and decode_source_record(next(tfrecord.read_records(
        os.path.join(out, corpus[0][0] + ".source.tfrecord")))).text == "mister smith paid three dollars, fifty cents in nineteen ninety-nine."
    # the statistics are float64 over the float32 frames: normalised with them the corpus has mean 0 and deviation 1 per bin
    h = json.load(open(os.path.join(out, "hparams.json")))
    allf = np.concatenate(frames).astype(np.float64)
    z = (allf - np.asarray(h["average_mel_level_db"])) / np.asarray(h["stddev_mel_level_db"])
    assert np.abs(z.mean(axis=0)).max() <= 1e-4 and np.abs(z.std(axis=0) - 1.0).max() <= 1e-4
    assert np.array_equal(np.asarray(h["min_mel_level_db"]), allf.min(axis=0))
    # and the records hold the yardstick's dB values
    y = ac.harmonic(corpus[0][2], ac.LJ_RATE, seed=10)
    y16 = (np.round(y.astype(np.float64) * 32767.0) / 32768.0).astype(np.float32)
    sr, n_fft, win, hop, mels = ac.CONFIGS["ljspeech"]
    db64, _ = ac.yardstick_db(ac.yardstick_mag(y16, n_fft, hop, win), ac.slaney_basis(sr, n_fft, mels))
    assert np.abs(frames[0] - db64).max() <= ac.C_DB / 8


def test_ljspeech_driver_source_only_and_target_only(lj, tmp_path):
    in_dir, out, corpus = lj
    keys = [k for k, _, _ in corpus]
    so, to = str(tmp_path / "so"), str(tmp_path / "to")
    ac.run_driver("preprocess_ljspeech.py", "--hparam-json-file", ac.LJ_JSON, "--backend", "numpy", "--source-only", in_dir, so)
    assert set(os.listdir(so)) == {"list.csv"} | {k + ".source.tfrecord" for k in keys}
    ac.run_driver("preprocess_ljspeech.py", "--hparam-json-file", ac.LJ_JSON, "--backend", "numpy", "--target-only", in_dir, to)
    assert set(os.listdir(to)) == {"list.csv", "hparams.json"} | {k + ".target.tfrecord" for k in keys}
    for k in keys:
        for d, kind in ((so, "source"), (to, "target")):
            name = "%s.%s.tfrecord" % (k, kind)
            assert open(os.path.join(d, name), "rb").read() == open(os.path.join(out, name), "rb").read()
    assert json.load(open(os.path.join(to, "hparams.json"))) == json.load(open(os.path.join(out, "hparams.json")))


def test_ljspeech_driver_refuses_wrong_rate_and_stereo(lj, tmp_path):
    in_dir, _, corpus = lj
    for name, rate, channels, words in (("rate", 16000, 1, ("16000", "22050")), ("stereo", 22050, 2, ("mono",))):
        bad = str(tmp_path / name)
        os.makedirs(os.path.join(bad, "wavs"))
        open(os.path.join(bad, "metadata.csv"), "w").write("X1|hello|hello\n")
        ac.write_wav(os.path.join(bad, "wavs", "X1.wav"), ac.harmonic(3000, rate), rate, channels)
        r = ac.run_driver("preprocess_ljspeech.py", "--hparam-json-file", ac.LJ_JSON, "--backend", "numpy", bad, str(tmp_path / (name + "_out")),
                          check=False)
        assert r.returncode != 0 and "ValueError" in r.stderr and "X1.wav" in r.stderr and all(w in r.stderr for w in words), r.stderr[-800:]


# ---- the VCTK driver -------------------------------------------------------------------------------------------------------------
def test_vctk_driver(tmp_path):
    in_dir, out = str(tmp_path / "in"), str(tmp_path / "out")
    os.makedirs(in_dir)
    corpus = ac.write_toy_vctk(in_dir)
    ac.run_driver("preprocess_vctk.py", "--backend", "numpy", in_dir, out)          # the hparams defaults are VCTK's
    keys = [c[0] for c in corpus]
    assert keys == ["p225_001", "p225_002", "p226_001", "p226_002"]                  # header and speaker 315 left out
    assert set(os.listdir(out)) == {"list.csv", "hparams.json"} | {"%s.%s.tfrecord" % (k, s) for k in keys for s in ("source", "target")}
    assert [r[0] for r in csv.reader(open(os.path.join(out, "list.csv"), newline=""))] == keys
    assert list(json.load(open(os.path.join(out, "hparams.json")))) == EIGHT_KEYS
    widen = int(4 * 12.5 * 48000 / 1000)
    trimmed = (70 * 256 + widen) - (36 * 256 - widen)          # tone at [9600, 17280): trim frames 36 .. 69 (test_melspec_cpu.py)
    for i, (key, spk, age, gender, n) in enumerate(corpus):
        s = decode_source_record(next(tfrecord.read_records(os.path.join(out, key + ".source.tfrecord"))))
        t = decode_target_record(next(tfrecord.read_records(os.path.join(out, key + ".target.tfrecord"))))
        assert (s.id, s.key, s.speaker_id, s.age, s.gender) == (i, key, spk, age, gender)
        assert s.text == ("please call stella." if key.endswith("1") else "ask her to bring these things.")
        assert s.source.tolist() == text_to_sequence(s.text, basic_cleaners)[0]
        assert t["target_length"] == 1 + trimmed // ac.VCTK_HOP < 1 + n // ac.VCTK_HOP and t["mel"].shape == (t["target_length"], 80)
    r = ac.run_driver("preprocess_vctk.py", "--backend", "numpy", "--version", "0.91", in_dir, out, check=False)
    assert r.returncode != 0 and "0.8" in r.stderr
