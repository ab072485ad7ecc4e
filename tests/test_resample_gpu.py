"""csrc/resample.hip against the float64 yardstick of tests/resample_common.py, its batching guarantees (bit-identical between
batchings and launches, nothing written outside an accepted utterance), its phase and workgroup seams on unit impulses (exact
equality to the float32 table), 64-bit positions, and the Python surface over it."""
import json
import os

import numpy as np
import pytest
import torch

import audio_common as ac
import resample_common as rc
import satt_amd  # noqa: F401
from satt_amd import ops
from satt_amd.datasets.ljspeech import decode_target_record
from satt_amd.hparams import hparams
from satt_amd.utils import audio, tfrecord

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = rc.cases()
POISON = -77.25


def launch(t, signals, counts=None, tail=0):
    """one launch over `signals`; counts: the output count claimed for each (default: the right one); returns (the whole output buffer
    behind the launch - poisoned in front of it, `tail` words longer than the claims - and out_offsets)"""
    lens = np.asarray([len(s) for s in signals], np.int64)
    right = (lens * t.up + t.down - 1) // t.down
    counts = right if counts is None else np.asarray(counts, np.int64)
    io = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    oo = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    x = torch.from_numpy(np.concatenate([np.asarray(s, np.float32) for s in signals])).to(DEV)
    y = torch.full((int(oo[-1]) + tail,), POISON, dtype=torch.float32, device=DEV)
    ops.resample(x, torch.from_numpy(io).to(DEV), torch.from_numpy(oo).to(DEV), t.up, t.down, t.device(DEV), y)
    return y.cpu().numpy(), oo


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0].replace(" ", "_") for c in CASES])
def test_kernel_against_the_yardstick(i):
    name, a, b, x = CASES[i]
    (y,) = audio.resample_hip(audio.resample_tables(a, b), [x], DEV)
    y64 = rc.reference(name, a, b, x)
    assert y.dtype == np.float32 and y.shape == y64.shape
    e = rc.deviation(y, y64)
    print("%s: %.3e of the output maximum (bar %.3e)" % (name, e, rc.C_KERNEL))
    assert e <= rc.C_KERNEL
    # the same operations in the same order as the NumPy backend: the same bits
    assert y.tobytes() == audio.resample_numpy(audio.resample_tables(a, b), x).tobytes()


def test_batching_is_bit_identical_and_writes_nothing_else():
    t = audio.resample_tables(22050, 16000)
    lens = [1, 2, t.half, 777, 4096, 4097, 30000]
    ys = [rc.noise(n, 200 + i) for i, n in enumerate(lens)]
    whole, oo = launch(t, ys, tail=1000)
    again, _ = launch(t, ys, tail=1000)
    assert whole.tobytes() == again.tobytes()
    assert np.all(whole[oo[-1]:] == POISON)                                            # beyond the last utterance
    for u, y in enumerate(ys):
        alone, o1 = launch(t, [y])
        assert o1[-1] == oo[u + 1] - oo[u] == t.length(len(y))
        assert whole[oo[u]:oo[u + 1]].tobytes() == alone.tobytes(), lens[u]
        assert not np.any(alone == POISON)
    # the same utterances with gaps between them: a one-sample "utterance" that claims 5 outputs (its count is 1) is left untouched,
    # and so is whatever follows the last one; the neighbours are written as before
    gapped, counts = [], []
    for y in ys:
        gapped += [y, np.ones(1, np.float32)]
        counts += [t.length(len(y)), 5]
    out, og = launch(t, gapped, counts, tail=7)
    for u, y in enumerate(ys):
        assert out[og[2 * u]:og[2 * u + 1]].tobytes() == whole[oo[u]:oo[u + 1]].tobytes(), lens[u]
        assert np.all(out[og[2 * u + 1]:og[2 * u + 2]] == POISON)
    assert np.all(out[og[-1]:] == POISON)
    # a count off by one in either direction: that utterance is left untouched, the others are written
    for u_bad, off in ((3, 1), (4, -1), (0, 1), (6, -1)):
        counts = [t.length(n) for n in lens]
        counts[u_bad] += off
        out, ob = launch(t, ys, counts)
        for u in range(len(ys)):
            got = out[ob[u]:ob[u + 1]]
            if u == u_bad:
                assert np.all(got == POISON), (u_bad, off)
            else:
                assert got.tobytes() == whole[oo[u]:oo[u + 1]].tobytes(), (u_bad, off, u)


def test_offsets_outside_the_buffers_are_refused_per_utterance():
    t = audio.resample_tables(48000, 16000)
    ys = [rc.noise(900, 1), rc.noise(1500, 2), rc.noise(601, 3)]
    whole, oo = launch(t, ys)
    x = torch.from_numpy(np.concatenate(ys)).to(DEV)                                    # 3001 samples
    # in_offsets past the end of the buffer / negative / an empty utterance in front of one whose length then disagrees with its count
    for io, untouched in (([0, 900, 2400, 3002], {2}), ([-1, 900, 2400, 3001], {0}), ([0, 900, 900, 3001], {1, 2})):
        y = torch.full((int(oo[-1]),), POISON, dtype=torch.float32, device=DEV)
        ops.resample(x, torch.tensor(io, dtype=torch.int64, device=DEV), torch.from_numpy(oo).to(DEV), t.up, t.down, t.device(DEV), y)
        y = y.cpu().numpy()
        for u in range(3):
            if u in untouched:
                assert np.all(y[oo[u]:oo[u + 1]] == POISON), (io, u)
            else:
                assert y[oo[u]:oo[u + 1]].tobytes() == whole[oo[u]:oo[u + 1]].tobytes(), (io, u)
    # out_offsets past the end of the buffer: the last utterance is left untouched
    y = torch.full((int(oo[-1]) - 1,), POISON, dtype=torch.float32, device=DEV)
    ops.resample(x, torch.tensor([0, 900, 2400, 3001], dtype=torch.int64, device=DEV), torch.from_numpy(oo).to(DEV), t.up, t.down,
                 t.device(DEV), y)
    y = y.cpu().numpy()
    assert y[:oo[2]].tobytes() == whole[:oo[2]].tobytes() and np.all(y[oo[2]:] == POISON)
    with pytest.raises(ValueError):                                                     # 2 / 4 is not in lowest terms: nothing is launched
        ops.resample(x, torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV), 2, 4,
                     torch.zeros((2, 8), device=DEV), torch.zeros(4, device=DEV))


def impulse_response(t, n, pos):
    """what a unit impulse at `pos` of n samples gives: y[m] = table[phase][pos - k0 + half - 1], 0 where that column does not exist"""
    m = np.arange(t.length(n), dtype=np.int64) * t.down
    k0 = m // t.up
    jj = pos - k0 + t.half - 1
    inside = (jj >= 0) & (jj < t.taps)
    return np.where(inside, t.table[m - k0 * t.up, np.clip(jj, 0, t.taps - 1)], np.float32(0.0))


@pytest.mark.parametrize("a,b", [(22050, 16000), (16000, 22050), (48000, 16000), (24000, 16000), (8000, 48000)])
def test_unit_impulses_reproduce_table_columns_across_phase_and_workgroup_seams(a, b):
    t = audio.resample_tables(a, b)
    run = ops.resample_run_length()
    n_lo = run * t.down // t.up                     # the longest signal whose outputs one workgroup takes
    assert t.length(n_lo) <= run < t.length(n_lo + 1)
    for n in (n_lo, n_lo + 1, 2 * n_lo + 1):
        places = [0, 1, n - 1, n // 2 + 3]
        out, oo = launch(t, [ac.impulse(n, p) for p in places])
        for u, p in enumerate(places):
            want = impulse_response(t, n, p)
            assert np.count_nonzero(want) > 0
            assert np.array_equal(out[oo[u]:oo[u + 1]], want), (n, p)                  # equality to the fp32 table: no tolerance


def test_positions_beyond_2_to_the_31():
    a, b, n = 22050, 16000, 7000000
    t = audio.resample_tables(a, b)
    x = rc.noise(n, 7)
    (y,) = audio.resample_hip(t, [x], DEV)
    n_out = t.length(n)
    assert len(y) == n_out and (n_out - 1) * t.down > 2 ** 31
    seam = 2 ** 31 // t.down
    for outputs in (range(seam - 32, seam + 32), range(n_out - 64, n_out)):
        y64 = rc.yardstick(x, a, b, outputs)
        e = rc.deviation(y[outputs.start:outputs.stop], y64)
        print("outputs %d .. %d: %.3e of their maximum (bar %.3e)" % (outputs.start, outputs.stop, e, rc.C_KERNEL))
        assert e <= rc.C_KERNEL


def hp_at_16k():
    hp = hparams.copy()
    hp.parse("num_freq=513,sample_rate=16000,frame_length_ms=50.0,frame_shift_ms=12.5,num_mels=80,ref_level_db=20")
    return hp


def test_audio_resample_batch_equals_load_wav(tmp_path, monkeypatch):
    a = audio.Audio(hp_at_16k(), backend="hip", device=DEV, resample=True)
    rates = [22050, 48000, 16000, 22050, 48000, 44100]
    paths = []
    for i, rate in enumerate(rates):
        paths.append(str(tmp_path / ("u%d.wav" % i)))
        ac.write_wav(paths[-1], ac.harmonic(2000 + 731 * i, rate, seed=i), rate)
    each = [a.load_wav(p) for p in paths]
    read = [a.read_wav(p) for p in paths]
    assert [r for r, _ in read] == rates
    whole = a.resample_batch([y for _, y in read], rates)
    assert whole[2] is read[2][1]
    for i, (e, w) in enumerate(zip(each, whole)):
        assert len(w) == -(-len(read[i][1]) * 16000 // rates[i]) and e.tobytes() == w.tobytes(), i
    monkeypatch.setattr(audio, "MAX_LAUNCH_SAMPLES", 3000)                               # several launches per rate
    split = a.resample_batch([y for _, y in read], rates)
    assert all(s.tobytes() == w.tobytes() for s, w in zip(split, whole))
    # and the NumPy backend gives the same bits
    nb = audio.Audio(hp_at_16k(), backend="numpy", resample=True).resample_batch([y for _, y in read], rates)
    assert all(w.tobytes() == v.tobytes() for w, v in zip(whole, nb))


def test_ljspeech_driver_with_resample_on_the_hip_backend(tmp_path):
    in_dir = str(tmp_path / "in")
    os.makedirs(in_dir)
    corpus = ac.write_toy_ljspeech(in_dir)
    outs = {}
    for backend in ("hip", "numpy"):
        outs[backend] = str(tmp_path / backend)
        ac.run_driver("preprocess_ljspeech.py", "--hparam-json-file", ac.LJ_JSON, "--hparams", "sample_rate=16000,num_freq=513",
                      "--backend", backend, "--resample", in_dir, outs[backend])
    assert sorted(os.listdir(outs["hip"])) == sorted(os.listdir(outs["numpy"]))
    for key, _, n in corpus:
        mel = {k: decode_target_record(next(tfrecord.read_records(os.path.join(outs[k], key + ".target.tfrecord"))))["mel"] for k in outs}
        assert mel["hip"].shape == mel["numpy"].shape == (1 + -(-n * 320 // 441) // 200, 80)
        d = float(np.abs(mel["hip"] - mel["numpy"]).max())
        print("%s: %.3e dB between the backends (bar %.3e)" % (key, d, ac.C_DB))
        assert d <= ac.C_DB
    h = {k: json.load(open(os.path.join(outs[k], "hparams.json"))) for k in outs}
    for k in ("average_mel_level_db", "stddev_mel_level_db", "min_mel_level_db"):
        assert np.abs(np.asarray(h["hip"][k]) - np.asarray(h["numpy"][k])).max() <= ac.C_DB, k
