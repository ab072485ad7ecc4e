"""Host side of the mel distance (no GPU): the float32 NumPy DTW against the float64 programme of tests/dtw_common.py, exact cases
and the hand-worked tie-break table, mel_cepstrum against scipy's DCT, the value scalings, the C-ABI declaration of satt_dtw, and
evaluate_mel.py on a toy prediction directory."""
import csv
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.fft

import audio_common as ac
import dtw_common as dc
import satt_amd  # noqa: F401
from satt_amd.hparams import hparams
from satt_amd.utils import audio, tfrecord
from satt_amd.utils import mel_distance as md

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 13), (1, 7, 13), (7, 1, 13), (2, 2, 1), (65, 63, 13), (120, 200, 80), (300, 417, 13)]


# ---- the NumPy backend against the float64 programme -----------------------------------------------------------------------------------
@pytest.mark.parametrize("Ta,Tb,K", SHAPES)
def test_numpy_backend_against_float64(Ta, Tb, K):
    a, b = dc.warped_pair(Ta, Tb, K)
    cost, steps, path = md.dtw_numpy(a, b, want_path=True)
    assert cost.dtype == np.float32 and path.dtype == np.int32
    assert not dc.path_problems(path, Ta, Tb, steps)
    dc.check_against_float64(cost, steps, path, a, b)
    c2, s2 = md.dtw_numpy(a, b)                                                         # without the path: the same cost and steps
    assert c2.tobytes() == cost.tobytes() and s2 == steps


def test_identical_sequences_take_the_diagonal():
    a, _ = dc.warped_pair(37, 37, 13)
    cost, steps, path = md.dtw_numpy(a, a, want_path=True)
    assert cost == 0 and steps == 37 and np.array_equal(path, np.stack([np.arange(37)] * 2, axis=1))


def test_every_frame_repeated_twice_costs_nothing():
    a, _ = dc.warped_pair(29, 29, 5)
    cost, steps, path = md.dtw_numpy(a, np.repeat(a, 2, axis=0), want_path=True)
    assert cost == 0 and steps == 58 and not dc.path_problems(path, 29, 58, 58)
    assert np.array_equal(path[:, 0], path[:, 1] // 2)


def test_hand_worked_examples_pin_the_tie_break_cell_by_cell():
    """D, L and the direction of every cell of the two hand-worked tables, for the NumPy backend and for the float64 yardstick; cell
    (2, 3) of the second example is the one with up == left < diagonal"""
    for e, i, j in dc.HAND_CELLS:
        (a, b), want = dc.hand_prefix(e, i, j)
        cost, steps, path = md.dtw_numpy(a, b, want_path=True)
        assert (cost, steps, dc.last_move(path)) == want, (e, i, j)
        D64, steps64, path64, _ = dc.dp64(a, b)
        assert (D64, steps64, dc.last_move(path64)) == want, (e, i, j)
    for x in dc.HAND_EXAMPLES:
        assert np.array_equal(md.dtw_numpy(x["a"], x["b"], want_path=True)[2], x["path"])
        assert np.array_equal(dc.dp64(x["a"], x["b"])[2], x["path"])


def test_integer_ties_follow_the_definition():
    for Ta, Tb in ((9, 14), (20, 11)):
        a, b = dc.tie_pair(Ta, Tb, 2)
        cost, steps, path = md.dtw_numpy(a, b, want_path=True)
        D64, steps64, path64, _ = dc.dp64(a, b)
        # sums of a few small integer square roots: float32 and float64 need not tie alike, the cost and validity must hold
        assert not dc.path_problems(path, Ta, Tb, steps)
        dc.check_against_float64(cost, steps, path, a, b, (D64, steps64, path64, dc.costs64(a, b)))
    a = np.asarray([[0.0], [3.0], [4.0], [0.0]], np.float32)                              # K = 1, integer costs: exact in both
    b = np.asarray([[0.0], [4.0], [3.0], [0.0], [0.0]], np.float32)
    cost, steps, path = md.dtw_numpy(a, b, want_path=True)
    D64, steps64, path64, _ = dc.dp64(a, b)
    assert cost == D64 and steps == steps64 and np.array_equal(path, path64)


def test_shapes_outside_the_limits_are_refused():
    one = np.zeros((1, 3), np.float32)
    for a, b in ((np.zeros((0, 3), np.float32), one), (one, np.zeros((2049, 3), np.float32)), (np.zeros((2, 129), np.float32),) * 2,
                 (one, np.zeros((1, 4), np.float32)), (np.zeros(3, np.float32), one)):
        with pytest.raises(ValueError):
            md.dtw_numpy(a, b)
    assert md.dtw_numpy(np.zeros((2048, 3), np.float32), one)[1] == 2048


# ---- mel_cepstrum and the value scalings -----------------------------------------------------------------------------------------------
def test_mel_cepstrum_is_the_orthonormal_dct_without_c0():
    S = 20.0 * np.random.default_rng(3).standard_normal((11, 80)) - 30.0
    for order in (1, 13, 79):
        want = scipy.fft.dct(S * np.log(10.0) / 20.0, type=2, norm="ortho", axis=1)[:, 1:order + 1]
        got = md.mel_cepstrum(S, order)
        assert got.dtype == np.float32 and got.shape == (11, order)
        assert np.abs(got - want).max() <= 2.0 ** -23 * np.abs(want).max() + 1e-12       # one float32 rounding of a float64 value
        # a constant level offset leaves it unchanged (c_0 is dropped): to float64 rounding of the offset's own DCT
        assert np.abs(md.mel_cepstrum(S + 17.0, order).astype(np.float64) - got).max() <= 2.0 ** -22 * np.abs(want).max()
    for bad in (0, 80):
        with pytest.raises(ValueError):
            md.mel_cepstrum(S, bad)


def hp_toy(num_mels=4):
    hp = hparams.copy()
    hp.parse("num_freq=513,sample_rate=16000,frame_length_ms=50.0,frame_shift_ms=12.5,num_mels=%d" % num_mels)
    hp.set("average_mel_level_db", [-40.0, -42.0, -44.0, -46.0][:num_mels])
    hp.set("stddev_mel_level_db", [10.0, 12.0, 8.0, 9.0][:num_mels])
    return hp


def test_value_scaling_on_a_two_frame_example_by_hand():
    au = audio.Audio(hp_toy(), backend="numpy")
    # dB rows chosen by hand; the normalised mels are (dB - average) / stddev
    pred_db = np.asarray([[-40.0, -42.0, -44.0, -46.0], [-30.0, -42.0, -44.0, -46.0]])
    ref_db = np.asarray([[-40.0, -42.0, -44.0, -46.0], [-30.0, -42.0, -47.0, -50.0]])
    norm = lambda S: ((S - au.average_mel_level_db) / au.stddev_mel_level_db).astype(np.float32)
    # "mel": frame 0 equal (cost 0), frame 1 differs by (0, 0, 3, 4) dB: distance 5; the diagonal path, 2 steps
    (r,) = au.mel_distance_batch([norm(pred_db)], [norm(ref_db)], feature="mel")
    assert (r["frames_pred"], r["frames_ref"], r["steps"]) == (2, 2, 2)
    assert abs(r["cost"] - 5.0) <= 1e-5 and abs(r["value"] - 5.0 / 2 / np.sqrt(4.0)) <= 1e-5
    # "mcep", order 3 of 4: the DCT is orthonormal, so the distance of the cepstra without c_0 is that of x = dB ln 10 / 20 without
    # its mean: the difference (0, 0, 3, 4) has mean 7 / 4, |d|^2 - 4 mean^2 = 25 - 12.25
    (m,) = au.mel_distance_batch([norm(pred_db)], [norm(ref_db)], feature="mcep", order=3, want_paths=True)
    dist = np.sqrt(25.0 - 12.25) * np.log(10.0) / 20.0
    assert m["steps"] == 2 and np.array_equal(m["path"], [[0, 0], [1, 1]])
    assert abs(m["cost"] - dist) <= 1e-5 and abs(m["value"] - 10.0 * np.sqrt(2.0) / np.log(10.0) * dist / 2) <= 1e-5


def test_mel_distance_batch_refuses_bad_input_by_name():
    au = audio.Audio(hp_toy(), backend="numpy")
    good = np.zeros((3, 4), np.float32)
    nan = good.copy()
    nan[1, 2] = np.nan
    for preds, refs, kw, word in (([good, nan], [good, good], {}, "pair 1"), ([good], [nan], dict(keys=["utt7"]), "utt7"),
                                  ([good[:0]], [good], dict(keys=["empty"]), "empty"),
                                  ([np.zeros((2049, 4), np.float32)], [good], dict(keys=["long"]), "long"),
                                  ([good], [np.zeros((3, 5), np.float32)], dict(keys=["wide"]), "wide")):
        with pytest.raises(ValueError) as e:
            au.mel_distance_batch(preds, refs, order=3, **kw)
        assert word in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        au.mel_distance_batch([good], [good], feature="mgc")
    with pytest.raises(ValueError):
        au.mel_distance_batch([good], [good, good])
    assert au.mel_distance_batch([], []) == []


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_dtw_struct_layout_matches_c(tmp_path):
    from satt_amd import _lib
    names = [n for n, _ in _lib.DtwParams._fields_]
    assert names == ["n_pairs", "K", "max_ta", "max_tb", "total_a", "total_b", "total_dirs", "total_path", "a", "b", "a_offsets",
                     "b_offsets", "cost", "steps", "dirs", "dir_offsets", "path", "path_offsets"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "satt_hip.h"\nint main() {\n  printf("%zu", sizeof(satt_dtw_params));\n'
    src += "".join('  printf(" %%zu", offsetof(satt_dtw_params, %s));\n' % n for n in names) + "  return 0; }\n"
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    vals = list(map(int, subprocess.check_output([str(tmp_path / "t")]).split()))
    P = _lib.DtwParams
    assert vals == [ctypes.sizeof(P)] + [getattr(P, n).offset for n in names]
    header = open(os.path.join(ROOT, "include", "satt_hip.h")).read()
    for sym in ("satt_dtw_supported", "satt_dtw_max_frames", "satt_dtw"):
        assert sym + "(" in header and sym in _lib.SIGNATURES
    assert _lib.SIGNATURES["satt_dtw"][1][-1] is ctypes.c_void_p                        # the stream comes last, as everywhere


def test_dtw_supported_agrees_with_the_python_predicate():
    from satt_amd import ops
    assert ops.dtw_max_frames() == md.DTW_MAX_FRAMES == 2048 and md.DTW_MAX_K == 128
    grid_t, grid_k = (-1, 0, 1, 2, 2047, 2048, 2049, 1 << 20), (-1, 0, 1, 13, 127, 128, 129)
    for Ta in grid_t:
        for Tb in grid_t:
            for K in grid_k:
                assert ops.dtw_supported(Ta, Tb, K) == md.dtw_supported(Ta, Tb, K), (Ta, Tb, K)
    assert ops.dtw_supported(2048, 1, 128) and not ops.dtw_supported(2049, 1, 1) and not ops.dtw_supported(1, 1, 129)


def test_bad_arguments_return_before_any_launch():
    """there is no GPU here: every one of these calls has to come back with its code before the library touches the runtime"""
    from satt_amd import _lib
    lib = _lib.lib()
    BADARG, UNSUPPORTED = -1, -2
    assert b"bad argument" in lib.satt_strerror(BADARG) and b"unsupported" in lib.satt_strerror(UNSUPPORTED)
    keep = [(ctypes.c_int64 * 4)() for _ in range(10)]                                  # host memory: never dereferenced by the entry point
    ptr = [ctypes.addressof(k) for k in keep]

    def params(**kw):
        f = dict(n_pairs=1, K=13, max_ta=3, max_tb=4, total_a=3, total_b=4, total_dirs=12, total_path=6, a=ptr[0], b=ptr[1],
                 a_offsets=ptr[2], b_offsets=ptr[3], cost=ptr[4], steps=ptr[5], dirs=ptr[6], dir_offsets=ptr[7], path=ptr[8],
                 path_offsets=ptr[9])
        f.update(kw)
        return _lib.DtwParams(**f)
    assert lib.satt_dtw(None, None) == BADARG
    for kw in (dict(a=None), dict(b=None), dict(a_offsets=None), dict(b_offsets=None), dict(cost=None), dict(steps=None),
               dict(n_pairs=0), dict(total_a=0), dict(total_b=-1), dict(dirs=None), dict(path=None), dict(dir_offsets=None),
               dict(path_offsets=None), dict(total_dirs=0), dict(total_path=0), dict(max_ta=4), dict(max_tb=5)):
        assert lib.satt_dtw(ctypes.byref(params(**kw)), None) == BADARG, kw
    for kw in (dict(K=0), dict(K=129), dict(max_ta=0), dict(max_tb=0), dict(max_ta=2049, total_a=4000), dict(max_tb=2049, total_b=4000)):
        assert lib.satt_dtw(ctypes.byref(params(**kw)), None) == UNSUPPORTED, kw


WALK_PROGRAM = r"""
#include <stdio.h>
#include <vector>
#include "dtw_walk.h"
int main() {
  const int shapes[][2] = {{1, 1}, {1, 7}, {7, 1}, {3, 5}, {5, 3}, {64, 65}};
  const int fills[] = {0, 1, 2, 0xEE};
  int bad = 0, runs = 0;
  for (auto& sh : shapes) for (int fill : fills) for (int which = 0; which < 3; ++which) {
    const int Ta = sh[0], Tb = sh[1], nd = Ta + Tb - 1, pad = Ta * Tb + Ta + Tb;
    const int n = which == 0 ? 1 : (which == 1 ? nd : nd + 1000);          // too short, the capacity, far too long
    std::vector<uint8_t> dirs(pad + Ta * Tb + pad, (uint8_t)fill);
    std::vector<int32_t> path(2 * (pad + nd + pad), -9);
    int32_t* out = path.data() + 2 * pad;
    const int last = dtw_walk_back(dirs.data() + pad, Ta, Tb, n, out);
    const int cnt = n < nd ? n : nd;
    for (int e = -pad; e < nd + pad; ++e) {
      const int i = out[2 * e], j = out[2 * e + 1];
      if (e < last || e >= cnt) bad += i != -9 || j != -9;                  // nothing outside the entries it reports
      else {
        bad += i < 0 || i >= Ta || j < 0 || j >= Tb;                        // every entry inside the pair
        if (e + 1 < cnt) {
          const int di = out[2 * e + 2] - i, dj = out[2 * e + 3] - j;
          bad += !((di == 1 && dj == 1) || (di == 1 && dj == 0) || (di == 0 && dj == 1));
        }
      }
    }
    bad += out[2 * cnt - 2] != Ta - 1 || out[2 * cnt - 1] != Tb - 1;      // the corner comes first
    if (which > 0) bad += last != 0 && !(out[2 * last] == 0 && out[2 * last + 1] == 0);   // it ends at (0, 0) or at entry 0
    ++runs;
  }
  printf("%d %d\n", runs, bad);
  return 0;
}
"""


def test_walk_back_stays_inside_the_pair_whatever_the_bytes_say(tmp_path):
    """the kernel's walk back (csrc/dtw_walk.h) as a host program on direction bytes no launch would write - all diagonal, all up,
    all left, a byte that is no direction - and on carried lengths that are too short and far too long: every entry lies inside the
    pair, the moves are steps of a path, at most Ta + Tb - 1 entries are written and nothing else is touched"""
    (tmp_path / "walk.cpp").write_text(WALK_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "self-attention-tacotron_amd", "csrc"),
                           str(tmp_path / "walk.cpp"), "-o", str(tmp_path / "walk")])
    runs, bad = map(int, subprocess.check_output([str(tmp_path / "walk")]).split())
    assert runs == 6 * 4 * 3 and bad == 0


# ---- evaluate_mel.py -------------------------------------------------------------------------------------------------------------------
def write_toy_predictions(root, with_truth=(True, True, False, True), nan_key=None):
    """four prediction records of 80-bin normalised mels, the third without ground truth; returns {key: (mel, ground truth or None)}"""
    os.makedirs(root, exist_ok=True)
    rng = np.random.default_rng(5)
    out = {}
    for u, truth in enumerate(with_truth):
        key = "utt%03d" % u
        gt = rng.standard_normal((23 + 5 * u, 80)).astype(np.float32)
        idx = np.sort(rng.integers(0, len(gt), 19 + 7 * u))
        mel = (gt[idx] + 0.1 * rng.standard_normal((len(idx), 80))).astype(np.float32)
        if key == nan_key:
            mel[3, 5] = np.nan
        tfrecord.write_prediction_result(u, key, [np.zeros((4, len(mel)), np.float32)], mel, gt if truth else None, "text %d" % u, np.arange(4), None,
                                         os.path.join(root, key + ".tfrecord"))
        out[key] = (mel, gt if truth else None)
    return out


def write_stats(path, with_stats=True):
    h = dict(num_mels=80, num_freq=513, sample_rate=16000)
    if with_stats:
        h.update(average_mel_level_db=[-40.0 - 0.1 * m for m in range(80)], stddev_mel_level_db=[10.0 + 0.05 * m for m in range(80)])
    with open(path, "w") as f:
        json.dump(h, f)
    return path


def test_evaluate_mel_driver_on_a_toy_directory(tmp_path):
    pred, out = str(tmp_path / "pred"), str(tmp_path / "out")
    records = write_toy_predictions(pred)
    stats = write_stats(str(tmp_path / "hparams.json"))
    r = ac.run_driver("evaluate_mel.py", "--hparam-json-file", stats, "--backend", "numpy", "--write-paths", pred, out)
    assert "utt002: no ground-truth mel, skipped" in r.stdout
    hp = hparams.copy()
    hp.parse_json(open(stats).read())
    au = audio.Audio(hp, backend="numpy")
    keys = [k for k in sorted(records) if records[k][1] is not None]
    want = au.mel_distance_batch([records[k][0] for k in keys], [records[k][1] for k in keys], want_paths=True)
    rows = list(csv.reader(open(os.path.join(out, "mel_distance.csv"))))
    assert rows[0] == ["key", "frames_pred", "frames_ref", "steps", "value"] and [row[0] for row in rows[1:]] == keys
    for row, key, w in zip(rows[1:], keys, want):
        assert [int(x) for x in row[1:4]] == [len(records[key][0]), len(records[key][1]), w["steps"]] and float(row[4]) == w["value"]
        assert w["value"] > 0 and ("%s: %d frames against %d" % (key, w["frames_pred"], w["frames_ref"])) in r.stdout
        path = np.load(os.path.join(out, key + ".dtw.npz"))["path"]
        assert path.shape == (w["steps"], 2) and np.array_equal(path, w["path"])
    s = json.load(open(os.path.join(out, "summary.json")))
    assert s["count"] == 3 and s["feature"] == "mcep" and s["order"] == 13 and s["skipped"] == ["utt002"]
    assert abs(s["mean"] - np.mean([w["value"] for w in want])) <= 1e-12
    assert abs(s["step_weighted_mean"] - md.MCD_SCALE * sum(w["cost"] for w in want) / sum(w["steps"] for w in want)) <= 1e-12
    assert abs(s["mean_length_ratio"] - np.mean([w["frames_pred"] / w["frames_ref"] for w in want])) <= 1e-12
    assert not os.path.exists(os.path.join(out, "utt002.dtw.npz"))
    # --feature mel, the default output directory, no paths
    ac.run_driver("evaluate_mel.py", "--hparam-json-file", stats, "--backend", "numpy", "--feature", "mel", pred)
    s = json.load(open(os.path.join(pred, "summary.json")))
    mel = au.mel_distance_batch([records[k][0] for k in keys], [records[k][1] for k in keys], feature="mel")
    assert s["feature"] == "mel" and s["order"] is None and abs(s["mean"] - np.mean([w["value"] for w in mel])) <= 1e-12
    assert not [f for f in os.listdir(pred) if f.endswith(".dtw.npz")]


def test_evaluate_mel_driver_refusals(tmp_path):
    stats = write_stats(str(tmp_path / "hparams.json"))
    none = str(tmp_path / "none")
    write_toy_predictions(none, with_truth=(False, False))
    r = ac.run_driver("evaluate_mel.py", "--hparam-json-file", stats, "--backend", "numpy", none, check=False)
    assert r.returncode != 0 and "holds a ground-truth mel" in r.stderr and "--target-data-root" in r.stderr
    pred = str(tmp_path / "pred")
    write_toy_predictions(pred)
    bare = write_stats(str(tmp_path / "bare.json"), with_stats=False)
    r = ac.run_driver("evaluate_mel.py", "--hparam-json-file", bare, "--backend", "numpy", pred, check=False)
    assert r.returncode != 0 and "average_mel_level_db" in r.stderr and "the preprocessing run wrote" in r.stderr
    bad = str(tmp_path / "nan")
    write_toy_predictions(bad, nan_key="utt001")
    r = ac.run_driver("evaluate_mel.py", "--hparam-json-file", stats, "--backend", "numpy", bad, check=False)
    assert r.returncode != 0 and "ValueError" in r.stderr and "utt001" in r.stderr and "non-finite" in r.stderr
    r = ac.run_driver("evaluate_mel.py", "--hparam-json-file", stats, "--backend", "numpy", str(tmp_path), check=False)
    assert r.returncode != 0 and "no *.tfrecord" in r.stderr
