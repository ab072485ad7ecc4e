"""The float32 NumPy backend of the non-negative mel inversion (utils/audio.py mel_nnls_numpy) against the dense float64 iteration of
tests/mel_nnls_common.py and a scalar float32 restatement of the definition, what it buys (residual, round trip), its exact
properties, the transposed table, edge frames, the C ABI of satt_mel_nnls without a GPU, and the drivers on the numpy backend."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import audio_common as ac
import griffin_lim_common as gc
import mel_nnls_common as mc
import satt_amd  # noqa: F401
from satt_amd.utils import audio

ROOT = ac.ROOT


def solve(name, iters):
    a, x0 = mc.inputs(name)
    return audio.mel_nnls_numpy(audio.mel_nnls_tables(mc.tables(name)), a, x0, iters)


# ---- against float64 -------------------------------------------------------------------------------------------------------------------
def test_the_bar_is_eight_times_a_rounding_sized_figure():
    assert mc.C == 8 * mc.WORST_NUMPY and mc.WORST_NUMPY <= mc.WORST_ALLOWED


@pytest.mark.parametrize("iters", mc.KS)
@pytest.mark.parametrize("name", mc.NAMES)
def test_numpy_backend_against_float64(name, iters):
    err = mc.frame_errors(solve(name, iters), mc.yardstick_of(name, iters))
    print("%s K=%d: worst frame %.3e of the frame maximum (bar %.3e)" % (name, iters, err.max(), mc.C))
    assert err.max() <= mc.WORST_NUMPY * 1.0001, "the recorded worst figure no longer holds"
    assert err.max() <= mc.C


@pytest.mark.parametrize("kind", mc.HAND)
def test_hand_made_tables_against_float64(kind):
    nt, B, a, x0 = mc.hand(kind)
    for iters in mc.KS:
        err = mc.frame_errors(audio.mel_nnls_numpy(nt, a, x0, iters), mc.yardstick(B, a, x0, iters))
        assert err.max() <= mc.C, (kind, iters, err.max())


# ---- the written definition, operation by operation ---------------------------------------------------------------------------------
def test_numpy_backend_equals_the_scalar_definition_bit_for_bit():
    name = "fft512_hop_beyond_window"
    t = mc.tables(name)
    nt = audio.mel_nnls_tables(t)
    assert t.num_mels == 13
    a, x0 = mc.inputs(name)
    got = audio.mel_nnls_numpy(nt, a[:2], x0[:2], 3)
    for n in range(2):
        want = mc.scalar32(t.band_start, t.band_offset, t.band_weight, 257, a[n], x0[n], 3, nt.step, nt.beta(3))
        assert got[n].tobytes() == want.tobytes()
    assert not np.array_equal(got, x0[:2])


def test_hand_made_table_equals_the_scalar_definition_bit_for_bit():
    """an empty band, a band of one bin, a bin under three bands, bands between a bin's first and last that do not hold it"""
    nt, _, a, x0 = mc.hand("odd")
    got = audio.mel_nnls_numpy(nt, a, x0, 5)
    for n in range(3):
        want = mc.scalar32(nt.band_start, nt.band_offset, nt.band_weight, nt.num_bins, a[n], x0[n], 5, nt.step, nt.beta(5))
        assert got[n].tobytes() == want.tobytes()


def test_step_and_beta():
    for name in mc.NAMES:
        nt = audio.mel_nnls_tables(mc.tables(name))
        L = np.linalg.norm(mc.dense_of(name), 2) ** 2
        assert nt.step.dtype == np.float32 and float(nt.step) * nt.lipschitz <= 1.0
        assert abs(float(nt.step) * L - 1.0) <= 3 * 2.0 ** -24                  # 1 / L rounded to float32, at most one step below
        assert audio.mel_nnls_tables(mc.tables(name)) is nt                      # cached on the tables
    beta = nt.beta(64)
    t = [1.0]
    for _ in range(64):
        t.append((1.0 + np.sqrt(1.0 + 4.0 * t[-1] ** 2)) / 2.0)
    assert beta.dtype == np.float32 and beta[0] == 0.0 and np.all(np.diff(beta) > 0) and beta[-1] < 1.0
    assert beta.tobytes() == np.asarray([(t[k] - 1.0) / t[k + 1] for k in range(64)]).astype(np.float32).tobytes()
    assert nt.beta(3).tobytes() == beta[:3].tobytes() and nt.beta(128)[:64].tobytes() == beta.tobytes()


# ---- what it buys ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.NAMES)
def test_residual(name):
    a, x0 = mc.inputs(name)
    B = mc.dense_of(name)
    before, after = mc.residuals(B, x0, a), mc.residuals(B, solve(name, 64), a)
    print("%s: worst frame %.4f with the floored pseudo-inverse, %.3e behind 64 iterations" % (name, before.max(), after.max()))
    assert before.max() >= mc.DEFECT_BOUND                                       # the inputs do contain the defect
    assert after.max() <= mc.RESIDUAL_BOUND


def test_end_to_end_round_trip():
    au = gc.lj_audio("numpy")
    pinv, nnls = mc.round_trip(au, 3, inversion="pinv"), mc.round_trip(au, 3, inversion="nnls")
    print("mean |dB| difference behind 30 Griffin-Lim iterations: %.3f with pinv, %.3f with nnls" % (pinv, nnls))
    assert nnls < 0.8 * pinv
    assert mc.round_trip(au, 3) == pinv                                          # the default is the pseudo-inverse


# ---- exact properties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.NAMES)
def test_non_negative_and_uncovered_bins(name):
    nt = audio.mel_nnls_tables(mc.tables(name))
    a, x0 = mc.inputs(name)
    count = np.diff(nt.bin_offset)
    F = nt.num_bins
    # bins 0 and F - 1 lie under no band - but for vctk, whose float64 basis holds a rounding residue of 2.5e-18 in its last band at
    # bin F - 1: that bin is covered, as it is in the operator csrc/melspec.hip applies
    uncovered = [0] if name == "vctk" else [0, F - 1]
    assert list(np.nonzero(count == 0)[0]) == uncovered
    assert list(np.nonzero(~mc.tables(name).basis.astype(np.float32).any(axis=0))[0]) == uncovered
    for iters in (1, 2, 64):
        x = solve(name, iters)
        assert x.dtype == np.float32 and x.shape == x0.shape and np.all(x >= 0) and np.isfinite(x).all()
        assert x[:, uncovered].tobytes() == x0[:, uncovered].tobytes()
        assert not np.array_equal(x[:, 1:F - 1], x0[:, 1:F - 1])


def test_a_frame_does_not_depend_on_its_batch():
    name = "fft1024"
    nt = audio.mel_nnls_tables(mc.tables(name))
    a, x0 = mc.inputs(name)
    whole = solve(name, 5)
    reps = -(-(2 * audio.MEL_NNLS_NUMPY_BLOCK + 3) // len(a))
    tiled = audio.mel_nnls_numpy(nt, np.tile(a, (reps, 1)), np.tile(x0, (reps, 1)), 5)   # several blocks of the backend
    assert tiled.tobytes() == np.tile(whole, (reps, 1)).tobytes()
    for n in (0, len(a) - 1):
        assert audio.mel_nnls_numpy(nt, a[n:n + 1], x0[n:n + 1], 5).tobytes() == whole[n:n + 1].tobytes()


def today(t, S, ref, power=1.0):
    """mel_to_linear as it was before the switch"""
    amp = 10.0 ** ((np.asarray(S, np.float64) + ref) / 20.0)
    return np.maximum(1e-10, amp @ np.linalg.pinv(t.basis).T) ** power


@pytest.mark.parametrize("name", ["fft1024", "ljspeech"])
def test_mel_to_linear(name):
    t = audio.MelspecTables(*ac.CONFIGS[name])
    S = np.concatenate(mc.mels(name))
    for power in (1.0, 1.5):
        want = today(t, S, 20.0, power)
        assert audio.mel_to_linear(t, S, 20.0, power).tobytes() == want.tobytes()
        assert audio.mel_to_linear(t, S, 20.0, power, inversion="pinv", nnls_iters=64).tobytes() == want.tobytes()
        assert audio.mel_to_linear(t, S, 20.0, power, inversion="nnls", nnls_iters=0).tobytes() == want.tobytes()
    a, x0 = mc.inputs(name)
    x = audio.mel_nnls_numpy(audio.mel_nnls_tables(t), a, x0, 7)
    got = audio.mel_to_linear(t, S, 20.0, 1.5, inversion="nnls", nnls_iters=7)
    assert got.dtype == np.float64 and got.tobytes() == (np.maximum(1e-10, x.astype(np.float64)) ** 1.5).tobytes()
    assert audio.mel_to_linear(t, S, 20.0, inversion="nnls").tobytes() == np.maximum(1e-10, solve(name, 64).astype(np.float64)).tobytes()
    # a list of spectrograms is solved together and cut apart again
    parts = audio.mel_to_linear_batch(t, mc.mels(name), 20.0, 1.5, inversion="nnls", nnls_iters=7)
    assert [len(p) for p in parts] == [len(S_) for S_ in mc.mels(name)] and np.concatenate(parts).tobytes() == got.tobytes()
    for kw in (dict(inversion="lbfgs"), dict(inversion="nnls", nnls_iters=-1), dict(inversion="nnls", backend="triton")):
        with pytest.raises(ValueError):
            audio.mel_to_linear(t, S, 20.0, **kw)
    with pytest.raises(ValueError):
        audio.mel_to_linear(t, S, 20.0, inversion="nnls", nnls_iters=1025)


def test_inv_melspectrogram_default_is_unchanged():
    au = gc.lj_audio("numpy")
    S = au.melspectrogram(ac.harmonic(3308, 22050, seed=3))
    plain = au.inv_melspectrogram(S, iters=3)
    assert au.inv_melspectrogram(S, iters=3, inversion="pinv").tobytes() == plain.tobytes()
    assert au.inv_melspectrogram(S, iters=3, inversion="nnls", nnls_iters=0).tobytes() == plain.tobytes()
    # the bytes of the chain as it was: the floored pseudo-inverse, rounded to float32, into Griffin-Lim from the seeded phase
    mag = today(au.tables, S.T, 20.0).astype(np.float32)
    ang = np.exp(2j * np.pi * np.random.default_rng(0).random(mag.shape)).astype(np.complex64)
    assert audio.griffin_lim_numpy(au.tables, mag, ang, 3, 0.99).tobytes() == plain.tobytes()
    other = au.inv_melspectrogram(S, iters=3, inversion="nnls")
    assert other.shape == plain.shape and np.isfinite(other).all() and other.tobytes() != plain.tobytes()
    batch = au.inv_melspectrogram_batch([S.T, S.T[:9]], iters=3, inversion="nnls")
    assert batch[0].tobytes() == other.tobytes() and batch[1].shape == (8 * 275,)


# ---- the transposed table --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.NAMES)
def test_transposed_table(name):
    t = mc.tables(name)
    nt = audio.mel_nnls_tables(t)
    F, M = t.n_fft // 2 + 1, t.num_mels
    basis32 = t.basis.astype(np.float32)
    assert nt.bin_first.dtype == nt.bin_offset.dtype == np.int32 and nt.bin_weight.dtype == np.float32
    assert nt.bin_first.shape == (F,) and nt.bin_offset.shape == (F + 1,) and nt.bin_offset[0] == 0 and nt.bin_offset[-1] == len(nt.bin_weight)
    count = np.diff(nt.bin_offset)
    assert count.min() >= 0 and count.max() == 2 and np.all(nt.bin_first >= 0) and np.all(nt.bin_first + count <= M)
    Bt = np.zeros((F, M), np.float32)
    for f in range(F):
        for c in range(count[f]):
            Bt[f, nt.bin_first[f] + c] = nt.bin_weight[nt.bin_offset[f] + c]
    assert np.array_equal(Bt, basis32.T)                                         # entry for entry (the basis holds a -0 at bin 0)
    assert len(nt.bin_weight) == np.count_nonzero(basis32)


def test_transposed_table_of_hand_made_bases():
    nt, B, _, _ = mc.hand("odd")
    assert np.array_equal(nt.dense_transposed(), B.T) and np.array_equal(nt.dense(), B)
    assert list(np.diff(nt.bin_offset)) == [0, 1, 1, 4, 3, 1, 5, 1, 0]           # bin 3: bands 0 .. 3, bin 4: 2 .. 4, bin 6: 0 .. 4
    assert list(nt.bin_first) == [0, 0, 0, 0, 2, 4, 0, 3, 0]
    assert list(nt.bin_weight[nt.bin_offset[6]:nt.bin_offset[7]]) == [np.float32(0.3), 0, 0, 0, np.float32(0.2)]
    for kind in ("wide", "dense"):
        nt, B, _, _ = mc.hand(kind)
        assert np.array_equal(nt.dense_transposed(), B.T)
    assert np.diff(mc.hand("wide")[0].bin_offset).max() >= 4 and np.diff(mc.hand("dense")[0].bin_offset).min() == 16
    # no positive weight at all, and tables that do not lie inside the bins
    with pytest.raises(ValueError):
        audio.MelNnlsTables(*audio.banded(np.zeros((3, 8))), 8)
    start, offset, weight = audio.banded(mc.hand_basis("odd"))
    with pytest.raises(ValueError):
        audio.MelNnlsTables(start, offset, weight, 7)                            # band 3 ends at bin 7
    with pytest.raises(ValueError):
        audio.MelNnlsTables(start, offset, weight[:-1], 9)


# ---- edge frames -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level_db", [-300.0, -100.0])
def test_silent_frames_come_out_finite(level_db):
    for name in ("ljspeech", "fft512_hop_beyond_window"):
        a, x0 = mc.level_frames(name, level_db)
        x = audio.mel_nnls_numpy(audio.mel_nnls_tables(mc.tables(name)), a, x0, 64)
        assert np.isfinite(x).all() and np.all(x >= 0)
        S = np.full((3, mc.tables(name).num_mels), level_db)
        lin = audio.mel_to_linear(mc.tables(name), S, 20.0, inversion="nnls")
        assert np.isfinite(lin).all() and np.all(lin >= 1e-10)


def test_a_nan_and_an_inf_amplitude_stay_in_their_frame():
    for name in ("ljspeech", "fft512_hop_beyond_window"):
        nt = audio.mel_nnls_tables(mc.tables(name))
        bad, good, x0 = mc.nonfinite_frames(name)
        for iters in (1, 2, 64):
            want = audio.mel_nnls_numpy(nt, good, x0, iters)
            got = audio.mel_nnls_numpy(nt, bad, x0, iters)
            assert got[[0, 2]].tobytes() == want[[0, 2]].tobytes()
            assert not np.isnan(got).any() and np.all(got >= 0)               # the select turns a NaN into 0
            assert got[1].tobytes() != want[1].tobytes()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
FIELDS = ["num_bins", "num_mels", "iters", "n_weights", "n_tweights", "step", "n_frames", "amp", "start", "beta", "band_start", "band_offset",
          "band_weight", "bin_first", "bin_offset", "bin_weight", "out"]


def test_struct_layout_matches_c(tmp_path):
    from satt_amd import _lib
    assert [n for n, _ in _lib.MelNnlsParams._fields_] == FIELDS
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "satt_hip.h"\nint main() {\n  printf("%zu", sizeof(satt_mel_nnls_params));\n'
    src += "".join('  printf(" %%zu", offsetof(satt_mel_nnls_params, %s));\n' % n for n in FIELDS) + "  return 0; }\n"
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    vals = list(map(int, subprocess.check_output([str(tmp_path / "t")]).split()))
    P = _lib.MelNnlsParams
    assert vals == [ctypes.sizeof(P)] + [getattr(P, n).offset for n in FIELDS]
    header = open(os.path.join(ROOT, "include", "satt_hip.h")).read()
    for sym in ("satt_mel_nnls_supported", "satt_mel_nnls"):
        assert sym + "(" in header and sym in _lib.SIGNATURES
    assert _lib.SIGNATURES["satt_mel_nnls"][1][-1] is ctypes.c_void_p


def test_supported_set():
    from satt_amd import ops
    assert (audio.MEL_NNLS_MAX_BINS, audio.MEL_NNLS_MAX_MELS, audio.MEL_NNLS_MAX_ITERS) == (2049, 128, 1024)
    for bins, mels, iters, want in ((2049, 128, 1024, True), (2050, 128, 1024, False), (2049, 129, 64, False), (2049, 128, 0, False),
                                    (2049, 128, 1, True), (2049, 128, 1025, False), (1, 1, 1, True), (0, 80, 64, False), (1025, 0, 64, False),
                                    (1025, 80, -1, False), (257, 13, 64, True)):
        assert ops.mel_nnls_supported(bins, mels, iters) == want, (bins, mels, iters)


def test_bad_arguments_return_before_any_launch():
    """there is no GPU here: every one of these calls has to come back with its code before the library touches the runtime"""
    from satt_amd import _lib
    lib = _lib.lib()
    BADARG, UNSUPPORTED = -1, -2
    assert b"bad argument" in lib.satt_strerror(BADARG) and b"unsupported" in lib.satt_strerror(UNSUPPORTED)
    keep = [(ctypes.c_int64 * 4)() for _ in range(10)]                                  # host memory: never dereferenced by the entry point
    ptr = [ctypes.addressof(k) for k in keep]
    pointers = FIELDS[7:]

    def params(**kw):
        f = dict(num_bins=1025, num_mels=80, iters=64, n_weights=2000, n_tweights=2000, step=1e-3, n_frames=5, **dict(zip(pointers, ptr)))
        f.update(kw)
        return _lib.MelNnlsParams(**f)
    assert lib.satt_mel_nnls(None, None) == BADARG
    for kw in [{p: None} for p in pointers] + [dict(n_weights=0), dict(n_tweights=0), dict(step=0.0), dict(step=-1.0), dict(step=float("nan")),
                                               dict(step=float("inf"))]:
        assert lib.satt_mel_nnls(ctypes.byref(params(**kw)), None) == BADARG, kw
    for kw in (dict(num_bins=2050), dict(num_bins=0), dict(num_mels=129), dict(num_mels=0), dict(iters=0), dict(iters=1025), dict(n_frames=0),
               dict(n_frames=-3), dict(n_frames=1 << 31)):
        assert lib.satt_mel_nnls(ctypes.byref(params(**kw)), None) == UNSUPPORTED, kw


def test_python_refusals():
    nt = audio.mel_nnls_tables(mc.tables("fft1024"))
    a, x0 = mc.inputs("fft1024")
    for args in ((a, x0, 0), (a, x0, 1025), (a[:3], x0, 4), (a[:, :-1], x0, 4), (a, x0[:, :-1], 4), (a[:0], x0[:0], 4), (a[0], x0[0], 4)):
        with pytest.raises(ValueError):
            audio.mel_nnls_numpy(nt, *args)


# ---- the drivers -----------------------------------------------------------------------------------------------------------------------
def test_mel_to_wav_driver_with_the_non_negative_inversion(tmp_path):
    cfg, mel_dir, mels = gc.write_mel_dir(tmp_path)
    out = {}
    for inv in ("pinv", "nnls"):
        out[inv] = str(tmp_path / inv)
        ac.run_driver("mel_to_wav.py", "--hparam-json-file", cfg, "--backend", "numpy", "--iters", "4", "--inversion", inv, mel_dir, out[inv])
    plain = str(tmp_path / "plain")
    ac.run_driver("mel_to_wav.py", "--hparam-json-file", cfg, "--backend", "numpy", "--iters", "4", mel_dir, plain)
    wavs = {k: gc.check_wav_dir(d) for k, d in list(out.items()) + [("plain", plain)]}
    for i in range(3):
        assert wavs["plain"][i].tobytes() == wavs["pinv"][i].tobytes()           # without the switch: the same files
        assert open(os.path.join(plain, "utt%d.wav" % i), "rb").read() == open(os.path.join(out["pinv"], "utt%d.wav" % i), "rb").read()
        assert wavs["nnls"][i].tobytes() != wavs["pinv"][i].tobytes()
    # the driver's nnls wavs are Audio's
    au = gc.lj_audio("numpy")
    want = au.inv_melspectrogram_batch([au.denormalize_mel(((S + 30.0) / 12.0).astype("<f4")) for S in mels], iters=4, inversion="nnls")
    for i, w in enumerate(want):
        top = float(np.abs(w.astype(np.float64)).max())
        assert np.array_equal(wavs["nnls"][i], np.round(w.astype(np.float64) * (0.95 * 32767.0 / top)).astype(np.int16))
    r = ac.run_driver("mel_to_wav.py", "--hparam-json-file", cfg, "--backend", "numpy", "--inversion", "nnls", "--nnls-iters", "1025", mel_dir,
                      str(tmp_path / "x"), check=False)
    assert r.returncode != 0 and "--nnls-iters" in r.stderr


def test_evaluate_f0_driver_with_the_non_negative_inversion(tmp_path):
    import test_yin_cpu as tc
    pred, out, out_plain = str(tmp_path / "pred"), str(tmp_path / "out"), str(tmp_path / "plain")
    records = tc.write_toy_records(pred)
    stats = tc.write_stats(str(tmp_path / "hparams.json"))
    common = ["evaluate_f0.py", "--hparam-json-file", stats, "--backend", "numpy", "--iters", "4", "--seed", "3"]
    ac.run_driver(*common, "--inversion", "nnls", "--nnls-iters", "16", pred, out)
    ac.run_driver(*common, pred, out_plain)
    keys = [k for k in sorted(records) if records[k][1] is not None]
    au = audio.Audio(tc.toy_hparams(), backend="numpy")
    mp, mr = [records[k][0] for k in keys], [records[k][1] for k in keys]
    wavs = au.inv_melspectrogram_batch([au.denormalize_mel(S.astype(np.float64)) for S in mp + mr], iters=4, seed=3, inversion="nnls",
                                       nnls_iters=16)                                # the same inversion on both sides
    want, _, _ = tc.expected(au, keys, wavs[:3], wavs[3:], mp, mr)
    assert tc.read_csv(os.path.join(out, "f0_distance.csv")) == want
    s = json.load(open(os.path.join(out, "summary.json")))
    tc.check_summary(s, want, "griffin_lim", ["utt002"])
    assert (s["inversion"], s["nnls_iters"], s["iters"], s["seed"]) == ("nnls", 16, 4, 3)
    plain = json.load(open(os.path.join(out_plain, "summary.json")))
    assert "inversion" not in plain and "nnls_iters" not in plain                  # a summary without `inversion` is a pinv run
    assert [k for k in s if k not in ("inversion", "nnls_iters")] == list(plain)
    assert tc.read_csv(os.path.join(out_plain, "f0_distance.csv")) != want
    r = ac.run_driver(*common, "--inversion", "nnls", "--pred-wav-dir", pred, "--ref-wav-dir", pred, pred, check=False)
    assert r.returncode != 0 and "--inversion" in r.stderr
