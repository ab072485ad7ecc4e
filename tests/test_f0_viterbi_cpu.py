"""The float32 NumPy backend of the Viterbi pitch tracker (utils/pitch.py): the candidates against a scalar float32 programme of the
rule, the path against a float64 enumeration of all paths and a hand-written tie table, the trap signal of
tests/f0_viterbi_common.py (plain YIN fails it, the Viterbi path does not, and not without its transition term), the edge cases,
the C ABI of satt_yin_candidates / satt_f0_viterbi without a GPU, and evaluate_f0.py --tracker viterbi in both of its modes."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import audio_common as ac
import f0_viterbi_common as fc
import satt_amd  # noqa: F401
from satt_amd.utils import audio, pitch

ROOT = ac.ROOT
K = fc.K
TINY = dict(sr=400, hop=20, fmin=10.0, fmax=100.0, window_ms=40.0)        # W = 16, lags 4 .. 40: room for more than 8 dips


def test_defaults():
    assert (pitch.F0_CANDIDATES, pitch.F0_VITERBI_MAX_FRAMES, pitch.TRACKERS) == (8, 2048, ("yin", "viterbi"))
    assert (pitch.JUMP_COST, pitch.SWITCH_COST, pitch.LAG_BIAS) == (0.3, 0.1, 0.1)
    assert pitch.yin_sizes(**{k: v for k, v in TINY.items() if k != "hop"}) == (16, 4, 40)


# ---- candidates --------------------------------------------------------------------------------------------------------------------------
def tiny_signals():
    rng = np.random.default_rng(5)
    k = np.arange(400)
    return dict(noise=rng.standard_normal(400).astype(np.float32),                       # more than 8 dips a frame
                periodic=np.float32([0.0, 1.0, 0.5, -0.25, -1.0, 0.75, 0.25])[k % 7],    # period 7 exactly: d' = 0 at 7, 14, .. 35
                silence=np.zeros(90, np.float32), one=np.float32([0.5]),
                tone=(np.sin(2 * np.pi * k / 13.3) + 0.4 * np.sin(4 * np.pi * k / 13.3 + 1)).astype(np.float32))


def test_candidates_equal_the_scalar_rule_bit_for_bit():
    _, tau_min, tau_max = pitch.yin_sizes(**{k: v for k, v in TINY.items() if k != "hop"})
    counts = {}
    for name, y in tiny_signals().items():
        dp, power = pitch.yin_dprime_numpy(y, **TINY)
        per, val, pw = pitch.yin_candidates_numpy(y, **TINY)
        want_per, want_val = fc.candidates32(dp, tau_min, tau_max)
        assert per.dtype == val.dtype == np.float32 and per.shape == val.shape == (1 + len(y) // TINY["hop"], K)
        assert per.tobytes() == want_per.tobytes() and val.tobytes() == want_val.tobytes(), name
        assert pw.tobytes() == power.tobytes() == pitch.yin_numpy(y, **TINY)[2].tobytes()
        used = per > 0
        assert np.array_equal(used, np.isfinite(val)) and np.all(val[~used] == np.inf) and np.all(per[~used] == 0)
        assert np.all(np.diff(used.astype(int), axis=1) <= 0)                           # the used slots come first
        assert np.all((np.diff(per, axis=1) > 0) | ~used[:, 1:])                        # in ascending lag order
        dips = ((dp[:, tau_min:tau_max] < dp[:, tau_min - 1:tau_max - 1]) & (dp[:, tau_min:tau_max] <= dp[:, tau_min + 1:tau_max + 1])).sum(axis=1)
        assert np.array_equal(used.sum(axis=1), np.minimum(dips, K))
        counts[name] = dips
    assert counts["noise"].max() > K and (counts["noise"] > K).sum() >= 5               # the truncation was exercised
    assert np.all(counts["silence"] == 0) and counts["one"].shape == (1,)
    # the exactly periodic signal: equal values (d' = 0) at the multiples of the period, all kept, the smaller lags first
    per, val, _ = pitch.yin_candidates_numpy(tiny_signals()["periodic"], **TINY)
    t = 10
    assert list(np.rint(per[t][val[t] == 0])) == [7.0, 14.0, 21.0, 28.0, 35.0]


def test_truncation_keeps_the_smallest_values_and_ties_go_to_the_smaller_lag():
    """a hand-written d' with 10 dips, two pairs of equal values"""
    tau_min, tau_max = 2, 40
    dp = np.ones((1, tau_max + 1), np.float32)
    dips = {3: 0.5, 6: 0.25, 9: 0.75, 12: 0.25, 15: 0.125, 18: 0.875, 21: 0.75, 24: 0.0625, 27: 0.375, 30: 0.625}
    for k, v in dips.items():
        dp[0, k] = v
    per, val = pitch.yin_candidates_pick_numpy(dp, tau_min, tau_max)
    # ranked by (value, lag): 24, 15, 6, 12, 27, 3, 30, 9 | 21 (0.75, the larger lag of the tie) and 18 fall out
    assert list(per[0]) == [3.0, 6.0, 9.0, 12.0, 15.0, 24.0, 27.0, 30.0]
    assert list(val[0]) == [0.5, 0.25, 0.75, 0.25, 0.125, 0.0625, 0.375, 0.625]
    w_per, w_val = fc.candidates32(dp, tau_min, tau_max)
    assert per.tobytes() == w_per.tobytes() and val.tobytes() == w_val.tobytes()
    # a plateau: d'(k) < d'(k - 1) and d'(k) <= d'(k + 1) holds at its first lag only; a NaN neighbour makes no dip
    dp = np.ones((1, tau_max + 1), np.float32)
    dp[0, 10:13] = 0.5
    dp[0, 20], dp[0, 21] = 0.25, np.nan
    dp[0, 30], dp[0, 31] = np.nan, 0.25
    per, val = pitch.yin_candidates_pick_numpy(dp, tau_min, tau_max)
    assert list(per[0, :2]) == [10.5, 0.0] and list(val[0, :2]) == [0.5, np.inf]          # (a = 1, b = c = 1/2: the parabola's 1/2)


# ---- the path ----------------------------------------------------------------------------------------------------------------------------
def test_viterbi_against_the_enumeration_of_all_paths():
    rng = np.random.default_rng(11)
    unique = 0
    for draw in range(200):
        T = int(rng.integers(1, 6))
        per, val, gate = fc.exact_table(rng, T)
        jump, switch, unvoiced, bias = fc.exact_costs(rng)
        f0, state, cost = pitch.f0_viterbi_numpy(per, val, gate, 16000, 128, jump, switch, unvoiced, bias)
        paths = fc.enumerate_paths(per, val, gate, 128, jump, switch, unvoiced, bias)
        assert state.dtype == np.uint8 and f0.dtype == np.float32 and isinstance(cost, np.float32)
        assert float(cost) == paths[0][0], (draw, cost, paths[:2])                      # exact: every sum is on a grid of 1/256
        if len(paths) == 1 or paths[1][0] > paths[0][0]:
            unique += 1
            assert tuple(int(s) for s in state) == paths[0][1], draw
        for t, s in enumerate(state):
            assert f0[t] == (np.float32(16000) / per[t, s] if s < K else 0)
    assert unique >= 100, unique                                                        # a condition on the inputs


def test_tie_rule_on_a_hand_written_table():
    per, val = np.zeros((3, K), np.float32), np.full((3, K), np.inf, np.float32)
    per[:, 0], per[:, 1] = 64.0, 128.0
    val[0, :2], val[1, :2], val[2, :2] = (0.25, 0.25), (0.5, 0.25), (0.125, 0.125)
    gate = np.ones(3, bool)
    # no jump cost: delta_1 = (0.75, 0.5), both from the tie delta_0(0) = delta_0(1) -> predecessor 0; delta_2 = (0.625, 0.625), both
    # from state 1; the end is the smaller index of the tie
    f0, state, cost = pitch.f0_viterbi_numpy(per, val, gate, 16000, 128, 0.0, 8.0, 8.0, 0.0)
    assert list(state) == [0, 1, 0] and cost == 0.625 and list(f0) == [250.0, 125.0, 250.0]
    # one slot of value 1/4 a frame, unvoiced at 1/4 as well, free switches: all 8 paths cost 3/4, the tie keeps the smaller state
    per, val = np.zeros((3, K), np.float32), np.full((3, K), np.inf, np.float32)
    per[:, 0], val[:, 0] = 64.0, 0.25
    f0, state, cost = pitch.f0_viterbi_numpy(per, val, gate, 16000, 128, 0.0, 0.0, 0.25, 0.0)
    assert list(state) == [0, 0, 0] and cost == 0.75
    # ... and the unvoiced state once it is cheaper by the smallest step
    f0, state, cost = pitch.f0_viterbi_numpy(per, val, gate, 16000, 128, 0.0, 0.0, 0.25 - 2.0 ** -20, 0.0)
    assert list(state) == [8, 8, 8] and np.all(f0 == 0)


# ---- the trap signal ---------------------------------------------------------------------------------------------------------------------
_TRAP = {}


def trap_tracks(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _TRAP:
        _TRAP[key] = pitch.track_f0([fc.trap()[0]], fc.SR, fc.HOP, with_state=kw.get("tracker") == "viterbi", **kw)[0]
    return _TRAP[key]


def test_plain_yin_falls_into_the_trap():
    _, truth, judged, _ = fc.trap()
    assert judged.sum() == 61
    g = fc.gpe(trap_tracks()[0], truth, judged)
    print("plain YIN: GPE %.4f" % g)
    assert g > 0.2
    octave = np.abs(trap_tracks()[0][judged] / truth[judged] - 2.0) < 0.2
    assert octave.sum() / 61.0 == g                                                     # every gross error is the octave above


def test_viterbi_at_the_defaults_does_not():
    _, truth, judged, voiced_truth = fc.trap()
    f0, ap, power, voiced, state = trap_tracks(tracker="viterbi")
    g = fc.gpe(f0, truth, judged)
    wrong = np.nonzero(voiced != voiced_truth)[0]
    print("viterbi: GPE %.4f, voicing differs at frames %s" % (g, list(wrong)))
    assert g == 0.0
    assert np.all(fc.edge_distance(wrong) <= 2), wrong
    assert np.array_equal(voiced, state != K) and np.array_equal(f0 > 0, voiced)
    per, val, pw = pitch.yin_candidates_numpy(fc.trap()[0], fc.SR, fc.HOP)
    assert ap.tobytes() == np.where(voiced, val[np.arange(len(val)), np.minimum(state, K - 1)], val.min(axis=1)).tobytes()
    assert pw.tobytes() == power.tobytes() == trap_tracks()[2].tobytes()


def test_the_transition_term_is_live():
    _, truth, judged, _ = fc.trap()
    g = fc.gpe(trap_tracks(tracker="viterbi", jump_cost=0.0, switch_cost=0.0)[0], truth, judged)
    print("viterbi without transition costs: GPE %.4f" % g)
    assert g > 0.2


# ---- edge cases --------------------------------------------------------------------------------------------------------------------------
def test_silence_a_constant_and_gated_frames_are_unvoiced():
    for y in (np.zeros(1000, np.float32), np.full(1000, 0.37, np.float32)):
        f0, ap, power, voiced, state = pitch.track_f0([y], 16000, 200, tracker="viterbi", with_state=True)[0]
        assert len(f0) == 6 and np.all(f0 == 0) and not voiced.any() and np.all(state == K)
    f0, ap, _, _ = pitch.track_f0([np.zeros(1000, np.float32)], 16000, 200, tracker="viterbi")[0]
    assert np.all(ap == np.inf)                                                         # no candidate anywhere
    per, val, _ = fc.grid_table(3, 50)
    f0, state, cost = pitch.f0_viterbi_numpy(per, val, np.zeros(50, bool), 16000, 267)
    chain = np.float32(0)
    for _ in range(50):
        chain = np.float32(chain + np.float32(0.15))
    assert np.all(state == K) and np.all(f0 == 0) and cost == chain
    nan = np.full(1000, np.nan, np.float32)
    per, val, _ = pitch.yin_candidates_numpy(nan, 16000, 200)
    assert np.all(per == 0) and np.all(val == np.inf)                                   # a frame of NaN samples has no dip
    assert not pitch.track_f0([nan], 16000, 200, tracker="viterbi")[0][3].any()


def test_one_frame():
    f0, ap, power, voiced = pitch.track_f0([np.float32([0.5])], 16000, 200, tracker="viterbi")[0]
    assert len(f0) == 1 and f0[0] == 0 and not voiced[0]
    per, val = np.zeros((1, K), np.float32), np.full((1, K), np.inf, np.float32)
    per[0, :2], val[0, :2] = (50.0, 100.0), (0.125, 0.0625)
    f0, state, cost = pitch.f0_viterbi_numpy(per, val, [1], 16000, 200, lag_bias=0.0)
    assert list(state) == [1] and f0[0] == 160.0 and cost == np.float32(0.0625)
    f0, state, cost = pitch.f0_viterbi_numpy(per, val, [1], 16000, 200, unvoiced_cost=0.03, lag_bias=0.0)
    assert list(state) == [K] and f0[0] == 0 and cost == np.float32(0.03)


def test_refusals():
    per, val = np.zeros((2049, K), np.float32), np.full((2049, K), np.inf, np.float32)
    with pytest.raises(ValueError, match="2048"):
        pitch.f0_viterbi_numpy(per, val, np.ones(2049, bool), 16000, 267)
    pitch.f0_viterbi_numpy(per[:2048], val[:2048], np.ones(2048, bool), 16000, 267)
    with pytest.raises(ValueError, match="2048"):
        pitch.track_f0([np.zeros(2048 * 200, np.float32)], 16000, 200, tracker="viterbi")
    with pytest.raises(ValueError, match="2048"):
        audio.Audio(toy_hparams(), backend="numpy").f0_batch([np.zeros(2048 * 200, np.float32)], tracker="viterbi")
    for kw in (dict(jump_cost=-0.1), dict(switch_cost=float("nan")), dict(unvoiced_cost=float("inf")), dict(lag_bias=-1.0)):
        with pytest.raises(ValueError):
            pitch.f0_viterbi_numpy(per[:4], val[:4], np.ones(4, bool), 16000, 267, **kw)
    with pytest.raises(ValueError):
        pitch.f0_viterbi_numpy(per[:4, :7], val[:4, :7], np.ones(4, bool), 16000, 267)
    with pytest.raises(ValueError):
        pitch.track_f0([np.zeros(100, np.float32)], 16000, 200, tracker="pyin")


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_struct_layouts_match_c(tmp_path):
    from satt_amd import _lib
    structs = (("satt_yin_candidates_params", _lib.YinCandidatesParams,
                ["window", "tau_min", "tau_max", "hop", "n_utts", "total_in", "total_frames", "signal", "in_offsets", "frame_offsets",
                 "cand_period", "cand_value", "power"]),
               ("satt_f0_viterbi_params", _lib.F0ViterbiParams,
                ["n_utts", "max_frames", "tau_max", "sample_rate", "jump_cost", "switch_cost", "unvoiced_cost", "lag_bias", "total_frames",
                 "cand_period", "cand_value", "gate", "frame_offsets", "f0", "state", "cost"]))
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "satt_hip.h"\nint main() {\n  printf("%d", SATT_F0_CANDIDATES);\n'
    for cname, P, names in structs:
        assert [n for n, _ in P._fields_] == names
        src += '  printf(" %%zu", sizeof(%s));\n' % cname + "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (cname, n) for n in names)
    (tmp_path / "t.c").write_text(src + "  return 0; }\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    vals = list(map(int, subprocess.check_output([str(tmp_path / "t")]).split()))
    want = [pitch.F0_CANDIDATES]
    for _, P, names in structs:
        want += [ctypes.sizeof(P)] + [getattr(P, n).offset for n in names]
    assert vals == want
    header = open(os.path.join(ROOT, "include", "satt_hip.h")).read()
    for sym in ("satt_yin_candidates", "satt_f0_viterbi_supported", "satt_f0_viterbi_max_frames", "satt_f0_viterbi"):
        assert sym + "(" in header and sym in _lib.SIGNATURES and hasattr(_lib.lib(), sym)
    assert _lib.SIGNATURES["satt_yin_candidates"][1][-1] is ctypes.c_void_p and _lib.SIGNATURES["satt_f0_viterbi"][1][-1] is ctypes.c_void_p


def test_supported_agrees_with_the_python_limit():
    from satt_amd import ops
    assert ops.f0_viterbi_max_frames() == pitch.F0_VITERBI_MAX_FRAMES == 2048
    for T in (-1, 0, 1, 2, 2047, 2048, 2049, 1 << 20):
        assert ops.f0_viterbi_supported(T) == (1 <= T <= 2048), T


def test_bad_arguments_return_before_any_launch():
    """there is no GPU here: every one of these calls has to come back with its code before the library touches the runtime"""
    from satt_amd import _lib
    lib = _lib.lib()
    BADARG, UNSUPPORTED = -1, -2
    keep = [(ctypes.c_int64 * 4)() for _ in range(7)]                                   # host memory: never dereferenced by the entry points
    ptr = [ctypes.addressof(k) for k in keep]

    def cand(**kw):
        f = dict(window=400, tau_min=32, tau_max=267, hop=200, n_utts=1, total_in=1000, total_frames=6, signal=ptr[0], in_offsets=ptr[1],
                 frame_offsets=ptr[2], cand_period=ptr[3], cand_value=ptr[4], power=ptr[5])
        f.update(kw)
        return _lib.YinCandidatesParams(**f)
    assert lib.satt_yin_candidates(None, None) == BADARG
    for kw in (dict(signal=None), dict(in_offsets=None), dict(frame_offsets=None), dict(cand_period=None), dict(cand_value=None),
               dict(power=None), dict(n_utts=0), dict(total_in=0), dict(total_frames=-1), dict(tau_min=1), dict(tau_min=267)):
        assert lib.satt_yin_candidates(ctypes.byref(cand(**kw)), None) == BADARG, kw
    for kw in (dict(window=0), dict(window=1537), dict(tau_max=2, tau_min=2), dict(tau_max=1024), dict(hop=0), dict(hop=(1 << 20) + 1)):
        assert lib.satt_yin_candidates(ctypes.byref(cand(**kw)), None) == UNSUPPORTED, kw

    def vit(**kw):
        f = dict(n_utts=1, max_frames=6, tau_max=267, sample_rate=16000.0, jump_cost=0.3, switch_cost=0.1, unvoiced_cost=0.15, lag_bias=0.1,
                 total_frames=6, cand_period=ptr[0], cand_value=ptr[1], gate=ptr[2], frame_offsets=ptr[3], f0=ptr[4], state=ptr[5], cost=ptr[6])
        f.update(kw)
        return _lib.F0ViterbiParams(**f)
    assert lib.satt_f0_viterbi(None, None) == BADARG
    for kw in (dict(cand_period=None), dict(cand_value=None), dict(gate=None), dict(frame_offsets=None), dict(f0=None), dict(state=None),
               dict(cost=None), dict(n_utts=0), dict(total_frames=0), dict(max_frames=0), dict(tau_max=0), dict(sample_rate=0.0),
               dict(sample_rate=float("nan")), dict(jump_cost=-1.0), dict(switch_cost=float("nan")), dict(unvoiced_cost=float("inf")),
               dict(lag_bias=-0.5)):
        assert lib.satt_f0_viterbi(ctypes.byref(vit(**kw)), None) == BADARG, kw
    for kw in (dict(max_frames=2049), dict(max_frames=1 << 20)):
        assert lib.satt_f0_viterbi(ctypes.byref(vit(**kw)), None) == UNSUPPORTED, kw


def test_ops_refuse_2049_frames_naming_the_limit():
    import torch
    from satt_amd import ops
    T = 2049
    per, val = torch.zeros(T, K), torch.zeros(T, K)
    with pytest.raises(ValueError, match="2048"):
        ops.f0_viterbi(per, val, torch.zeros(T, dtype=torch.uint8), torch.tensor([0, T]), T, 267, 16000, 0.3, 0.1, 0.15, 0.1,
                       torch.zeros(T), torch.zeros(T, dtype=torch.uint8), torch.zeros(1))


# ---- evaluate_f0.py ----------------------------------------------------------------------------------------------------------------------
def toy_hparams():
    import test_yin_cpu as tc
    return tc.toy_hparams()


COSTS = dict(jump_cost=0.3, switch_cost=0.1, unvoiced_cost=0.15, lag_bias=0.1)


def test_evaluate_f0_viterbi_on_wav_directories(tmp_path):
    import test_yin_cpu as tc
    pred_dir, ref_dir, out = str(tmp_path / "pw"), str(tmp_path / "rw"), str(tmp_path / "out")
    keys, skipped = tc.write_toy_wavs(pred_dir, ref_dir)
    stats = tc.write_stats(str(tmp_path / "hparams.json"))
    ac.run_driver("evaluate_f0.py", "--hparam-json-file", stats, "--backend", "numpy", "--tracker", "viterbi", "--pred-wav-dir", pred_dir,
                  "--ref-wav-dir", ref_dir, "--write-tracks", str(tmp_path / "unused"), out)
    au = audio.Audio(toy_hparams(), backend="numpy")
    sp = [au.load_wav(os.path.join(pred_dir, k + ".wav")) for k in keys]
    sr_ = [au.load_wav(os.path.join(ref_dir, k + ".wav")) for k in keys]
    mels = [au.normalize_mel(S).astype(np.float32) for S in au.melspectrogram_batch(sp + sr_)]
    want, tracks, dist = tc.expected(au, keys, sp, sr_, mels[:2], mels[2:], tracker="viterbi")
    assert tc.read_csv(os.path.join(out, "f0_distance.csv")) == want
    assert want["utt000"]["voiced_both"] >= 15 and abs(want["utt000"]["f0_rmse_cents"] - 100.0) <= 3.0 and want["utt000"]["gpe"] == 0.0
    s = json.load(open(os.path.join(out, "summary.json")))
    tc.check_summary(s, want, "wav", skipped)
    assert s["tracker"] == "viterbi" and {k: s[k] for k in COSTS} == COSTS and s["threshold"] == 0.15
    z = np.load(os.path.join(out, "utt000.f0.npz"))
    assert z["state_pred"].dtype == np.uint8 and z["state_pred"].tobytes() == tracks[0]["state"].tobytes()
    assert z["state_ref"].tobytes() == tracks[2]["state"].tobytes() and z["f0_pred"].tobytes() == tracks[0]["f0"].tobytes()
    assert np.array_equal(z["voiced_ref"], tracks[2]["state"] != K)
    # the costs reach the tracker; --unvoiced-cost follows --threshold unless given
    ac.run_driver("evaluate_f0.py", "--hparam-json-file", stats, "--backend", "numpy", "--tracker", "viterbi", "--pred-wav-dir", pred_dir,
                  "--ref-wav-dir", ref_dir, "--threshold", "0.2", "--jump-cost", "0.5", "--switch-cost", "0.25", "--lag-bias", "0.0", out)
    par = dict(threshold=0.2, jump_cost=0.5, switch_cost=0.25, lag_bias=0.0)
    want2, _, _ = tc.expected(au, keys, sp, sr_, mels[:2], mels[2:], tracker="viterbi", **par)
    assert tc.read_csv(os.path.join(out, "f0_distance.csv")) == want2
    s = json.load(open(os.path.join(out, "summary.json")))
    assert {k: s[k] for k in par} == par and s["unvoiced_cost"] == 0.2 and s["tracker"] == "viterbi"
    # the default run names no tracker and takes no cost
    ac.run_driver("evaluate_f0.py", "--hparam-json-file", stats, "--backend", "numpy", "--pred-wav-dir", pred_dir, "--ref-wav-dir", ref_dir, out)
    s = json.load(open(os.path.join(out, "summary.json")))
    assert "tracker" not in s and not any(k in s for k in COSTS)
    r = ac.run_driver("evaluate_f0.py", "--hparam-json-file", stats, "--backend", "numpy", "--jump-cost", "0.5", "--pred-wav-dir", pred_dir,
                      "--ref-wav-dir", ref_dir, out, check=False)
    assert r.returncode != 0 and "--tracker viterbi" in r.stderr


def test_evaluate_f0_viterbi_on_prediction_records(tmp_path):
    import test_yin_cpu as tc
    pred, out = str(tmp_path / "pred"), str(tmp_path / "out")
    records = tc.write_toy_records(pred)
    stats = tc.write_stats(str(tmp_path / "hparams.json"))
    ac.run_driver("evaluate_f0.py", "--hparam-json-file", stats, "--backend", "numpy", "--tracker", "viterbi", "--iters", "4", "--seed", "3",
                  pred, out)
    keys = [k for k in sorted(records) if records[k][1] is not None]
    au = audio.Audio(toy_hparams(), backend="numpy")
    mp, mr = [records[k][0] for k in keys], [records[k][1] for k in keys]
    wavs = au.inv_melspectrogram_batch([au.denormalize_mel(S.astype(np.float64)) for S in mp + mr], iters=4, seed=3)
    want, _, _ = tc.expected(au, keys, wavs[:3], wavs[3:], mp, mr, tracker="viterbi")
    assert tc.read_csv(os.path.join(out, "f0_distance.csv")) == want
    s = json.load(open(os.path.join(out, "summary.json")))
    tc.check_summary(s, want, "griffin_lim", ["utt002"])
    assert s["tracker"] == "viterbi" and {k: s[k] for k in COSTS} == COSTS and (s["iters"], s["seed"]) == (4, 3)
