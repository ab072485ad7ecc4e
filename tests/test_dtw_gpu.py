"""csrc/dtw.hip against the float32 NumPy backend (cost bits, steps and the whole path equal), its batching guarantees, what it
leaves untouched (poisoned outputs and workspace, bad offset tables), LDS poison, the float64 bounds of tests/dtw_common.py, and the
Python surface over it."""
import os

import numpy as np
import pytest
import torch

import audio_common as ac
import dtw_common as dc
import satt_amd  # noqa: F401
from satt_amd import _lib, ops
from satt_amd.hparams import hparams
from satt_amd.utils import audio
from satt_amd.utils import mel_distance as md

pytestmark = pytest.mark.gpu

DEV = "cuda"
NT = md.DTW_NT
SMALL = [(1, 1), (1, 7), (7, 1), (2, 2), (63, 64), (64, 65), (65, 63)]
SEAMS = [(t, c) for t in (NT - 1, NT, NT + 1) for c in (3, 70)]
SHAPES = SMALL + SEAMS + [(c, t) for t, c in SEAMS] + [(2048, 5), (5, 2048), (300, 417)]
P_COST, P_STEPS, P_DIR, P_PATH = -77.25, -7, 0xEE, -9
GAP = 13                                                             # bytes / entries of slack behind every pair's workspace and path


def raw_launch(a, b, ao, bo, max_ta, max_tb, do=None, po=None, tail=0):
    """one launch on poisoned buffers; a, b: float32 [total, K]; the offset tables as given (int64 lists).  Returns cost, steps,
    dirs, path as NumPy arrays (dirs and path None without do / po); `tail` more elements than the tables claim in every buffer."""
    n = len(ao) - 1
    t = lambda x, dt=torch.int64: torch.as_tensor(np.asarray(x), dtype=dt).to(DEV)
    cost = torch.full((n + tail,), P_COST, dtype=torch.float32, device=DEV)
    steps = torch.full((n + tail,), P_STEPS, dtype=torch.int32, device=DEV)
    dirs = path = None
    if do is not None:
        dirs = torch.full((int(do[-1]) + tail,), P_DIR, dtype=torch.uint8, device=DEV)
        path = torch.full((int(po[-1]) + tail, 2), P_PATH, dtype=torch.int32, device=DEV)
    ops.dtw(t(a, torch.float32), t(b, torch.float32), t(ao), t(bo), max_ta, max_tb, cost, steps, dirs, None if do is None else t(do),
            path, None if po is None else t(po))
    torch.cuda.synchronize()
    return cost.cpu().numpy(), steps.cpu().numpy(), None if dirs is None else dirs.cpu().numpy(), None if path is None else path.cpu().numpy()


def tables(pairs):
    ta, tb = [len(a) for a, _ in pairs], [len(b) for _, b in pairs]
    off = lambda c: np.concatenate([[0], np.cumsum(c)]).astype(np.int64)
    return off(ta), off(tb), off([x * y + GAP for x, y in zip(ta, tb)]), off([x + y - 1 + GAP for x, y in zip(ta, tb)])


def launch(pairs, want_path=True, tail=0):
    """the batch in one launch: (list of (cost, steps, path), raw buffers, offset tables)"""
    ao, bo, do, po = tables(pairs)
    raw = raw_launch(np.concatenate([a for a, _ in pairs]), np.concatenate([b for _, b in pairs]), ao, bo,
                     max(len(a) for a, _ in pairs), max(len(b) for _, b in pairs), do if want_path else None, po if want_path else None, tail)
    cost, steps, _, path = raw
    res = [(cost[u], int(steps[u]), path[po[u]:po[u] + max(steps[u], 0)] if want_path else None) for u in range(len(pairs))]
    return res, raw, (ao, bo, do, po)


def same(got, want):
    return got[0].tobytes() == np.float32(want[0]).tobytes() and got[1] == want[1] and (got[2] is None or np.array_equal(got[2], want[2]))


_REF = {}


def reference(Ta, Tb, K):
    """the pair and its NumPy result, computed once"""
    if (Ta, Tb, K) not in _REF:
        a, b = dc.warped_pair(Ta, Tb, K)
        _REF[Ta, Tb, K] = (a, b, md.dtw_numpy(a, b, want_path=True))
    return _REF[Ta, Tb, K]


# ---- the kernel against the NumPy backend --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 13, 80, 128])
def test_kernel_equals_the_numpy_backend(K):
    refs = [reference(Ta, Tb, K) for Ta, Tb in SHAPES]
    res, _, _ = launch([(a, b) for a, b, _ in refs])
    for (Ta, Tb), got, (_, _, want) in zip(SHAPES, res, refs):
        assert not dc.path_problems(got[2], Ta, Tb, got[1]), (Ta, Tb, dc.path_problems(got[2], Ta, Tb, got[1]))
        assert same(got, want), (Ta, Tb, K, got[:2], want[:2])


def test_the_longest_pair():
    a, b, want = reference(2048, 2048, 2)
    res, raw, (_, _, do, po) = launch([(a, b)], tail=64)
    assert not dc.path_problems(res[0][2], 2048, 2048, res[0][1]) and same(res[0], want)
    assert np.all(raw[2][2048 * 2048:] == P_DIR) and np.all(raw[3][res[0][1]:] == P_PATH)


def test_exact_ties_give_the_numpy_path():
    for K in (2, 1):                                                                    # (one feature width per launch)
        pairs = [dc.tie_pair(Ta, Tb, K) for Ta, Tb in ((40, 55), (NT + 5, 90), (33, 2 * NT + 1), (3, 4))]
        res, _, _ = launch(pairs)
        for (a, b), got in zip(pairs, res):
            assert same(got, md.dtw_numpy(a, b, want_path=True)), (a.shape, b.shape)


def test_hand_worked_examples_pin_the_tie_break_cell_by_cell():
    """D, L and the direction of every cell of the two hand-worked tables of tests/dtw_common.py: every prefix of either pair as a
    pair of its own, all in one launch; cell (2, 3) of the second example is the one with up == left < diagonal"""
    res, _, _ = launch([dc.hand_prefix(e, i, j)[0] for e, i, j in dc.HAND_CELLS])
    for (e, i, j), got in zip(dc.HAND_CELLS, res):
        assert (got[0], got[1], dc.last_move(got[2])) == dc.hand_prefix(e, i, j)[1], (e, i, j)
    res, _, _ = launch([(x["a"], x["b"]) for x in dc.HAND_EXAMPLES])
    for x, got in zip(dc.HAND_EXAMPLES, res):
        assert np.array_equal(got[2], x["path"])


# ---- batching ------------------------------------------------------------------------------------------------------------------------
def test_a_pair_does_not_depend_on_its_batch_or_its_place():
    shapes = SMALL + SEAMS[:4] + [(c, t) for t, c in SEAMS[:4]] + [(300, 417), (5, 2048)]
    assert len(shapes) == 17
    refs = [reference(Ta, Tb, 13) for Ta, Tb in shapes]
    pairs = [(a, b) for a, b, _ in refs]
    whole, raw, _ = launch(pairs)
    again, raw2, _ = launch(pairs)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(raw, raw2))                  # two launches: identical bits, workspace included
    back, _, _ = launch(pairs[::-1])
    for u, (pair, (_, _, want)) in enumerate(zip(pairs, refs)):
        alone, _, _ = launch([pair])
        assert same(alone[0], want) and same(whole[u], alone[0]) and same(back[len(pairs) - 1 - u], alone[0]), shapes[u]


# ---- outputs and workspace -----------------------------------------------------------------------------------------------------------
def test_nothing_outside_a_pairs_own_ranges_is_written():
    shapes = [(7, 1), (NT + 1, 3), (64, 65), (1, 1), (70, NT)]
    refs = [reference(Ta, Tb, 13) for Ta, Tb in shapes]
    pairs = [(a, b) for a, b, _ in refs]
    res, (cost, steps, dirs, path), (ao, bo, do, po) = launch(pairs, tail=100)
    n = len(pairs)
    assert np.all(cost[n:] == P_COST) and np.all(steps[n:] == P_STEPS) and np.all(dirs[do[-1]:] == P_DIR) and np.all(path[po[-1]:] == P_PATH)
    for u, ((Ta, Tb), got, (_, _, want)) in enumerate(zip(shapes, res, refs)):
        assert same(got, want)
        assert np.all(dirs[do[u]:do[u] + Ta * Tb] <= 2)                                 # every cell's byte was written
        assert np.all(dirs[do[u] + Ta * Tb:do[u + 1]] == P_DIR)                         # and nothing behind them
        assert np.all(path[po[u] + got[1]:po[u + 1]] == P_PATH)
    # without the path pointers: the same cost and steps
    bare, (cost2, steps2, _, _), _ = launch(pairs, want_path=False, tail=100)
    assert cost2[:n].tobytes() == cost[:n].tobytes() and steps2[:n].tobytes() == steps[:n].tobytes()
    assert np.all(cost2[n:] == P_COST) and np.all(steps2[n:] == P_STEPS)


def test_a_partial_set_of_path_pointers_is_refused_before_any_launch():
    """the entry point takes all four path pointers or none (without them no workspace is known to the launch at all): a
    workspace without its offsets comes back SATT_E_BADARG and stays as it was"""
    ws = torch.full((65 * 63 + 100,), P_DIR, dtype=torch.uint8, device=DEV)
    p = _lib.DtwParams(n_pairs=1, K=13, max_ta=65, max_tb=63, total_a=65, total_b=63, total_dirs=ws.numel(), total_path=0,
                       a=ws.data_ptr(), b=ws.data_ptr(), a_offsets=ws.data_ptr(), b_offsets=ws.data_ptr(), cost=ws.data_ptr(),
                       steps=ws.data_ptr(), dirs=ws.data_ptr(), dir_offsets=None, path=None, path_offsets=None)
    with pytest.raises(_lib.SattError):
        _lib.check(_lib.lib().satt_dtw(_lib.C.byref(p), ops._s()), "dtw")
    torch.cuda.synchronize()
    assert bool((ws == P_DIR).all())


# ---- bad offset tables ---------------------------------------------------------------------------------------------------------------
def check_bad_tables(a, b, ao, bo, do, po, untouched, max_ta, max_tb, total_a=None):
    """launch with the tables as given; the pairs of `untouched` keep their poison, the others equal NumPy on their own slices"""
    cost, steps, dirs, path = raw_launch(a[:total_a], b, ao, bo, max_ta, max_tb, do, po, tail=10)
    n = len(ao) - 1
    for u in range(n):
        if u in untouched:
            assert cost[u] == np.float32(P_COST) and steps[u] == P_STEPS, u
            assert np.all(dirs[do[u]:do[u + 1]] == P_DIR) and np.all(path[po[u]:po[u + 1]] == P_PATH), u
        else:
            want = md.dtw_numpy(a[ao[u]:ao[u + 1]], b[bo[u]:bo[u + 1]], want_path=True)
            assert same((cost[u], int(steps[u]), path[po[u]:po[u] + steps[u]]), want), u
    assert np.all(cost[n:] == P_COST) and np.all(dirs[do[-1]:] == P_DIR) and np.all(path[po[-1]:] == P_PATH)


def test_bad_offset_tables_leave_their_pairs_untouched():
    rng = np.random.default_rng(11)
    a, b = rng.standard_normal((30, 13)).astype(np.float32), rng.standard_normal((36, 13)).astype(np.float32)
    bo = [0, 9, 20, 36]
    do, po = [0, 400, 800, 1200], [0, 40, 80, 120]                                       # room for any pair of these tables
    check_bad_tables(a, b, [0, 10, 18, 30], bo, do, po, set(), 12, 16)                   # the good tables first
    check_bad_tables(a, b, [0, 10, 18, 30], bo, do, po, {2}, 12, 16, total_a=29)         # a range past total_a
    check_bad_tables(a, b, [0, 10, 10, 30], bo, do, po, {1}, 20, 16)                     # a length of 0
    check_bad_tables(a, b, [0, 10, 5, 30], bo, do, po, {1}, 25, 16)                      # a negative length
    check_bad_tables(a, b, [-1, 10, 18, 30], bo, do, po, {0}, 12, 16)                    # a range in front of the buffer
    check_bad_tables(a, b, [0, 10, 18, 30], bo, [0, 400, 480, 900], po, {1}, 12, 16)     # 8 x 11 = 88 cells, 80 bytes of workspace
    check_bad_tables(a, b, [0, 10, 18, 30], bo, do, [0, 40, 57, 120], {1}, 12, 16)       # 8 + 11 - 1 = 18 entries, room for 17
    # a length of 2049: K = 1, the long pair in the middle; the caller's max_ta = 2048 is what gets the launch past the entry point
    a = rng.standard_normal((2049 + 12, 1)).astype(np.float32)
    b = rng.standard_normal((15, 1)).astype(np.float32)
    check_bad_tables(a, b, [0, 5, 2054, 2061], [0, 4, 9, 15], [0, 100, 12000, 12100], [0, 20, 2100, 2120], {1}, 2048, 6)
    with pytest.raises(ValueError):                                                     # stated honestly, nothing is launched
        raw_launch(a, b, [0, 5, 2054, 2061], [0, 4, 9, 15], 2049, 6)


def test_nan_features_neither_hang_nor_fault():
    a, b, want = reference(64, 65, 13)
    bad = a.copy()
    bad[17, 3] = np.nan
    bad[40] = np.inf
    res, _, _ = launch([(bad, b), (a, b)])
    assert np.isnan(res[0][0]) and 1 <= res[0][1] <= 64 + 65 - 1 and not dc.path_problems(res[0][2], 64, 65, res[0][1])
    assert same(res[1], want)


# ---- LDS poison ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", [0x7FC00000, 0xFF800000, 0x00000000], ids=["nan", "minus_inf", "zero"])
def test_bits_do_not_depend_on_what_lds_held(pattern):
    """satt_debug_poison_lds leaves the pattern in every LDS word of every CU in front of the launch: -inf would win every minimum
    and a NaN in the first candidate would stay chosen, so a predecessor read before it was written changes the result"""
    shapes = [(NT + 1, 70), (65, 63), (1, 7), (300, 417)]
    refs = [reference(Ta, Tb, 13) for Ta, Tb in shapes]
    _lib.check(_lib.lib().satt_debug_poison_lds(pattern, 100, ops.current_stream().cuda_stream), "poison_lds")
    res, _, _ = launch([(a, b) for a, b, _ in refs])
    for got, (_, _, want) in zip(res, refs):
        assert same(got, want)


# ---- float64 -------------------------------------------------------------------------------------------------------------------------
def test_kernel_meets_the_float64_bounds():
    a, b, _ = reference(300, 417, 13)
    (got,), _, _ = launch([(a, b)])
    dc.check_against_float64(got[0], got[1], got[2], a, b)


# ---- the public surface --------------------------------------------------------------------------------------------------------------
def toy_hparams():
    hp = hparams.copy()
    hp.parse("num_freq=513,sample_rate=16000,frame_length_ms=50.0,frame_shift_ms=12.5,num_mels=80")
    hp.set("average_mel_level_db", [-40.0 - 0.1 * m for m in range(80)])
    hp.set("stddev_mel_level_db", [10.0 + 0.05 * m for m in range(80)])
    return hp


@pytest.mark.parametrize("feature", ["mcep", "mel"])
def test_mel_distance_batch_hip_equals_numpy(feature, monkeypatch):
    rng = np.random.default_rng(21)
    refs = [rng.standard_normal((n, 80)).astype(np.float32) for n in (31, 77, NT + 3, 120)]
    preds = [(r[np.sort(rng.integers(0, len(r), len(r) + 9 - 6 * u))] + 0.1 * rng.standard_normal((len(r) + 9 - 6 * u, 80))).astype(np.float32)
             for u, r in enumerate(refs)]
    hp = toy_hparams()
    h = audio.Audio(hp, backend="hip", device=DEV).mel_distance_batch(preds, refs, feature=feature, want_paths=True)
    n = audio.Audio(hp, backend="numpy").mel_distance_batch(preds, refs, feature=feature, want_paths=True)
    for x, y in zip(h, n):
        assert {k: v for k, v in x.items() if k != "path"} == {k: v for k, v in y.items() if k != "path"} and x["value"] > 0
        assert np.array_equal(x["path"], y["path"])
    plain = audio.Audio(hp, backend="hip", device=DEV).mel_distance_batch(preds, refs, feature=feature)
    assert plain == [{k: v for k, v in x.items() if k != "path"} for x in h]
    # a workspace budget that cuts the batch into several launches: the same results
    feats = [(md.mel_cepstrum(p.astype(np.float64), 13), md.mel_cepstrum(r.astype(np.float64), 13)) for p, r in zip(preds, refs)]
    whole = md.dtw_hip(feats, True, DEV)
    cut = md.dtw_hip(feats, True, DEV, workspace_bytes=10000)
    assert all(same(x, y) for x, y in zip(cut, whole))


def test_evaluate_mel_driver_on_the_hip_backend(tmp_path):
    from test_dtw_cpu import write_stats, write_toy_predictions
    pred = str(tmp_path / "pred")
    write_toy_predictions(pred)
    stats = write_stats(str(tmp_path / "hparams.json"))
    outs = {}
    for backend in ("hip", "numpy"):
        outs[backend] = str(tmp_path / backend)
        ac.run_driver("evaluate_mel.py", "--hparam-json-file", stats, "--backend", backend, "--write-paths", pred, outs[backend])
    assert sorted(os.listdir(outs["hip"])) == sorted(os.listdir(outs["numpy"]))
    for f in os.listdir(outs["hip"]):
        if f.endswith(".npz"):
            assert np.array_equal(np.load(os.path.join(outs["hip"], f))["path"], np.load(os.path.join(outs["numpy"], f))["path"]), f
        else:
            assert open(os.path.join(outs["hip"], f)).read() == open(os.path.join(outs["numpy"], f)).read(), f
