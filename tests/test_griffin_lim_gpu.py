"""csrc/griffin_lim.hip against the float64 yardstick of tests/griffin_lim_common.py (torch.stft / torch.istft on the CPU): the inverse
STFT, one iteration from a seeded random phase, iterations 1 .. 6 one step at a time from the kernel's own state, the monotone
decrease of plain Griffin-Lim, the bit-level properties (batch = singles, repeat, 3 + 2 = 5, c_prev = NULL) and the refusals."""
import functools

import numpy as np
import pytest
import torch

import audio_common as ac
import griffin_lim_common as gc
import satt_amd  # noqa: F401
from satt_amd import ops
from satt_amd.utils import audio

pytestmark = pytest.mark.gpu
NAMES = gc.NAMES


@functools.lru_cache(maxsize=None)
def tables(name):
    return audio.MelspecTables(*ac.CONFIGS[name])


def run(name, mags, angs, iters, alpha, c_prevs=None):
    return gc.hip_run(tables(name))(mags, angs, iters, alpha, c_prevs)


@functools.lru_cache(maxsize=None)
def singles(name):
    """five iterations at alpha = 0.99 from the random phase, every utterance in a call of its own: [(y, ang, c_prev, c)]"""
    return [tuple(r[0] for r in run(name, [m], [rnd], 5, 0.99)) for _, m, _, rnd in gc.inputs(name)]


@pytest.mark.parametrize("name", NAMES)
def test_inverse_stft_matches_torch_istft_and_returns_the_signal(name):
    _, n_fft, win, hop, _ = ac.CONFIGS[name]
    cases = gc.inputs(name)
    ys, angs, _, _ = run(name, [c[1] for c in cases], [c[2] for c in cases], 0, 0.0)
    for (y0, mag, ang, _), y, a in zip(cases, ys, angs):
        T = mag.shape[0]
        assert y.shape == ((T - 1) * hop,) and 1 + len(y) // hop == T
        assert a.tobytes() == ang.tobytes()                      # iters = 0 leaves the state alone
        y64 = gc.istft64(mag.astype(np.float64) * ang, n_fft, hop, win)
        e = np.abs(y - y64).max() / np.abs(y64).max()
        e0 = np.abs(y - y0[:len(y)].astype(np.float64)).max() / np.abs(y0).max()
        print("%s T=%d: istft %.3e  round trip %.3e (bound %.3e)" % (name, T, e, e0, gc.C_ISTFT))
        assert e <= gc.C_ISTFT, (name, T, e)
        assert e0 <= gc.C_ISTFT, (name, T, e0)


def _check_step(name, tag, mag, a0, p0, a1, p1, c, alpha):
    _, n_fft, win, hop, _ = ac.CONFIGS[name]
    _, c64, u64, a64 = gc.step64(mag, a0, p0, alpha, n_fft, hop, win)
    e_c, e_a = gc.frame_err(c, c64).max(), gc.ang_err(a1, a64, u64, c64, alpha).max()
    print("%s %s T=%d alpha=%.2f: c %.3e  ang %.3e (bound %.3e)" % (name, tag, mag.shape[0], alpha, e_c, e_a, gc.C_ITER))
    assert e_c <= gc.C_ITER, (name, tag, e_c)
    assert e_a <= gc.C_ITER, (name, tag, e_a)
    assert p1.tobytes() == c.tobytes()                           # c_prev' = c
    assert np.abs(np.abs(a1) - 1.0).max() <= 1e-6


@pytest.mark.parametrize("alpha", gc.ALPHAS)
@pytest.mark.parametrize("name", NAMES)
def test_one_iteration_from_a_seeded_random_phase(name, alpha):
    cases = gc.inputs(name)
    mags, angs = [c[1] for c in cases], [c[3] for c in cases]
    prevs = [np.zeros_like(a) for a in angs]
    _, angs1, prevs1, cs = run(name, mags, angs, 1, alpha, prevs)
    for mag, a0, p0, a1, p1, c in zip(mags, angs, prevs, angs1, prevs1, cs):
        _check_step(name, "iteration 1", mag, a0, p0, a1, p1, c, alpha)


@pytest.mark.parametrize("alpha", gc.ALPHAS)
@pytest.mark.parametrize("name", NAMES)
def test_iterations_one_step_at_a_time_from_the_kernels_own_state(name, alpha):
    """iteration k against ONE float64 step applied to the kernel's state behind k - 1 iterations (a free-running float32 run
    drifts from a free-running float64 one: the iteration amplifies rounding)"""
    cases = gc.inputs(name)
    mags, angs = [c[1] for c in cases], [c[3] for c in cases]
    prevs = [np.zeros_like(a) for a in angs]
    for k in range(1, gc.STEPS + 1):
        _, angs1, prevs1, cs = run(name, mags, angs, 1, alpha, prevs)
        for mag, a0, p0, a1, p1, c in zip(mags, angs, prevs, angs1, prevs1, cs):
            _check_step(name, "iteration %d" % k, mag, a0, p0, a1, p1, c, alpha)
        angs, prevs = angs1, prevs1


@pytest.mark.parametrize("name", NAMES)
def test_plain_griffin_lim_never_increases_the_spectral_distance(name):
    cases = gc.inputs(name)
    mags, angs = [c[1] for c in cases], [c[3] for c in cases]
    dist = [[] for _ in cases]
    for _ in range(8):
        _, angs, _, cs = run(name, mags, angs, 1, 0.0)
        for d, c, mag in zip(dist, cs, mags):
            d.append(gc.convergence(c, mag))
    for d, mag in zip(dist, mags):
        print("%s T=%d: %s  last / first %.3f" % (name, mag.shape[0], " ".join("%.4f" % v for v in d), d[-1] / d[0]))
        assert all(b <= a + 1e-5 for a, b in zip(d, d[1:])), (name, d)
        assert d[-1] <= 0.75 * d[0], (name, d)


@pytest.mark.parametrize("name", NAMES)
def test_a_mixed_batch_equals_the_single_launches_bit_for_bit(name):
    cases, one = gc.inputs(name), singles(name)
    order = [0, 4, 2, 3, 0]
    ys, angs, prevs, cs = run(name, [cases[i][1] for i in order], [cases[i][3] for i in order], 5, 0.99)
    for i, y, a, p, c in zip(order, ys, angs, prevs, cs):
        assert [x.tobytes() for x in (y, a, p, c)] == [x.tobytes() for x in one[i]], (name, i)


@pytest.mark.parametrize("name", NAMES)
def test_repeat_launch_and_split_runs_are_bit_equal(name):
    """a repeat call; iters = 3 then 2 against iters = 5 (state and signal); c_prev = NULL at alpha = 0 against a buffer"""
    cases, one = gc.inputs(name), singles(name)
    mags, angs = [c[1] for c in cases], [c[3] for c in cases]
    again = run(name, mags, angs, 5, 0.99)
    _, a3, p3, _ = run(name, mags, angs, 3, 0.99)
    split = run(name, mags, a3, 2, 0.99, p3)
    for i in range(len(cases)):
        for res in (again, split):
            assert [res[j][i].tobytes() for j in range(4)] == [x.tobytes() for x in one[i]], (name, i)
    with_buffer = run(name, mags, angs, 4, 0.0, [np.full_like(a, np.nan) for a in angs])      # written, never read
    ys = audio.griffin_lim_hip(tables(name), mags, angs, 4, 0.0)                               # c_prev = NULL
    assert all(y.tobytes() == z.tobytes() for y, z in zip(ys, with_buffer[0]))
    assert all(np.isfinite(p).all() and p.tobytes() == c.tobytes() for p, c in zip(with_buffer[2], with_buffer[3]))


def _direct(t, mags, angs, iters, alpha, sentinel):
    """ops.griffin_lim without the host checks of utils/audio.py: (signal, ang) as arrays, signal prefilled with the sentinel"""
    dev = "cuda"
    NF = t.n_fft // 2 + 1
    Ts = np.asarray([len(m) for m in mags], np.int64)
    fo = np.concatenate([[0], np.cumsum(Ts)]).astype(np.int64)
    so = np.concatenate([[0], np.cumsum((Ts - 1) * t.hop)]).astype(np.int64)
    mag = torch.from_numpy(np.concatenate(mags)).to(dev)
    ang = torch.view_as_real(torch.from_numpy(np.concatenate(angs)).to(dev)).contiguous()
    prev = torch.zeros_like(ang)
    signal = torch.full((int(so[-1]),), sentinel, dtype=torch.float32, device=dev)
    ws = torch.zeros(int(fo[-1]) * t.n_fft, dtype=torch.float32, device=dev)
    env = torch.from_numpy(audio.overlap_envelope_tables(audio.padded_window(t.n_fft, t.win), t.hop)).to(dev)
    ops.griffin_lim(mag, ang, prev, signal, torch.from_numpy(so).to(dev), torch.from_numpy(fo).to(dev), t.n_fft, t.win, t.hop, iters, alpha,
                    torch.from_numpy(t.window).to(dev), torch.from_numpy(t.twiddle).to(dev), env, ws)
    return signal.cpu().numpy(), torch.view_as_complex(ang).cpu().numpy(), so, fo


@pytest.mark.parametrize("name", NAMES)
def test_an_utterance_of_too_few_frames_is_refused_and_left_untouched(name):
    t = tables(name)
    cases, one = gc.inputs(name), singles(name)
    mag0, ang0 = gc.refused_input(name)
    with pytest.raises(ValueError, match="frames"):
        audio.griffin_lim_hip(t, [cases[0][1], mag0], [cases[0][3], ang0], 5, 0.99)
    order = [1, None, 2]                                         # the refused utterance between two accepted ones
    mags = [mag0 if i is None else cases[i][1] for i in order]
    angs = [ang0 if i is None else cases[i][3] for i in order]
    y, a, so, fo = _direct(t, mags, angs, 5, 0.99, 123.0)
    for u, i in enumerate(order):
        yu, au = y[so[u]:so[u + 1]], a[fo[u]:fo[u + 1]]
        if i is None:
            assert (yu == 123.0).all() and au.tobytes() == ang0.tobytes()
        else:
            assert yu.tobytes() == one[i][0].tobytes() and au.tobytes() == one[i][1].tobytes()


def test_unsupported_parameters_are_refused_by_name():
    assert all(ops.griffin_lim_supported(*ac.CONFIGS[n][1:4]) for n in NAMES)
    sr, n_fft, win, hop, mels = ac.CONFIGS["fft512_hop_beyond_window"]
    bad = [("hop=256", audio.MelspecTables(sr, n_fft, win, hop, mels)), ("n_fft=256", audio.MelspecTables(16000, 256, 256, 64, 20)),
           ("hop=201", audio.MelspecTables(16000, 512, 400, 201, 20)), ("win=12", audio.MelspecTables(16000, 512, 12, 4, 20))]
    for what, t in bad:
        assert not ops.griffin_lim_supported(t.n_fft, t.win, t.hop)
        T = 4 + t.n_fft // t.hop
        mag = np.ones((T, t.n_fft // 2 + 1), np.float32)
        ang = np.ones(mag.shape, np.complex64)
        with pytest.raises(ValueError, match=what):
            audio.griffin_lim_hip(t, [mag], [ang], 1, 0.0)
        with pytest.raises(ValueError, match="does not take"):
            _direct(t, [mag], [ang], 1, 0.0, 0.0)
    assert ops.griffin_lim_supported(512, 400, 200) and ops.griffin_lim_workspace_bytes(2048, 800) == 800 * 2048 * 4


def test_audio_class_inverts_its_own_mel_spectrogram_on_the_hip_backend():
    a = gc.lj_audio("hip")
    assert a.backend == "hip"
    gc.check_end_to_end(a)
    # the sample cap splits a batch into several entry calls without changing a bit
    Ss = [a.melspectrogram_batch([ac.harmonic(n, 22050, seed=s)])[0] for s, n in enumerate((3308, 2800, 4000))]
    whole = a.inv_melspectrogram_batch(Ss, iters=4)
    cap, audio.MAX_LAUNCH_SAMPLES = audio.MAX_LAUNCH_SAMPLES, 5000
    try:
        split = a.inv_melspectrogram_batch(Ss, iters=4)
    finally:
        audio.MAX_LAUNCH_SAMPLES = cap
    assert all(x.tobytes() == y.tobytes() for x, y in zip(whole, split))
