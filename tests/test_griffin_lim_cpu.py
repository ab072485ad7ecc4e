"""The host side of Griffin-Lim: the float32 NumPy backend against the float64 yardstick (held to C / 8 of the kernel's bounds), the
envelope tables against a direct sum, mel_to_linear on the basis's row space, the supported set and the struct layout."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import audio_common as ac
import griffin_lim_common as gc
import satt_amd  # noqa: F401
from satt_amd.utils import audio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_griffin_lim_struct_layout_matches_c(tmp_path):
    """sizeof / offsetof of the ctypes mirror == the C struct (host compiler), and the entry points are declared on both sides"""
    from satt_amd import _lib
    names = [n for n, _ in _lib.GriffinLimParams._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "satt_hip.h"\nint main() {\n  printf("%zu", sizeof(satt_griffin_lim_params));\n'
    src += "".join('  printf(" %%zu", offsetof(satt_griffin_lim_params, %s));\n' % n for n in names) + "  return 0; }\n"
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    vals = list(map(int, subprocess.check_output([str(tmp_path / "t")]).split()))
    G = _lib.GriffinLimParams
    assert vals == [ctypes.sizeof(G)] + [getattr(G, n).offset for n in names]
    header = open(os.path.join(ROOT, "include", "satt_hip.h")).read()
    for sym in ("satt_griffin_lim_supported", "satt_griffin_lim_workspace_bytes", "satt_griffin_lim"):
        assert sym + "(" in header and sym in _lib.SIGNATURES
    assert _lib.SIGNATURES["satt_griffin_lim"][1][-1] is ctypes.c_void_p


def test_supported_set_and_each_single_violation():
    from satt_amd import ops
    for n_fft in (512, 1024, 2048, 4096):
        for win, hop in ((16, 1), (16, 8), (n_fft, n_fft // 2), (n_fft, 1)):
            assert ops.griffin_lim_supported(n_fft, win, hop), (n_fft, win, hop)
    for name in gc.NAMES:
        assert ops.griffin_lim_supported(*ac.CONFIGS[name][1:4])
    for bad in ((256, 200, 64), (8192, 2400, 600), (1000, 800, 200), (2048, 15, 4), (2048, 2049, 275), (2048, 1102, 0),
                (2048, 1102, 552), ac.CONFIGS["fft512_hop_beyond_window"][1:4]):
        assert not ops.griffin_lim_supported(*bad), bad
    assert ops.griffin_lim_workspace_bytes(4096, 3) == 3 * 4096 * 4


def test_refusals_name_the_offending_quantity():
    for what, cfg in (("hop=256", ac.CONFIGS["fft512_hop_beyond_window"]), ("n_fft=256", (16000, 256, 256, 64, 20)),
                      ("win=12", (16000, 512, 12, 4, 20))):
        t = audio.MelspecTables(*cfg)
        mag = np.ones((4 + t.n_fft // t.hop, t.n_fft // 2 + 1), np.float32)
        with pytest.raises(ValueError, match=what):
            audio.griffin_lim_numpy(t, mag, np.ones(mag.shape, np.complex64), 1, 0.0)
    for name in gc.NAMES:
        mag0, ang0 = gc.refused_input(name)
        with pytest.raises(ValueError, match="frames=%d" % len(mag0)):
            audio.griffin_lim_numpy(audio.MelspecTables(*ac.CONFIGS[name]), mag0, ang0, 1, 0.0)


@pytest.mark.parametrize("n_fft,win,hop,frames", [(512, 512, 128, (4, 5, 9)), (1024, 800, 200, (5, 8)), (2048, 1102, 275, (5, 6, 40)),
                                                  (512, 512, 3, (87, 200)), (512, 301, 7, (38, 90))])
def test_envelope_tables_against_a_direct_sum(n_fft, win, hop, frames):
    """F - H - G reproduces sum_t w^2[p - t hop] for every frame count - the small hops are those at which a position is short of
    frames at BOTH ends at once - and the envelope stays away from zero over the samples kept"""
    w = [0.0] * n_fft
    lead = (n_fft - win) // 2
    for i in range(win):
        w[lead + i] = 0.5 - 0.5 * math.cos(2.0 * math.pi * i / win)
    assert np.abs(audio.padded_window(n_fft, win) - np.asarray(w)).max() <= 1e-15
    tab = audio.overlap_envelope_tables(audio.padded_window(n_fft, win), hop)
    assert tab.dtype == np.float64 and tab.shape == (hop + 2 * n_fft,)
    F, H, G = tab[:hop], tab[hop:hop + n_fft], tab[hop + n_fft:]
    for T in frames:
        assert (T - 1) * hop >= n_fft // 2 + 1
        direct = np.zeros(n_fft + hop * (T - 1))
        for t in range(T):
            for i in range(lead, lead + win):
                direct[t * hop + i] += w[i] * w[i]
        p = np.arange(len(direct))
        env = F[p % hop] - np.where(p < n_fft, H[np.minimum(p, n_fft - 1)], 0.0) - np.where(p >= T * hop, G[np.maximum(p - T * hop, 0)], 0.0)
        assert np.abs(env - direct).max() <= 1e-12 * direct.max()
        assert np.abs(audio.overlap_envelope(audio.padded_window(n_fft, win), hop, T) - direct).max() <= 1e-12 * direct.max()
        assert direct[n_fft // 2:n_fft // 2 + (T - 1) * hop].min() >= 0.99       # frame 0 / T - 1 alone give ~1 at the two ends


@pytest.mark.parametrize("name", gc.NAMES)
def test_numpy_backend_is_held_to_an_eighth_of_the_kernels_bounds(name):
    m = gc.measure(name, gc.numpy_run(audio.MelspecTables(*ac.CONFIGS[name])))
    print(name, m)
    assert m["istft"] <= gc.C_ISTFT / 8 and m["roundtrip"] <= gc.C_ISTFT / 8
    assert max(m["iter_c"], m["iter_ang"], m["step_c"]) <= gc.C_ITER / 8


def test_the_float64_round_trip_is_an_identity():
    for name in gc.NAMES:
        _, n_fft, win, hop, _ = ac.CONFIGS[name]
        for y0, mag, ang, _ in gc.inputs(name):
            X = gc.stft64(y0, n_fft, hop, win)
            y = gc.istft64(X, n_fft, hop, win)
            assert np.abs(y - y0[:len(y)]).max() <= 1e-14 * np.abs(y0).max()


@pytest.mark.parametrize("name", gc.NAMES)
def test_plain_griffin_lim_on_the_numpy_backend_never_increases_the_distance(name):
    t = audio.MelspecTables(*ac.CONFIGS[name])
    for _, mag, _, rnd in gc.inputs(name):
        a, d = rnd, []
        for _ in range(8):
            _, a, _, c = audio.griffin_lim_numpy(t, mag, a, 1, 0.0, want_state=True)
            d.append(gc.convergence(c, mag))
        assert all(y <= x + 1e-5 for x, y in zip(d, d[1:])) and d[-1] <= 0.75 * d[0], (name, d)
    # split runs continue the state: 3 + 2 iterations are 5
    y5, a5, p5, _ = audio.griffin_lim_numpy(t, mag, rnd, 5, 0.99, want_state=True)
    _, a3, p3, _ = audio.griffin_lim_numpy(t, mag, rnd, 3, 0.99, want_state=True)
    y2, a2, p2, _ = audio.griffin_lim_numpy(t, mag, a3, 2, 0.99, c_prev=p3, want_state=True)
    assert y2.tobytes() == y5.tobytes() and a2.tobytes() == a5.tobytes() and p2.tobytes() == p5.tobytes()


def test_mel_to_linear_is_the_identity_on_the_row_space_of_the_basis():
    for name in ("ljspeech", "vctk", "fft1024"):
        t = audio.MelspecTables(*ac.CONFIGS[name])
        coef = np.random.default_rng(5).uniform(0.5, 2.0, (7, t.num_mels))
        mag = coef @ t.basis                                     # [7, NF], non-negative, in the row space
        S = 20.0 * np.log10(mag @ t.basis.T) - ac.REF_LEVEL_DB
        back = audio.mel_to_linear(t, S, ac.REF_LEVEL_DB)
        assert back.dtype == np.float64 and back.shape == mag.shape
        # (bins 0 and n_fft / 2 lie under no triangle: there the row space holds 0 and mel_to_linear returns its floor)
        assert np.abs(back - np.maximum(1e-10, mag)).max() <= 1e-9 * mag.max()
        assert np.abs(audio.mel_to_linear(t, S, ac.REF_LEVEL_DB, power=1.5) - np.maximum(1e-10, mag) ** 1.5).max() <= 1e-9 * mag.max() ** 1.5
        assert audio.mel_to_linear(t, np.full((2, t.num_mels), -300.0), ac.REF_LEVEL_DB).min() == 1e-10      # the floor


def test_audio_class_inverts_its_own_mel_spectrogram_on_the_numpy_backend():
    a = gc.lj_audio("numpy")
    gc.check_end_to_end(a)
    S = a.melspectrogram(ac.harmonic(3308, 22050, seed=3))
    assert np.abs(a.denormalize_mel(a.normalize_mel(S.T)) - S.T).max() <= 1e-4
    one = a.inv_melspectrogram(S, iters=2)
    assert a.inv_melspectrogram(S, iters=2).tobytes() == one.tobytes()                   # the seed fixes the initial phase
    assert a.inv_melspectrogram(S, iters=2, seed=1).tobytes() != one.tobytes()
    assert a.inv_melspectrogram_batch([S.T, S.T[:9]], iters=2)[0].tobytes() == one.tobytes()
    with pytest.raises(ValueError, match="frames=4"):
        a.inv_melspectrogram(S[:, :4])
