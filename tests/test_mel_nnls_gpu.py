"""csrc/mel_nnls.hip against the float32 NumPy backend (equal bit for bit), its launch guarantees, what it writes (poisoned output with
guard rows), LDS poison, the float64 bar of tests/mel_nnls_common.py, refusals, and the Python surface and drivers over it.  No test
feeds the kernel a corrupted table: the bounding of table-derived indices is checked by review."""
import json
import os

import numpy as np
import pytest
import torch

import audio_common as ac
import griffin_lim_common as gc
import mel_nnls_common as mc
import satt_amd  # noqa: F401
from satt_amd import _lib, ops
from satt_amd.utils import audio

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 3
POISON = 0x7FC12345                     # a NaN with a payload: an output word left alone keeps exactly these bits
KS = (1, 2, 3, 64)
TILED = 257                             # frames: no multiple of anything a workgroup could take


def nnls_tables(name):
    return audio.mel_nnls_tables(mc.tables(name))


_REF = {}


def reference(name, iters):
    """the NumPy backend's result over inputs(name), computed once and left unchanged"""
    if (name, iters) not in _REF:
        a, x0 = mc.inputs(name)
        x = audio.mel_nnls_numpy(nnls_tables(name), a, x0, iters)
        x.setflags(write=False)
        _REF[name, iters] = x
    return _REF[name, iters]


def launch(nt, a, x0, iters):
    """one launch into a poisoned buffer with GUARD rows on either side: (result [N, F], the whole buffer as uint32)"""
    N, F = x0.shape
    d = nt.device(DEV)
    buf = torch.full((N + 2 * GUARD, F), POISON, dtype=torch.int32, device=DEV).view(torch.float32)
    ops.mel_nnls(torch.from_numpy(np.array(a, np.float32)).to(DEV), torch.from_numpy(np.array(x0, np.float32)).to(DEV),
                 torch.from_numpy(np.array(nt.beta(iters))).to(DEV), float(nt.step), d["band_start"], d["band_offset"],
                 d["band_weight"], d["bin_first"], d["bin_offset"], d["bin_weight"], buf[GUARD:GUARD + N])
    torch.cuda.synchronize()
    raw = buf.view(torch.int32).cpu().numpy().view(np.uint32)
    return raw[GUARD:GUARD + N].view(np.float32).copy(), raw


def tiled(x, n):
    return np.tile(x, (-(-n // len(x)), 1))[:n]


# ---- the kernel against the NumPy backend --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", KS)
@pytest.mark.parametrize("name", mc.NAMES)
def test_kernel_equals_the_numpy_backend(name, iters):
    nt = nnls_tables(name)
    a, x0 = mc.inputs(name)
    want = reference(name, iters)
    got, _ = launch(nt, a, x0, iters)                                                   # the 5 - 9 frame cases concatenated
    assert got.tobytes() == want.tobytes()
    one, _ = launch(nt, a[4:5], x0[4:5], iters)                                          # N = 1
    assert one.tobytes() == want[4:5].tobytes()
    many, _ = launch(nt, tiled(a, TILED), tiled(x0, TILED), iters)
    assert many.tobytes() == tiled(want, TILED).tobytes()


@pytest.mark.parametrize("kind", mc.HAND)
def test_hand_made_tables_equal_the_numpy_backend(kind):
    """an empty band, a band of one bin, a bin under three and under five bands, two rounds of teams, and weights read from global memory"""
    nt, _, a, x0 = mc.hand(kind)
    for iters in KS:
        got, _ = launch(nt, a, x0, iters)
        assert got.tobytes() == audio.mel_nnls_numpy(nt, a, x0, iters).tobytes(), (kind, iters)


def test_a_nan_and_an_inf_amplitude_stay_in_their_frame():
    for name in ("ljspeech", "fft512_hop_beyond_window"):
        nt = nnls_tables(name)
        bad, good, x0 = mc.nonfinite_frames(name)
        for iters in (1, 2, 64):
            got, _ = launch(nt, bad, x0, iters)
            assert got.tobytes() == audio.mel_nnls_numpy(nt, bad, x0, iters).tobytes()
            clean, _ = launch(nt, good, x0, iters)
            assert got[[0, 2]].tobytes() == clean[[0, 2]].tobytes() and not np.isnan(got).any()


def test_silent_frames():
    for level_db in (-300.0, -100.0):
        a, x0 = mc.level_frames("vctk", level_db)
        got, _ = launch(nnls_tables("vctk"), a, x0, 64)
        assert np.isfinite(got).all() and got.tobytes() == audio.mel_nnls_numpy(nnls_tables("vctk"), a, x0, 64).tobytes()


# ---- launch behaviour -----------------------------------------------------------------------------------------------------------------
def test_launches_are_reproducible_and_frames_independent():
    name = "ljspeech"
    nt = nnls_tables(name)
    a, x0 = mc.inputs(name)
    want = reference(name, 64)
    whole, raw = launch(nt, a, x0, 64)
    again, raw2 = launch(nt, a, x0, 64)
    assert raw.tobytes() == raw2.tobytes() and whole.tobytes() == want.tobytes()        # two launches: identical bits
    cut = 17
    first, _ = launch(nt, a[:cut], x0[:cut], 64)
    second, _ = launch(nt, a[cut:], x0[cut:], 64)
    assert np.concatenate([first, second]).tobytes() == whole.tobytes()                 # a batch split into two launches
    back, _ = launch(nt, a[::-1], x0[::-1], 64)
    assert back[::-1].tobytes() == whole.tobytes()                                      # a frame's place does not matter
    for n in (0, 20, len(a) - 1):
        alone, _ = launch(nt, a[n:n + 1], x0[n:n + 1], 64)
        assert alone.tobytes() == whole[n:n + 1].tobytes()


@pytest.mark.parametrize("name", ["fft512_hop_beyond_window", "vctk"])
def test_every_output_row_is_written_and_the_guards_are_intact(name):
    nt = nnls_tables(name)
    a, x0 = mc.inputs(name)
    got, raw = launch(nt, a, x0, 2)
    assert raw.shape == (len(a) + 2 * GUARD, nt.num_bins)
    assert np.all(raw[:GUARD] == POISON) and np.all(raw[GUARD + len(a):] == POISON)
    assert not np.any(raw[GUARD:GUARD + len(a)] == POISON) and got.tobytes() == reference(name, 2).tobytes()


# ---- LDS poison ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", [0x7FC00000, 0x7F800000, 0xFF800000, 0x3F800000], ids=["nan", "inf", "minus_inf", "one"])
def test_bits_do_not_depend_on_what_lds_held(pattern):
    """satt_debug_poison_lds leaves the pattern in every LDS word of every CU in front of the launch: a y, an r, an amplitude, a band
    entry or a weight read before the kernel wrote it changes the sums"""
    for name in ("fft512_hop_beyond_window", "ljspeech", "vctk"):
        a, x0 = mc.inputs(name)
        _lib.check(_lib.lib().satt_debug_poison_lds(pattern, 100, ops.current_stream().cuda_stream), "poison_lds")
        got, _ = launch(nnls_tables(name), a, x0, 3)
        assert got.tobytes() == reference(name, 3).tobytes(), name
    for kind in ("odd", "dense"):
        nt, _, a, x0 = mc.hand(kind)
        _lib.check(_lib.lib().satt_debug_poison_lds(pattern, 100, ops.current_stream().cuda_stream), "poison_lds")
        got, _ = launch(nt, a, x0, 3)
        assert got.tobytes() == audio.mel_nnls_numpy(nt, a, x0, 3).tobytes(), kind


# ---- float64 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.NAMES)
def test_kernel_meets_the_float64_bar(name):
    a, x0 = mc.inputs(name)
    for iters in mc.KS:
        got, _ = launch(nnls_tables(name), a, x0, iters)
        err = mc.frame_errors(got, mc.yardstick_of(name, iters))
        print("%s K=%d: worst frame %.3e of the frame maximum (bar %.3e)" % (name, iters, err.max(), mc.C))
        assert err.max() <= mc.C
    assert mc.residuals(mc.dense_of(name), got, a).max() <= mc.RESIDUAL_BOUND


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    nt = nnls_tables("fft1024")
    a, x0 = mc.inputs("fft1024")
    d = nt.device(DEV)
    out = torch.full(x0.shape, -77.25, device=DEV)
    ta, tx = torch.from_numpy(a.copy()).to(DEV), torch.from_numpy(x0.copy()).to(DEV)
    tabs = [d[k] for k in ("band_start", "band_offset", "band_weight", "bin_first", "bin_offset", "bin_weight")]
    for iters in (0, 1025):
        with pytest.raises(ValueError):
            ops.mel_nnls(ta, tx, torch.zeros(iters, device=DEV), float(nt.step), *tabs, out)
    with pytest.raises(ValueError):
        ops.mel_nnls(ta[:0], tx[:0], torch.zeros(4, device=DEV), float(nt.step), *tabs, out[:0])
    beta = torch.zeros(4, device=DEV)
    for kw in (dict(step=0.0), dict(step=float("nan")), dict(amp=None), dict(out=None), dict(bin_weight=None), dict(n_tweights=0), dict(num_mels=129),
               dict(n_frames=0)):
        f = dict(num_bins=513, num_mels=40, iters=4, n_weights=len(nt.band_weight), n_tweights=len(nt.bin_weight), step=float(nt.step),
                 n_frames=len(a), amp=ta.data_ptr(), start=tx.data_ptr(), beta=beta.data_ptr(), band_start=tabs[0].data_ptr(),
                 band_offset=tabs[1].data_ptr(), band_weight=tabs[2].data_ptr(), bin_first=tabs[3].data_ptr(), bin_offset=tabs[4].data_ptr(),
                 bin_weight=tabs[5].data_ptr(), out=out.data_ptr())
        f.update(kw)
        with pytest.raises(_lib.SattError):
            _lib.check(_lib.lib().satt_mel_nnls(_lib.C.byref(_lib.MelNnlsParams(**f)), ops._s()), "mel_nnls")
    torch.cuda.synchronize()
    assert bool((out == -77.25).all())


# ---- the public surface --------------------------------------------------------------------------------------------------------------
def test_mel_nnls_hip_and_its_launch_groups():
    name = "fft1024"
    nt = nnls_tables(name)
    a, x0 = mc.inputs(name)
    want = reference(name, 3)
    assert audio.mel_nnls_hip(nt, a, x0, 3, DEV).tobytes() == want.tobytes()
    for group in (1, 7, len(a), len(a) + 5):
        assert audio.mel_nnls_hip(nt, a, x0, 3, DEV, max_launch_frames=group).tobytes() == want.tobytes()
    S = np.concatenate(mc.mels(name))
    t = mc.tables(name)
    got = audio.mel_to_linear(t, S, 20.0, 1.5, inversion="nnls", nnls_iters=3, backend="hip", device=DEV)
    assert got.tobytes() == audio.mel_to_linear(t, S, 20.0, 1.5, inversion="nnls", nnls_iters=3).tobytes()


def test_inv_melspectrogram_batch_on_hip():
    h, n = gc.lj_audio("hip"), gc.lj_audio("numpy")
    Ss = [audio.melspec_numpy(n.tables, ac.harmonic(m, 22050, seed=20 + i), 20.0) for i, m in enumerate(gc.MEL_DIR_SAMPLES)]
    mh, mn = h.mel_to_linear_batch(Ss, inversion="nnls"), n.mel_to_linear_batch(Ss, inversion="nnls")
    assert all(x.tobytes() == y.tobytes() and x.shape == (len(S), 1025) for x, y, S in zip(mh, mn, Ss))   # what Griffin-Lim is handed
    plain = n.mel_to_linear_batch(Ss)
    assert all(x.tobytes() != y.tobytes() for x, y in zip(mn, plain))
    wavs = h.inv_melspectrogram_batch(Ss, iters=4, inversion="nnls")
    base = h.inv_melspectrogram_batch(Ss, iters=4)
    for w, b, S in zip(wavs, base, Ss):
        assert w.dtype == np.float32 and w.shape == ((len(S) - 1) * 275,) and np.isfinite(w).all() and w.tobytes() != b.tobytes()
    dist = [mc.round_trip(h, 3, inversion=inv) for inv in ("pinv", "nnls")]
    print("mean |dB| difference behind 30 Griffin-Lim iterations on hip: %.3f with pinv, %.3f with nnls" % tuple(dist))
    assert dist[1] < 0.8 * dist[0]


def test_drivers_on_the_hip_backend(tmp_path):
    cfg, mel_dir, _ = gc.write_mel_dir(tmp_path)
    out = str(tmp_path / "wav")
    ac.run_driver("mel_to_wav.py", "--hparam-json-file", cfg, "--backend", "hip", "--iters", "4", "--inversion", "nnls", mel_dir, out)
    gc.check_wav_dir(out)
    import test_yin_cpu as tc
    stats = tc.write_stats(str(tmp_path / "stats.json"))
    pred, out = str(tmp_path / "pred"), str(tmp_path / "f0")
    records = tc.write_toy_records(pred)
    ac.run_driver("evaluate_f0.py", "--hparam-json-file", stats, "--backend", "hip", "--iters", "4", "--seed", "3", "--inversion", "nnls", pred, out)
    keys = [k for k in sorted(records) if records[k][1] is not None]
    au = audio.Audio(tc.toy_hparams(), backend="hip", device=DEV)
    mp, mr = [records[k][0] for k in keys], [records[k][1] for k in keys]
    wavs = au.inv_melspectrogram_batch([au.denormalize_mel(S.astype(np.float64)) for S in mp + mr], iters=4, seed=3, inversion="nnls")
    want, _, _ = tc.expected(au, keys, wavs[:3], wavs[3:], mp, mr)
    assert tc.read_csv(os.path.join(out, "f0_distance.csv")) == want
    s = json.load(open(os.path.join(out, "summary.json")))
    tc.check_summary(s, want, "griffin_lim", ["utt002"])
    assert (s["inversion"], s["nnls_iters"]) == ("nnls", 64)


def test_predict_mel_wav_with_the_non_negative_inversion(tmp_path):
    """predict_mel.py --wav --inversion nnls: the wav is Audio's inversion of the .mfbsp written beside it"""
    from satt_amd.hparams import hparams
    from satt_amd.models.models import tacotron_model_factory
    from satt_amd.utils import tfrecord
    data, lists, ckpt, out = tmp_path / "data", tmp_path / "lists", tmp_path / "ckpt", tmp_path / "out"
    for d in (data, lists, ckpt):
        d.mkdir()
    s = np.concatenate([[0], np.random.default_rng(0).integers(1, 60, 9), [0]]).astype("<i8")
    tfrecord.write_records(str(data / "LJ000.source.tfrecord"), [tfrecord.make_example(
        {"id": 0, "key": b"LJ000", "source": s.tobytes(), "source_length": len(s), "text": b"abc"})])
    (lists / "test.csv").write_text("LJ000\n")
    d = json.load(open(ac.LJ_JSON))
    d.pop("_comment", None)
    d.update(average_mel_level_db=[-40.0], stddev_mel_level_db=[10.0])
    cfg = str(tmp_path / "hparams.json")
    json.dump(d, open(cfg, "w"))
    hp = hparams.copy()
    hp.parse_json(json.dumps(d))
    tacotron_model_factory(hp, str(ckpt), device="cuda").save()                    # model-0.pt: the initial parameters
    ac.run_driver("predict_mel.py", "--output-dir", str(out), "--wav", "--griffin-lim-iters", "4", "--inversion", "nnls", "--nnls-iters", "8",
                  "--source-data-root", str(data), "--checkpoint-dir", str(ckpt), "--selected-list-dir", str(lists), "--hparam-json-file", cfg,
                  "--hparams", "max_iters=12")
    mel = np.fromfile(str(out / "LJ000.mfbsp"), "<f4").reshape(-1, 80)
    au = audio.Audio(hp, backend="hip", device=DEV)
    rate, pcm = gc.read_wav(str(out / "LJ000.wav"))
    assert rate == 22050 and len(pcm) == (len(mel) - 1) * 275
    for inv, same in (("nnls", True), ("pinv", False)):
        w = au.inv_melspectrogram(au.denormalize_mel(mel).T, iters=4, inversion=inv, nnls_iters=8).astype(np.float64)
        assert np.array_equal(pcm, np.round(w * (0.95 * 32767.0 / np.abs(w).max())).astype(np.int16)) == same
