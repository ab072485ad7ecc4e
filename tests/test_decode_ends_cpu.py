"""CPU half of the per-utterance stop (csrc/decode_ends.hip): the export, the header declaration and the ctypes signature of
satt_dec_ends_scan agree, every refusal returns SATT_E_BADARG before anything is launched, and the NumPy model the GPU suites hold
the kernel against (tests/decode_ends_common.py: numpy_ends) agrees with the plain per-sample loop of the definition."""
import ctypes
import os
import re

import numpy as np
import pytest

import satt_amd  # noqa: F401
from decode_ends_common import MARGIN, ends_of_logits, logit, loop_ends, margin_ok, numpy_ends, pick_threshold, synthetic_yout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "satt_hip.h")
C_TYPES = {"const float*": ctypes.c_void_p, "int*": ctypes.c_void_p, "void*": ctypes.c_void_p, "int": ctypes.c_int, "float": ctypes.c_float}


def declaration(name):
    """(return type, [parameter types]) of `name` as include/satt_hip.h declares it"""
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, name + " is not declared"
    params = [re.sub(r"\s*\b\w+$", "", p.strip()).replace(" *", "*") for p in m.group(2).split(",")]
    return m.group(1), params


def test_export_header_and_signature_agree():
    from satt_amd import _lib
    ret, params = declaration("satt_dec_ends_scan")
    assert ret == "int" and len(params) == 11, params
    res, args = _lib.SIGNATURES["satt_dec_ends_scan"]
    assert res is ctypes.c_int and list(args) == [C_TYPES[p] for p in params], params
    # the sibling it follows: the same arguments with `ends` in front of `flag`
    ret2, params2 = declaration("satt_dec_stop_scan")
    assert params[:8] == params2[:8] and params[8:] == ["int*", "int*", "void*"] and params2[8:] == ["int*", "void*"]
    fn = _lib.lib().satt_dec_ends_scan          # resolved with the signature above
    assert fn.restype is ctypes.c_int
    from satt_amd import ops
    assert callable(ops.dec_ends_scan)


GOOD = dict(yout=4096, B=2, rows=9, NO=161, t0=0, nsteps=8, min_steps=0, thr=0.5, ends=8192, flag=12288)


@pytest.mark.parametrize("bad", [dict(yout=None), dict(ends=None), dict(flag=None), dict(B=0), dict(B=-1), dict(NO=0), dict(t0=-1),
                                 dict(nsteps=0), dict(nsteps=-3), dict(nsteps=9), dict(t0=1), dict(t0=8, nsteps=1),
                                 dict(t0=2 ** 31 - 1, nsteps=2 ** 31 - 1), dict(rows=8), dict(rows=0)])
def test_badarg_before_any_launch(bad):
    """fake addresses: a call that got as far as a launch would fault, a refusal never touches them (no GPU here)"""
    from satt_amd import _lib
    a = dict(GOOD, **bad)
    rc = _lib.lib().satt_dec_ends_scan(a["yout"], a["B"], a["rows"], a["NO"], a["t0"], a["nsteps"], a["min_steps"], a["thr"], a["ends"],
                                       a["flag"], None)
    assert rc == -1          # SATT_E_BADARG
    with pytest.raises(_lib.SattError):
        _lib.check(rc, "dec_ends_scan")


@pytest.mark.parametrize("seed", range(6))
def test_numpy_model_equals_the_plain_loop(seed):
    g = np.random.default_rng(seed)
    B, rows, NO = int(g.integers(1, 9)), 70, int(g.integers(1, 6))
    thr = float(g.uniform(0.2, 0.8))
    y = g.standard_normal((B, rows, NO)).astype(np.float32)
    y[:, :, -1] += np.float32(logit(thr) - 1.5)          # roughly one step in fifteen qualifies
    close = np.abs(y[:, :, -1].astype(np.float64) - logit(thr)) < MARGIN
    y[:, :, -1][close] -= np.float32(0.01)
    assert margin_ok(y[:, :, -1], thr)
    min_steps = int(g.integers(0, 20))
    e_np, f_np = np.zeros(B, np.int64), 0
    e_lp, f_lp = np.zeros(B, np.int64), 0
    t0, fired_at = 0, None
    while t0 < rows - 1:
        n = int(min(g.integers(1, 24), rows - 1 - t0))
        e_np, f_np = numpy_ends(y, t0, n, min_steps, thr, e_np, f_np)
        e_lp, f_lp = loop_ends(y, t0, n, min_steps, thr, e_lp, f_lp)
        assert np.array_equal(e_np, e_lp) and f_np == f_lp, (t0, n)
        assert ((e_np == 0) | (e_np > min_steps + 1)).all()
        if f_np and fired_at is None:
            fired_at = t0
            assert f_np == e_np.max() and t0 < f_np <= t0 + n          # it appears in the call in which the last sample ends
        t0 += n
    assert np.array_equal(np.where(e_np > 0, e_np, rows - 1), ends_of_logits(y[:, 1:, -1], min_steps, thr, rows - 1))


def test_numpy_model_edges():
    thr = 0.5
    g = np.random.default_rng(1)
    y = synthetic_yout(g, 3, 41, 5, thr, fires=[(0, 10), (0, 11), (1, 12), (1, 30), (2, 39)])
    z = np.zeros(3, np.int64)
    assert numpy_ends(y, 0, 40, 10, thr, z, 0)[0].tolist() == [12, 13, 40]          # t == min_steps does not fire, min_steps + 1 does
    assert numpy_ends(y, 0, 40, 10, thr, z, 0)[1] == 40
    e, f = numpy_ends(y, 0, 39, 10, thr, z, 0)          # a sample that never ends inside the window: no flag
    assert e.tolist() == [12, 13, 0] and f == 0
    e, f = numpy_ends(y, 0, 12, 9, thr, z, 0)
    assert e.tolist() == [11, 0, 0] and f == 0
    e, f = numpy_ends(y, 12, 8, 9, thr, e, f)          # sticky: sample 0 is not looked at again
    assert e.tolist() == [11, 13, 0] and f == 0
    e2, f2 = numpy_ends(y, 20, 20, 9, thr, e, 7)          # a non-zero flag: nothing changes
    assert e2.tolist() == e.tolist() and f2 == 7


def test_pick_threshold_meets_its_conditions():
    g = np.random.default_rng(3)
    logits = np.cumsum(g.normal(0.02, 0.05, (5, 80)), axis=1) - 2.0          # five slowly rising curves
    thr = pick_threshold(logits, 10, 32)
    assert thr is not None and margin_ok(logits, thr)
    e = ends_of_logits(logits, 10, thr, 0)
    assert len(set(e[e > 0].tolist())) >= 2 and e.max() > 32
    assert pick_threshold(np.zeros((3, 40)), 10, 8) is None
