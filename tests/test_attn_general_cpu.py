"""Host-side acceptance rule of the single-workgroup attention kernels (satt_attn_rnn_check, csrc/attn_rnn.hip): every
first-source option and the sentence lengths whose bf16 key image does not fit LDS are taken; attention_filters != 5 and
forced alignments stay refused.  No launch: runs without a GPU."""
import ctypes

import pytest

import satt_amd  # noqa: F401
from satt_amd import _lib, ops

OK, BADARG, UNSUPPORTED = 0, -1, -2
PTR = 1 << 12          # a non-NULL stand-in: the check never dereferences device pointers

PRODUCTION = dict(A=256, U1=224, V1=256, U2=32, V2=32)
MEDIUM = dict(A=64, U1=72, V1=80, U2=16, V2=16)


def params(dims=PRODUCTION, B=2, Td=4, Ti=64, bf16=0, **kw):
    return ops.attn_rnn_params(B=B, Td=Td, Ti=Ti, kernel=10, filters=5, training=1, keys_lds_bf16=bf16, **{**dims, **kw})


def check(p):
    return _lib.lib().satt_attn_rnn_check(ctypes.byref(p))


def lds_floats_bwd(dims, Ti, klds, F=5, KW=10, ANT=512):
    """carve_bwd of csrc/attn_rnn.hip"""
    u = lambda x: (x + 3) & ~3
    A, CT, UQ = dims["A"], dims["V1"] + dims["V2"], dims["U1"] + dims["U2"]
    o = 4 * A + u(CT + A) + u(A) + 2 * u(UQ) + u(CT) + 9 * u(Ti) + 2 * u(Ti * F) + u(KW * F) + ANT * 8 + 4
    return o + (u((Ti * UQ + 1) // 2) if klds else 0)


@pytest.mark.parametrize("dims", [PRODUCTION, MEDIUM])
@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("opts", [dict(), dict(att1_mode=1), dict(att1_mode=1, cumulative=1, acum=PTR), dict(cumulative=1, acum=PTR),
                                  dict(agentW=PTR, agentb=PTR, ustate=PTR),
                                  dict(agentW=PTR, agentb=PTR, ustate=PTR, cumulative=1, acum=PTR)])
def test_every_first_source_option_is_accepted(dims, bf16, opts):
    assert check(params(dims, bf16=bf16, **opts)) == OK


def test_incomplete_option_blocks_are_bad_arguments():
    assert check(params(cumulative=1)) == BADARG                      # no acum
    assert check(params(agentW=PTR)) == BADARG                        # no agentb / ustate
    assert check(params(att1_mode=2)) == BADARG


def test_a_sentence_whose_bf16_keys_do_not_fit_lds_is_accepted():
    """production widths, Ti = 400: the backward carve with the bf16 key image is over the 160 KB the launchers may ask for -
    the kernels then read the keys from global memory and round them on load"""
    assert 4 * lds_floats_bwd(PRODUCTION, 64, True) <= 160 * 1024
    assert 4 * lds_floats_bwd(PRODUCTION, 400, True) > 160 * 1024
    assert 4 * lds_floats_bwd(PRODUCTION, 400, False) <= 160 * 1024
    for Ti in (64, 400, 1000):
        assert check(params(Ti=Ti, bf16=1)) == OK, Ti
        assert check(params(Ti=Ti, bf16=0)) == OK, Ti
    assert check(params(Ti=4000, bf16=1)) == UNSUPPORTED               # beyond one workgroup's LDS in any key form


def test_filters_and_forced_alignments_stay_refused():
    p = params()
    p.filters = 8
    assert check(p) == UNSUPPORTED
    assert check(params(teach1=PTR, teach2=PTR)) == UNSUPPORTED
    assert check(params(att1_mode=1, teach1=PTR, teach2=PTR)) == UNSUPPORTED
    assert _lib.lib().satt_attn_rnn_check(None) == BADARG


def test_the_parameter_blocks_kept_their_layout():
    """this change appends nothing: the first-source option block and the backward block end where they ended"""
    A, Bp = _lib.AttnRnnParams, _lib.AttnRnnBwdParams
    names = [n for n, _ in A._fields_]
    assert names[-7:] == ["att1_mode", "cumulative", "acum", "agentW", "agentb", "ustate", "saf"]
    assert names.index("acum") < names.index("agentW") < names.index("ustate") < names.index("saf") == len(names) - 1
    assert [n for n, _ in Bp._fields_][-2:] == ["dfl", "dz"]
    assert Bp.dz.offset + ctypes.sizeof(ctypes.c_void_p) == ctypes.sizeof(Bp)
    assert A.saf.offset + ctypes.sizeof(ctypes.c_void_p) == ctypes.sizeof(A)
