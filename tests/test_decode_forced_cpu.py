"""Host side of forced alignments on the persistent decode kernel (csrc/decode_mega2.hip, template flag FRC; include/satt_hip.h:
satt_dec_mega_forced_params): the third block's layout, which instantiation a forced launch takes, and what the entry points
refuse.  No compute calls (there is no GPU here).
The forced instantiations are siblings of the GENERIC-width ones only: a block with the dimensions MEGA_VAR_LJ is keyed on runs
forced on its generic sibling, so the forced variant never carries MEGA_VAR_LJ - asserted below exactly as built.
FAILS ON THE PARENT, which has neither the block nor the entry points."""
import ctypes
import os
import subprocess

import pytest

import satt_amd  # noqa: F401
from decode_common import FAKE, LJ_KEYED, PRODUCTION, ROOT, SPEAKER, example_config, forced, medium_shape, options, shape_of


def test_forced_block_layout_matches_c(tmp_path):
    """sizeof / offsetof of the ctypes mirror == the C struct (compiled with the host compiler), the value of the variant bit, and
    the two frozen blocks did not grow"""
    from satt_amd import _lib, ops
    F = _lib.DecMegaForcedParams
    fields = [f[0] for f in F._fields_]
    assert fields == ["teach1", "teach2"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "satt_hip.h"\nint main() {\n  printf("%zu", sizeof(satt_dec_mega_forced_params));\n' + \
        "".join('  printf(" %%zu", offsetof(satt_dec_mega_forced_params, %s));\n' % f for f in fields) + \
        '  printf(" %d %zu %zu\\n", SATT_MEGA_VAR_FORCED, sizeof(satt_dec_mega_params), sizeof(satt_dec_mega_opt_params));\n  return 0; }\n'
    d = str(tmp_path)
    open(os.path.join(d, "t.c"), "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
    vals = list(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))
    assert vals == [ctypes.sizeof(F)] + [getattr(F, f).offset for f in fields] + \
        [ops.MEGA_VAR_FORCED, ctypes.sizeof(_lib.DecMegaParams), ctypes.sizeof(_lib.DecMegaOptParams)]
    assert ops.MEGA_VAR_FORCED == 256
    names = [f[0] for f in _lib.DecMegaParams._fields_]
    assert names[-4:] == ["nsteps", "Wp02", "bp02", "sproj"] and "teach1" not in names
    assert [f[0] for f in _lib.DecMegaOptParams._fields_][-1] == "drop_stream"
    f = forced()
    assert f.teach1 == FAKE and f.teach2 == FAKE + 64 and not forced(two=False).teach2


@pytest.mark.parametrize("widths", ["lj_keyed", "generic"])
@pytest.mark.parametrize("speaker", [False, True])
@pytest.mark.parametrize("B,Ti", [(1, 33), (1, 112), (1, 113), (1, 140), (2, 57), (2, 256)])
def test_forced_adds_its_bit_to_the_generic_variant(B, Ti, speaker, widths):
    """the shape list of tests/test_decode_options_cpu.py: forced_variant == opt_variant | FORCED without the LJ bit (no LJ sibling was built)"""
    from satt_amd import ops
    p = ops.dec_mega_params(B=B, Td=16, Ti=Ti, **(SPEAKER if speaker else {}), **(LJ_KEYED if widths == "lj_keyed" else PRODUCTION))
    plain = ops.dec_mega_opt_variant(p, None)
    assert bool(plain & ops.MEGA_VAR_LJ) == (widths == "lj_keyed")
    want = (plain & ~ops.MEGA_VAR_LJ) | ops.MEGA_VAR_FORCED
    assert ops.dec_mega_forced_variant(p, None, forced()) == want
    assert ops.dec_mega_forced_variant(p, options(False, False), forced()) == want
    assert ops.dec_mega_forced_variant(p, options(False, True), forced()) == want | ops.MEGA_VAR_DROPOUT
    # without teacher rows the call IS the option entry point
    for o in (None, options(False, False), options(True, False), options(False, True), options(True, True)):
        assert ops.dec_mega_forced_variant(p, o, None) == ops.dec_mega_opt_variant(p, o)
        assert ops.dec_mega_forced_variant(p, o, ops.dec_mega_forced_params(None, FAKE)) == ops.dec_mega_opt_variant(p, o)
    # the agent never runs under forced alignments; the dual form needs both histories
    assert ops.dec_mega_forced_variant(p, options(True, False), forced()) == -1
    assert ops.dec_mega_forced_variant(p, options(True, True), forced()) == -1
    assert ops.dec_mega_forced_variant(p, None, forced(two=False)) == -1


@pytest.mark.parametrize("example", ["ljspeech", "vctk"])
@pytest.mark.parametrize("speaker", [False, True])
def test_single_form_with_forced_alignments(example, speaker):
    from satt_amd import ops
    shape = shape_of(example_config(example))
    for B, Ti in ((1, 33), (1, 113), (2, 57)):
        p = ops.dec_mega_params(B=B, Td=16, Ti=Ti, **(SPEAKER if speaker else {}), **shape)
        plain = ops.dec_mega_variant(p)
        assert plain & ops.MEGA_VAR_SINGLE and not plain & ops.MEGA_VAR_LJ
        for f in (forced(), forced(two=False)):          # teach2 is never read in the single form
            assert ops.dec_mega_forced_variant(p, None, f) == plain | ops.MEGA_VAR_FORCED
            assert ops.dec_mega_forced_variant(p, None, f) & (ops.MEGA_VAR_SINGLE | ops.MEGA_VAR_FORCED) == ops.MEGA_VAR_SINGLE | ops.MEGA_VAR_FORCED
        for agent, dropout in ((True, False), (False, True), (True, True)):          # the single form takes no options, as ever
            assert ops.dec_mega_forced_variant(p, options(agent, dropout), forced()) == -1


@pytest.mark.parametrize("B,Ti,shape", [(3, 57, "production"), (1, 257, "production"), (2, 57, "medium"), (1, 33, "medium")])
def test_forced_does_not_widen_what_the_kernel_takes(B, Ti, shape):
    from satt_amd import ops
    p = ops.dec_mega_params(B=B, Td=16, Ti=Ti, **(PRODUCTION if shape == "production" else medium_shape()))
    assert ops.dec_mega_forced_variant(p, None, forced()) == -1
    assert ops.dec_mega_forced_variant(p, options(False, True), forced()) == -1


def test_launcher_refuses_before_it_launches():
    """the error codes of satt_dec_mega_forced for the refused pairs (returned before any GPU call is made)"""
    import ctypes as C
    from satt_amd import _lib, ops
    L = _lib.lib()
    p = ops.dec_mega_params(B=2, Td=16, Ti=57, nsteps=1, **PRODUCTION)
    f = forced()
    call = lambda o, ff: L.satt_dec_mega_forced(C.byref(p), None if o is None else C.byref(o), C.byref(ff), None)
    unsupported, badarg = L.satt_dec_mega_opt(C.byref(ops.dec_mega_params(B=3, Td=16, Ti=57, nsteps=1, **PRODUCTION)), None, None), call(None, f)
    assert unsupported != 0 and badarg != 0 and unsupported != badarg          # (NULL weight pointers: SATT_E_BADARG)
    assert call(options(True, False), f) == unsupported                       # agent + forced
    fakes = {n: FAKE for n, t in _lib.DecMegaParams._fields_ if t is C.c_void_p and n not in ("tin", "flag", "Wfh", "Wfl", "bfb", "Wp02", "bp02", "sproj")}
    q = ops.dec_mega_params(B=2, Td=16, Ti=57, nsteps=1, **PRODUCTION, **fakes)
    assert L.satt_dec_mega_forced(C.byref(q), None, C.byref(forced(two=False)), None) == badarg          # dual form, teach2 NULL
