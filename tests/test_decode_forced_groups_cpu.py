"""Host side of forced alignments in group mode of the persistent decode kernel (csrc/decode_mega2.hip, template flags GRP and FRC
together; include/satt_hip.h: satt_dec_mega_groups_forced, satt_dec_mega_groups_forced_variant): which instantiation a forced group
launch takes, what the entry points refuse and with which code, and that the three existing blocks kept their size.  No compute
calls (there is no GPU here): every launcher call below is one the launcher refuses before it touches the GPU.
EVERY TEST HERE FAILS ON THE PARENT: the symbols do not exist."""
import ctypes as C
import os
import subprocess

import pytest

import satt_amd  # noqa: F401
from decode_common import FAKE, FAMILIES, LJ_KEYED, PRODUCTION, ROOT, block, example_config, forced, groups, options

E_BADARG, E_UNSUPPORTED = -1, -2          # include/satt_hip.h: SATT_E_BADARG, SATT_E_UNSUPPORTED


def keyed(shape, n=2, opt=None, **kw):
    """n agreeing B = 2 blocks of a shape dictionary"""
    from satt_amd import ops
    blocks = []
    for _ in range(n):
        p = ops.dec_mega_params(**dict(dict(shape, B=2, Td=16, Ti=57), **kw))
        p.nsteps = 8
        blocks.append(p)
    return groups(blocks, opt)


@pytest.mark.parametrize("model,data", FAMILIES)
def test_forced_groups_variant_table(model, data):
    """dual and single form, speaker pre-net, dropout: the group variant without the LJ bit, plus the forced bit"""
    from satt_amd import ops
    c = example_config(model, data)
    assert ops.MEGA_VAR_FORCED | ops.MEGA_VAR_GROUPS == 384
    for n in (1, 2, 5, 8):
        arr = groups([block(c) for _ in range(n)])
        plain = ops.dec_mega_groups_variant(arr)
        assert plain > 0 and plain & ops.MEGA_VAR_GROUPS and plain & ops.MEGA_VAR_TWO_SAMPLES
        assert bool(plain & ops.MEGA_VAR_SINGLE) == (not c.dual) and bool(plain & ops.MEGA_VAR_SPEAKER) == bool(c.num_speakers)
        want = (plain & ~ops.MEGA_VAR_LJ) | ops.MEGA_VAR_FORCED
        assert ops.dec_mega_groups_forced_variant(arr, forced()) == want
        assert want & (ops.MEGA_VAR_FORCED | ops.MEGA_VAR_GROUPS) == ops.MEGA_VAR_FORCED | ops.MEGA_VAR_GROUPS and not want & ops.MEGA_VAR_LJ
        # teach2: the dual form needs it, the single form never reads it
        assert ops.dec_mega_groups_forced_variant(arr, forced(two=False)) == (-1 if c.dual else want)
        # without teacher rows the call IS the group entry point
        assert ops.dec_mega_groups_forced_variant(arr, None) == plain
        assert ops.dec_mega_groups_forced_variant(arr, ops.dec_mega_forced_params(None, FAKE)) == plain
    # options: dropout rides along in the dual form, the agent is refused, the single form takes none
    for agent, dropout in ((False, True), (True, False), (True, True)):
        arr = groups([block(c), block(c), block(c)], options(agent, dropout))
        plain = ops.dec_mega_groups_variant(arr)
        assert ops.dec_mega_groups_forced_variant(arr, None) == plain
        if c.dual and not agent:
            assert ops.dec_mega_groups_forced_variant(arr, forced()) == (plain & ~ops.MEGA_VAR_LJ) | ops.MEGA_VAR_FORCED
            assert ops.dec_mega_groups_forced_variant(arr, forced()) & ops.MEGA_VAR_DROPOUT
        else:
            assert ops.dec_mega_groups_forced_variant(arr, forced()) == -1


def test_an_lj_keyed_block_runs_forced_on_its_generic_sibling():
    from satt_amd import ops
    lj, gen = keyed(LJ_KEYED, 3), keyed(PRODUCTION, 3)
    assert ops.dec_mega_groups_variant(lj) & ops.MEGA_VAR_LJ and not ops.dec_mega_groups_variant(gen) & ops.MEGA_VAR_LJ
    assert ops.dec_mega_groups_forced_variant(lj, forced()) == ops.dec_mega_groups_forced_variant(gen, forced())
    assert ops.dec_mega_groups_forced_variant(lj, forced()) == ops.dec_mega_groups_variant(gen) | ops.MEGA_VAR_FORCED
    assert ops.dec_mega_groups_forced_variant(lj, None) == ops.dec_mega_groups_variant(lj)          # f == NULL: the LJ kernel, as ever


def test_forced_groups_does_not_widen_what_a_group_launch_takes():
    from satt_amd import ops
    L = satt_amd._lib.lib()
    f = forced()
    nine = keyed(PRODUCTION, 9)
    assert L.satt_dec_mega_groups_forced_variant(nine, 9, C.byref(f)) == -1
    assert L.satt_dec_mega_groups_forced_variant(nine, 0, C.byref(f)) == -1
    assert L.satt_dec_mega_groups_forced_variant(nine, 8, C.byref(f)) > 0
    assert L.satt_dec_mega_groups_forced_variant(None, 2, C.byref(f)) == -1
    a, b = keyed(PRODUCTION, 1), keyed(PRODUCTION, 1, Ti=58)
    disagree = groups([a[0].p, b[0].p])
    assert ops.dec_mega_groups_forced_variant(disagree, f) == -1
    one_sample = ops.dec_mega_params(B=1, Td=16, Ti=57, nsteps=8, **PRODUCTION)
    assert ops.dec_mega_groups_forced_variant(groups([one_sample]), f) == -1
    assert ops.dec_mega_groups_forced_variant(keyed(PRODUCTION, 2, A=64), f) == -1


def test_launcher_refusals_and_their_codes():
    """every call returns before a GPU call is made: the codes of satt_dec_mega_groups_forced for what it refuses"""
    from satt_amd import _lib, ops
    L = _lib.lib()
    f, dev = forced(), C.c_void_p(FAKE)
    call = lambda arr, n, ff: L.satt_dec_mega_groups_forced(arr, dev, n, None if ff is None else C.byref(ff), None)
    # the agent (on in every block: the blocks agree)
    assert call(keyed(PRODUCTION, 2, options(True, False)), 2, f) == E_UNSUPPORTED
    assert call(keyed(PRODUCTION, 2, options(True, True)), 2, f) == E_UNSUPPORTED
    # nine groups, zero groups, blocks that disagree, no blocks
    nine = keyed(PRODUCTION, 9)
    assert call(nine, 9, f) == E_UNSUPPORTED and call(nine, 0, f) == E_UNSUPPORTED and call(None, 2, f) == E_UNSUPPORTED
    a, b = keyed(PRODUCTION, 1), keyed(PRODUCTION, 1, Ti=58)
    assert call(groups([a[0].p, b[0].p]), 2, f) == E_UNSUPPORTED
    # the dual form without teach2 - with every other pointer in place, so nothing else is the reason
    fakes = {n: FAKE for n, t in _lib.DecMegaParams._fields_ if t is C.c_void_p and n not in ("tin", "flag", "Wfh", "Wfl", "bfb", "Wp02", "bp02", "sproj")}
    whole = keyed(dict(PRODUCTION, **fakes), 1)
    assert ops.dec_mega_groups_forced_variant(whole, forced(two=False)) == -1
    assert call(whole, 1, forced(two=False)) == E_BADARG
    # a block with the stop flag set (one group, every other pointer in place)
    flagged = keyed(dict(PRODUCTION, **fakes), 1, flag=FAKE)
    assert ops.dec_mega_groups_forced_variant(flagged, f) > 0          # (the variant is a matter of shapes)
    assert call(flagged, 1, f) == E_BADARG
    # two groups that share their exchange region, step words and state
    assert call(keyed(dict(PRODUCTION, **fakes), 2), 2, f) == E_BADARG
    # no device copy of the blocks
    assert L.satt_dec_mega_groups_forced(whole, None, 1, C.byref(f), None) == E_BADARG
    # f == NULL: the call IS satt_dec_mega_groups - and refuses what that refuses
    assert call(nine, 9, None) == L.satt_dec_mega_groups(nine, dev, 9, None) == E_UNSUPPORTED
    assert call(flagged, 1, None) == L.satt_dec_mega_groups(flagged, dev, 1, None) == E_BADARG


def test_the_existing_blocks_kept_their_size_and_the_header_declares_the_symbols(tmp_path):
    from satt_amd import _lib, ops
    src = '#include <stdio.h>\n#include "satt_hip.h"\n' \
          'int (*v)(const satt_dec_mega_group*, int, const satt_dec_mega_forced_params*) = satt_dec_mega_groups_forced_variant;\n' \
          'int (*l)(const satt_dec_mega_group*, const void*, int, const satt_dec_mega_forced_params*, void*) = satt_dec_mega_groups_forced;\n' \
          'int main() { printf("%zu %zu %zu %zu %d\\n", sizeof(satt_dec_mega_params), sizeof(satt_dec_mega_opt_params), ' \
          'sizeof(satt_dec_mega_forced_params), sizeof(satt_dec_mega_group), SATT_MEGA_VAR_FORCED | SATT_MEGA_VAR_GROUPS); return v == 0 || l == 0; }\n'
    d = str(tmp_path)
    open(os.path.join(d, "t.c"), "w").write(src)
    # (compiled, not linked: the two initialisers only compile if the header declares the symbols with these signatures)
    subprocess.check_call(["gcc", "-c", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
    sizes = 'int main() { printf("%zu %zu %zu %zu\\n", sizeof(satt_dec_mega_params), sizeof(satt_dec_mega_opt_params), ' \
            'sizeof(satt_dec_mega_forced_params), sizeof(satt_dec_mega_group)); return 0; }\n'
    open(os.path.join(d, "s.c"), "w").write('#include <stdio.h>\n#include "satt_hip.h"\n' + sizes)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
    vals = list(map(int, subprocess.check_output([os.path.join(d, "s")]).split()))
    assert vals == [C.sizeof(_lib.DecMegaParams), C.sizeof(_lib.DecMegaOptParams), C.sizeof(_lib.DecMegaForcedParams), C.sizeof(_lib.DecMegaGroup)]
    # the sizes the parent commit had (x86-64): the frozen blocks did not grow
    assert vals == [528, 64, 16, 600]
    assert [f[0] for f in _lib.DecMegaParams._fields_][-4:] == ["nsteps", "Wp02", "bp02", "sproj"]
    assert [f[0] for f in _lib.DecMegaGroup._fields_] == ["p", "o", "has_opt", "b0"]
    # exported by the library
    lib = C.CDLL(os.path.join(ROOT, "self-attention-tacotron_amd", "libsatt_hip.so"))
    for name in ("satt_dec_mega_groups_forced", "satt_dec_mega_groups_forced_variant"):
        assert getattr(lib, name) is not None and hasattr(_lib.lib(), name)
    assert callable(ops.dec_mega_groups_forced) and callable(ops.dec_mega_groups_forced_variant)
