"""Host side of the group mode of the persistent decode kernel (include/satt_hip.h: satt_dec_mega_group, satt_dec_mega_groups_*;
csrc/decode_mega2.hip): which arrays of B = 2 blocks a group launch takes, which instantiation they get, the layout of the block, and
that nothing of the single-launch contract moved.  No compute calls (there is no GPU here).
EVERY TEST HERE FAILS ON THE PARENT: the symbols do not exist."""
import ctypes as C
import os
import subprocess

import pytest

import satt_amd  # noqa: F401
from decode_common import FAMILIES, ROOT, SPEAKER, block, example_config, groups, options, shape_of

@pytest.mark.parametrize("model,data", FAMILIES)
def test_groups_supported_truth_table(model, data):
    from satt_amd import ops
    c = example_config(model, data)
    for n in (1, 2, 8):
        arr = groups([block(c) for _ in range(n)])
        assert ops.dec_mega_groups_supported(arr), n
    # the group count
    lib = satt_amd._lib.lib()
    nine = groups([block(c) for _ in range(9)])
    assert lib.satt_dec_mega_groups_supported(nine, 9) == 0 and lib.satt_dec_mega_groups_variant(nine, 9) == -1
    assert lib.satt_dec_mega_groups_supported(nine, 0) == 0 and lib.satt_dec_mega_groups_variant(nine, 0) == -1
    assert lib.satt_dec_mega_groups_supported(nine, 8) == 1
    assert lib.satt_dec_mega_groups_supported(None, 2) == 0
    # a block with one sample; blocks that disagree in Ti, in the form, in nsteps; a block satt_dec_mega_supported refuses
    assert ops.dec_mega_supported(block(c, B=1))
    single = dict(Ds=0, heads=0, U2=0, V2=0)
    other_form = block(c, Ds=256, heads=2, U2=32, V2=32, U1=224) if not c.dual else block(c, **single)
    assert ops.dec_mega_supported(other_form)
    unsupported = block(c, A=64)
    assert not ops.dec_mega_supported(unsupported)
    no_speaker = ops.dec_mega_params(B=2, Td=16, Ti=57, **shape_of(c)) if c.num_speakers else ops.dec_mega_params(B=2, Td=16, Ti=57, **SPEAKER, **shape_of(c))
    no_speaker.nsteps = 8
    for bad in (block(c, B=1), block(c, Ti=58), other_form, block(c, nsteps=9), unsupported, no_speaker, block(c, B=3)):
        for arr in (groups([block(c), bad]), groups([bad, block(c)]), groups([block(c), block(c), bad, block(c)])):
            assert not ops.dec_mega_groups_supported(arr) and ops.dec_mega_groups_variant(arr) == -1
    assert not ops.dec_mega_groups_supported(groups([block(c, B=1)])) and not ops.dec_mega_groups_supported(groups([unsupported]))


@pytest.mark.parametrize("model,data", FAMILIES)
def test_groups_variant_is_the_two_sample_variant_of_the_block(model, data):
    from satt_amd import ops
    c = example_config(model, data)
    for Ti in (7, 57, 256):
        p = block(c, Ti=Ti)
        want = ops.dec_mega_variant(p)
        assert want > 0 and want & ops.MEGA_VAR_TWO_SAMPLES and not want & ops.MEGA_VAR_TABLES_LDS
        assert bool(want & ops.MEGA_VAR_SINGLE) == (not c.dual) and bool(want & ops.MEGA_VAR_SPEAKER) == bool(c.num_speakers)
        for n in (1, 3, 8):
            assert ops.dec_mega_groups_variant(groups([block(c, Ti=Ti) for _ in range(n)])) == want | ops.MEGA_VAR_GROUPS
    assert ops.MEGA_VAR_GROUPS == 128


@pytest.mark.parametrize("model,data", FAMILIES)
def test_groups_with_options(model, data):
    """the dual form takes the options of its blocks (every group the same ones); the single form takes none"""
    from satt_amd import ops
    c = example_config(model, data)
    plain = ops.dec_mega_variant(block(c))
    for agent, dropout in ((True, False), (False, True), (True, True)):
        o = options(agent, dropout)
        arr = groups([block(c), block(c)], o)
        if c.dual:
            want = plain | (ops.MEGA_VAR_AGENT if agent else 0) | (ops.MEGA_VAR_DROPOUT if dropout else 0) | ops.MEGA_VAR_GROUPS
            assert ops.dec_mega_opt_variant(block(c), o) | ops.MEGA_VAR_GROUPS == want
            assert ops.dec_mega_groups_variant(arr) == want
            mixed = ops.dec_mega_groups_blocks([(block(c), o, 0), (block(c), None, 2)])
            assert ops.dec_mega_groups_variant(mixed) == -1
        else:
            assert ops.dec_mega_groups_variant(arr) == -1
    assert ops.dec_mega_groups_variant(groups([block(c), block(c)], options(False, False))) == plain | ops.MEGA_VAR_GROUPS


def test_group_block_layout_matches_the_header(tmp_path):
    from satt_amd import _lib, ops
    fields = ["p", "o", "has_opt", "b0"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "satt_hip.h"\nint main() { printf("%d %d %zu %zu %zu", SATT_MEGA_VAR_GROUPS, SATT_MEGA_GROUPS_MAX, ' \
          'sizeof(satt_dec_mega_group), sizeof(satt_dec_mega_params), sizeof(satt_dec_mega_opt_params));\n' + \
          "".join('printf(" %%zu", offsetof(satt_dec_mega_group, %s));\n' % f for f in fields) + 'printf("\\n"); return 0; }\n'
    d = str(tmp_path)
    open(os.path.join(d, "t.c"), "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
    vals = list(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))
    G = _lib.DecMegaGroup
    assert vals == [ops.MEGA_VAR_GROUPS, ops.MEGA_GROUPS_MAX, C.sizeof(G), C.sizeof(_lib.DecMegaParams), C.sizeof(_lib.DecMegaOptParams)] + \
        [getattr(G, f).offset for f in fields]
    assert [f[0] for f in G._fields_] == fields
    # the host array is a copy of its blocks, b0 = 2 g
    c = example_config("self-attention-tacotron", "ljspeech")
    arr = groups([block(c), block(c, Ti=9)])
    assert (arr[0].p.Ti, arr[1].p.Ti, arr[0].b0, arr[1].b0, arr[0].has_opt) == (57, 9, 0, 2, 0)


def test_the_single_launch_contract_did_not_move():
    from satt_amd import ops
    for model, data in FAMILIES:
        c = example_config(model, data)
        p = block(c, B=3)
        assert not ops.dec_mega_supported(p) and ops.dec_mega_variant(p) == -1
        assert ops.dec_mega_supported(block(c, B=2)) and ops.dec_mega_supported(block(c, B=1))
    assert ops.dec_mega_scratch_floats(2, 2, 128) == 2 * 2 * (12 * 256 + 32 * 130 + 168 + 32 + 256)
    assert ops.dec_mega_scratch_floats(1, 0, 0) == 2 * (7 * 256 + 168 + 32 + 256)
    assert ops.dec_mega_scratch_floats(2, 0, 0) == 2 * ops.dec_mega_scratch_floats(1, 0, 0)
    assert ops.dec_mega_scratch_floats(1, 0, 128) == 0 and ops.dec_mega_scratch_floats(1, 3, 0) == 0


def test_groups_scratch_size():
    from satt_amd import ops
    for heads, hd in ((2, 128), (4, 64), (0, 0)):
        one = ops.dec_mega_scratch_floats(2, heads, hd)
        assert one > 0
        for n in (1, 2, 5, 8):
            assert ops.dec_mega_groups_scratch_floats(n, heads, hd) == n * one
    assert ops.dec_mega_groups_scratch_floats(0, 2, 128) == 0 and ops.dec_mega_groups_scratch_floats(9, 2, 128) == 0
    assert ops.dec_mega_groups_scratch_floats(2, 3, 128) == 0
