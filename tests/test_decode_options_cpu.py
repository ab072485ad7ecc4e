"""Host side of the persistent decode kernel's options (csrc/decode_mega2.hip, template flag OPT; include/satt_hip.h:
satt_dec_mega_opt_params): the option block's layout, how an instantiation is chosen with the transition agent and with pre-net
dropout, and the wide memories of the spk-decoder example.  No compute calls (there is no GPU here).
FAILS ON THE PARENT, which has neither the block nor the entry points."""
import ctypes
import os
import subprocess

import pytest

import satt_amd  # noqa: F401
from decode_common import FAKE, LJ_KEYED, PRODUCTION, ROOT, SPEAKER, example_config, medium_shape, options, shape_of


def test_option_block_layout_matches_c(tmp_path):
    """sizeof / offsetof of the ctypes mirror == the C struct (compiled with the host compiler), and the frozen block is untouched"""
    from satt_amd import _lib
    O = _lib.DecMegaOptParams
    fields = [f[0] for f in O._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "satt_hip.h"\nint main() {\n  printf("%zu", sizeof(satt_dec_mega_opt_params));\n' + \
        "".join('  printf(" %%zu", offsetof(satt_dec_mega_opt_params, %s));\n' % f for f in fields) + \
        '  printf(" %d %d\\n", SATT_MEGA_VAR_AGENT, SATT_MEGA_VAR_DROPOUT);\n  return 0; }\n'
    d = str(tmp_path)
    open(os.path.join(d, "t.c"), "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
    vals = list(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))
    from satt_amd import ops
    assert vals == [ctypes.sizeof(O)] + [getattr(O, f).offset for f in fields] + [ops.MEGA_VAR_AGENT, ops.MEGA_VAR_DROPOUT]
    assert fields == ["agentW", "agentb", "agent_tab", "u_state", "drop_seed", "drop_thresh", "drop_scale", "drop_T", "drop_stream"]
    names = [f[0] for f in _lib.DecMegaParams._fields_]          # the options did not grow satt_dec_mega_params
    assert names[-4:] == ["nsteps", "Wp02", "bp02", "sproj"] and names[0] == "B" and names[names.index("nsteps") - 1] == "err"
    o = options(True, True)
    assert o.drop_thresh == 1 << 31 and o.drop_scale == 2.0 and o.drop_T == 16 and list(o.drop_stream) == [7, 8] and o.u_state == FAKE
    assert options(False, False).drop_thresh == 0 and not options(False, False).agentW


@pytest.mark.parametrize("widths", ["lj_keyed", "generic"])
@pytest.mark.parametrize("speaker", [False, True])
@pytest.mark.parametrize("B,Ti", [(1, 33), (1, 112), (1, 113), (1, 140), (2, 57), (2, 256)])
def test_options_add_their_bits_to_the_plain_variant(B, Ti, speaker, widths):
    """B = 1 with LDS tables, B = 1 with global tables, B = 2; with and without the speaker term; LJ-keyed and generic widths"""
    from satt_amd import ops
    p = ops.dec_mega_params(B=B, Td=16, Ti=Ti, **(SPEAKER if speaker else {}), **(LJ_KEYED if widths == "lj_keyed" else PRODUCTION))
    plain = ops.dec_mega_variant(p)
    want = (ops.MEGA_VAR_TABLES_LDS if (B == 1 and Ti <= 112) else 0) | (ops.MEGA_VAR_TWO_SAMPLES if B == 2 else 0) | \
        (ops.MEGA_VAR_LJ if widths == "lj_keyed" else 0) | (ops.MEGA_VAR_SPEAKER if speaker else 0)
    assert plain == want
    assert ops.dec_mega_opt_variant(p, None) == plain
    assert ops.dec_mega_opt_variant(p, options(False, False)) == plain
    assert ops.dec_mega_opt_variant(p, options(True, False)) == plain | ops.MEGA_VAR_AGENT
    assert ops.dec_mega_opt_variant(p, options(False, True)) == plain | ops.MEGA_VAR_DROPOUT
    assert ops.dec_mega_opt_variant(p, options(True, True)) == plain | ops.MEGA_VAR_AGENT | ops.MEGA_VAR_DROPOUT


@pytest.mark.parametrize("B,Ti,shape", [(3, 57, "production"), (1, 257, "production"), (2, 57, "medium"), (1, 33, "medium")])
def test_options_do_not_widen_what_the_kernel_takes(B, Ti, shape):
    from satt_amd import ops
    p = ops.dec_mega_params(B=B, Td=16, Ti=Ti, **(PRODUCTION if shape == "production" else medium_shape()))
    assert ops.dec_mega_variant(p) == -1 and not ops.dec_mega_supported(p)
    for agent, dropout in ((False, False), (True, False), (False, True), (True, True)):
        assert ops.dec_mega_opt_variant(p, options(agent, dropout)) == -1


def test_the_spk_decoder_example_is_supported_with_its_wide_memories():
    """examples/vctk/self-attention-tacotron-spk-decoder.json: the memories are [encoder output | speaker vector] - V1 = 272,
    V2 = 48 - and the kernel, generic in the memory widths, takes them for B <= 2, Ti <= 256: the generic instantiation with the
    speaker bit (the model has the multi-speaker pre-net too)"""
    from satt_amd import ops
    c = example_config("self-attention-tacotron-spk-decoder", "vctk")
    assert c.speaker_to_decoder and c.mem_speaker == 16
    shape = shape_of(c)
    assert (shape["V1"], shape["V2"], shape["feed"]) == (272, 48, 160)
    assert shape == dict(PRODUCTION, V1=272, V2=48, zc=c.zc, zh=c.zh)
    for B, Ti, base in ((1, 33, ops.MEGA_VAR_TABLES_LDS), (1, 140, 0), (1, 256, 0), (2, 57, ops.MEGA_VAR_TWO_SAMPLES), (2, 256, ops.MEGA_VAR_TWO_SAMPLES)):
        p = ops.dec_mega_params(B=B, Td=16, Ti=Ti, **SPEAKER, **shape)
        assert ops.dec_mega_supported(p)
        assert ops.dec_mega_variant(p) == base | ops.MEGA_VAR_SPEAKER
    for B, Ti in ((3, 57), (1, 257)):
        assert not ops.dec_mega_supported(ops.dec_mega_params(B=B, Td=16, Ti=Ti, **SPEAKER, **shape))
