"""Host side of the single-source form of the persistent decode kernel (csrc/decode_mega2.hip dec_mega2_single_k; include/satt_hip.h):
which blocks satt_dec_mega_supported takes as the baseline model's form, which instantiation they get, and that nothing of the dual
form's contract moved.  No compute calls (there is no GPU here).
FAILS ON THE PARENT, which refuses every block with Ds == 0 and has no SATT_MEGA_VAR_SINGLE."""
import os
import subprocess

import pytest

import satt_amd  # noqa: F401
from decode_common import ROOT, SPEAKER, example_config, options, shape_of

EXAMPLES = ("ljspeech", "vctk")


@pytest.mark.parametrize("example", EXAMPLES)
def test_the_baseline_examples_are_single_source_models(example):
    c = example_config(example)
    assert not c.dual and c.dec_sa_units == 0 and c.att2_units == 0 and len(c.dec_prenet) == 2
    assert (c.att_rnn_units, c.dec_units) == (256, 256)
    assert (c.num_speakers > 0) == (example == "vctk")


@pytest.mark.parametrize("example", EXAMPLES)
@pytest.mark.parametrize("speaker", [False, True])
def test_supported_table_and_variants(example, speaker):
    from satt_amd import ops
    LDS, SPK, TWO, SINGLE = ops.MEGA_VAR_TABLES_LDS, ops.MEGA_VAR_SPEAKER, ops.MEGA_VAR_TWO_SAMPLES, ops.MEGA_VAR_SINGLE
    shape = shape_of(example_config(example))
    extra = SPEAKER if speaker else {}
    for B, Ti, want in ((1, 33, LDS | SINGLE), (1, 112, LDS | SINGLE), (1, 113, SINGLE), (1, 256, SINGLE), (2, 57, TWO | SINGLE),
                        (2, 256, TWO | SINGLE)):
        p = ops.dec_mega_params(B=B, Td=16, Ti=Ti, **extra, **shape)
        assert ops.dec_mega_supported(p), (B, Ti)
        assert ops.dec_mega_variant(p) == want | (SPK if speaker else 0), (B, Ti)
    for B, Ti in ((3, 57), (1, 257)):
        p = ops.dec_mega_params(B=B, Td=16, Ti=Ti, **extra, **shape)
        assert not ops.dec_mega_supported(p) and ops.dec_mega_variant(p) == -1, (B, Ti)


@pytest.mark.parametrize("B,Ti", [(1, 33), (2, 57)])
def test_half_single_blocks_are_refused(B, Ti):
    from satt_amd import ops
    shape = shape_of(example_config("ljspeech"))
    for half in (dict(U2=32, V2=32), dict(Ds=256, heads=2), dict(U2=32), dict(V2=32), dict(heads=2), dict(Ds=256)):
        p = ops.dec_mega_params(B=B, Td=16, Ti=Ti, **dict(shape, **half))
        assert not ops.dec_mega_supported(p) and ops.dec_mega_variant(p) == -1, half


@pytest.mark.parametrize("B,Ti", [(1, 33), (2, 57)])
def test_the_single_form_keeps_the_production_widths_of_the_cells(B, Ti):
    """MEDIUM widths (A = D = 64), and the edges of the single form's own conditions"""
    from satt_amd import ops
    shape = shape_of(example_config("ljspeech"))
    for bad in (dict(A=64, D=64, U1=32, V1=32, P0=32, P1=32), dict(A=64), dict(D=64), dict(U1=4), dict(U1=260), dict(U1=130), dict(V1=0),
                dict(V1=1028), dict(P0=260), dict(P1=12), dict(NO=169), dict(kernel=17), dict(filters=9)):
        assert not ops.dec_mega_supported(ops.dec_mega_params(B=B, Td=16, Ti=Ti, **dict(shape, **bad))), bad
    for good in (dict(U1=8), dict(U1=12), dict(U1=128), dict(V1=4), dict(V1=1024), dict(att1_mode=1), dict(cumulative=1)):
        assert ops.dec_mega_supported(ops.dec_mega_params(B=B, Td=16, Ti=Ti, **dict(shape, **good))), good


@pytest.mark.parametrize("speaker", [False, True])
@pytest.mark.parametrize("B,Ti", [(1, 33), (1, 140), (2, 57)])
def test_the_single_form_takes_no_options(B, Ti, speaker):
    from satt_amd import ops
    p = ops.dec_mega_params(B=B, Td=16, Ti=Ti, **(SPEAKER if speaker else {}), **shape_of(example_config("vctk")))
    plain = ops.dec_mega_variant(p)
    assert plain > 0 and plain & ops.MEGA_VAR_SINGLE
    assert ops.dec_mega_opt_variant(p, None) == plain
    assert ops.dec_mega_opt_variant(p, options(False, False)) == plain
    for agent, dropout in ((True, False), (False, True), (True, True)):
        assert ops.dec_mega_opt_variant(p, options(agent, dropout)) == -1


def test_header_constant_and_frozen_block(tmp_path):
    from satt_amd import _lib, ops
    src = '#include <stdio.h>\n#include "satt_hip.h"\nint main() { printf("%d %d %d %d %d %d %d\\n", SATT_MEGA_VAR_SINGLE, SATT_MEGA_VAR_TABLES_LDS, ' \
          'SATT_MEGA_VAR_LJ, SATT_MEGA_VAR_SPEAKER, SATT_MEGA_VAR_TWO_SAMPLES, SATT_MEGA_VAR_AGENT, SATT_MEGA_VAR_DROPOUT); return 0; }\n'
    d = str(tmp_path)
    open(os.path.join(d, "t.c"), "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
    vals = list(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))
    assert vals == [ops.MEGA_VAR_SINGLE, ops.MEGA_VAR_TABLES_LDS, ops.MEGA_VAR_LJ, ops.MEGA_VAR_SPEAKER, ops.MEGA_VAR_TWO_SAMPLES,
                    ops.MEGA_VAR_AGENT, ops.MEGA_VAR_DROPOUT]
    assert ops.MEGA_VAR_SINGLE == 64
    names = [f[0] for f in _lib.DecMegaParams._fields_]          # the single form did not touch satt_dec_mega_params
    assert names == ["B", "Td", "Ti", "A", "D", "Ds", "heads", "U1", "V1", "U2", "V2", "kernel", "filters", "att1_mode", "cumulative",
                     "P0", "P1", "feed", "NO", "ldout", "zc", "zh", "stop_threshold", "min_steps",
                     "Wp0", "Wp1", "Wa", "Wq", "W1", "W2", "Wkvq", "Wot", "Wout", "bp0", "bp1", "ba", "b1l", "b2l", "bkvq", "bot", "bout",
                     "locF", "locFb", "locU", "v1", "b1", "v2", "lengths", "keys1", "values1", "keys2", "values2",
                     "ca", "ha", "c1", "h1", "c2", "h2", "a_state", "alpha_state", "ctx", "yout", "tin", "align1", "align2", "kvq", "part",
                     "ctab", "Wfh", "Wfl", "bfb", "step", "flag", "err", "nsteps", "Wp02", "bp02", "sproj"]


def test_scratch_size():
    from satt_amd import ops
    assert ops.dec_mega_scratch_floats(2, 2, 128) == 2 * 2 * (12 * 256 + 32 * 130 + 168 + 32 + 256)          # the dual form: unchanged
    # the single form, per sample: 6 vectors of 256 granules + the energies (256) + the output row + the handshake + the vector
    # between the two Dense layers of the multi-speaker pre-net; two floats per granule
    assert ops.dec_mega_scratch_floats(1, 0, 0) == 2 * (7 * 256 + 168 + 32 + 256) > 0
    assert ops.dec_mega_scratch_floats(2, 0, 0) == 2 * ops.dec_mega_scratch_floats(1, 0, 0)
    assert ops.dec_mega_scratch_floats(1, 0, 128) == 0 and ops.dec_mega_scratch_floats(1, 3, 0) == 0
