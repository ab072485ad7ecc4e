"""Host side of the persistent decode kernel's multi-speaker form (csrc/decode_mega2.hip, template flag SPK): the parameter block
ends with the speaker term, and neither the shapes the kernel takes nor the way an instantiation is chosen depend on anything but
the dimensions and `sproj != NULL`.  No compute calls (there is no GPU here).  FAILS ON THE PARENT, whose block has no such field."""
import pytest

import satt_amd  # noqa: F401
from decode_common import LJ_KEYED, PRODUCTION, example_config, medium_shape, shape_of


def test_production_is_what_the_session_builds_for_the_vctk_example():
    c = example_config("self-attention-tacotron", "vctk")
    got = {k: v for k, v in shape_of(c).items() if k in ("A", "D", "Ds", "heads", "U1", "V1", "U2", "V2", "kernel", "filters", "P0", "P1",
                                                         "feed", "NO", "ldout")}
    assert c.num_speakers == 152 and len(got) == 15 and got == {k: PRODUCTION[k] for k in got}


def test_the_parameter_block_ends_with_the_speaker_term():
    from satt_amd import _lib
    names = [f[0] for f in _lib.DecMegaParams._fields_]
    assert names[-1] == "sproj"
    # the multi-speaker pre-net's second Dense sits in front of it, and everything that was there stays where it was
    assert names[-4:] == ["nsteps", "Wp02", "bp02", "sproj"]
    assert names.index("nsteps") == len(names) - 4 and names[0] == "B" and names[names.index("nsteps") - 1] == "err"


@pytest.mark.parametrize("B,Ti", [(1, 33), (1, 140), (2, 57), (2, 256), (3, 57), (1, 257)])
def test_supported_shapes_do_not_depend_on_the_speaker_term(B, Ti):
    from satt_amd import ops
    want = {"production": B <= 2 and Ti <= 256, "medium": False}          # (medium: A = D = Ds = 64 - not the kernel's widths)
    want["one fed frame"] = want["production"]
    for name, shape in (("production", PRODUCTION), ("one fed frame", LJ_KEYED), ("medium", medium_shape())):
        plain = ops.dec_mega_params(B=B, Td=16, Ti=Ti, **shape)
        spk = ops.dec_mega_params(B=B, Td=16, Ti=Ti, sproj=4096, Wp02=4096, bp02=4096, **shape)      # (never dereferenced here)
        assert ops.dec_mega_supported(plain) == ops.dec_mega_supported(spk) == want[name], (name, B, Ti)


def test_the_speaker_flag_is_keyed_on_sproj_and_the_lj_specialisation_on_the_dimensions():
    from satt_amd import ops
    LDS, LJ, SPK, TWO = ops.MEGA_VAR_TABLES_LDS, ops.MEGA_VAR_LJ, ops.MEGA_VAR_SPEAKER, ops.MEGA_VAR_TWO_SAMPLES
    for B, Ti, base in ((1, 33, LDS), (1, 112, LDS), (1, 113, 0), (2, 57, TWO)):
        plain = ops.dec_mega_params(B=B, Td=16, Ti=Ti, **LJ_KEYED)
        spk = ops.dec_mega_params(B=B, Td=16, Ti=Ti, sproj=4096, Wp02=4096, bp02=4096, **LJ_KEYED)
        assert ops.dec_mega_variant(plain) == base | LJ
        assert ops.dec_mega_variant(spk) == base | LJ | SPK
        # any other width - the examples' two fed-back frames among them: the generic instantiation, with and without the speaker term
        for other in (PRODUCTION, dict(LJ_KEYED, P1=120)):
            assert ops.dec_mega_variant(ops.dec_mega_params(B=B, Td=16, Ti=Ti, **other)) == base
            assert ops.dec_mega_variant(ops.dec_mega_params(B=B, Td=16, Ti=Ti, sproj=4096, Wp02=4096, bp02=4096, **other)) == base | SPK
    assert ops.dec_mega_variant(ops.dec_mega_params(B=3, Td=16, Ti=57, **PRODUCTION)) == -1
    # the exchange buffer covers the multi-speaker layout (one more vector per sample than the plain one)
    # per sample: 12 vectors of 256 granules, the self-attention partials, the output row, the placement handshake - and the vector
    # between the two Dense layers of the multi-speaker pre-net; two floats per granule
    assert ops.dec_mega_scratch_floats(2, 2, 128) == 2 * 2 * (12 * 256 + 32 * 130 + 168 + 32 + 256)
