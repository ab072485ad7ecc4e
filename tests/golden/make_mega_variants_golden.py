"""Freezes the host side of the persistent decode kernel (csrc/decode_mega2.hip: the seven variant / supported functions and the five
launchers of include/satt_hip.h) over a fixed grid of calls into tests/golden/mega_variants.json; tests/test_decode_launcher_cpu.py
replays the file against the built library and asserts equality row by row.

The file is generated from the library of the commit BEFORE a change of that host code, never from the changed one:
    python tests/golden/make_mega_variants_golden.py <hash of the commit the library was built from>
It holds the grid's parameters and the recorded integers, nothing else.  A row is self-contained: `block_row` / `group_row` below
rebuild its calls from the parameters alone.

NO CALL OF THE GRID CAN REACH A LAUNCH, under any revision whose pointer checks work at all: every block leaves `err` (and every other
pointer but the speaker term's and the option / forced blocks') NULL, so the best a launcher can answer is SATT_E_BADARG.  The codes
still tell a refusal of the shapes (SATT_E_UNSUPPORTED) from one of the pointers (SATT_E_BADARG), and nsteps = 0 (SATT_E_UNSUPPORTED
from the block's own check) shows which of the two a launcher looks at first.  No GPU is needed or touched.

The grid:
  blocks   the four shipped example configurations, PRODUCTION and LJ_KEYED (tests/decode_common.py), each with
           B in {1, 2, 3} x Ti in {1, 57, 112, 113, 256 (the largest), 257} x nsteps in {0, 8} x speaker term set / unset, plus eight
           single-field perturbations that make the block unsupported (B = 2, Ti = 57, nsteps = 8);
           per block: supported, variant, satt_dec_mega; per option block (OPTS): opt_variant, satt_dec_mega_opt; per option block
           and forced block (FORCED): forced_variant, satt_dec_mega_forced - 53 integers in that order.
  groups   the same six shapes x GROUP_CASES x nsteps in {0, 8} x speaker term set / unset;
           per option block: groups_variant, groups_supported, satt_dec_mega_groups, then per forced block groups_forced_variant,
           satt_dec_mega_groups_forced - 55 integers."""
import ctypes as C
import functools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (os.path.join(ROOT, "tests"), ROOT):
    if d not in sys.path:
        sys.path.insert(0, d)

PATH = os.path.join(HERE, "mega_variants.json")
OPTS = [None, "off", "agent", "dropout", "both"]
FORCED = [None, "no_teach1", "teach1", "both"]
GROUP_CASES = ["n1", "n2", "n8", "n9", "n0", "null", "ti_disagree", "b0_negative", "flag"]
SHAPES = ["self-attention-tacotron/ljspeech", "self-attention-tacotron/vctk", "tacotron/ljspeech", "tacotron/vctk", "PRODUCTION", "LJ_KEYED"]


@functools.lru_cache(None)
def _shape(name):
    from decode_common import LJ_KEYED, PRODUCTION, example_config, shape_of
    if "/" not in name:
        return dict(PRODUCTION=PRODUCTION, LJ_KEYED=LJ_KEYED)[name]
    return shape_of(example_config(*name.split("/")))


def shape(name):
    return dict(_shape(name))


def perturbations(s):
    """single-field changes that make a supported block unsupported (half single: Ds = 0 with a second query width kept)"""
    return [dict(A=64), dict(heads=3), dict(Ds=0, heads=0, V2=0, U2=32), dict(P0=4), dict(NO=176, ldout=176), dict(ldout=(s["NO"] - 1) // 8 * 8),
            dict(kernel=17), dict(filters=9)]


def make_block(name, B, Ti, nsteps, speaker, change):
    from satt_amd import ops
    from decode_common import SPEAKER
    return ops.dec_mega_params(B=B, Td=16, Ti=Ti, nsteps=nsteps, **(SPEAKER if speaker else {}), **dict(shape(name), **change))


def make_opt(o):
    from decode_common import options
    return None if o is None else options(o in ("agent", "both"), o in ("dropout", "both"))


def make_forced(f):
    from satt_amd import ops
    from decode_common import FAKE
    return None if f is None else ops.dec_mega_forced_params(FAKE if f in ("teach1", "both") else None, FAKE + 64 if f in ("no_teach1", "both") else None)


def ref(x):
    return None if x is None else C.byref(x)


def block_row(name, B, Ti, nsteps, speaker, change):
    from satt_amd import _lib
    L = _lib.lib()
    p = C.byref(make_block(name, B, Ti, nsteps, speaker, change))
    out = [L.satt_dec_mega_supported(p), L.satt_dec_mega_variant(p), L.satt_dec_mega(p, None)]
    opts = [make_opt(o) for o in OPTS]
    for o in opts:
        out += [L.satt_dec_mega_opt_variant(p, ref(o)), L.satt_dec_mega_opt(p, ref(o), None)]
    for o in opts:
        for f in map(make_forced, FORCED):
            out += [L.satt_dec_mega_forced_variant(p, ref(o), ref(f)), L.satt_dec_mega_forced(p, ref(o), ref(f), None)]
    return [int(v) for v in out]


def make_groups(name, case, nsteps, speaker, opt):
    """(host array or None, ngroups) of a group case"""
    from satt_amd import ops
    from decode_common import FAKE
    n = dict(n1=1, n2=2, n8=8, n9=9, n0=9).get(case, 2)
    blocks = [make_block(name, 2, 57, nsteps, speaker, {}) for _ in range(n)]
    if case == "ti_disagree":
        blocks[1] = make_block(name, 2, 58, nsteps, speaker, {})
    if case == "flag":
        for p in blocks:
            p.flag = FAKE
    arr = ops.dec_mega_groups_blocks([(p, opt, 2 * g) for g, p in enumerate(blocks)])
    if case == "b0_negative":
        arr[1].b0 = -1
    return (None, 2) if case == "null" else (arr, 0 if case == "n0" else n)


def group_row(name, case, nsteps, speaker):
    from satt_amd import _lib
    from decode_common import FAKE
    L = _lib.lib()
    dev = C.c_void_p(FAKE)          # (never read: no block holds the pointers a launch needs)
    out = []
    for o in OPTS:
        arr, n = make_groups(name, case, nsteps, speaker, make_opt(o))
        out += [L.satt_dec_mega_groups_variant(arr, n), L.satt_dec_mega_groups_supported(arr, n), L.satt_dec_mega_groups(arr, dev, n, None)]
        for f in map(make_forced, FORCED):
            out += [L.satt_dec_mega_groups_forced_variant(arr, n, ref(f)), L.satt_dec_mega_groups_forced(arr, dev, n, ref(f), None)]
    return [int(v) for v in out]


def grid():
    blocks, groups = [], []
    for name in SHAPES:
        for B in (1, 2, 3):
            for Ti in (1, 57, 112, 113, 256, 257):
                for nsteps in (0, 8):
                    for speaker in (0, 1):
                        blocks.append([name, B, Ti, nsteps, speaker, {}])
        blocks += [[name, 2, 57, 8, 0, change] for change in perturbations(shape(name))]
        groups += [[name, case, nsteps, speaker] for case in GROUP_CASES for nsteps in (0, 8) for speaker in (0, 1)]
    return blocks, groups


if __name__ == "__main__":
    import satt_amd  # noqa: F401
    assert len(sys.argv) == 2 and len(sys.argv[1]) == 40, "usage: make_mega_variants_golden.py <full hash of the commit the library was built from>"
    assert "SATT_DECODE_GENERIC" not in os.environ
    blocks, groups = grid()
    doc = dict(commit=sys.argv[1], opts=OPTS, forced=FORCED,
               block_rows=[row + [block_row(*row)] for row in blocks], group_rows=[row + [group_row(*row)] for row in groups])
    with open(PATH, "w") as fh:
        fh.write('{"commit": %s, "opts": %s, "forced": %s,\n"block_rows": [\n%s\n],\n"group_rows": [\n%s\n]}\n' % (
            json.dumps(doc["commit"]), json.dumps(OPTS), json.dumps(FORCED),
            ",\n".join(json.dumps(r, separators=(",", ":")) for r in doc["block_rows"]),
            ",\n".join(json.dumps(r, separators=(",", ":")) for r in doc["group_rows"])))
    print("wrote %s: %d block rows, %d group rows, %.0f KB" % (PATH, len(blocks), len(groups), os.path.getsize(PATH) / 1024))
