"""The host side of the persistent decode kernel answers every call of a fixed grid as the commit named in
tests/golden/mega_variants.json did (the commit before the launchers were folded into one resolver and one dispatcher): the seven
variant / supported functions and the refusal codes of the five launchers, row by row.  The grid, its conditions (no call can reach a
launch) and the row layout: tests/golden/make_mega_variants_golden.py.  No GPU is needed or touched."""
import json

import satt_amd  # noqa: F401


def test_every_call_of_the_grid_answers_as_the_recorded_commit(monkeypatch):
    from golden import make_mega_variants_golden as G
    monkeypatch.delenv("SATT_DECODE_GENERIC", raising=False)          # (the switch would take the LJ bit out of every variant)
    doc = json.load(open(G.PATH))
    assert len(doc["commit"]) == 40 and doc["opts"] == G.OPTS and doc["forced"] == G.FORCED
    blocks, groups = G.grid()
    assert [r[:-1] for r in doc["block_rows"]] == blocks and [r[:-1] for r in doc["group_rows"]] == groups          # the whole grid, nothing else
    assert len(blocks) >= 480 and len(groups) >= 216
    for *row, want in doc["block_rows"]:
        assert len(want) == 3 + 2 * len(G.OPTS) + 2 * len(G.OPTS) * len(G.FORCED)
        assert max(want[2::2]) < 0, ("a launcher did not refuse", row)          # (index 2, 4, ...: the launchers' codes)
        assert G.block_row(*row) == want, row
    for *row, want in doc["group_rows"]:
        assert len(want) == len(G.OPTS) * (3 + 2 * len(G.FORCED))
        assert G.group_row(*row) == want, row
