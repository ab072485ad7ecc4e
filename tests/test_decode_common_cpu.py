"""tests/decode_common.py itself: the two context managers put back exactly what they found, and expected_variant - the one statement
of which instantiation of the persistent decode kernel a model and a shape take, which the GPU suites assert against - agrees with
the library for every model of every suite.  Needs the built library, no GPU: the blocks hold fake addresses, nothing is launched."""
import importlib

import pytest

from decode_common import (LAUNCHERS, Launch, block, example_config, expected_variant, forced, groups, options, recording, switches)

SUITES = ("speaker", "options", "single", "forced", "groups", "forced_groups", "rows")


def test_switches_put_back_what_they_found():
    from satt_amd.inference import DecodeSession as S
    names = ("MEGA", "MEGA_STEPS", "MEGA_FOLD_FEEDBACK", "MEGA_GROUPS")
    found = {k: S.__dict__[k] for k in names}
    with switches(MEGA=False, MEGA_STEPS=5):          # values that are no defaults: what comes back is what was there, not a constant
        with switches("MEGA_GROUPS", MEGA=True, MEGA_STEPS=8):
            assert (S.MEGA, S.MEGA_STEPS) == (True, 8)
            S.MEGA_GROUPS = not found["MEGA_GROUPS"]          # (a name without a value: the body's own change is undone)
            S.MEGA = "changed again in the body"
        assert (S.MEGA, S.MEGA_STEPS, S.MEGA_GROUPS) == (False, 5, found["MEGA_GROUPS"])
        with pytest.raises(KeyError):
            with switches(MEGA=True, MEGA_FOLD_FEEDBACK=not found["MEGA_FOLD_FEEDBACK"]):
                raise KeyError("the body raises")
        assert (S.MEGA, S.MEGA_STEPS, S.MEGA_FOLD_FEEDBACK) == (False, 5, found["MEGA_FOLD_FEEDBACK"])
        with pytest.raises(AttributeError):
            with switches(NO_SUCH_SWITCH=1):
                pass
        assert "NO_SUCH_SWITCH" not in S.__dict__
    assert {k: S.__dict__[k] for k in names} == found


def test_recording_wraps_the_five_launchers_and_puts_them_back(monkeypatch):
    from satt_amd import ops
    calls = []
    stand_ins = {name: (lambda *a, name=name: calls.append(name) or "result of " + name) for name in LAUNCHERS}
    for name, fn in stand_ins.items():
        monkeypatch.setattr(ops, name, fn)
    c = example_config("self-attention-tacotron", "ljspeech")
    p, o, f, arr = block(c), options(False, True), forced(), groups([block(c) for _ in range(3)])
    with recording() as launches:
        assert not any(getattr(ops, name) is fn for name, fn in stand_ins.items())
        assert ops.dec_mega(p, 8) == "result of dec_mega"
        ops.dec_mega_opt(p, o, 5)
        ops.dec_mega_forced(p, o, f, 3)
        ops.dec_mega_groups(arr, None)
        ops.dec_mega_groups_forced(arr, None, f)
    assert all(getattr(ops, name) is fn for name, fn in stand_ins.items())
    assert calls == list(LAUNCHERS) == ["dec_mega", "dec_mega_opt", "dec_mega_forced", "dec_mega_groups", "dec_mega_groups_forced"]
    assert launches == [Launch("dec_mega", ops.dec_mega_variant(p), 0, 8), Launch("dec_mega_opt", ops.dec_mega_opt_variant(p, o), 0, 5),
                        Launch("dec_mega_forced", ops.dec_mega_forced_variant(p, o, f), 0, 3),
                        Launch("dec_mega_groups", ops.dec_mega_groups_variant(arr), 3, 8),
                        Launch("dec_mega_groups_forced", ops.dec_mega_groups_forced_variant(arr, f), 3, 8)]
    assert len({l.variant for l in launches}) == 5 and min(l.variant for l in launches) > 0
    with pytest.raises(KeyError):
        with recording():
            raise KeyError("the body raises")
    assert all(getattr(ops, name) is fn for name, fn in stand_ins.items())


def models():
    """(suite, model, ModelConfig keywords) of every model of every GPU suite (the suites' own tables: only they are read)"""
    for suite in SUITES:
        m = importlib.import_module("test_decode_%s_gpu" % suite)
        for name, kw in (m.SOURCES if suite == "speaker" else m.MODELS).items():
            yield pytest.param(kw, id="%s: %s" % (suite, name))


@pytest.mark.parametrize("kw", models())
def test_expected_variant_agrees_with_the_library(kw, monkeypatch):
    """the shapes of the suites - B = 1 with the context tables in LDS (Ti = 33) and in global memory (113, 140), B = 2 with Ti = 57,
    groups of 2 and 3 blocks; tests/test_decode_rows_gpu.py: both ends of the range (2, 256), both sides of 112 / 113 and 128 / 129,
    groups of 3 and 8 blocks at Ti = 256 -, free and forced, with the option and forced blocks the session would pass.  Where the session stays
    off the kernel (-1: the single-source form with the agent or live dropout) the library refuses the block it would be asked with."""
    from satt_amd import ops
    from satt_amd.params import ModelConfig
    monkeypatch.delenv("SATT_DECODE_GENERIC", raising=False)          # (the switch would take the LJ bit out of every variant)
    cfg = ModelConfig(**kw)          # (what common.make_params builds the suites' configurations with)
    seen = set()
    for frc in (False, True):
        agent, drop = cfg.transition_agent and not frc, cfg.apply_dropout_on_inference
        opt = options(agent, drop) if (agent or drop) else None
        f = forced(two=cfg.dual) if frc else None
        for B, Ti in ((1, 33), (1, 113), (1, 140), (2, 57), (1, 2), (1, 112), (1, 128), (1, 129), (1, 256), (2, 64), (2, 129), (2, 256)):
            want = expected_variant(cfg, B, Ti, forced=frc)
            p = block(cfg, B, Ti)
            assert ops.dec_mega_forced_variant(p, opt, f) == want, (frc, B, Ti)
            if not frc:
                assert ops.dec_mega_opt_variant(p, opt) == want, (B, Ti)
                if opt is None:
                    assert ops.dec_mega_variant(p) == want, (B, Ti)
            seen.add(want)
        for n, Ti in ((2, 57), (3, 57), (3, 256), (8, 256)):
            arr = groups([block(cfg, Ti=Ti) for _ in range(n)], opt)
            for B in (2 * n - 1, 2 * n):
                want = expected_variant(cfg, B, Ti, forced=frc, groups=True)
                assert ops.dec_mega_groups_forced_variant(arr, f) == want, (frc, n)
                if not frc:
                    assert ops.dec_mega_groups_variant(arr) == want, n
                seen.add(want)
    single_with_options = not cfg.dual and (cfg.transition_agent or cfg.apply_dropout_on_inference)
    assert (-1 in seen) == single_with_options and (len(seen) == 8 or single_with_options), seen
