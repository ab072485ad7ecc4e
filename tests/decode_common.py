"""Shared scaffolding of the decode test family (tests/test_decode_*_{cpu,gpu}.py, tests/golden/make_mega_variants_golden.py).

CPU half: shape dictionaries and parameter blocks with fake addresses, as DecodeSession would hand them to the library - no compute
calls.  GPU half: one engine cache per suite (Engines), the DecodeSession switches and the five launchers of the persistent kernel
as context managers (switches, recording, sessions_used - together: traced_infer), the one statement of which instantiation a
model and a shape take (expected_variant), and the comparison helpers the suites share.  Importing this module touches no GPU."""
import collections
import contextlib
import os

import numpy as np
import torch

import satt_amd  # noqa: F401
from common import MEDIUM, make_params, rel_err, small_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------------------------------------------------------- CPU half
FAKE = 4096          # a non-NULL address (never dereferenced on the CPU side)
SPEAKER = dict(sproj=FAKE, Wp02=FAKE, bp02=FAKE)
FAMILIES = [(m, d) for m in ("self-attention-tacotron", "tacotron") for d in ("ljspeech", "vctk")]
# examples/vctk/self-attention-tacotron.json (= the LJSpeech layer sizes, two fed-back frames): the shape block DecodeSession hands to
# the library; LJ_KEYED: the same with ONE fed-back frame - the widths the compile-time specialisation of the kernel is keyed on
PRODUCTION = dict(A=256, D=256, Ds=256, heads=2, U1=224, V1=256, U2=32, V2=32, kernel=10, filters=5, att1_mode=0, cumulative=0,
                  P0=256, P1=128, feed=160, NO=161, ldout=168, zc=0.1, zh=0.1, stop_threshold=0.5, min_steps=10)
LJ_KEYED = dict(PRODUCTION, feed=80)
LJ_KEYS = ("U1", "U2", "V1", "V2", "heads", "NO", "feed", "P0", "P1", "kernel", "filters")          # (csrc/decode_mega2.hip: `lj`)


def example_config(model, data=None):
    """the ModelConfig of examples/<data>/<model>.json; example_config(data) is the baseline model's, examples/<data>/tacotron.json"""
    from satt_amd.hparams import hparams
    from satt_amd.params import ModelConfig
    if data is None:
        model, data = "tacotron", model
    hp = hparams.copy()
    hp.parse_json(open(os.path.join(ROOT, "examples", data, model + ".json")).read())
    return ModelConfig.from_hparams(hp)


def shape_of(c):
    """the shape block DecodeSession offers for a configuration: the dual form, or the baseline model's single-source form
    (Ds = heads = U2 = V2 = 0); speaker_to_decoder widens the memories by mem_speaker columns"""
    NO = c.num_mels * c.r + 1
    second = dict(Ds=c.dec_sa_units, heads=c.dec_sa_heads, U2=c.att2_units, V2=c.sa_units + c.mem_speaker) if c.dual else \
        dict(Ds=0, heads=0, U2=0, V2=0)
    return dict(A=c.att_rnn_units, D=c.dec_units, U1=c.att1_units, V1=c.cbhg_out_units + c.mem_speaker, **second, kernel=c.att_kernel,
                filters=c.att_filters, att1_mode=int(c.attention == "location_sensitive"), cumulative=int(c.cumulative_weights),
                P0=c.dec_prenet[0], P1=c.dec_prenet[1], feed=c.num_mels * c.n_feed_frame, NO=NO, ldout=(NO + 7) // 8 * 8, zc=c.zc, zh=c.zh,
                stop_threshold=0.5, min_steps=10)


def medium_shape():
    """tests/common.py MEDIUM (A = D = Ds = 64): not the kernel's widths"""
    from satt_amd.params import ModelConfig
    return shape_of(ModelConfig(**MEDIUM))


def block(c, B=2, Ti=57, nsteps=8, **kw):
    """the parameter block of configuration `c` (with the speaker term if it has speakers); kw overrides fields of the shape"""
    from satt_amd import ops
    extra = SPEAKER if c.num_speakers else {}
    p = ops.dec_mega_params(B=B, Td=16, Ti=Ti, **extra, **dict(shape_of(c), **kw))
    p.nsteps = nsteps
    return p


def groups(blocks, opt=None):
    from satt_amd import ops
    return ops.dec_mega_groups_blocks([(p, opt, 2 * g) for g, p in enumerate(blocks)])


def options(agent, dropout):
    from satt_amd import ops
    kw = dict(agentW=FAKE, agentb=FAKE, agent_tab=FAKE, u_state=FAKE) if agent else {}
    return ops.dec_mega_opt_params(drop=ops.Drop(0.5, 0, FAKE) if dropout else None, drop_T=16, drop_streams=(7, 8), **kw)


def forced(two=True):
    from satt_amd import ops
    return ops.dec_mega_forced_params(FAKE, FAKE + 64 if two else None)


def expected_variant(cfg, B, Ti, forced=False, groups=False):
    """the MEGA_VAR_* bits of the instantiation a session of model `cfg` launches for B samples and a memory of Ti rows (groups: B > 2,
    every group a B = 2 problem); -1 where the session stays on the launch-per-layer path because the library would refuse - the
    single-source form takes no options (the agent is dead under forced alignments, so there it is no option)"""
    from satt_amd import ops
    agent = cfg.transition_agent and not forced
    drop = cfg.apply_dropout_on_inference and cfg.dec_prenet_drop > 0
    two = groups or B == 2
    var = ops.MEGA_VAR_TWO_SAMPLES if two else (ops.MEGA_VAR_TABLES_LDS if Ti <= 112 else 0)          # the context tables fit LDS beside one sample
    var |= ops.MEGA_VAR_SPEAKER if cfg.num_speakers else 0
    var |= (ops.MEGA_VAR_GROUPS if groups else 0) | (ops.MEGA_VAR_FORCED if forced else 0)
    if not cfg.dual:
        return -1 if (agent or drop) else var | ops.MEGA_VAR_SINGLE
    shape = shape_of(cfg)
    lj = not forced and all(shape[k] == LJ_KEYED[k] for k in LJ_KEYS)          # (the compile-time widths have no forced sibling)
    return var | (ops.MEGA_VAR_LJ if lj else 0) | (ops.MEGA_VAR_AGENT if agent else 0) | (ops.MEGA_VAR_DROPOUT if drop else 0)


# ---------------------------------------------------------------------------------------------------------------- GPU half
BAR = 2e-5          # relative to the largest element: same bf16 weights, same buffers, fp32 sums in another order, fed back through the steps
BASELINE = dict(sa_units=0, att2_units=0, dec_sa_units=0, att1_units=256)          # the single-source model: baseline_kw(dict()) of tests/test_model_gpu.py
KEYS = ("mel", "stop", "alignment1", "alignment2")


class Engines:
    """one bf16 engine per (model, stop-logit bias) of a suite's `models`, shared by the tests of that suite (sessions are cached on it).
    Every suite has its own instance: what an engine returns depends on the sessions it has seen (the session cache is cleared at
    eight entries, the per-call dropout seed counts infer() calls).
    stats: the BatchNorm moving statistics are randomised and returned for the oracle - engine() gives (engine, cfg, P, mv), else (engine, cfg).
    agent: None leaves the transition agent's weights as they are; a dictionary model -> (scale of Wa, value of ba), key None for every
    model it does not name, rewrites them (u far from 0.5, different per step and sample; (0, 0): u = 0.5 at every step)."""

    def __init__(self, models, stats=False, agent=None):
        self.models, self.stats, self.agent, self._params, self._engines = models, stats, agent, {}, {}

    def params(self, model, stop=False):
        """(cfg, parameters) of `model` - CPU only"""
        key = (model, stop)
        if key not in self._params:
            cfg, P = make_params(self.models[model], seed=4)
            P = dict(P)
            if cfg.num_speakers:
                P["speaker_embedding"] = np.random.default_rng(9).normal(0, 0.5, P["speaker_embedding"].shape).astype(np.float32)
            if cfg.transition_agent and self.agent is not None:
                scale, bias = self.agent.get(model, self.agent[None])
                P["dec.att1.Wa"] = (scale * P["dec.att1.Wa"]).astype(np.float32)
                P["dec.att1.ba"] = np.full_like(P["dec.att1.ba"], bias)
            if stop:
                b = np.array(P["dec.out.b"], dtype=np.float32).copy(); b[-1] = 50.0          # stop logit always large
                P["dec.out.b"] = b
            self._params[key] = (cfg, P)
        return self._params[key]

    def config(self, model):
        return self.params(model)[0]

    def engine(self, model, stop=False):
        from satt_amd import ops
        from satt_amd.engine import Engine
        key = (model, stop)
        if key not in self._engines:
            cfg, P = self.params(model, stop)
            ops.set_precision("bf16")
            eng = Engine(cfg, "cuda", params=P, rng_seed=7)
            if self.stats:
                g = np.random.default_rng(11)
                mv = {}
                for name, (mean, var) in eng.bn.items():        # non-trivial moving statistics, shared with the oracle
                    m = g.normal(0, 0.2, mean.shape[0]).astype(np.float32); v = g.uniform(0.5, 1.5, var.shape[0]).astype(np.float32)
                    mean.copy_(torch.as_tensor(m)); var.copy_(torch.as_tensor(v))
                    mv[name] = (torch.as_tensor(m, dtype=torch.float64), torch.as_tensor(v, dtype=torch.float64))
            self._engines[key] = (eng, cfg, P, mv) if self.stats else (eng, cfg)
        ops.set_precision("bf16")
        return self._engines[key]

    __call__ = engine


@contextlib.contextmanager
def switches(*names, **values):
    """DecodeSession class attributes (MEGA, MEGA_STEPS, FUSE, ...) set to `values` inside the body, then back to what they were;
    `names`: attributes the body sets itself, put back as well"""
    from satt_amd.inference import DecodeSession
    found = {k: getattr(DecodeSession, k) for k in names + tuple(values)}
    try:
        for k, v in values.items():
            setattr(DecodeSession, k, v)
        yield
    finally:
        for k, v in found.items():
            setattr(DecodeSession, k, v)


Launch = collections.namedtuple("Launch", "name variant groups nsteps")          # groups: 0 for the launchers of a single block
# entry point -> (the variant the library reports, group count, nsteps) of a call's own arguments (inference.py calls each launcher
# through the attribute of `ops`, with these positional arguments)
LAUNCHERS = dict(
    dec_mega=lambda ops, p, n: (ops.dec_mega_variant(p), 0, n),
    dec_mega_opt=lambda ops, p, o, n: (ops.dec_mega_opt_variant(p, o), 0, n),
    dec_mega_forced=lambda ops, p, o, f, n: (ops.dec_mega_forced_variant(p, o, f), 0, n),
    dec_mega_groups=lambda ops, arr, dev: (ops.dec_mega_groups_variant(arr), len(arr), arr[0].p.nsteps),
    dec_mega_groups_forced=lambda ops, arr, dev, f: (ops.dec_mega_groups_forced_variant(arr, f), len(arr), arr[0].p.nsteps))


@contextlib.contextmanager
def recording(poison=None):
    """yields the list of the launches of the persistent kernel made inside the body, one Launch per call of any of the five entry
    points.  poison: that pattern is written to every LDS word of every CU in front of EVERY launch (satt_debug_poison_lds)."""
    from satt_amd import _lib, ops
    real = {name: getattr(ops, name) for name in LAUNCHERS}
    launches = []

    def wrap(name):
        def launch(*a):
            if poison is not None:
                _lib.check(_lib.lib().satt_debug_poison_lds(poison, 100, ops.current_stream().cuda_stream), "poison_lds")
            launches.append(Launch(name, *LAUNCHERS[name](ops, *a)))
            return real[name](*a)
        return launch
    try:
        for name in real:
            setattr(ops, name, wrap(name))
        yield launches
    finally:
        for name, fn in real.items():
            setattr(ops, name, fn)


@contextlib.contextmanager
def sessions_used():
    """yields the list of the sessions infer() ran on inside the body: it calls build_context_tables once per call on the session
    it uses, cached or new"""
    from satt_amd.inference import DecodeSession
    tables, used = DecodeSession.build_context_tables, []
    DecodeSession.build_context_tables = lambda self: (used.append(self), tables(self))[1]
    try:
        yield used
    finally:
        DecodeSession.build_context_tables = tables


def last_session(eng):
    """the session inserted last - the one infer() just used only if it had to build it"""
    return eng._decode_sessions[next(reversed(eng._decode_sessions))]


def traced_infer(eng, source, source_length, sw, poison=None, **kw):
    """one infer() under the DecodeSession switches `sw`; returns (outputs, the session it ran on, the launches it made)"""
    from satt_amd.inference import infer
    with switches(**sw), recording(poison) as launches, sessions_used() as used:
        out = infer(eng, source, source_length, **kw)
    ses, = used
    return out, ses, launches


def infer_kwargs(mode, steps, mel, ids=None, seed=None):
    """infer()'s arguments for mode "free" (`steps` steps), "teacher" (fed the frames `mel`) or "stop" (the rule may fire after 5 steps)"""
    kw = dict(teacher=torch.as_tensor(mel)) if mode == "teacher" else dict(max_steps=steps, min_steps=(5 if mode == "stop" else 10 ** 6))
    if ids is not None:
        kw["speaker_id"] = torch.as_tensor(np.array(ids, np.int64))
    if seed is not None:
        kw["dropout_seed"] = seed
    return kw


def host_outputs(out, keys=KEYS):
    res = {k: None if out[k] is None else out[k].detach().cpu() for k in keys}
    res["steps"] = out["steps"]
    return res


def keys_of(cfg):
    return ("mel", "stop", "alignment1") + (("alignment2",) if cfg.dual else ())


def same(new, old, what, keys=("mel", "stop")):
    assert new["steps"] == old["steps"], (what, new["steps"], old["steps"])
    for k in keys:
        e = rel_err(new[k].numpy(), old[k].numpy())
        print("%s %-10s rel_err=%.3e (bar %.0e)" % (what, k, e, BAR))
        assert e < BAR, (what, k, e)
    assert torch.isfinite(new["mel"]).all()


def history_is_as_given(res, ta):
    n = res["steps"]
    assert torch.equal(res["alignment1"], ta[0][:, :n]), "alignment1 is not bit-equal to the rows given"
    if ta[1] is not None:
        assert torch.equal(res["alignment2"], ta[1][:, :n]), "alignment2 is not bit-equal to the rows given"
    else:
        assert res["alignment2"] is None


def inputs(cfg, B, Ti, steps, lens=None):
    """source, lengths (the batch's own ragged ones unless given) and the target frames"""
    batch = small_batch(cfg, B, Ti, steps * cfg.r, seed=6)
    sl = np.array(batch["source_length"] if lens is None else lens, np.int64)
    src = np.array(batch["source"]).copy()
    src[np.arange(Ti)[None, :] >= sl[:, None]] = 0
    return torch.as_tensor(src), torch.as_tensor(sl), torch.as_tensor(batch["mel"])


def teacher_rows(B, steps, Ti, lens, dual, masked=True, seed=3, sharp=1):
    """random row-normalised alignments (tests/test_inference_gpu.py test_forced_alignment_mode); masked=False: mass beyond the lengths;
    sharp > 1: the uniform draws raised to that power before the normalisation - rows with a few large entries, whose contexts differ
    from row to row (the contexts of flat rows over one memory are all close to the memory's mean)"""
    g = torch.Generator().manual_seed(seed)
    mask = (torch.arange(Ti)[None, None, :] < torch.as_tensor(lens)[:, None, None]).double()
    ta = []
    for _ in range(2 if dual else 1):
        a = torch.rand(B, steps, Ti, generator=g, dtype=torch.float64) ** sharp
        if masked:
            a = a * mask
        ta.append((a / a.sum(-1, keepdim=True)).float())
    return (ta[0], ta[1] if dual else None)


# ---- inputs that look at the memory rows (tests/test_decode_rows_{cpu,gpu}.py, tests/golden/make_decode_rows_golden.py)
# the kernel's row ownership changes at these rows: 32 rows of energies per workgroup at the most, 64 rows per wave (softmax, recursion,
# teacher rows, gather_vec), the table forms at 112 / 113 (B = 1) and 128, the second table row of a row lane from 128 on
FOCUS_BOUNDARIES = (32, 64, 96, 112, 128, 192, 224)
ROWS_STEPS = 16          # the steps of the memory-length suites: two launches of 8


def focus_visits(length):
    """the rows a sample of `length` rows must have been focused on: both ends and both sides of every boundary below the length"""
    rows = [0, 1, length - 1, length - 2] + [r for b in FOCUS_BOUNDARIES if b < length for r in (b - 1, b)]
    return sorted({r for r in rows if 0 <= r < length})


def focus_steps(lens, dual):
    """ROWS_STEPS, or - the baseline model above 224 rows, whose one mechanism has 18 rows to visit - 24 (three launches of 8)"""
    need = max(len(focus_visits(int(n))) for n in lens)
    return ROWS_STEPS if need <= ROWS_STEPS * (2 if dual else 1) else 24


def focus_plan(B, steps, lens, dual):
    """int64 [mechanisms, B, steps]: the focus row of every (mechanism, sample, step).  Mechanism 1 walks the visit list of its
    sample from entry b on, mechanism 2 half a list ahead of it: together they cover the list, and never the same row at one step"""
    plan = np.zeros((2 if dual else 1, B, steps), np.int64)
    for b in range(B):
        v = focus_visits(int(lens[b]))
        n = len(v)
        assert 2 <= n <= steps * plan.shape[0], (int(lens[b]), n, steps)
        for m in range(plan.shape[0]):
            plan[m, b] = [v[(t + b + m * (n // 2)) % n] for t in range(steps)]
    return plan


def focus_rows(B, steps, Ti, lens, dual, weight=0.6, seed=5, plan=None):
    """forced-alignment teacher histories in the shape teacher_rows returns, that LOOK at single rows: every row is a random masked
    background of mass 1 - weight plus `weight` on the focus row of focus_plan (plan: another one).  The context of such a row is
    weight * memory[focus] + a near-mean rest, so a mix-up of two rows inside the kernel's tables moves the frame of that step"""
    g = torch.Generator().manual_seed(seed)
    plan = focus_plan(B, steps, lens, dual) if plan is None else plan
    mask = (torch.arange(Ti)[None, None, :] < torch.as_tensor(np.asarray(lens, np.int64))[:, None, None]).double()
    ta = []
    for m in range(2 if dual else 1):
        a = torch.rand(B, steps, Ti, generator=g, dtype=torch.float64) * mask
        a = (1.0 - weight) * a / a.sum(-1, keepdim=True)
        a.scatter_add_(2, torch.as_tensor(plan[m])[:, :, None], torch.full((B, steps, 1), weight, dtype=torch.float64))
        ta.append(a.float())
    return (ta[0], ta[1] if dual else None)


@contextlib.contextmanager
def seeded_start(rows):
    """DecodeSession.reset inside the body: the reset as it is, then the one-hot start of the forward variable moved from row 0 to
    rows[b] of sample b - in alpha_state[0], which the persistent kernel and the launch-per-layer steps both read at the first step,
    and in a group session's _galpha_state[:, 0] (group g holds samples 2 g, 2 g + 1; the padding sample starts where the last one
    does).  A forward-attention run moves at most one row per step from where it starts: seeded, 16 steps weight the high rows"""
    from satt_amd.inference import DecodeSession
    real = DecodeSession.reset

    def reset(self):
        real(self)
        at = [int(r) for r in rows]
        assert len(at) == self.B and all(0 <= r < self.Ti for r in at), (at, self.B, self.Ti)
        self.alpha_state[0].zero_()
        for b, r in enumerate(at):
            self.alpha_state[0, b, r] = 1.0
        if self.mega_groups is not None:
            self._galpha_state[:, 0].zero_()
            for b in range(self.Ba):
                self._galpha_state[b // 2, 0, b % 2, at[min(b, self.B - 1)]] = 1.0
    DecodeSession.reset = reset
    try:
        yield
    finally:
        DecodeSession.reset = real


# ---- the frozen float64 decode vectors (tests/golden/decode_ljspeech_*.npz)
# (mel abs, stop abs, alignment rows abs, per-step mean |mel| abs, argmax path agreement)
# measured (MI355X, r5): bf16 mel 7.4e-4 (the float64 oracle with bf16-rounded weights: 7.7e-4 - the path sits AT the rounding floor
# of its weights), stop 1.5e-4, alignment rows 4.0e-4, drift 2.5e-5, path 0.995; f32 mode (recurrent weights are consumed as bf16 in
# both modes): mel 2.0e-4, stop 2.3e-5, alignment rows 8.0e-5, drift 1.1e-5, path 1.000
GOLDEN_BARS = {"bf16": dict(mel=2.2e-3, stop=4.5e-4, align=1.2e-3, drift=8e-5, path=0.985),
               "f32": dict(mel=6e-4, stop=7e-5, align=2.5e-4, drift=3.5e-5, path=0.995)}


def golden_engine(z, prec, stop_shift=0.0, case="", cfg_kw=None, sharpen=None):
    """(cfg, engine) of the fixture `z`: its parameters (sharpened for the *_sharp cases), its moving statistics, precision `prec`;
    cfg_kw / sharpen: the model and the sharpening of a tests/golden/decode_rows_*.npz case, whose parameters are common.make_params'"""
    from satt_amd import ops
    from satt_amd.engine import Engine
    from satt_amd.params import ModelConfig, init_params
    if cfg_kw is None:
        cfg = ModelConfig()
        P = dict(init_params(cfg, int(z["param_seed"])))
    else:          # (make_decode_rows_golden.case_params)
        cfg, P = make_params(cfg_kw, seed=int(z["param_seed"]), bias_noise=0.0)
        P = dict(P)
    if sharpen:
        from golden.make_bench_golden import sharpen_params
        P = sharpen_params(P, **sharpen)
    if case.endswith("_sharp"):
        from golden.make_bench_golden import sharpen_params
        from golden.make_decode_golden import CASES
        P = sharpen_params(P, **CASES[case]["sharpen"])
    if stop_shift:
        b = np.array(P["dec.out.b"], dtype=np.float32).copy()
        b[-1] += np.float32(stop_shift)
        P["dec.out.b"] = b
    ops.set_precision(prec)
    eng = Engine(cfg, "cuda", params=P, rng_seed=7)
    for name, (mean, var) in eng.bn.items():
        mean.copy_(torch.as_tensor(z["bn_mean." + name])); var.copy_(torch.as_tensor(z["bn_var." + name]))
    return cfg, eng
