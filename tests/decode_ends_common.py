"""Shared by the suites of the per-utterance stop (satt_dec_ends_scan, infer(stop="each"), predict_mel.py --stop-per-utterance):
the NumPy model of the scan, input builders that keep every logit away from the threshold, and the small corpus of the driver test.
Not a test file."""
import math
import os

import numpy as np

MARGIN = 1e-3          # no stop logit of a test input lies this close to logit(threshold): the fp32 sigmoid cannot decide otherwise


def logit(p):
    return math.log(p / (1.0 - p))


def margin_ok(logits, thr):
    """every logit is at least MARGIN away from logit(thr)"""
    return bool((np.abs(np.asarray(logits, np.float64) - logit(thr)) >= MARGIN).all())


def numpy_ends(yout, t0, n, min_steps, thr, ends, flag):
    """one call of satt_dec_ends_scan on yout [B, rows, NO] (row t + 1 = step t) over steps t0 .. t0 + n - 1: (ends, flag) after it.
    sigmoid(x) > thr  <=>  x > logit(thr) - exact for inputs that keep MARGIN."""
    yout, ends = np.asarray(yout), np.array(ends, dtype=np.int64)
    if flag != 0:
        return ends, int(flag)
    assert t0 >= 0 and n >= 1 and t0 + n < yout.shape[1]
    t = np.arange(t0, t0 + n)
    fire = (yout[:, t0 + 1:t0 + n + 1, -1].astype(np.float64) > logit(thr)) & (t > min_steps)[None]
    first = np.where(fire.any(1), t[fire.argmax(1)] + 1, 0)
    ends = np.where(ends != 0, ends, first)
    return ends, int(ends.max()) if (ends != 0).all() else 0


def loop_ends(yout, t0, n, min_steps, thr, ends, flag):
    """the same, as the plain per-sample loop of the definition"""
    ends = [int(e) for e in ends]
    if flag != 0:
        return np.array(ends, dtype=np.int64), int(flag)
    for b in range(len(ends)):
        if ends[b] != 0:
            continue
        for t in range(t0, t0 + n):
            if t > min_steps and 1.0 / (1.0 + math.exp(-float(yout[b][t + 1][-1]))) > thr:
                ends[b] = t + 1
                break
    return np.array(ends, dtype=np.int64), (max(ends) if all(ends) else 0)


def ends_of_logits(logits, min_steps, thr, Td):
    """steps_each of a whole run from its full-length stop logits [B, T]: the scan in one window, Td where a sample never ends"""
    logits = np.asarray(logits)
    B, T = logits.shape
    y = np.zeros((B, T + 1, 1), np.float32)
    y[:, 1:, 0] = logits
    e, _ = numpy_ends(y, 0, T, min_steps, thr, np.zeros(B, np.int64), 0)
    return np.where(e > 0, e, Td)


def synthetic_yout(g, B, rows, NO, thr, fires=()):
    """random yout [B, rows, NO] whose stop logits all sit clearly BELOW logit(thr), except the (b, t) of `fires`, clearly above"""
    y = g.standard_normal((B, rows, NO)).astype(np.float32)
    y[:, :, -1] = (logit(thr) - 0.5 - np.abs(g.standard_normal((B, rows)))).astype(np.float32)
    for b, t in fires:
        y[b, t + 1, -1] = np.float32(logit(thr) + 0.5 + abs(g.standard_normal()))
    assert margin_ok(y[:, :, -1], thr)
    return y


def pick_threshold(logits, min_steps, launch, others=None):
    """a stop threshold for full-length stop logits [B, T], chosen from the gaps of their values so that with it at least two samples
    end at different steps inside the run, at least one end lies in a launch other than the first (more than `launch` steps) and no
    logit lies within MARGIN of the threshold's logit.  Among such gaps: as many samples ending as possible, then as many different
    ends, then the widest gap.  None if no gap does.  others: further logits that must keep MARGIN as well."""
    logits = np.asarray(logits, np.float64)
    vals = np.unique(logits if others is None else np.concatenate([logits.ravel(), np.asarray(others, np.float64).ravel()]))
    best = None
    for lo, hi in zip(vals[:-1], vals[1:]):
        if hi - lo < 2.5 * MARGIN:
            continue
        thr = float(np.float32(1.0 / (1.0 + math.exp(-0.5 * (lo + hi)))))
        if not 0.0 < thr < 1.0 or not margin_ok(vals, thr):
            continue
        e = ends_of_logits(logits, min_steps, thr, 0)
        ended = e[e > 0]
        if len(set(ended.tolist())) < 2 or ended.max() <= launch:
            continue
        score = (len(ended), len(set(ended.tolist())), hi - lo)
        if best is None or score > best[0]:
            best = (score, thr)
    return None if best is None else best[1]


def write_corpus(root, lengths):
    """a corpus of len(lengths) utterances with (source symbols, raw target frames) as given, the way tests/test_drivers_gpu.py
    builds its corpus; returns the keys"""
    from satt_amd.utils import tfrecord
    g = np.random.default_rng(0)
    keys = ["LJ%03d" % i for i in range(len(lengths))]
    for i, (k, (L, T)) in enumerate(zip(keys, lengths)):
        s = np.concatenate([[0], g.integers(1, 60, L - 2), [0]]).astype("<i8")
        tfrecord.write_records(os.path.join(root, k + ".source.tfrecord"), [tfrecord.make_example(
            {"id": i, "key": k.encode(), "source": s.tobytes(), "source_length": L, "text": b"abc"})])
        mel = g.normal(-40, 10, (T, 80)).astype("<f4")
        tfrecord.write_records(os.path.join(root, k + ".target.tfrecord"), [tfrecord.make_example(
            {"id": i, "key": k.encode(), "mel": mel.tobytes(), "mel_width": 80, "target_length": T})])
    return keys
