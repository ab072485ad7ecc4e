#!/usr/bin/env python
"""Say how far the pitch of the predictions of a directory lies from that of their ground truth: YIN F0 tracks of both sides,
compared along the dynamic-time-warping path of their mel spectrograms.

Usage: evaluate_f0.py --hparam-json-file=<hparams.json> [--hparams=<a=b>] [--backend=hip|numpy] [--fmin=<Hz>] [--fmax=<Hz>]
                      [--window-ms=<ms>] [--threshold=<x>] [--silence-db=<dB>] [--iters=<N>] [--seed=<S>]
                      [--tracker=yin|viterbi] [--jump-cost=<x>] [--switch-cost=<x>] [--unvoiced-cost=<x>] [--lag-bias=<x>]
                      [--inversion=pinv|nnls] [--nnls-iters=<N>]
                      [--pred-wav-dir=<D> --ref-wav-dir=<D>] [--write-tracks] <prediction_dir> [<out_dir>]

Default mode: every `<key>.tfrecord` of <prediction_dir> (predict_mel.py's prediction record) holds the predicted `mel` and, when the
run had a --target-data-root, the `ground_truth_mel`; records without one are listed and skipped.  The predicted AND the ground-truth
mel both go through Audio.inv_melspectrogram_batch (Griffin-Lim) with the same --iters (default 60) and --seed (default 0), so the
phase reconstruction biases both sides alike; --inversion nnls (default pinv) gives both sides the non-negative mel inversion of
--nnls-iters (64) iterations in front of it (csrc/mel_nnls.hip; summary.json then holds inversion and nnls_iters, a summary without
`inversion` is a pinv run); F0 is tracked on both signals and the path comes from Audio.mel_distance_batch on the
record's mels.  The hparams.json must be the one the preprocessing run wrote (the corpus statistics de-normalise the mels).
Wav mode (--pred-wav-dir and --ref-wav-dir, both): the `<key>.wav` files of the two directories are matched by basename, unmatched
keys are listed and skipped; the wavs are read with Audio.load_wav, their mels come from melspectrogram_batch + normalize_mel, and
path and F0 both come from the wavs.  <prediction_dir> is then only the default <out_dir>.

The tracker is YIN on the mel frame grid (utils/pitch.py; csrc/yin.hip on the "hip" backend, one launch per batch; a float32 NumPy
restatement on "numpy", the same bits): lags floor(sr / fmax) .. ceil(sr / fmin) (defaults 500 and 60 Hz), a window of --window-ms
(25), threshold 0.15; a frame is voiced when a lag passes the threshold and its power lies less than --silence-db (50) below the
loudest frame.  These are arguments of this tool, not hparams.  Per key on stdout and in <out_dir>/f0_distance.csv (default
<out_dir>: <prediction_dir>): key, frames_pred, frames_ref, steps, voiced_both, vuv_error, f0_rmse_cents, f0_rmse_hz, log_f0_corr,
gpe (empty where undefined: no step voiced on both sides; the correlation below 2 such steps or at zero variance);
<out_dir>/summary.json: count, the means over the keys where defined, the voiced-step-weighted RMSEs, every parameter, and the skipped
keys.  --write-tracks adds <key>.f0.npz with both tracks and the path.

--tracker yin (the default) decides every frame alone and has no octave-error smoothing: on Griffin-Lim audio it reports the octave
above wherever the fundamental is weak.  --tracker viterbi keeps the 8 deepest dips of d' of every frame and chooses among them and
an "unvoiced" state along the utterance by dynamic programming (csrc/f0_viterbi.hip, or its NumPy restatement: the same bits):
an octave between neighbouring frames costs --jump-cost (0.3), entering or leaving "unvoiced" --switch-cost (0.1), an unvoiced frame
--unvoiced-cost (default: the value of --threshold), and a candidate d' + --lag-bias (0.1) * period / longest lag.  A frame is then
voiced when the path takes a candidate there; utterances of more than 2048 frames are refused.  summary.json then also holds
tracker and the four costs (a summary without `tracker` is a yin run), and --write-tracks the state track of both sides.  Neither
tracker is WORLD or pYIN: values compare between runs of this tool with the same tracker only."""
import argparse
import csv
import glob
import json
import math
import os
import sys

import numpy as np

METRICS = ("vuv_error", "f0_rmse_cents", "f0_rmse_hz", "log_f0_corr", "gpe")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--hparam-json-file", required=True)
    ap.add_argument("--hparams", default="")
    ap.add_argument("--backend", choices=("hip", "numpy"), default=None, help="default: hip when a GPU is there, else numpy")
    ap.add_argument("--fmin", type=float, default=None, metavar="HZ")
    ap.add_argument("--fmax", type=float, default=None, metavar="HZ")
    ap.add_argument("--window-ms", type=float, default=None, metavar="MS")
    ap.add_argument("--threshold", type=float, default=None)
    ap.add_argument("--silence-db", type=float, default=None, metavar="DB")
    ap.add_argument("--iters", type=int, default=60, metavar="N", help="Griffin-Lim iterations of both sides (default mode)")
    ap.add_argument("--seed", type=int, default=0, metavar="S", help="seed of the starting phase of both sides (default mode)")
    ap.add_argument("--tracker", choices=("yin", "viterbi"), default="yin")
    ap.add_argument("--jump-cost", type=float, default=None, help="viterbi: the cost of an octave between neighbouring frames")
    ap.add_argument("--switch-cost", type=float, default=None, help="viterbi: the cost of entering or leaving the unvoiced state")
    ap.add_argument("--unvoiced-cost", type=float, default=None, help="viterbi: the cost of an unvoiced frame (default: --threshold)")
    ap.add_argument("--lag-bias", type=float, default=None, help="viterbi: added to a candidate's d', times period / longest lag")
    ap.add_argument("--inversion", choices=("pinv", "nnls"), default="pinv",
                    help="mel -> linear magnitudes of both sides (default mode): the floored pseudo-inverse or the non-negative solve")
    ap.add_argument("--nnls-iters", type=int, default=64, metavar="N", help="iterations of --inversion nnls (default 64)")
    ap.add_argument("--pred-wav-dir", default=None, metavar="D")
    ap.add_argument("--ref-wav-dir", default=None, metavar="D")
    ap.add_argument("--write-tracks", action="store_true", help="write <key>.f0.npz with both tracks and the path")
    ap.add_argument("prediction_dir")
    ap.add_argument("out_dir", nargs="?", default=None)
    a = ap.parse_args(argv)
    if (a.pred_wav_dir is None) != (a.ref_wav_dir is None):
        raise SystemExit("--pred-wav-dir and --ref-wav-dir go together")
    if not 0 <= a.nnls_iters <= 1024:
        raise SystemExit("--nnls-iters: 0 .. 1024")
    if a.inversion == "nnls" and a.pred_wav_dir is not None:
        raise SystemExit("--inversion belongs to the default mode: wav mode inverts no mel")

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import satt_amd  # noqa: F401
    from satt_amd.hparams import hparams
    from satt_amd.utils import pitch, tfrecord
    from satt_amd.utils.audio import Audio

    text = open(a.hparam_json_file).read()
    missing = [k for k in ("average_mel_level_db", "stddev_mel_level_db") if k not in json.loads(text)]
    if missing:
        raise SystemExit("%s holds no %s: pass the hparams.json that the preprocessing run wrote (the corpus statistics de-normalise "
                         "the spectrograms)" % (a.hparam_json_file, " / ".join(missing)))
    hparams.parse_json(text)
    hparams.parse(a.hparams)
    audio = Audio(hparams, backend=a.backend)
    par = dict(fmin=pitch.FMIN if a.fmin is None else a.fmin, fmax=pitch.FMAX if a.fmax is None else a.fmax,
               window_ms=pitch.WINDOW_MS if a.window_ms is None else a.window_ms,
               threshold=pitch.THRESHOLD if a.threshold is None else a.threshold,
               silence_db=pitch.SILENCE_DB if a.silence_db is None else a.silence_db)
    costs = {}
    if a.tracker == "viterbi":
        costs = dict(tracker=a.tracker, jump_cost=pitch.JUMP_COST if a.jump_cost is None else a.jump_cost,
                     switch_cost=pitch.SWITCH_COST if a.switch_cost is None else a.switch_cost,
                     unvoiced_cost=par["threshold"] if a.unvoiced_cost is None else a.unvoiced_cost,
                     lag_bias=pitch.LAG_BIAS if a.lag_bias is None else a.lag_bias)
    elif not all(v is None for v in (a.jump_cost, a.switch_cost, a.unvoiced_cost, a.lag_bias)):
        raise SystemExit("--jump-cost, --switch-cost, --unvoiced-cost and --lag-bias belong to --tracker viterbi")

    skipped = []
    if a.pred_wav_dir is not None:
        mode = "wav"
        names = [{os.path.basename(p)[:-4] for p in glob.glob(os.path.join(d, "*.wav"))} for d in (a.pred_wav_dir, a.ref_wav_dir)]
        keys, skipped = sorted(names[0] & names[1]), sorted(names[0] ^ names[1])
        for key in skipped:
            print("%s: in %s only, skipped" % (key, a.pred_wav_dir if key in names[0] else a.ref_wav_dir))
        if not keys:
            raise SystemExit("no <key>.wav is in both %s and %s" % (a.pred_wav_dir, a.ref_wav_dir))
        sig_pred = [audio.load_wav(os.path.join(a.pred_wav_dir, k + ".wav")) for k in keys]
        sig_ref = [audio.load_wav(os.path.join(a.ref_wav_dir, k + ".wav")) for k in keys]
        mels = [audio.normalize_mel(S).astype(np.float32) for S in audio.melspectrogram_batch(sig_pred + sig_ref)]
        preds, refs = mels[:len(keys)], mels[len(keys):]
    else:
        mode = "griffin_lim"
        paths = sorted(glob.glob(os.path.join(a.prediction_dir, "*.tfrecord")))
        if not paths:
            raise SystemExit("no *.tfrecord under %s" % a.prediction_dir)
        keys, preds, refs = [], [], []
        for p in paths:
            r = tfrecord.parse_prediction_result(next(tfrecord.read_records(p)))
            if r["ground_truth_mel"].shape[0] == 0:
                skipped.append(r["key"])
                continue
            keys.append(r["key"])
            preds.append(r["mel"])
            refs.append(r["ground_truth_mel"])
        for key in skipped:
            print("%s: no ground-truth mel, skipped" % key)
        if not keys:
            raise SystemExit("none of the %d records under %s holds a ground-truth mel: run predict_mel.py with --target-data-root"
                             % (len(paths), a.prediction_dir))
        for key, S in zip(keys + keys, preds + refs):
            if not np.isfinite(S).all():
                raise ValueError("%s: a mel holds non-finite values" % key)
        wavs = audio.inv_melspectrogram_batch([audio.denormalize_mel(np.asarray(S, np.float64)) for S in preds + refs],
                                              iters=a.iters, seed=a.seed, inversion=a.inversion, nnls_iters=a.nnls_iters)
        sig_pred, sig_ref = wavs[:len(keys)], wavs[len(keys):]
    dist = audio.mel_distance_batch(preds, refs, want_paths=True, keys=keys)
    tracks = audio.f0_batch(sig_pred + sig_ref, **par, **costs)
    tr_pred, tr_ref = tracks[:len(keys)], tracks[len(keys):]

    out_dir = a.out_dir or a.prediction_dir
    os.makedirs(out_dir, exist_ok=True)
    rows = []
    cell = lambda v: "" if v is None else repr(v)
    with open(os.path.join(out_dir, "f0_distance.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["key", "frames_pred", "frames_ref", "steps", "voiced_both"] + list(METRICS))
        for key, d, tp, tr in zip(keys, dist, tr_pred, tr_ref):
            if (len(tp["f0"]), len(tr["f0"])) != (d["frames_pred"], d["frames_ref"]):
                raise ValueError("%s: %d / %d F0 frames against %d / %d mel frames" % (key, len(tp["f0"]), len(tr["f0"]), d["frames_pred"], d["frames_ref"]))
            m = pitch.f0_metrics(tp["f0"], tp["voiced"], tr["f0"], tr["voiced"], d["path"])
            rows.append(m)
            w.writerow([key, d["frames_pred"], d["frames_ref"], m["steps"], m["voiced_both"]] + [cell(m[k]) for k in METRICS])
            print("%s: %d frames against %d, %d steps, %d voiced on both sides, V/UV error %.4f, %s" % (
                key, d["frames_pred"], d["frames_ref"], m["steps"], m["voiced_both"], m["vuv_error"],
                "no F0 to compare" if m["f0_rmse_cents"] is None else "F0 RMSE %.2f cents" % m["f0_rmse_cents"]))
            if a.write_tracks:
                np.savez(os.path.join(out_dir, key + ".f0.npz"), path=d["path"], **{"%s_%s" % (k, side): t[k] for side, t in (("pred", tp), ("ref", tr)) for k in t})

    def mean(k):
        v = [m[k] for m in rows if m[k] is not None]
        return float(np.mean(v)) if v else None

    def weighted(k):
        nb = sum(m["voiced_both"] for m in rows)
        return math.sqrt(sum(m["voiced_both"] * m[k] ** 2 for m in rows if m[k] is not None) / nb) if nb else None
    inv = dict(inversion=a.inversion, nnls_iters=a.nnls_iters) if a.inversion != "pinv" else {}
    summary = dict(count=len(rows), mode=mode, steps=sum(m["steps"] for m in rows), voiced_both=sum(m["voiced_both"] for m in rows),
                   mean={k: mean(k) for k in METRICS}, weighted_f0_rmse_cents=weighted("f0_rmse_cents"),
                   weighted_f0_rmse_hz=weighted("f0_rmse_hz"), sample_rate=hparams.sample_rate, hop=audio.tables.hop, **par, **costs,
                   iters=a.iters if mode == "griffin_lim" else None, seed=a.seed if mode == "griffin_lim" else None, **inv, skipped=skipped)
    with open(os.path.join(out_dir, "summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
    print("%d pairs, %d steps, %d voiced on both sides: mean V/UV error %.4f, voiced-step-weighted F0 RMSE %s cents"
          % (summary["count"], summary["steps"], summary["voiced_both"], summary["mean"]["vuv_error"],
             "-" if summary["weighted_f0_rmse_cents"] is None else "%.2f" % summary["weighted_f0_rmse_cents"]))


if __name__ == "__main__":
    main()
