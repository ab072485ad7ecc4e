#!/usr/bin/env python
"""Say how far the predicted mel spectrograms of a directory lie from their ground truth: a dynamic-time-warping alignment of every
pair and the mean distortion along its path.

Usage: evaluate_mel.py --hparam-json-file=<hparams.json> [--hparams=<a=b>] [--backend=hip|numpy] [--feature=mcep|mel]
                       [--order=<N>] [--write-paths] <prediction_dir> [<out_dir>]

Every `<key>.tfrecord` of <prediction_dir> (predict_mel.py's prediction record) holds the predicted `mel` and, when the run had a
--target-data-root, the `ground_truth_mel`; records without one are listed and skipped.  Both are normalised log-mel and are
de-normalised with average_mel_level_db / stddev_mel_level_db - the hparams.json must be the one the preprocessing run wrote.
--feature mcep (default): a cepstrum of the mel filterbank, coefficients 1 .. --order (default 13); the value is a mel-cepstral
distortion in dB.  --feature mel: the dB mel rows; the value is an RMS log-spectral distance in dB.  All pairs go through one
Audio.mel_distance_batch call (csrc/dtw.hip on the "hip" backend, one launch; a float32 NumPy restatement on "numpy", the same bits).
Per key on stdout and in <out_dir>/mel_distance.csv (default <out_dir>: <prediction_dir>): key, frames_pred, frames_ref, steps,
value; <out_dir>/summary.json: count, mean, step_weighted_mean (sum cost / sum steps, scaled as the values), mean_length_ratio
(frames_pred / frames_ref), feature, order, skipped.  --write-paths adds <key>.dtw.npz with path [steps, 2] = (predicted frame,
ground-truth frame).  The cepstrum is of this project's mel filterbank, not a WORLD / MGC cepstrum: values compare between runs of
this tool only."""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--hparam-json-file", required=True)
    ap.add_argument("--hparams", default="")
    ap.add_argument("--backend", choices=("hip", "numpy"), default=None, help="default: hip when a GPU is there, else numpy")
    ap.add_argument("--feature", choices=("mcep", "mel"), default="mcep")
    ap.add_argument("--order", type=int, default=13, metavar="N", help="cepstral coefficients 1 .. N (default 13; --feature mcep)")
    ap.add_argument("--write-paths", action="store_true", help="write <key>.dtw.npz with the warping path")
    ap.add_argument("prediction_dir")
    ap.add_argument("out_dir", nargs="?", default=None)
    a = ap.parse_args(argv)

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import satt_amd  # noqa: F401
    from satt_amd.hparams import hparams
    from satt_amd.utils import tfrecord
    from satt_amd.utils.audio import Audio

    text = open(a.hparam_json_file).read()
    missing = [k for k in ("average_mel_level_db", "stddev_mel_level_db") if k not in json.loads(text)]
    if missing:
        raise SystemExit("%s holds no %s: pass the hparams.json that the preprocessing run wrote (the corpus statistics de-normalise "
                         "the spectrograms)" % (a.hparam_json_file, " / ".join(missing)))
    hparams.parse_json(text)
    hparams.parse(a.hparams)
    audio = Audio(hparams, backend=a.backend)
    paths = sorted(glob.glob(os.path.join(a.prediction_dir, "*.tfrecord")))
    if not paths:
        raise SystemExit("no *.tfrecord under %s" % a.prediction_dir)
    keys, preds, refs, skipped = [], [], [], []
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
    res = audio.mel_distance_batch(preds, refs, feature=a.feature, order=a.order, want_paths=a.write_paths, keys=keys)

    out_dir = a.out_dir or a.prediction_dir
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "mel_distance.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["key", "frames_pred", "frames_ref", "steps", "value"])
        for key, r in zip(keys, res):
            w.writerow([key, r["frames_pred"], r["frames_ref"], r["steps"], repr(r["value"])])
            print("%s: %d frames against %d, %d steps, %.4f dB" % (key, r["frames_pred"], r["frames_ref"], r["steps"], r["value"]))
            if a.write_paths:
                np.savez(os.path.join(out_dir, key + ".dtw.npz"), path=r["path"])
    from satt_amd.utils.mel_distance import MCD_SCALE
    scale = MCD_SCALE if a.feature == "mcep" else 1.0 / np.sqrt(hparams.num_mels)       # cost / steps -> dB, as the values
    summary = dict(count=len(res), mean=float(np.mean([r["value"] for r in res])),
                   step_weighted_mean=float(scale * sum(r["cost"] for r in res) / sum(r["steps"] for r in res)),
                   mean_length_ratio=float(np.mean([r["frames_pred"] / r["frames_ref"] for r in res])),
                   feature=a.feature, order=a.order if a.feature == "mcep" else None, skipped=skipped)
    with open(os.path.join(out_dir, "summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
    print("%d pairs: mean %.4f dB, step-weighted mean %.4f dB, mean length ratio %.4f"
          % (summary["count"], summary["mean"], summary["step_weighted_mean"], summary["mean_length_ratio"]))


if __name__ == "__main__":
    main()
