#!/usr/bin/env python
"""Turn the predicted mel spectrograms of a directory into audio by Griffin-Lim phase reconstruction - a quick listen, not a vocoder.

Usage: mel_to_wav.py --hparam-json-file=<hparams.json> [--hparams=<a=b>] [--backend=hip|numpy] [--iters=<N>] [--alpha=<a>]
                     [--power=<P>] [--seed=<s>] [--inversion=pinv|nnls] [--nnls-iters=<N>] <in_dir> <out_dir>

Every `<key>.mfbsp` of <in_dir> (predict_mel.py's output: raw little-endian float32 [T, num_mels], normalised log-mel) becomes
`<out_dir>/<key>.wav`: 16-bit PCM at hparams.sample_rate, (T - 1) * hop samples, the peak scaled to 0.95.  The spectrogram is
de-normalised with average_mel_level_db / stddev_mel_level_db - the hparams.json must be the one the preprocessing run wrote -
mapped to linear magnitudes through the pseudo-inverse of the mel basis and handed to Griffin-Lim (csrc/griffin_lim.hip on the
"hip" backend, all utterances in one entry call; a float32 scipy.fft restatement on "numpy").  --inversion nnls refines the
floored pseudo-inverse by --nnls-iters (64) iterations of a non-negative solve, so that the magnitudes handed to Griffin-Lim have
the band amplitudes of the mel (csrc/mel_nnls.hip, all utterances in one launch; float32 NumPy with the same bits on "numpy")."""
import argparse
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
    ap.add_argument("--iters", type=int, default=60, metavar="N", help="Griffin-Lim iterations (default 60)")
    ap.add_argument("--alpha", type=float, default=0.99, help="momentum: 0 = classic Griffin-Lim, 0.99 = the fast variant (default)")
    ap.add_argument("--power", type=float, default=1.0, metavar="P", help="exponent on the linear magnitudes (default 1.0)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the initial phase (default 0)")
    ap.add_argument("--inversion", choices=("pinv", "nnls"), default="pinv",
                    help="mel -> linear magnitudes: the floored pseudo-inverse (default) or the non-negative solve that starts from it")
    ap.add_argument("--nnls-iters", type=int, default=64, metavar="N", help="iterations of --inversion nnls (default 64)")
    ap.add_argument("in_dir")
    ap.add_argument("out_dir")
    a = ap.parse_args(argv)
    if a.iters < 0:
        raise SystemExit("--iters: >= 0")
    if not 0 <= a.nnls_iters <= 1024:
        raise SystemExit("--nnls-iters: 0 .. 1024")

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import satt_amd  # noqa: F401
    from satt_amd.hparams import hparams
    from satt_amd.utils.audio import Audio

    text = open(a.hparam_json_file).read()
    missing = [k for k in ("average_mel_level_db", "stddev_mel_level_db") if k not in json.loads(text)]
    if missing:
        raise SystemExit("%s holds no %s: pass the hparams.json that the preprocessing run wrote (the corpus statistics de-normalise "
                         "the spectrograms)" % (a.hparam_json_file, " / ".join(missing)))
    hparams.parse_json(text)
    hparams.parse(a.hparams)
    audio = Audio(hparams, backend=a.backend)
    paths = sorted(glob.glob(os.path.join(a.in_dir, "*.%s" % hparams.predicted_mel_extension)))
    if not paths:
        raise SystemExit("no *.%s under %s" % (hparams.predicted_mel_extension, a.in_dir))
    mels = [audio.denormalize_mel(np.fromfile(p, dtype="<f4").reshape(-1, hparams.num_mels)) for p in paths]
    os.makedirs(a.out_dir, exist_ok=True)
    wavs = audio.inv_melspectrogram_batch(mels, iters=a.iters, alpha=a.alpha, power=a.power, seed=a.seed, inversion=a.inversion,
                                          nnls_iters=a.nnls_iters)
    for p, w in zip(paths, wavs):
        key = os.path.basename(p)[:-len(hparams.predicted_mel_extension) - 1]
        audio.save_wav_pcm16(w, os.path.join(a.out_dir, key + ".wav"))
        print("%s: %d samples" % (key, len(w)))


if __name__ == "__main__":
    main()
