#!/usr/bin/env python
"""Preprocess the VCTK corpus, with the reference's command line (reference preprocess_vctk.py:7-16).

Usage: preprocess_vctk.py [--hparams=<a=b,c=d>] [--hparam-json-file=<path>] [--version=0.8] [--source-only] [--target-only]
                          [--backend=hip|numpy] [--resample] <in_dir> <out_dir>

Reads `<in_dir>/speaker-info.txt`, `<in_dir>/txt/p<ID>/*.txt` and `<in_dir>/wav48/p<ID>/*.wav` (48000 Hz mono, the hparams
defaults), trims leading and trailing silence, and writes `<key>.source.tfrecord` (with speaker_id, age, gender),
`<key>.target.tfrecord`, `list.csv` and, unless --source-only, `hparams.json` with the per-bin mel statistics.
The log-mel spectrograms run in the HIP kernel (csrc/melspec.hip); --backend numpy needs no GPU.  With --resample, wavs at another
rate than hparams.sample_rate are converted (csrc/resample.hip) before the trim; without it they are refused."""
import os
import sys


def main(argv=None):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import satt_amd  # noqa: F401
    from satt_amd.hparams import hparams, hparams_debug_string
    from satt_amd.preprocess import corpus
    from satt_amd.preprocess.vctk import VCTK

    a = corpus.parse_args(__doc__, argv, version=True)
    if a.version != "0.8":
        raise SystemExit("Supported version of VCTK: 0.8 (the 0.91 layout is not built)")
    if a.hparam_json_file:
        hparams.parse_json(open(a.hparam_json_file).read())
    hparams.parse(a.hparams)
    print(hparams_debug_string())
    corpus.run(VCTK(a.in_dir, a.out_dir, hparams, backend=a.backend, resample=a.resample), a, hparams)


if __name__ == "__main__":
    main()
