#!/usr/bin/env python
"""Preprocess the LJSpeech corpus, with the reference's command line (reference preprocess_ljspeech.py:7-15).

Usage: preprocess_ljspeech.py [--hparams=<a=b,c=d>] [--hparam-json-file=<path>] [--source-only] [--target-only]
                              [--backend=hip|numpy] [--resample] <in_dir> <out_dir>

Reads `<in_dir>/metadata.csv` and `<in_dir>/wavs/<key>.wav` (22050 Hz mono; pass examples/ljspeech/*.json with
--hparam-json-file for the LJSpeech audio parameters) and writes `<key>.source.tfrecord`, `<key>.target.tfrecord`, `list.csv` and,
unless --source-only, `hparams.json` with the per-bin mel statistics that train.py takes through --hparam-json-file.
The log-mel spectrograms run in the HIP kernel (csrc/melspec.hip); --backend numpy needs no GPU.  With --resample, wavs at another
rate than hparams.sample_rate are converted (csrc/resample.hip; e.g. --hparams sample_rate=16000,num_freq=513); without it they
are refused."""
import os
import sys


def main(argv=None):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import satt_amd  # noqa: F401
    from satt_amd.hparams import hparams, hparams_debug_string
    from satt_amd.preprocess import corpus
    from satt_amd.preprocess.ljspeech import LJSpeech

    a = corpus.parse_args(__doc__, argv)
    if a.hparam_json_file:
        hparams.parse_json(open(a.hparam_json_file).read())
    hparams.parse(a.hparams)
    print(hparams_debug_string())
    corpus.run(LJSpeech(a.in_dir, a.out_dir, hparams, backend=a.backend, resample=a.resample), a, hparams)


if __name__ == "__main__":
    main()
