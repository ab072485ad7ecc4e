#!/usr/bin/env python
"""Write the LJSpeech corpus as the (normalised mel, wav) pairs a WaveNet vocoder trains on (the behaviour of the reference's
preprocess_ljspeech_wavenet.py).

Usage: preprocess_ljspeech_wavenet.py [--hparams=<a=b,c=d>] [--hparam-json-file=<path>] [--backend=hip|numpy] [--resample]
                                      <in_dir> <mel_out_dir> <wav_out_dir>

For every line of `<in_dir>/metadata.csv` it reads `<in_dir>/wavs/<key>.wav` and writes
  <mel_out_dir>/<key>.mfbsp   (S - average_mel_level_db) / stddev_mel_level_db as little-endian float32 [T, num_mels], T = 1 + n // hop
                              (the layout predict_mel.py writes)
  <wav_out_dir>/<key>.wav     the n samples the mel was computed from, float32 at hparams.sample_rate
average_mel_level_db / stddev_mel_level_db come from the hparams.json of a preprocess_ljspeech.py run at the same sample rate (pass
it with --hparam-json-file; it also carries that run's audio parameters).  With --resample,
wavs at another rate than hparams.sample_rate are converted (csrc/resample.hip: e.g. 22050 Hz LJSpeech for a 16 kHz WaveNet with
--hparams sample_rate=16000,num_freq=513); without it they are refused."""
import argparse
import os
import sys
from concurrent.futures import ThreadPoolExecutor


def main(argv=None):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import numpy as np
    import satt_amd  # noqa: F401
    from satt_amd.hparams import hparams, hparams_debug_string
    from satt_amd.preprocess import corpus
    from satt_amd.preprocess.ljspeech import LJSpeech

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("in_dir")
    ap.add_argument("mel_out_dir")
    ap.add_argument("wav_out_dir")
    ap.add_argument("--hparams", default="")
    ap.add_argument("--hparam-json-file", default=None)
    ap.add_argument("--backend", choices=("hip", "numpy"), default=None)
    ap.add_argument("--resample", action="store_true")
    a = ap.parse_args(argv)
    if a.hparam_json_file:
        hparams.parse_json(open(a.hparam_json_file).read())
    hparams.parse(a.hparams)
    print(hparams_debug_string())
    for name in ("average_mel_level_db", "stddev_mel_level_db"):
        if len(getattr(hparams, name)) != hparams.num_mels:
            raise SystemExit("hparams.%s has %d values, num_mels is %d: pass the hparams.json that preprocess_ljspeech.py wrote at this "
                             "sample rate with --hparam-json-file" % (name, len(getattr(hparams, name)), hparams.num_mels))

    lj = LJSpeech(a.in_dir, a.mel_out_dir, hparams, backend=a.backend, resample=a.resample)
    audio, records = lj.audio, lj.list_records()
    os.makedirs(a.mel_out_dir, exist_ok=True)
    os.makedirs(a.wav_out_dir, exist_ok=True)

    def write(item):
        rec, wav, mel = item
        np.ascontiguousarray(audio.normalize_mel(mel), dtype="<f4").tofile(os.path.join(a.mel_out_dir, "%s.mfbsp" % rec.key))
        audio.save_wav(np.ascontiguousarray(wav, np.float32), os.path.join(a.wav_out_dir, "%s.wav" % rec.key))
        return rec.key

    keys = []
    with ThreadPoolExecutor(max_workers=corpus.workers()) as pool:
        for i in range(0, len(records), corpus.CHUNK):
            chunk = records[i:i + corpus.CHUNK]
            wavs = corpus.load_chunk(pool, chunk, audio)
            keys += list(pool.map(write, zip(chunk, wavs, audio.melspectrogram_batch(wavs))))
    print("%d utterances: %s/<key>.mfbsp, %s/<key>.wav" % (len(keys), a.mel_out_dir, a.wav_out_dir))
    return keys


if __name__ == "__main__":
    main()
