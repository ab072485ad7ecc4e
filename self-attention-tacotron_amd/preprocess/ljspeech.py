"""LJSpeech -> record files (the behaviour of reference preprocess/ljspeech.py): `metadata.csv` lines `key|_|text`, the id is the
line index, audio at `wavs/<key>.wav`, text through the English cleaners."""
import os
from collections import namedtuple

import numpy as np

from . import corpus
from .cleaners import english_cleaners
from .text import text_to_sequence
from ..utils.audio import Audio

TextAndPath = namedtuple("TextAndPath", ["id", "key", "wav_path", "text"])


class LJSpeech:
    def __init__(self, in_dir, out_dir, hparams, backend=None, resample=False):
        self.in_dir, self.out_dir = in_dir, out_dir
        self.audio = Audio(hparams, backend=backend, resample=resample)

    def list_records(self):
        out = []
        with open(os.path.join(self.in_dir, "metadata.csv"), mode="r", encoding="utf-8") as f:
            for index, line in enumerate(f):
                parts = line.strip().split("|")
                if len(parts) < 3:
                    raise ValueError("metadata.csv line %d: expected key|_|text, got %r" % (index + 1, line))
                out.append(TextAndPath(index, parts[0], os.path.join(self.in_dir, "wavs", "%s.wav" % parts[0]), parts[2]))
        return out

    def process_sources(self, records):
        def write(rec):
            seq, clean = text_to_sequence(rec.text, english_cleaners, key=rec.key)
            corpus.write_source_record(rec.id, rec.key, np.asarray(seq, np.int64), clean,
                                       os.path.join(self.out_dir, "%s.source.tfrecord" % rec.key))
            return rec.key
        return corpus.process_sources(records, write)

    def process_targets(self, records):
        return corpus.process_targets(records, self.audio, self.out_dir)
