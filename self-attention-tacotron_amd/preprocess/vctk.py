"""VCTK (release 0.8 layout) -> record files (the behaviour of reference preprocess/vctk.py): `speaker-info.txt` gives id, age and
gender (F -> 0, anything else -> 1; the header line and speaker 315 are left out), the sorted `txt/p<ID>/*.txt` pair with the
sorted `wav48/p<ID>/*.wav`, the audio is trimmed before the mel, text goes through the basic cleaners, and the source records
also carry speaker_id, age and gender."""
import os
from collections import namedtuple

import numpy as np

from . import corpus
from .cleaners import basic_cleaners
from .text import text_to_sequence
from ..utils.audio import Audio

SpeakerInfo = namedtuple("SpeakerInfo", ["id", "age", "gender"])
TxtWavRecord = namedtuple("TxtWavRecord", ["id", "key", "txt_path", "wav_path", "speaker_info"])


class VCTK:
    def __init__(self, in_dir, out_dir, hparams, speaker_info_filename="speaker-info.txt", backend=None, resample=False):
        self.in_dir, self.out_dir, self.speaker_info_filename = in_dir, out_dir, speaker_info_filename
        self.audio = Audio(hparams, backend=backend, resample=resample)

    def load_speaker_info(self):
        with open(os.path.join(self.in_dir, self.speaker_info_filename), mode="r", encoding="utf8") as f:
            for line in f.readlines()[1:]:
                si = line.split()
                if len(si) < 3 or si[0] == "315":             # the reference leaves speaker 315 out (its txt/ directory is missing)
                    continue
                yield SpeakerInfo(int(si[0]), int(si[1]), 0 if si[2] == "F" else 1)

    def list_records(self):
        def files(sub, si, ext):
            d = os.path.join(self.in_dir, sub, "p%d" % si.id)
            return [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith(ext)]

        out = []
        for si in self.load_speaker_info():
            txts, wavs = files("txt", si, ".txt"), files("wav48", si, ".wav")
            assert len(txts) == len(wavs), "speaker %d: %d txt files, %d wav files" % (si.id, len(txts), len(wavs))
            for t, w in zip(txts, wavs):
                key = os.path.splitext(os.path.basename(w))[0]
                assert key == os.path.splitext(os.path.basename(t))[0], (t, w)
                out.append(TxtWavRecord(len(out), key, t, w, si))
        return out

    def process_sources(self, records):
        def write(rec):
            with open(rec.txt_path, mode="r", encoding="utf8") as f:
                txt = f.readline().rstrip("\n")
            seq, clean = text_to_sequence(txt, basic_cleaners, key=rec.key)
            corpus.write_source_record(rec.id, rec.key, np.asarray(seq, np.int64), clean,
                                       os.path.join(self.out_dir, "%s.source.tfrecord" % rec.key),
                                       speaker_id=rec.speaker_info.id, age=rec.speaker_info.age, gender=rec.speaker_info.gender)
            return rec.key
        return corpus.process_sources(records, write)

    def process_targets(self, records):
        return corpus.process_targets(records, self.audio, self.out_dir, self.audio.trim)      # with --resample: trim after it
