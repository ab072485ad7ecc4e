"""What the two corpus drivers share: record writers, the per-bin mel statistics, the batched target pass and the command line.
The reference maps utterances over Spark workers; here file I/O runs on a thread pool of at most 16 workers and the mel
spectrograms of a chunk of utterances go through Audio.melspectrogram_batch - one GPU stream, a few launches per chunk.  With
--resample the chunk's wavs are read at their own rates and go through Audio.resample_batch in front of that."""
import argparse
import csv
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from ..utils import tfrecord

MAX_WORKERS = 16
CHUNK = 64                    # utterances loaded, transformed and written together


def write_target_record(id_, key, mel, filename):
    """`<key>.target.tfrecord` (reference preprocess/ljspeech.py:23-32): id, key, mel (raw float32 [T, num_mels]), target_length,
    mel_width"""
    mel = np.ascontiguousarray(mel, dtype="<f4")
    tfrecord.write_records(filename, [tfrecord.make_example({
        "id": int(id_), "key": key.encode("utf-8"), "mel": mel.tobytes(), "target_length": int(mel.shape[0]),
        "mel_width": int(mel.shape[1])})])


def write_source_record(id_, key, source, text, filename, **speaker):
    """`<key>.source.tfrecord`: id, key, source (raw int64), source_length, text [, speaker_id, age, gender]"""
    tfrecord.write_records(filename, [tfrecord.make_source_example(id_, key, np.asarray(source, np.int64), text,
                                                                   **{k: int(v) for k, v in speaker.items()})])


class MelStatistics:
    """per-bin sum, second moment and minimum over every frame of the corpus, accumulated in float64"""

    def __init__(self, width):
        self.sum, self.moment2 = np.zeros(width, np.float64), np.zeros(width, np.float64)
        self.min = np.full(width, np.inf)
        self.frames = 0

    def add(self, mel):
        m = mel.astype(np.float64)
        self.sum += m.sum(axis=0)
        self.moment2 += np.square(m).sum(axis=0)
        self.min = np.minimum(self.min, m.min(axis=0))
        self.frames += len(m)

    def average(self):
        return self.sum / self.frames

    def stddev(self):
        return np.sqrt(self.moment2 / self.frames - np.square(self.average()))


def workers():
    return max(1, min(MAX_WORKERS, os.cpu_count() or 1))


def load_chunk(pool, chunk, audio, post=None):
    """the signals of a chunk of records (objects with .key and .wav_path) at hparams.sample_rate, behind `post` (a per-signal step
    such as Audio.trim, or None).  Without audio.resample every file goes through Audio.load_wav on the pool.  With it the files
    are read at their own rates on the pool, Audio.resample_batch converts the chunk in one call, and `post` runs on the pool on
    the converted signals.  A signal too short for one frame is refused by its record's key."""
    post = post or (lambda wav: wav)
    if not audio.resample:
        wavs = list(pool.map(lambda rec: post(audio.load_wav(rec.wav_path)), chunk))
    else:
        read = list(pool.map(lambda rec: audio.read_wav(rec.wav_path), chunk))
        wavs = list(pool.map(post, audio.resample_batch([y for _, y in read], [rate for rate, _ in read])))
    need = audio.tables.n_fft // 2 + 1
    for rec, wav in zip(chunk, wavs):
        if len(wav) < need:
            raise ValueError("%s: %d samples, fewer than the %d a frame of n_fft = %d needs" % (rec.key, len(wav), need, audio.tables.n_fft))
    return wavs


def process_targets(records, audio, out_dir, post=None):
    """records: objects with .id, .key and .wav_path; post: a per-signal step between loading and the mel (see load_chunk).  Writes
    every target record and returns (keys, MelStatistics)."""
    stats = MelStatistics(audio.hparams.num_mels)
    with ThreadPoolExecutor(max_workers=workers()) as pool:
        for i in range(0, len(records), CHUNK):
            chunk = records[i:i + CHUNK]
            mels = audio.melspectrogram_batch(load_chunk(pool, chunk, audio, post))
            for mel in mels:
                stats.add(mel)
            list(pool.map(lambda rm: write_target_record(rm[0].id, rm[0].key, rm[1],
                                                         os.path.join(out_dir, "%s.target.tfrecord" % rm[0].key)), zip(chunk, mels)))
    return [r.key for r in records], stats


def process_sources(records, write):
    """write(record) -> key on the thread pool, in order"""
    with ThreadPoolExecutor(max_workers=workers()) as pool:
        return list(pool.map(write, records))


def write_hparams_json(out_dir, hparams, stats):
    """exactly the reference's eight keys (preprocess_ljspeech.py:70-79)"""
    obj = {
        "num_mels": hparams.num_mels,
        "num_freq": hparams.num_freq,
        "sample_rate": hparams.sample_rate,
        "frame_length_ms": hparams.frame_length_ms,
        "frame_shift_ms": hparams.frame_shift_ms,
        "average_mel_level_db": stats.average().tolist(),
        "stddev_mel_level_db": stats.stddev().tolist(),
        "min_mel_level_db": stats.min.tolist(),
    }
    with open(os.path.join(out_dir, "hparams.json"), "w") as f:
        json.dump(obj, f, indent=4)
    return obj


def write_list_csv(out_dir, keys):
    with open(os.path.join(out_dir, "list.csv"), "w", newline="") as f:
        w = csv.writer(f)
        for k in keys:
            w.writerow([k])


def parse_args(doc, argv=None, version=False):
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("in_dir")
    ap.add_argument("out_dir")
    ap.add_argument("--hparams", default="")
    ap.add_argument("--hparam-json-file", default=None)
    ap.add_argument("--source-only", action="store_true")
    ap.add_argument("--target-only", action="store_true")
    ap.add_argument("--backend", choices=("hip", "numpy"), default=None,
                    help="mel extraction: the HIP kernel (default when a GPU is bound) or the float32 NumPy restatement")
    ap.add_argument("--resample", action="store_true",
                    help="convert wavs whose rate differs from hparams.sample_rate (Kaiser-windowed sinc; without it they are refused)")
    if version:
        ap.add_argument("--version", default="0.8", help="VCTK release; only the 0.8 layout (wav48/, txt/, speaker-info.txt) is built")
    return ap.parse_args(argv)


def run(instance, a, hparams):
    """the body both drivers share (reference preprocess_ljspeech.py:43-86): sources, targets + hparams.json, list.csv"""
    if a.source_only and a.target_only:
        raise SystemExit("--source-only and --target-only exclude each other")
    os.makedirs(a.out_dir, exist_ok=True)
    records = instance.list_records()
    keys = [r.key for r in records]
    if not a.target_only:
        keys = instance.process_sources(records)
    if not a.source_only:
        keys, stats = instance.process_targets(records)
        print(json.dumps(write_hparams_json(a.out_dir, hparams, stats), indent=4))
    write_list_csv(a.out_dir, keys)
    return keys
