"""Corpus preprocessing (reference preprocess/): text front end, LJSpeech and VCTK record writers.  No Spark, no TensorFlow:
file I/O on a thread pool, the log-mel spectrograms in batches through utils/audio.py (csrc/melspec.hip)."""
