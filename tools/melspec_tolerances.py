"""Measure the deviation from the float64 yardstick (tests/audio_common.py) over the inputs of tests/test_melspec_gpu.py:
the float32 NumPy backend always (needs no GPU - C_MAG and C_DB of audio_common are 8 x its worst case), the kernel with --hip.
    python tools/melspec_tolerances.py [--hip]          (profiles/melspec_tolerances.txt holds a recorded run)"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import audio_common as ac  # noqa: E402
import satt_amd  # noqa: E402,F401
from satt_amd.utils import audio  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hip", action="store_true", help="measure the kernel as well (needs the GPU)")
    args = ap.parse_args()
    worst = {}
    for name, (sr, n_fft, win, hop, mels) in ac.CONFIGS.items():
        tables = audio.MelspecTables(sr, n_fft, win, hop, mels)
        basis64 = ac.slaney_basis(sr, n_fft, mels)
        ys = ac.kernel_cases(name)
        got = {"numpy": [audio.melspec_numpy(tables, y, ac.REF_LEVEL_DB, want_mag=True) for y in ys]}
        if args.hip:
            m, g = audio.melspec_hip(tables, ys, ac.REF_LEVEL_DB, want_mag=True)
            got["hip"] = list(zip(m, g))
        for backend, res in got.items():
            e_mag = e_db = 0.0
            amin = np.inf
            for y, (db, mag) in zip(ys, res):
                mag64 = ac.yardstick_mag(y, n_fft, hop, win)
                db64, amp = ac.yardstick_db(mag64, basis64)
                amin = min(amin, amp.min())
                e_mag = max(e_mag, ac.frame_errors(mag, mag64).max())
                e_db = max(e_db, np.abs(db - db64).max())
            worst[backend] = (max(worst.get(backend, (0, 0))[0], e_mag), max(worst.get(backend, (0, 0))[1], e_db))
            print("%-26s %-5s mag %.3e of the frame maximum   dB %.3e   (smallest float64 mel amplitude %.2e, %d signals)"
                  % (name, backend, e_mag, e_db, amin, len(ys)))
    for backend, (e_mag, e_db) in worst.items():
        print("worst %-5s mag %.3e  dB %.3e" % (backend, e_mag, e_db))
    print("C_MAG %.3e  C_DB %.3e" % (ac.C_MAG, ac.C_DB))


if __name__ == "__main__":
    main()
