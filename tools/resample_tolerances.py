"""Measure the deviation from the float64 yardstick (tests/resample_common.py) over cases() of that module - the inputs of
tests/test_resample_cpu.py and tests/test_resample_gpu.py: the float32 NumPy backend always (needs no GPU - E_NUMPY of
resample_common is its worst case, rounded up), the kernel with --hip; and the tones of test_resample_cpu.py in dB.
    python tools/resample_tolerances.py [--hip]          (profiles/resample_tolerances.txt holds a recorded run)"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import resample_common as rc  # noqa: E402
import satt_amd  # noqa: E402,F401
from satt_amd.utils import audio  # noqa: E402

PASS_BAND = [(22050, 16000, 1000.0), (22050, 16000, 7000.0), (48000, 16000, 7000.0), (16000, 22050, 7000.0)]
STOP_BAND = [(22050, 16000, 8500.0), (22050, 16000, 10500.0), (48000, 16000, 9000.0)]


def tone_levels(run, a, b, hz, amplitude=0.5):
    """(error against the same sine at rate b, level of the output), both in dB re the amplitude, over the middle half of the output
    of half a second of tone"""
    y = run(audio.resample_tables(a, b), rc.tone(a // 2, a, hz, amplitude)).astype(np.float64)
    mid = slice(len(y) // 4, 3 * len(y) // 4)
    want = amplitude * np.sin(2.0 * np.pi * hz * np.arange(len(y)) / b)
    return rc.db(np.abs(y - want)[mid].max() / amplitude), rc.db(np.abs(y)[mid].max() / amplitude)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hip", action="store_true", help="measure the kernel as well (needs the GPU)")
    args = ap.parse_args()
    backends = {"numpy": audio.resample_numpy}
    if args.hip:
        backends["hip"] = lambda t, x: audio.resample_hip(t, [x])[0]
    worst = {k: 0.0 for k in backends}
    for name, a, b, x in rc.cases():
        y64 = rc.reference(name, a, b, x)
        line = "%-30s" % name
        for k, run in backends.items():
            e = rc.deviation(run(audio.resample_tables(a, b), x), y64)
            worst[k] = max(worst[k], e)
            line += "  %s %.3e" % (k, e)
        print(line + "   of the output maximum (%d outputs)" % len(y64))
    for k, e in worst.items():
        print("worst %-5s %.3e" % (k, e))
    print("E_NUMPY %.3e  C_NUMPY %.3e  C_KERNEL %.3e" % (rc.E_NUMPY, rc.C_NUMPY, rc.C_KERNEL))
    for a, b in rc.RATIOS:
        t = audio.resample_tables(a, b)
        rows = t.table.astype(np.float64).sum(axis=1)
        print("table %5d -> %5d  up / down %3d / %3d  taps %3d  %7d bytes  row sums within %.2e of 1" %
              (a, b, t.up, t.down, t.taps, t.table.nbytes, np.abs(rows - 1.0).max()))
    for k, run in backends.items():
        for a, b, hz in PASS_BAND:
            print("%-5s pass band %5d -> %5d %7.1f Hz: error %7.1f dB re the amplitude" % (k, a, b, hz, tone_levels(run, a, b, hz)[0]))
        for a, b, hz in STOP_BAND:
            print("%-5s stop band %5d -> %5d %7.1f Hz: output %7.1f dB re the amplitude" % (k, a, b, hz, tone_levels(run, a, b, hz)[1]))


if __name__ == "__main__":
    main()
