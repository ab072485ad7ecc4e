"""Measure the deviation of the non-negative mel inversion from the dense float64 iteration of tests/mel_nnls_common.py over
inputs(name) of that module - the inputs of tests/test_mel_nnls_cpu.py and tests/test_mel_nnls_gpu.py - at K = 1, 3, 64: the
float32 NumPy backend always (needs no GPU; WORST_NUMPY of mel_nnls_common is its worst case, rounded up, and C is 8 x that), the
kernel with --hip (it has the NumPy backend's bits, so its figures are the same).
    python tools/mel_nnls_tolerances.py [--hip]          (profiles/mel_nnls_tolerances.txt holds a recorded run)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import mel_nnls_common as mc  # noqa: E402
import satt_amd  # noqa: E402,F401
from satt_amd.utils import audio  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hip", action="store_true", help="measure the kernel as well (needs the GPU)")
    args = ap.parse_args()
    worst = {}
    for name in mc.NAMES:
        nt = audio.mel_nnls_tables(mc.tables(name))
        a, x0 = mc.inputs(name)
        print("%s: %d frames, %d bins, %d bands, %d weights, step %.6e" % (name, len(a), nt.num_bins, nt.num_mels, len(nt.band_weight), nt.step))
        for iters in mc.KS:
            x64 = mc.yardstick_of(name, iters)
            results = {"numpy": audio.mel_nnls_numpy(nt, a, x0, iters)}
            if args.hip:
                results["hip"] = audio.mel_nnls_hip(nt, a, x0, iters)
            line = "  K = %2d " % iters
            for k, x in results.items():
                e = mc.frame_errors(x, x64).max()
                worst[k] = max(worst.get(k, 0.0), e)
                line += "  %s %.3e of the frame maximum" % (k, e)
            if args.hip:
                line += "  (bits equal: %s)" % (results["hip"].tobytes() == results["numpy"].tobytes())
            print(line)
    for kind in mc.HAND:
        nt, B, a, x0 = mc.hand(kind)
        e = max(mc.frame_errors(audio.mel_nnls_numpy(nt, a, x0, iters), mc.yardstick(B, a, x0, iters)).max() for iters in mc.KS)
        print("hand-made %-5s (%d x %d, not part of the worst figure): numpy %.3e" % (kind, nt.num_mels, nt.num_bins, e))
    for k, w in worst.items():
        print("worst %-5s %.3e" % (k, w))
    print("WORST_NUMPY %.3e  C = 8 x = %.3e  (the worst figure must stay <= %.0e)" % (mc.WORST_NUMPY, mc.C, mc.WORST_ALLOWED))


if __name__ == "__main__":
    main()
