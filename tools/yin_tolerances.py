"""Measure the deviation from the float64 yardstick (tests/pitch_common.py) over tone_set() of that module - the inputs of
tests/test_yin_cpu.py and tests/test_yin_gpu.py: the float32 NumPy backend always (needs no GPU; E_*_NUMPY of pitch_common are its
worst cases, rounded up), the kernel with --hip; and the float64 programme's own error in cents against the known periods, which
CENTS_64 of pitch_common rounds up.
    python tools/yin_tolerances.py [--hip]          (profiles/yin_tolerances.txt holds a recorded run)"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import pitch_common as pc  # noqa: E402
import satt_amd  # noqa: E402,F401
from satt_amd.utils import pitch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hip", action="store_true", help="measure the kernel as well (needs the GPU)")
    args = ap.parse_args()
    worst = {}
    worst_cents, frames, not_robust = 0.0, 0, 0
    for sr, hop in pc.CONFIGS:
        W, tau_min, tau_max = pc.sizes(sr)
        print("sr %d hop %d: W %d, lags %d .. %d" % (sr, hop, W, tau_min, tau_max))
        for period, y, ref in pc.tone_set(sr, hop):
            lead, inside = pc.frame_sets(sr, hop, len(y))
            c64 = np.abs(pc.cents(ref["f0"][inside], period, sr)).max()
            worst_cents = max(worst_cents, c64)
            frames += len(ref["robust"])
            not_robust += int((~ref["robust"]).sum())
            line = "  period %8.2f  %3d frames (%d lead-in, %d tone, %d not robust)  float64 %.3f cents, lead-in voiced %d" % (
                period, len(ref["f0"]), len(lead), len(inside), int((~ref["robust"]).sum()), c64, int((ref["f0"][lead] > 0).sum()))
            dp, power = pitch.yin_dprime_numpy(y, sr, hop)
            f0, apd = pitch.yin_pick_numpy(dp, sr, tau_min, tau_max)
            results = {"numpy": (f0, apd, power, dp)}
            if args.hip:
                results["hip"] = pitch.yin_hip([y], sr, hop)[0] + (None,)
            for k, r in results.items():
                e = pc.deviations(*r, ref)
                line += "\n      %-5s d' %s  power %.3e  f0 %.3e  aperiodicity %.3e  %.3f cents" % (
                    k, "%.3e" % e[0] if e[0] is not None else "    -    ", e[1], e[2], e[3], np.abs(pc.cents(r[0][inside], period, sr)).max())
                w = worst.setdefault(k, [0.0, 0.0, 0.0, 0.0])
                for i in range(4):
                    w[i] = max(w[i], e[i] or 0.0)
            print(line)
        for which, period in zip(("below tau_min", "above tau_max"), pc.outside(sr)):
            y = pc.tone(sr, period, 7)
            ref = pc.yin64(y, sr, hop)
            _, inside = pc.frame_sets(sr, hop, len(y))
            f = ref["f0"][inside]
            print("  period %8.2f (%s): float64 voiced on %d of %d tone frames%s" % (
                period, which, int((f > 0).sum()), len(f),
                ", %.3f cents from twice the period" % np.abs(pc.cents(f[f > 0], 2 * period, sr)).max() if (f > 0).any() else ""))
    for k, w in worst.items():
        print("worst %-5s d' %s  power %.3e  f0 %.3e  aperiodicity %.3e" % (k, "%.3e" % w[0] if k == "numpy" else "    -    ", w[1], w[2], w[3]))
    print("float64 worst %.3f cents; %d of %d frames not robust (%.4f)" % (worst_cents, not_robust, frames, not_robust / frames))
    print("E_DPRIME_NUMPY %.3e  E_POWER_NUMPY %.3e  E_F0_NUMPY %.3e  C_DPRIME %.3e  C_POWER %.3e  C_F0 %.3e  CENTS_64 %.3f  CENTS_BOUND %.3f"
          % (pc.E_DPRIME_NUMPY, pc.E_POWER_NUMPY, pc.E_F0_NUMPY, pc.C_DPRIME, pc.C_POWER, pc.C_F0, pc.CENTS_64, pc.CENTS_BOUND))


if __name__ == "__main__":
    main()
