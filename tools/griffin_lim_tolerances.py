"""Measure the deviation from the float64 yardstick (tests/griffin_lim_common.py: torch.stft / torch.istft) over the inputs of
tests/test_griffin_lim_gpu.py: the float32 NumPy backend always (needs no GPU - C_ISTFT and C_ITER are 8 x its worst case), the
kernel with --hip.
    python tools/griffin_lim_tolerances.py [--hip]          (profiles/griffin_lim_tolerances.txt holds a recorded run)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import audio_common as ac  # noqa: E402
import griffin_lim_common as gc  # noqa: E402
import satt_amd  # noqa: E402,F401
from satt_amd.utils import audio  # noqa: E402

KEYS = ("istft", "roundtrip", "iter_c", "iter_ang", "step_c")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hip", action="store_true", help="measure the kernel as well (needs the GPU)")
    args = ap.parse_args()
    worst = {}
    for name in gc.NAMES:
        tables = audio.MelspecTables(*ac.CONFIGS[name])
        for backend, run in [("numpy", gc.numpy_run(tables))] + ([("hip", gc.hip_run(tables))] if args.hip else []):
            m = gc.measure(name, run)
            worst[backend] = {k: max(worst.get(backend, {}).get(k, 0.0), m[k]) for k in KEYS}
            print("%-20s %-5s istft %.3e  roundtrip %.3e of the signal maximum   one iteration: c %.3e  ang %.3e   steps 1..%d: c %.3e "
                  "of the frame maximum" % (name, backend, m["istft"], m["roundtrip"], m["iter_c"], m["iter_ang"], gc.STEPS, m["step_c"]))
    for backend, w in worst.items():
        print("worst %-5s " % backend + "  ".join("%s %.3e" % (k, w[k]) for k in KEYS))
    print("C_ISTFT %.3e  C_ITER %.3e" % (gc.C_ISTFT, gc.C_ITER))


if __name__ == "__main__":
    main()
