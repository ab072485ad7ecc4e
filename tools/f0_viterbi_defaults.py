"""The table behind the default costs of the Viterbi pitch tracker (utils/pitch.py JUMP_COST, SWITCH_COST, LAG_BIAS; unvoiced_cost =
the threshold), on the NumPy backend, no GPU: the trap signal of tests/f0_viterbi_common.py (gross pitch error over its 61 judged
frames, the frames whose voicing differs from the truth) and the clean five-harmonic tones of tests/pitch_common.py at 16 kHz (worst
error in cents inside the tone, voiced frames in the noise lead-in), for plain YIN and for a grid of costs.
    python tools/f0_viterbi_defaults.py > profiles/f0_viterbi_defaults.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import f0_viterbi_common as fc  # noqa: E402
import pitch_common as pc  # noqa: E402
import satt_amd  # noqa: E402,F401
from satt_amd.utils import pitch  # noqa: E402


def main():
    y, truth, judged, voiced_truth = fc.trap()
    sr, hop = 16000, 200
    tones = [(p, pc.tone(sr, p, 100 + i)) for i, p in enumerate(pc.periods(sr))]

    def row(label, **kw):
        f0, _, _, voiced = pitch.track_f0([y], fc.SR, fc.HOP, **kw)[0]
        octave = int((np.abs(f0[judged] / truth[judged] - 2.0) < 0.2).sum())
        worst, lead_voiced, lost = 0.0, 0, 0
        for (p, s), (g0, _, _, gv) in zip(tones, pitch.track_f0([s for _, s in tones], sr, hop, **kw)):
            lead, inside = pc.frame_sets(sr, hop, len(s))
            lost += int((~gv[inside]).sum())
            ok = inside[gv[inside]]
            if len(ok):
                worst = max(worst, float(np.abs(pc.cents(g0[ok], p, sr)).max()))
            lead_voiced += int(gv[lead].sum())
        print("%-38s %6.4f %8d   %-14s %10.3f %8d %8d" % (label, fc.gpe(f0, truth, judged), octave,
                                                          " ".join(map(str, np.nonzero(voiced != voiced_truth)[0])) or "-", worst, lost, lead_voiced))

    print(__doc__.split("\n    python")[0])
    print()
    print("trap: 16000 Hz, hop 200, 81 frames, 61 judged (0.12 s < t < 0.88 s), truth voiced for 0.1 s <= t < 0.9 s (frames 8 .. 71)")
    print("tones: periods %s samples at 16000 Hz, 0.12 s of noise then 0.30 s of tone" % ", ".join("%.2f" % p for p, _ in tones))
    print("tracker arguments at their defaults: 60 - 500 Hz, 25 ms, threshold 0.15, silence 50 dB")
    print()
    print("%-38s %6s %8s   %-14s %10s %8s %8s" % ("jump switch unvoiced lag_bias", "GPE", "octave", "voicing differs", "tones: max", "unvoiced", "voiced"))
    print("%-38s %6s %8s   %-14s %10s %8s %8s" % ("", "trap", "frames", "at frames", "cents", "inside", "in lead"))
    row("plain YIN")
    for jump, switch, unv, bias in ((0.3, 0.1, 0.15, 0.1), (0.5, 0.2, 0.15, 0.1), (0.3, 0.1, 0.15, 0.0), (0.0, 0.0, 0.15, 0.1), (0.1, 0.1, 0.15, 0.1),
                                    (0.2, 0.1, 0.15, 0.1), (1.0, 0.1, 0.15, 0.1), (0.3, 0.05, 0.15, 0.1), (0.3, 0.2, 0.15, 0.1), (0.3, 0.3, 0.15, 0.1),
                                    (0.3, 0.1, 0.1, 0.1), (0.3, 0.1, 0.2, 0.1), (0.3, 0.1, 0.3, 0.1), (0.3, 0.1, 0.15, 0.05), (0.3, 0.1, 0.15, 0.2),
                                    (0.3, 0.1, 0.15, 0.3)):
        row("%-5g %-6g %-8g %-8g" % (jump, switch, unv, bias) + ("  (defaults)" if (jump, switch, unv, bias) == (0.3, 0.1, 0.15, 0.1) else ""),
            tracker="viterbi", jump_cost=jump, switch_cost=switch, unvoiced_cost=unv, lag_bias=bias)
    print()
    print("Read off: the defaults 0.3 / 0.1 / threshold / 0.1 stand.  Plain YIN reports the octave above in 22 of the 61 frames; the path at")
    print("the defaults in none, its voicing differs from the truth at the two onset frames only.  Without transition costs, or with")
    print("jump_cost 0.1, the 22 come back; switch_cost 0.05 lets two switches through \"unvoiced\" undercut one octave jump.  lag_bias 0 keeps")
    print("one more frame voiced at the offset and reports one clean tone an octave BELOW (1200 cents: with equal d' at a period and its")
    print("double the path may settle on the double); lag_bias >= 0.2 and unvoiced_cost 0.1 lose voiced frames of the long-period tones.")


if __name__ == "__main__":
    main()
