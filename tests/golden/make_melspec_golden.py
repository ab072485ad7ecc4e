"""Generator of tests/golden/melspec_small.npz: about 0.25 s of the harmonic test signal at the LJSpeech parameters with the float64
yardstick's magnitudes and dB mel (tests/audio_common.py: torch.stft on the CPU + the Slaney basis written from the formulas).
The fixture holds the yardstick itself still: tests compare today's yardstick, the NumPy backend and the kernel with it.
    python tests/golden/make_melspec_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import audio_common as ac  # noqa: E402


def main():
    sr, n_fft, win, hop, mels = ac.CONFIGS["ljspeech"]
    y = ac.harmonic(5800, sr, seed=123)
    mag = ac.yardstick_mag(y, n_fft, hop, win)
    db, amp = ac.yardstick_db(mag, ac.slaney_basis(sr, n_fft, mels))
    assert amp.min() >= 1e-4
    # float64 magnitudes of all 22 frames would be 180 KB: every third frame is kept (both edge frames among them), every dB row is
    frames = np.arange(0, mag.shape[0], 3)
    assert frames[-1] == mag.shape[0] - 1
    np.savez_compressed(os.path.join(HERE, "melspec_small.npz"), signal=y, mag_frames=frames, mag=mag[frames], db=db,
                        params=np.asarray([sr, n_fft, win, hop, mels, ac.REF_LEVEL_DB], np.float64))
    print(os.path.getsize(os.path.join(HERE, "melspec_small.npz")), mag.shape, db.shape)


if __name__ == "__main__":
    main()
