"""Shared yardstick of the resampling tests (test_resample_cpu / test_resample_gpu) and of tools/resample_tolerances.py.

The float64 yardstick evaluates the definition of DESIGN.md 3.6 directly - np.sinc, np.i0, one loop over the outputs - and shares
nothing with satt_amd.utils.audio: neither the table, nor its exact-rational argument, nor the gather.

    g = gcd(a, b), up = b / g, down = a / g, n_out = ceil(n up / down);  output m:  k0 = (m down) // up, phase = (m down) % up
    y[m] = sum_{j = -half + 1 .. half} h(phase / up - j) x[k0 + j],  x = 0 outside [0, n)
    h(tau) = s sinc(s tau) I0(beta sqrt(1 - (s tau / Z)^2)) / I0(beta) for |s tau| < Z, else 0;  s = rolloff min(1, up / down)

Tolerances (profiles/resample_tolerances.txt holds the measurements): the deviation of a result is max_m |y - y64| / max_m |y64|
over the outputs compared.  E_NUMPY is the worst deviation of the float32 NumPy backend over cases() below (7.63e-7: one float32
chain of up to 406 products); the NumPy backend is held to 4 x that, the kernel to 8 x (the project's rule for melspec and
Griffin-Lim; the factor is not derived from the kernel's own results).  The kernel performs the NumPy backend's operations in the
same order, so test_resample_gpu.py also asserts that the two agree bit for bit."""
import math

import numpy as np

ZEROS = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492

# (source rate, target rate): up / down, taps - the table of the conversions the front end meets
RATIOS = {(22050, 16000): (320, 441, 188), (48000, 16000): (1, 3, 406), (48000, 22050): (147, 320, 296), (48000, 8000): (1, 6, 812),
          (16000, 22050): (441, 320, 136)}

# measured worst deviation of the float32 NumPy backend over cases() (tools/resample_tolerances.py; profiles/resample_tolerances.txt)
E_NUMPY = 7.7e-7
C_NUMPY = 4 * E_NUMPY
C_KERNEL = 8 * E_NUMPY


def ratio(a, b):
    g = math.gcd(a, b)
    return b // g, a // g


def scale_half(up, down):
    s = ROLLOFF * min(1.0, up / down)
    return s, int(math.ceil(ZEROS / s))


def h(tau, s):
    """float64 h at an array of arguments"""
    u = s * np.asarray(tau, np.float64)
    inside = np.abs(u) < ZEROS
    w = np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - (u / ZEROS) ** 2))) / np.i0(BETA)
    return np.where(inside, s * np.sinc(u) * w, 0.0)


def out_length(n, up, down):
    return -((-n * up) // down)


def yardstick(x, a, b, outputs=None):
    """float64 results of the outputs listed (default: all ceil(n up / down)) for the signal x at rate a converted to rate b"""
    up, down = ratio(a, b)
    s, half = scale_half(up, down)
    x = np.asarray(x, np.float64)
    n = len(x)
    outputs = range(out_length(n, up, down)) if outputs is None else outputs
    j = np.arange(-half + 1, half + 1)
    y = np.zeros(len(outputs))
    for i, m in enumerate(outputs):
        k0, phase = divmod(int(m) * down, up)
        k = k0 + j
        ok = (k >= 0) & (k < n)
        y[i] = np.dot(h(phase / up - j[ok], s), x[k[ok]])
    return y


def noise(n, seed):
    return (0.5 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def tone(n, rate, hz, amplitude=0.5):
    return (amplitude * np.sin(2.0 * np.pi * hz * np.arange(n) / rate)).astype(np.float32)


NOISE_CASES = [(22050, 16000, 3001), (48000, 16000, 5000), (16000, 22050, 2000), (48000, 24000, 4001), (44100, 48000, 3000)]


def edge_lengths(a, b):
    """lengths around the filter: 1, 2, 3, half - 1, half, half + 1, taps - 1, taps, taps + 1"""
    _, half = scale_half(*ratio(a, b))
    return [1, 2, 3, half - 1, half, half + 1, 2 * half - 1, 2 * half, 2 * half + 1]


def cases():
    """[(name, a, b, x float32)]: seeded noise at NOISE_CASES, and the edge lengths at 22050 -> 16000 and 16000 -> 22050"""
    out = [("noise %d->%d n=%d" % (a, b, n), a, b, noise(n, seed)) for seed, (a, b, n) in enumerate(NOISE_CASES)]
    for a, b in ((22050, 16000), (16000, 22050)):
        out += [("edge %d->%d n=%d" % (a, b, n), a, b, noise(n, 100 + i)) for i, n in enumerate(edge_lengths(a, b))]
    return out


_REFERENCE = {}


def reference(name, a, b, x):
    """the yardstick of a case of cases(), computed once per process"""
    if name not in _REFERENCE:
        _REFERENCE[name] = yardstick(x, a, b)
        _REFERENCE[name].setflags(write=False)
    return _REFERENCE[name]


def deviation(y, y64):
    return float(np.abs(np.asarray(y, np.float64) - y64).max() / np.abs(y64).max())


def db(x):
    return 20.0 * math.log10(max(float(x), 1e-300))
