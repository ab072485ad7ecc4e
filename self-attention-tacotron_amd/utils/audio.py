"""Audio front end of the preprocessing drivers: the reference-named `Audio(hparams)` class (reference utils/audio.py) without
librosa.  The log-mel spectrogram runs in csrc/melspec.hip (backend "hip") or as a float32 scipy.fft restatement (backend
"numpy", for machines without a GPU); both follow librosa.stft's defaults: frames centred by reflect padding, a periodic Hann
window of `win` points zero-padded to n_fft, T = 1 + n // hop frames, Slaney's mel basis.  `trim` is O(n) host code (DESIGN.md
records the semantics chosen for it).  Resampling is opt-in (`Audio(..., resample=True)`): a Kaiser-windowed sinc on the rational grid
of the two rates, in csrc/resample.hip or as a float32 NumPy restatement on the same float32 table, operation for operation (the two
backends agree bit for bit; DESIGN.md 3.6 holds the definition; it is not librosa's bits).  Without it a wav whose rate differs
from hparams.sample_rate is refused.
The way back - `inv_melspectrogram`: the pseudo-inverse of the mel basis and Griffin-Lim phase reconstruction - runs in
csrc/griffin_lim.hip or as the same kind of restatement; it is a quick listen, not a vocoder.  Opt-in (`inversion="nnls"`), the
floored pseudo-inverse is refined by a non-negative solve in csrc/mel_nnls.hip, or in float32 NumPy with the kernel's bits."""
import math

import numpy as np

MAX_LAUNCH_SAMPLES = 1 << 23          # samples per kernel launch of melspectrogram_batch / resample_batch (32 MB of signal; one
                                      # longer utterance still goes out as a launch of its own)


def stft_parameters(hparams):
    """(n_fft, hop, win) - the reference's expressions in the reference's order (utils/audio.py:63-67)"""
    n_fft = (hparams.num_freq - 1) * 2
    hop = int(hparams.frame_shift_ms / 1000 * hparams.sample_rate)
    win = int(hparams.frame_length_ms / 1000 * hparams.sample_rate)
    return n_fft, hop, win


def padded_window(n_fft, win):
    """float64 [n_fft]: the periodic Hann window of `win` points behind (n_fft - win) // 2 zeros"""
    w = np.zeros(n_fft, np.float64)
    lead = (n_fft - win) // 2
    w[lead:lead + win] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    return w


def hz_to_mel(f):
    """Slaney's scale: 200 / 3 Hz per mel below 1 kHz (1000 Hz = 15 mel), above it logarithmic with step ln(6.4) / 27"""
    f = np.asarray(f, np.float64)
    return np.where(f < 1000.0, f * 3.0 / 200.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0))


def mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m < 15.0, m * 200.0 / 3.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)))


def mel_basis(sample_rate, n_fft, num_mels):
    """float64 [num_mels, n_fft // 2 + 1]: triangles over num_mels + 2 points equally spaced in mel from 0 to sample_rate / 2,
    each normalised by 2 / (f[m + 2] - f[m])"""
    freqs = np.linspace(0.0, sample_rate / 2.0, n_fft // 2 + 1)
    pts = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(sample_rate / 2.0), num_mels + 2))
    diff = np.diff(pts)
    ramps = pts[:, None] - freqs[None, :]
    lower = -ramps[:-2] / diff[:-1, None]
    upper = ramps[2:] / diff[1:, None]
    return np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (pts[2:] - pts[:-2]))[:, None]


def banded(basis):
    """the non-zero run of every row: (start int32 [M], offset int32 [M + 1], weight float32 [offset[M]]).  An empty band keeps one
    zero weight so that no table is empty."""
    start, offset, weight = [], [0], []
    for row in basis:
        nz = np.nonzero(row)[0]
        lo, hi = (int(nz[0]), int(nz[-1]) + 1) if nz.size else (0, 1)
        start.append(lo)
        weight.append(row[lo:hi])
        offset.append(offset[-1] + hi - lo)
    return np.asarray(start, np.int32), np.asarray(offset, np.int32), np.concatenate(weight).astype(np.float32)


def twiddles(n_fft):
    """float32 [n_fft, 2]: (cos, -sin)(2 pi k / n_fft), evaluated in float64"""
    a = 2.0 * np.pi * np.arange(n_fft) / n_fft
    return np.stack([np.cos(a), -np.sin(a)], axis=1).astype(np.float32)


def frame_count(n, hop):
    return 1 + n // hop


class MelspecTables:
    """host tables of one STFT / mel configuration, and their device copies (made on first use)"""

    def __init__(self, sample_rate, n_fft, win, hop, num_mels):
        self.sample_rate, self.n_fft, self.win, self.hop, self.num_mels = sample_rate, n_fft, win, hop, num_mels
        self.window = padded_window(n_fft, win).astype(np.float32)
        self.basis = mel_basis(sample_rate, n_fft, num_mels)
        self.band_start, self.band_offset, self.band_weight = banded(self.basis)
        self.twiddle = twiddles(n_fft)
        self._dev = {}
        self._basis_pinv = None              # mel_to_linear's, computed on first use
        self._nnls = None                    # mel_nnls_tables', built on first use

    def device(self, device):
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = {k: torch.from_numpy(np.ascontiguousarray(getattr(self, k))).to(device)
                              for k in ("window", "twiddle", "band_start", "band_offset", "band_weight")}
        return self._dev[key]

    def griffin_lim_device(self, device):
        """device() plus "envelope", the float64 overlap-add tables that only Griffin-Lim reads (made on first use)"""
        import torch
        d = self.device(device)
        if "envelope" not in d:
            d["envelope"] = torch.from_numpy(overlap_envelope_tables(padded_window(self.n_fft, self.win), self.hop)).to(device)
        return d


def melspec_hip(tables, signals, ref_level_db, device="cuda", want_mag=False):
    """one launch of csrc/melspec.hip over `signals` (float32 arrays, each >= n_fft // 2 + 1 samples): a list of [T, num_mels]
    arrays (and, with want_mag, the list of [T, n_fft // 2 + 1] magnitudes)"""
    import torch
    from .. import ops
    t = tables
    lens = np.asarray([len(s) for s in signals], np.int64)
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    fo = np.concatenate([[0], np.cumsum(1 + lens // t.hop)]).astype(np.int64)
    d = t.device(device)
    sig = torch.from_numpy(np.concatenate([np.ascontiguousarray(s, np.float32) for s in signals])).to(device)
    mel = torch.empty((int(fo[-1]), t.num_mels), dtype=torch.float32, device=device)
    mag = torch.empty((int(fo[-1]), t.n_fft // 2 + 1), dtype=torch.float32, device=device) if want_mag else None
    ops.melspec(sig, torch.from_numpy(so).to(device), torch.from_numpy(fo).to(device), t.n_fft, t.win, t.hop, d["window"],
                d["twiddle"], d["band_start"], d["band_offset"], d["band_weight"], ref_level_db, mel, mag)
    mel = mel.cpu().numpy()
    mels = [mel[fo[u]:fo[u + 1]] for u in range(len(signals))]
    if not want_mag:
        return mels
    mag = mag.cpu().numpy()
    return mels, [mag[fo[u]:fo[u + 1]] for u in range(len(signals))]


def _fft():
    """the module whose rfft / irfft the NumPy backend uses: scipy.fft, which transforms float32 in float32, or numpy.fft, which
    computes in float64 (the results are rounded to float32 behind it)"""
    try:
        import scipy.fft
        return scipy.fft
    except ImportError:
        return np.fft


def centred_frames(y, n_fft, hop, T):
    """read-only view [T, n_fft] of y reflect-padded by n_fft // 2 at either end: frame t starts at padded position t hop"""
    yp = np.pad(y, n_fft // 2, mode="reflect")
    return np.lib.stride_tricks.as_strided(yp, (T, n_fft), (yp.strides[0] * hop, yp.strides[0]), writeable=False)


def melspec_numpy(tables, y, ref_level_db, want_mag=False):
    """the same in float32 NumPy / scipy.fft: [T, num_mels] of one signal"""
    t = tables
    y = np.ascontiguousarray(y, np.float32)
    frames = centred_frames(y, t.n_fft, t.hop, frame_count(len(y), t.hop))
    mag = np.abs(_fft().rfft(frames * t.window[None, :], axis=1)).astype(np.float32)
    mel = mag @ t.basis.astype(np.float32).T
    db = (20.0 * np.log10(np.maximum(np.float32(1e-5), mel)) - np.float32(ref_level_db)).astype(np.float32)
    return (db, mag) if want_mag else db


# ---- mel -> audio: Griffin-Lim phase reconstruction (csrc/griffin_lim.hip, or float32 scipy.fft) ------------------------------------
#
# One utterance of T frames gives n = (T - 1) hop samples (torch.istft's / librosa's centred length; 1 + n // hop == T).  Padded
# position p = sample + n_fft / 2 lies in frame t at in-frame index p - t hop.  One iteration on the unit-complex `ang`:
#   y = istft(mag ang);  c = stft(y);  u = c + alpha (c - c_prev);  ang' = u / max(|u|, 1e-30);  c_prev' = c
# (alpha = 0: classic Griffin-Lim; 0.99: the "fast" variant).  The result is istft(mag ang) behind `iters` iterations.

def overlap_envelope_tables(window64, hop):
    """float64 [hop + 2 n_fft] = F | H | G, the pieces of the overlap-add envelope of ANY frame count T:
        sum_{0 <= t < T} w^2[p - t hop] = F[p mod hop] - (H[p] if p < n_fft) - (G[p - T hop] if p >= T hop)
    F[j] = sum over every integer t of w^2[j + t hop] (the value away from the ends), H[p] = sum_{t >= 1} w^2[p + t hop] (frames
    in front of the first), G[r] = sum_{t >= 0} w^2[r - t hop] (frames behind the last)."""
    w2 = np.asarray(window64, np.float64) ** 2
    N = len(w2)
    H, G = np.zeros(N), w2.copy()
    for m in range(1, -(-N // hop)):
        H[:N - m * hop] += w2[m * hop:]
        G[m * hop:] += w2[:N - m * hop]
    F = (H + w2)[:hop].copy() if hop <= N else np.concatenate([w2, np.zeros(hop - N)])
    return np.concatenate([F, H, G])


def overlap_envelope(window64, hop, T):
    """float64 [n_fft + hop (T - 1)]: sum_t w^2[p - t hop] by direct summation"""
    N = len(window64)
    env = np.zeros(N + hop * (T - 1))
    w2 = np.asarray(window64, np.float64) ** 2
    for t in range(T):
        env[t * hop:t * hop + N] += w2
    return env


def griffin_lim_check(tables, frames):
    """raises ValueError naming what csrc/griffin_lim.hip (and the NumPy restatement) does not take"""
    t = tables
    if t.n_fft not in (512, 1024, 2048, 4096):
        raise ValueError("Griffin-Lim: n_fft=%d is not one of 512 / 1024 / 2048 / 4096" % t.n_fft)
    if not 16 <= t.win <= t.n_fft:
        raise ValueError("Griffin-Lim: win=%d is outside 16 .. n_fft=%d" % (t.win, t.n_fft))
    if not 1 <= t.hop <= t.win // 2:
        raise ValueError("Griffin-Lim: hop=%d is outside 1 .. win / 2 = %d (the squared Hann windows must overlap)" % (t.hop, t.win // 2))
    for T in frames:
        if (T - 1) * t.hop < t.n_fft // 2 + 1:
            raise ValueError("Griffin-Lim: frames=%d gives (frames - 1) * hop = %d samples, fewer than n_fft / 2 + 1 = %d: the "
                             "re-analysis cannot reflect-pad" % (T, (T - 1) * t.hop, t.n_fft // 2 + 1))


def griffin_lim_numpy(tables, mag, ang0, iters, alpha, c_prev=None, want_state=False):
    """float32 scipy.fft restatement of csrc/griffin_lim.hip for one utterance.  mag float32 [T, n_fft / 2 + 1], ang0 complex64
    unit phases of the same shape, c_prev complex64 or None (zeros).  Returns the signal float32 [(T - 1) hop], or with want_state
    (signal, ang, c_prev, c): the state behind `iters` iterations and the last re-analysis (None when iters == 0)."""
    fft = _fft()
    t = tables
    mag = np.ascontiguousarray(mag, np.float32)
    T, M = mag.shape[0], t.n_fft // 2
    griffin_lim_check(t, [T])
    n = (T - 1) * t.hop
    w64 = padded_window(t.n_fft, t.win)
    w = w64.astype(np.float32)
    inv_env = (1.0 / overlap_envelope(w64, t.hop, T)[M:M + n].astype(np.float32)).astype(np.float32)
    ang = np.ascontiguousarray(ang0, np.complex64)
    prev = np.zeros_like(ang) if c_prev is None else np.ascontiguousarray(c_prev, np.complex64)
    alpha = np.float32(alpha)

    def synth(a):
        frames = fft.irfft(mag * a, n=t.n_fft, axis=1).astype(np.float32) * w[None, :]
        y = np.zeros(t.n_fft + t.hop * (T - 1), np.float32)
        for i in range(T):                                   # ascending frame order, as the kernel's gather
            y[i * t.hop:i * t.hop + t.n_fft] += frames[i]
        return y[M:M + n] * inv_env

    c = None
    for _ in range(iters):
        c = fft.rfft(centred_frames(synth(ang), t.n_fft, t.hop, T) * w[None, :], axis=1).astype(np.complex64)
        u = c + alpha * (c - prev) if alpha != 0 else c
        ang = (u / np.maximum(np.abs(u), np.float32(1e-30))).astype(np.complex64)
        prev = c
    y = synth(ang)
    return (y, ang, prev, c) if want_state else y


def griffin_lim_hip(tables, mags, ang0s, iters, alpha, device="cuda", c_prevs=None, want_state=False):
    """one entry call of csrc/griffin_lim.hip over a list of utterances (mags float32 [T_u, n_fft / 2 + 1], ang0s complex64): the
    list of signals float32 [(T_u - 1) hop]; with want_state (signals, angs, c_prevs, cs)."""
    import torch
    from .. import ops
    t = tables
    NF = t.n_fft // 2 + 1
    Ts = np.asarray([m.shape[0] for m in mags], np.int64)
    griffin_lim_check(t, Ts)
    fo = np.concatenate([[0], np.cumsum(Ts)]).astype(np.int64)
    so = np.concatenate([[0], np.cumsum((Ts - 1) * t.hop)]).astype(np.int64)
    d = t.griffin_lim_device(device)

    def up(xs, dtype):
        return torch.from_numpy(np.concatenate([np.ascontiguousarray(x, dtype).reshape(-1, NF) for x in xs])).to(device)
    mag = up(mags, np.float32)
    ang = torch.view_as_real(up(ang0s, np.complex64)).contiguous()
    keep_prev = alpha != 0 or c_prevs is not None or want_state
    prev = None
    if keep_prev:
        prev = torch.view_as_real(up(c_prevs, np.complex64)).contiguous() if c_prevs is not None else torch.zeros_like(ang)
    spec = torch.zeros_like(ang) if want_state and iters > 0 else None
    signal = torch.empty(int(so[-1]), dtype=torch.float32, device=device)
    ws = torch.empty(ops.griffin_lim_workspace_bytes(t.n_fft, int(fo[-1])) // 4, dtype=torch.float32, device=device)
    ops.griffin_lim(mag, ang, prev, signal, torch.from_numpy(so).to(device), torch.from_numpy(fo).to(device), t.n_fft, t.win, t.hop,
                    iters, alpha, d["window"], d["twiddle"], d["envelope"], ws, spec)
    y = signal.cpu().numpy()
    ys = [y[so[u]:so[u + 1]] for u in range(len(mags))]
    if not want_state:
        return ys

    def down(x):
        if x is None:
            return [None] * len(mags)
        z = torch.view_as_complex(x).cpu().numpy()
        return [z[fo[u]:fo[u + 1]] for u in range(len(mags))]
    return ys, down(ang), down(prev), down(spec)


def _mel_amp_and_start(tables, S_db, ref_level_db):
    """(amp, amp @ pinv(basis).T), both float64: the band amplitudes of a dB mel spectrogram and their least-norm spectrum, the
    pseudo-inverse computed once per table"""
    if tables._basis_pinv is None:
        tables._basis_pinv = np.linalg.pinv(tables.basis)
    amp = 10.0 ** ((np.asarray(S_db, np.float64) + ref_level_db) / 20.0)
    return amp, amp @ tables._basis_pinv.T


# ---- non-negative mel inversion (csrc/mel_nnls.hip, or float32 NumPy in the kernel's order) ------------------------------------------
#
# One frame with band amplitudes a (float32 [M]) and the start x_0 (float32 [F], the floored pseudo-inverse); W the float32 banded
# basis (band_start / band_offset / band_weight, the operator csrc/melspec.hip applies).  K iterations of accelerated projected
# gradient on min_{x >= 0} |W x - a|^2 / 2:
#   y_1 = x_0;  for k = 1 .. K:  p = W y_k;  r = p - a;  g = W^T r;  v = y_k - step g;  x_k = v > 0 ? v : 0;
#                                y_k+1 = x_k + beta_k (x_k - x_k-1);     result x_K
# every product, difference and sum rounded to float32.  p[m]: lane j = 0 .. 15 sums the band's terms j, j + 16, .. ascending in one
# chain from +0, the 16 partial sums are joined by the adjacent pairwise tree ((s0 + s1) + (s2 + s3)) + ..; g[f]: one chain from +0
# over the bin's bands, ascending.  A fixed K keeps the bits reproducible: there is no stopping rule.

MEL_NNLS_ITERS = 64                   # the default K (profiles/mel_nnls_quality.txt)
MEL_NNLS_TEAM = 16                    # lanes that share a band's sum
MEL_NNLS_MAX_BINS, MEL_NNLS_MAX_MELS, MEL_NNLS_MAX_ITERS = 2049, 128, 1024          # satt_mel_nnls_supported's bounds
MEL_NNLS_NUMPY_BLOCK = 64             # frames solved at a time by mel_nnls_numpy (the temporaries stay in cache)


def transposed_banded(band_start, band_offset, band_weight, num_bins):
    """the banded basis seen from the bins: (first int32 [F], offset int32 [F + 1], weight float32 [offset[F]]).  Bin f lies under
    the bands first[f] .. first[f] + c - 1, c = offset[f + 1] - offset[f]: from the first to the last band that holds a non-zero
    weight for it, bands ascending; a band of that range without one has weight 0.  A bin under no band has c = 0.  The weights are
    the float32 values of band_weight themselves; an empty table keeps one zero weight."""
    M = len(band_start)
    lo = np.full(num_bins, M, np.int64)
    hi = np.full(num_bins, -1, np.int64)
    for m in range(M):
        w = band_weight[band_offset[m]:band_offset[m + 1]]
        f = int(band_start[m]) + np.nonzero(w)[0]
        lo[f] = np.minimum(lo[f], m)
        hi[f] = np.maximum(hi[f], m)
    count = np.where(hi >= 0, hi - lo + 1, 0)
    offset = np.concatenate([[0], np.cumsum(count)])
    weight = np.zeros(max(1, int(offset[-1])), np.float32)
    for m in range(M):
        s, n = int(band_start[m]), int(band_offset[m + 1] - band_offset[m])
        f = s + np.arange(n)
        inside = (count[f] > 0) & (lo[f] <= m) & (m <= hi[f])
        weight[offset[f[inside]] + m - lo[f[inside]]] = band_weight[band_offset[m]:band_offset[m + 1]][inside]
    first = np.where(count > 0, lo, 0)
    return first.astype(np.int32), offset.astype(np.int32), weight


class MelNnlsTables:
    """what the non-negative inversion needs beside the banded basis: its transposed table (transposed_banded), `step` and
    beta(K), and the gather tables of the NumPy backend; device copies are made on first use.
      step = float32(1 / L), L the largest eigenvalue of W W^T in float64 from the float32 weights; the next float32 towards 0
             when float64(step) * L > 1
      beta_k = float32((t_k - 1) / t_k+1), t_1 = 1, t_k+1 = (1 + sqrt(1 + 4 t_k^2)) / 2 in float64"""

    def __init__(self, band_start, band_offset, band_weight, num_bins):
        self.band_start = np.ascontiguousarray(band_start, np.int32)
        self.band_offset = np.ascontiguousarray(band_offset, np.int32)
        self.band_weight = np.ascontiguousarray(band_weight, np.float32)
        self.num_bins, self.num_mels = int(num_bins), len(self.band_start)
        M, F = self.num_mels, self.num_bins
        length = np.diff(self.band_offset)
        if len(self.band_offset) != M + 1 or (length < 0).any() or self.band_offset[0] < 0 or self.band_offset[-1] > len(self.band_weight) \
                or (self.band_start < 0).any() or (self.band_start + length > F).any():
            raise ValueError("mel_nnls: the banded table does not lie inside %d bins / %d weights" % (F, len(self.band_weight)))
        self.bin_first, self.bin_offset, self.bin_weight = transposed_banded(self.band_start, self.band_offset, self.band_weight, F)
        dense = self.dense()
        L = float(np.linalg.eigvalsh(dense @ dense.T)[-1])
        if not (L > 0.0 and math.isfinite(L)):
            raise ValueError("mel_nnls: the basis has no positive weight")
        step = np.float32(1.0 / L)
        if float(step) * L > 1.0:
            step = np.nextafter(step, np.float32(0.0))
        self.lipschitz, self.step = L, np.float32(step)
        # the NumPy backend's gathers: band m's terms padded to rounds of MEL_NNLS_TEAM lanes, a bin's bands to the widest count.  A
        # padded term multiplies weight 0 with the zero appended behind y / r: it adds +0, which changes no bit of a chain that
        # started from +0
        R = max(1, -(-int(length.max()) // MEL_NNLS_TEAM))
        i = np.arange(R * MEL_NNLS_TEAM)[None, :]
        live = i < length[:, None]
        self._w_pad = np.where(live, self.band_weight[np.where(live, self.band_offset[:-1, None] + i, 0)], np.float32(0)) \
            .astype(np.float32).reshape(M, R, MEL_NNLS_TEAM)
        self._y_idx = np.where(live, self.band_start[:, None] + i, F).reshape(M, R, MEL_NNLS_TEAM)
        count = np.diff(self.bin_offset)
        C = max(1, int(count.max()))
        c = np.arange(C)[None, :]
        live = c < count[:, None]
        self._tw_pad = np.where(live, self.bin_weight[np.where(live, self.bin_offset[:-1, None] + c, 0)], np.float32(0)).astype(np.float32)
        self._r_idx = np.where(live, self.bin_first[:, None] + c, M)
        self._beta, self._dev = np.zeros(0, np.float32), {}

    def dense(self):
        """float64 [M, F] from the float32 banded weights"""
        B = np.zeros((self.num_mels, self.num_bins))
        for m in range(self.num_mels):
            n = self.band_offset[m + 1] - self.band_offset[m]
            B[m, self.band_start[m]:self.band_start[m] + n] = self.band_weight[self.band_offset[m]:self.band_offset[m + 1]]
        return B

    def dense_transposed(self):
        """float64 [F, M] from the transposed table"""
        Bt = np.zeros((self.num_bins, self.num_mels))
        for f in range(self.num_bins):
            n = self.bin_offset[f + 1] - self.bin_offset[f]
            Bt[f, self.bin_first[f]:self.bin_first[f] + n] = self.bin_weight[self.bin_offset[f]:self.bin_offset[f + 1]]
        return Bt

    def beta(self, iters):
        """float32 [iters]; a longer table begins with the shorter one"""
        if len(self._beta) < iters:
            t, out = 1.0, []
            for _ in range(iters):
                t_next = (1.0 + math.sqrt(1.0 + 4.0 * t * t)) / 2.0
                out.append((t - 1.0) / t_next)
                t = t_next
            self._beta = np.asarray(out, np.float64).astype(np.float32)
        return self._beta[:iters]

    def device(self, device):
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = {k: torch.from_numpy(getattr(self, k)).to(device)
                              for k in ("band_start", "band_offset", "band_weight", "bin_first", "bin_offset", "bin_weight")}
        return self._dev[key]


def mel_nnls_tables(tables):
    """the MelNnlsTables of a MelspecTables, built on first use and kept on it"""
    nt = getattr(tables, "_nnls", None)
    if nt is None:
        nt = tables._nnls = MelNnlsTables(tables.band_start, tables.band_offset, tables.band_weight, tables.n_fft // 2 + 1)
    return nt


def mel_nnls_check(nnls, amp, x0, iters):
    """(amp, x0) as contiguous float32 [N, M] and [N, F]; raises ValueError naming what csrc/mel_nnls.hip (and the NumPy
    restatement) does not take"""
    amp, x0 = np.ascontiguousarray(amp, np.float32), np.ascontiguousarray(x0, np.float32)
    if amp.ndim != 2 or x0.ndim != 2 or amp.shape != (len(x0), nnls.num_mels) or x0.shape[1] != nnls.num_bins or len(x0) < 1:
        raise ValueError("mel_nnls: amplitudes %r and starts %r, need [N, %d] and [N, %d] with N >= 1"
                         % (amp.shape, x0.shape, nnls.num_mels, nnls.num_bins))
    if not (nnls.num_bins <= MEL_NNLS_MAX_BINS and nnls.num_mels <= MEL_NNLS_MAX_MELS and 1 <= iters <= MEL_NNLS_MAX_ITERS):
        raise ValueError("mel_nnls: num_bins=%d num_mels=%d iters=%d is outside num_bins <= %d, num_mels <= %d, 1 <= iters <= %d"
                         % (nnls.num_bins, nnls.num_mels, iters, MEL_NNLS_MAX_BINS, MEL_NNLS_MAX_MELS, MEL_NNLS_MAX_ITERS))
    return amp, x0


def mel_nnls_numpy(nnls, amp, x0, iters):
    """float32 [N, F]: x_K of every frame, with the kernel's operations in the kernel's order - the bits of csrc/mel_nnls.hip.
    Vectorised over the frames (MEL_NNLS_NUMPY_BLOCK at a time), the bands and the bins; the loops are the chains' steps."""
    t = nnls
    amp, x0 = mel_nnls_check(t, amp, x0, iters)
    beta, step, zero = t.beta(iters), t.step, np.float32(0)
    out = np.empty_like(x0)
    R, C = t._w_pad.shape[1], t._tw_pad.shape[1]
    with np.errstate(all="ignore"):
        for n0 in range(0, len(x0), MEL_NNLS_NUMPY_BLOCK):
            a = amp[n0:n0 + MEL_NNLS_NUMPY_BLOCK]
            x = x0[n0:n0 + MEL_NNLS_NUMPY_BLOCK].copy()
            y = x.copy()
            n = len(x)
            y_ext, r_ext = np.zeros((n, t.num_bins + 1), np.float32), np.zeros((n, t.num_mels + 1), np.float32)
            for k in range(iters):
                y_ext[:, :-1] = y
                s = np.zeros((n, t.num_mels, MEL_NNLS_TEAM), np.float32)
                for i in range(R):                                     # a lane's chain: its terms ascending
                    s = s + t._w_pad[None, :, i, :] * y_ext[:, t._y_idx[:, i, :]]
                while s.shape[2] > 1:                                  # the adjacent pairwise tree
                    s = s[:, :, 0::2] + s[:, :, 1::2]
                r_ext[:, :-1] = s[:, :, 0] - a
                g = np.zeros_like(x)
                for c in range(C):                                     # a bin's chain: its bands ascending
                    g = g + t._tw_pad[None, :, c] * r_ext[:, t._r_idx[:, c]]
                v = y - step * g
                xn = np.where(v > zero, v, zero)
                y = xn + beta[k] * (xn - x)
                x = xn
            out[n0:n0 + n] = x
    return out


def mel_nnls_hip(nnls, amp, x0, iters, device="cuda", max_launch_frames=None):
    """the same on csrc/mel_nnls.hip: one launch per group of at most max_launch_frames frames (default: all in one)"""
    import torch
    from .. import ops
    t = nnls
    amp, x0 = mel_nnls_check(t, amp, x0, iters)
    d = t.device(device)
    beta = torch.from_numpy(np.ascontiguousarray(t.beta(iters))).to(device)
    N = len(x0)
    group = N if max_launch_frames is None else max(1, int(max_launch_frames))
    out = np.empty_like(x0)
    up = lambda v: torch.from_numpy(v if v.flags.writeable else v.copy()).to(device)
    for n0 in range(0, N, group):
        a, s = up(amp[n0:n0 + group]), up(x0[n0:n0 + group])
        o = torch.empty_like(s)
        ops.mel_nnls(a, s, beta, float(t.step), d["band_start"], d["band_offset"], d["band_weight"], d["bin_first"], d["bin_offset"],
                     d["bin_weight"], o)
        out[n0:n0 + group] = o.cpu().numpy()
    return out


def mel_to_linear_batch(tables, Ss_db, ref_level_db, power=1.0, *, inversion="pinv", nnls_iters=MEL_NNLS_ITERS, backend="numpy",
                        device="cuda"):
    """mel_to_linear of a list of dB mel spectrograms.  With inversion="nnls" the frames of all of them are solved together (on
    "hip": one launch per MAX_LAUNCH_SAMPLES // hop frames); a frame's result does not depend on what shares its batch."""
    if inversion not in ("pinv", "nnls"):
        raise ValueError("inversion must be 'pinv' or 'nnls', got %r" % (inversion,))
    if backend not in ("hip", "numpy"):
        raise ValueError("backend must be 'hip' or 'numpy', got %r" % (backend,))
    if nnls_iters < 0:
        raise ValueError("nnls_iters must be >= 0, got %d" % nnls_iters)
    pairs = [_mel_amp_and_start(tables, S, ref_level_db) for S in Ss_db]
    if inversion == "pinv" or nnls_iters == 0 or not pairs:
        return [np.maximum(1e-10, lin) ** power for _, lin in pairs]
    for amp, _ in pairs:
        if amp.ndim != 2:
            raise ValueError("mel_to_linear: inversion='nnls' takes [T, num_mels] spectrograms, got shape %r" % (amp.shape,))
    nt = mel_nnls_tables(tables)
    amp = np.concatenate([a for a, _ in pairs]).astype(np.float32)
    x0 = np.concatenate([np.maximum(1e-10, lin) for _, lin in pairs]).astype(np.float32)
    if backend == "numpy":
        x = mel_nnls_numpy(nt, amp, x0, nnls_iters)
    else:
        x = mel_nnls_hip(nt, amp, x0, nnls_iters, device, max(1, MAX_LAUNCH_SAMPLES // tables.hop))
    x = np.maximum(1e-10, x.astype(np.float64)) ** power
    ends = np.cumsum([len(a) for a, _ in pairs])
    return [x[e - len(a):e] for (a, _), e in zip(pairs, ends)]


def mel_to_linear(tables, S_db, ref_level_db, power=1.0, *, inversion="pinv", nnls_iters=MEL_NNLS_ITERS, backend="numpy", device="cuda"):
    """float64 [T, n_fft / 2 + 1] linear magnitudes of a dB mel spectrogram [T, num_mels] (Audio.melspectrogram's scale):
        amp = 10 ** ((S + ref_level_db) / 20);   mag = max(1e-10, amp @ pinv(basis).T) ** power
    The mel basis maps n_fft / 2 + 1 bins onto num_mels bands and is NOT invertible: the Moore-Penrose pseudo-inverse picks, among
    the spectra with these band amplitudes, the one of least norm (the least-squares choice, librosa's mel_to_stft without its
    non-negative solver) and the floor removes what it leaves negative.  The pseudo-inverse is computed once per table, in float64.
    The floored spectrum no longer has the band amplitudes asked for.  inversion="nnls" starts from it (rounded to float32) and
    runs nnls_iters iterations of accelerated projected gradient on |W x - amp|^2 over x >= 0 (mel_nnls_numpy / mel_nnls_hip by
    `backend`, the same bits), then applies max(1e-10, .) ** power in float64.  nnls_iters = 0 is the
    pseudo-inverse path, bit for bit."""
    return mel_to_linear_batch(tables, [S_db], ref_level_db, power, inversion=inversion, nnls_iters=nnls_iters, backend=backend,
                               device=device)[0]


# ---- sample-rate conversion (csrc/resample.hip, or float32 NumPy on the same table) -------------------------------------------------
#
# Source rate a, target rate b: g = gcd(a, b), up = b / g, down = a / g.  n samples give n_out = ceil(n up / down); output m sits at
# input time m down / up:  k0 = (m down) // up, phase = (m down) % up,
#   y[m] = sum_{j = -half + 1 .. half} h(phase / up - j) x[k0 + j]        (x = 0 outside [0, n))
#   h(tau) = s sinc(s tau) I0(beta sqrt(1 - (s tau / Z)^2)) / I0(beta) for |s tau| < Z, else 0;   s = rolloff min(1, up / down)
# half = ceil(Z / s), taps = 2 half.  The constants are those of a "kaiser best" design; the bits are this definition's, not those
# of any resampling library.

RESAMPLE_ZEROS = 64
RESAMPLE_ROLLOFF = 0.9475937167399596
RESAMPLE_BETA = 14.769656459379492
RESAMPLE_MAX_UP, RESAMPLE_MAX_DOWN, RESAMPLE_MAX_TAPS = 1024, 4096, 4096          # satt_resample_supported's bounds


def resample_ratio(src_rate, dst_rate):
    """(up, down) = (dst_rate, src_rate) in lowest terms"""
    src_rate, dst_rate = int(src_rate), int(dst_rate)
    if src_rate < 1 or dst_rate < 1:
        raise ValueError("resample: rates must be positive, got %d Hz -> %d Hz" % (src_rate, dst_rate))
    g = math.gcd(src_rate, dst_rate)
    return dst_rate // g, src_rate // g


def resample_length(n, up, down):
    return (int(n) * up + down - 1) // down


def resample_filter_half(up, down):
    """half = ceil(Z / s), s = rolloff min(1, up / down)"""
    return int(math.ceil(RESAMPLE_ZEROS / (RESAMPLE_ROLLOFF * min(1.0, up / down))))


def resample_check(src_rate, dst_rate):
    """raises ValueError naming both rates when csrc/resample.hip (and the NumPy restatement) does not take the pair: the predicate
    of satt_resample_supported, evaluated here so that both backends refuse the same pairs"""
    up, down = resample_ratio(src_rate, dst_rate)
    taps = 2 * resample_filter_half(up, down)
    if (up == 1 and down == 1) or up > RESAMPLE_MAX_UP or down > RESAMPLE_MAX_DOWN or taps > RESAMPLE_MAX_TAPS:
        raise ValueError("resample: %d Hz -> %d Hz is up / down = %d / %d with %d taps; supported are ratios other than 1 / 1 with "
                         "up <= %d, down <= %d and at most %d taps" % (src_rate, dst_rate, up, down, taps, RESAMPLE_MAX_UP,
                                                                        RESAMPLE_MAX_DOWN, RESAMPLE_MAX_TAPS))
    return up, down, taps


class ResampleTables:
    """the filter of one (source rate, target rate) pair: up, down, half, taps and table float32 [up, taps] with
    table[phase][j + half - 1] = h(phase / up - j), evaluated in float64 and rounded once; device copies are made on first use.
    The argument of h is formed as the exact rational |phase - j up| / up, so that table[p][jj] == table[up - p][taps - 1 - jj]
    bit for bit."""

    def __init__(self, src_rate, dst_rate):
        self.src_rate, self.dst_rate = int(src_rate), int(dst_rate)
        self.up, self.down, self.taps = resample_check(src_rate, dst_rate)
        self.half = self.taps // 2
        self.scale = RESAMPLE_ROLLOFF * min(1.0, self.up / self.down)
        j = np.arange(self.taps, dtype=np.int64) - (self.half - 1)
        q = np.abs(np.arange(self.up, dtype=np.int64)[:, None] - j[None, :] * self.up)            # |phase - j up|, exact
        u = self.scale * (q.astype(np.float64) / self.up)
        inside = u < RESAMPLE_ZEROS
        kaiser = np.i0(RESAMPLE_BETA * np.sqrt(np.where(inside, 1.0 - (u / RESAMPLE_ZEROS) ** 2, 0.0))) / np.i0(RESAMPLE_BETA)
        self.table = np.where(inside, self.scale * np.sinc(u) * kaiser, 0.0).astype(np.float32)
        self._dev, self._columns = {}, None

    def device(self, device):
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self.table).to(device)
        return self._dev[key]

    def columns(self):
        """the table transposed, float32 [taps, up] contiguous (made on first use): what resample_numpy gathers from"""
        if self._columns is None:
            self._columns = np.ascontiguousarray(self.table.T)
        return self._columns

    def length(self, n):
        return resample_length(n, self.up, self.down)


_RESAMPLE_TABLES = {}


def resample_tables(src_rate, dst_rate):
    """the ResampleTables of the pair, built once per process"""
    key = (int(src_rate), int(dst_rate))
    if key not in _RESAMPLE_TABLES:
        _RESAMPLE_TABLES[key] = ResampleTables(*key)
    return _RESAMPLE_TABLES[key]


RESAMPLE_NUMPY_BLOCK = 16384          # outputs summed at a time by resample_numpy (the temporaries stay in cache)


def resample_numpy(tables, y):
    """float32 [ceil(n up / down)] of one signal (n >= 1), with the kernel's operations in the kernel's order: for every output
    acc = acc + table[phase][jj] * x[k0 - half + 1 + jj], jj ascending, the product and the sum each rounded to float32 - the bits of
    csrc/resample.hip.  Vectorised over the outputs, a loop over the taps; the blocks only bound the temporaries."""
    t = tables
    y = np.ascontiguousarray(y, np.float32)
    if y.ndim != 1 or len(y) < 1:
        raise ValueError("resample: need a one-dimensional signal of at least one sample, got shape %r" % (y.shape,))
    n_out = t.length(len(y))
    padded = np.concatenate([np.zeros(t.half - 1, np.float32), y, np.zeros(t.half, np.float32)])     # x[k] at k + half - 1
    columns = t.columns()
    out = np.empty(n_out, np.float32)
    for m0 in range(0, n_out, RESAMPLE_NUMPY_BLOCK):
        pos = np.arange(m0, min(n_out, m0 + RESAMPLE_NUMPY_BLOCK), dtype=np.int64) * t.down
        k0 = pos // t.up
        phase = pos - k0 * t.up
        acc = np.zeros(len(pos), np.float32)
        for jj in range(t.taps):
            acc += columns[jj][phase] * padded[k0 + jj]
        out[m0:m0 + len(pos)] = acc
    return out


def resample_hip(tables, signals, device="cuda"):
    """one launch of csrc/resample.hip over `signals` (float32 arrays of >= 1 sample, all at tables.src_rate): the list of their
    float32 conversions"""
    import torch
    from .. import ops
    t = tables
    lens = np.asarray([len(s) for s in signals], np.int64)
    if lens.min() < 1:
        raise ValueError("resample: a signal of no samples")
    io = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    oo = np.concatenate([[0], np.cumsum((lens * t.up + t.down - 1) // t.down)]).astype(np.int64)
    x = torch.from_numpy(np.concatenate([np.ascontiguousarray(s, np.float32) for s in signals])).to(device)
    y = torch.empty(int(oo[-1]), dtype=torch.float32, device=device)
    ops.resample(x, torch.from_numpy(io).to(device), torch.from_numpy(oo).to(device), t.up, t.down, t.device(device), y)
    y = y.cpu().numpy()
    return [y[oo[u]:oo[u + 1]] for u in range(len(signals))]


class Audio:
    def __init__(self, hparams, backend=None, device="cuda", resample=False):
        self.hparams = hparams
        self.resample = bool(resample)
        if backend is None:
            backend = "hip" if _gpu_bound() else "numpy"
        if backend not in ("hip", "numpy"):
            raise ValueError("backend must be 'hip' or 'numpy', got %r" % (backend,))
        self.backend, self.device = backend, device
        n_fft, hop, win = stft_parameters(hparams)
        self.tables = MelspecTables(hparams.sample_rate, n_fft, win, hop, hparams.num_mels)
        if backend == "hip":
            from .. import ops
            if not ops.melspec_supported(n_fft, win, hop, hparams.num_mels):
                raise ValueError("the mel kernel does not take n_fft=%d win=%d hop=%d num_mels=%d (n_fft in 512 / 1024 / 2048 / 4096, "
                                 "16 <= win <= n_fft, 1 <= hop <= n_fft, num_mels <= 128)" % (n_fft, win, hop, hparams.num_mels))
        self.average_mel_level_db = np.array(hparams.average_mel_level_db, dtype=np.float32)
        self.stddev_mel_level_db = np.array(hparams.stddev_mel_level_db, dtype=np.float32)

    def read_wav(self, path):
        """(rate, float32 mono samples in [-1, 1) (int16 / 32768)) of a file, at the file's own rate"""
        from scipy.io import wavfile
        rate, data = wavfile.read(path)
        if data.ndim != 1:
            raise ValueError("%s: %d channels, need a mono file (rate %d Hz, hparams.sample_rate %d Hz)"
                             % (path, data.shape[1], rate, self.hparams.sample_rate))
        if data.dtype == np.int16:
            return rate, data.astype(np.float32) / np.float32(32768.0)
        if data.dtype == np.int32:
            return rate, (data.astype(np.float64) / 2147483648.0).astype(np.float32)
        if data.dtype == np.uint8:
            return rate, (data.astype(np.float32) - np.float32(128.0)) / np.float32(128.0)
        return rate, data.astype(np.float32)

    def check_rate(self, path, rate):
        """without `resample`, a file whose rate is not hparams.sample_rate is refused by name"""
        if rate != self.hparams.sample_rate and not self.resample:
            raise ValueError("%s: sample rate %d Hz differs from hparams.sample_rate %d Hz and resampling is not built"
                             % (path, rate, self.hparams.sample_rate))

    def load_wav(self, path):
        """float32 mono samples at hparams.sample_rate.  A file at another rate is refused, or with `resample` converted."""
        rate, y = self.read_wav(path)
        self.check_rate(path, rate)
        return self.resample_batch([y], [rate])[0] if self.resample else y

    def resample_batch(self, ys, rates):
        """the signals at hparams.sample_rate, in input order.  One already at that rate passes through as the same array; the rest
        are grouped by source rate and each group goes out in launches of at most MAX_LAUNCH_SAMPLES input samples (backend "numpy":
        one signal at a time).  A signal's result does not depend on what shares its batch."""
        if len(ys) != len(rates):
            raise ValueError("resample_batch: %d signals, %d rates" % (len(ys), len(rates)))
        target = self.hparams.sample_rate
        out, by_rate = list(ys), {}
        for i, rate in enumerate(rates):
            if int(rate) != target:
                by_rate.setdefault(int(rate), []).append(i)
        for rate, members in by_rate.items():
            tables = resample_tables(rate, target)
            if self.backend == "numpy":
                for i in members:
                    out[i] = resample_numpy(tables, ys[i])
                continue
            group, count = [], 0
            for i in members + [None]:
                if group and (i is None or count + len(ys[i]) > MAX_LAUNCH_SAMPLES):
                    for k, y in zip(group, resample_hip(tables, [ys[k] for k in group], self.device)):
                        out[k] = y
                    group, count = [], 0
                if i is not None:
                    group.append(i)
                    count += len(ys[i])
        return out

    def save_wav(self, wav, path):
        from scipy.io import wavfile
        wavfile.write(path, self.hparams.sample_rate, wav)

    def save_wav_pcm16(self, signal, path, peak=0.95):
        """16-bit PCM at hparams.sample_rate, the largest |sample| scaled to `peak` of full scale (a silent signal stays silent)"""
        signal = np.asarray(signal, np.float64)
        top = float(np.abs(signal).max()) if signal.size else 0.0
        pcm = np.round(signal * (peak * 32767.0 / top if top > 0.0 else 0.0)).astype(np.int16)
        self.save_wav(pcm, path)

    def trim(self, wav):
        """the signal without its leading and trailing silence, widened by num_silent_frames frame shifts on either side.  A frame
        (trim_frame_length samples every trim_hop_length, reflect-centred) is non-silent when 10 log10(max(1e-10, mean square)) lies
        less than trim_top_db below the loudest frame; a signal whose loudest frame is at or below the 1e-10 floor is empty."""
        hp = self.hparams
        wav = np.asarray(wav)
        n, fl, hop = len(wav), hp.trim_frame_length, hp.trim_hop_length
        if n == 0:
            return wav
        yp = np.pad(wav.astype(np.float64), fl // 2, mode="reflect") if n > 1 else np.full(n + 2 * (fl // 2), float(wav[0]))
        cs = np.concatenate([[0.0], np.cumsum(yp * yp)])
        starts = np.arange(1 + n // hop) * hop
        mse = (cs[starts + fl] - cs[starts]) / fl
        if mse.max() <= 1e-10:
            return wav[:0]
        db = 10.0 * np.log10(np.maximum(1e-10, mse))
        loud = np.nonzero(db - db.max() > -hp.trim_top_db)[0]
        start, end = int(loud[0]) * hop, min(n, (int(loud[-1]) + 1) * hop)
        sil = int(hp.num_silent_frames * hp.frame_shift_ms * hp.sample_rate / 1000)
        return wav[max(start - sil, 0):min(end + sil, n)]

    def _check_length(self, y):
        need = self.tables.n_fft // 2 + 1
        if len(y) < need:
            raise ValueError("a signal of %d samples is shorter than n_fft // 2 + 1 = %d: it cannot be reflect-padded" % (len(y), need))

    def melspectrogram_batch(self, ys):
        """list of float32 [T, num_mels], T = 1 + n // hop, one per signal"""
        for y in ys:
            self._check_length(y)
        if self.backend == "numpy":
            return [melspec_numpy(self.tables, y, self.hparams.ref_level_db) for y in ys]
        out, group, count = [], [], 0
        for y in ys:
            if group and count + len(y) > MAX_LAUNCH_SAMPLES:
                out += melspec_hip(self.tables, group, self.hparams.ref_level_db, self.device)
                group, count = [], 0
            group.append(y)
            count += len(y)
        if group:
            out += melspec_hip(self.tables, group, self.hparams.ref_level_db, self.device)
        return out

    def melspectrogram(self, y):
        """[num_mels, T], as the reference's"""
        return self.melspectrogram_batch([y])[0].T

    def normalize_mel(self, S):
        return (S - self.average_mel_level_db) / self.stddev_mel_level_db

    def denormalize_mel(self, S):
        """the inverse of normalize_mel: dB values from what the model predicts"""
        return S * self.stddev_mel_level_db + self.average_mel_level_db

    def inv_melspectrogram_batch(self, Ss, iters=60, alpha=0.99, power=1.0, seed=0, inversion="pinv", nnls_iters=MEL_NNLS_ITERS):
        """list of float32 signals of (T - 1) hop samples, one per dB mel spectrogram [T, num_mels] (melspectrogram_batch's layout):
        mel_to_linear, then `iters` Griffin-Lim iterations from a phase drawn uniformly on the host by np.random.default_rng(seed)
        - for every utterance afresh, so that neither the backend nor the batch changes the numbers it starts from.
        inversion="nnls": the non-negative mel inversion of mel_to_linear with nnls_iters iterations, the frames of all utterances
        solved together on this Audio's backend."""
        t = self.tables
        griffin_lim_check(t, [len(S) for S in Ss])
        mags = [m.astype(np.float32) for m in self.mel_to_linear_batch(Ss, power, inversion, nnls_iters)]
        angs = [np.exp(2j * np.pi * np.random.default_rng(seed).random(m.shape)).astype(np.complex64) for m in mags]
        if self.backend == "numpy":
            return [griffin_lim_numpy(t, m, a, iters, alpha) for m, a in zip(mags, angs)]
        out, group, count = [], [], 0
        for m, a in zip(mags, angs):
            n = (len(m) - 1) * t.hop
            if group and count + n > MAX_LAUNCH_SAMPLES:
                out += griffin_lim_hip(t, [g[0] for g in group], [g[1] for g in group], iters, alpha, self.device)
                group, count = [], 0
            group.append((m, a))
            count += n
        if group:
            out += griffin_lim_hip(t, [g[0] for g in group], [g[1] for g in group], iters, alpha, self.device)
        return out

    def mel_to_linear_batch(self, Ss, power=1.0, inversion="pinv", nnls_iters=MEL_NNLS_ITERS):
        """float64 linear magnitudes [T, n_fft / 2 + 1] of every dB mel spectrogram [T, num_mels]: what inv_melspectrogram_batch hands
        (as float32) to Griffin-Lim"""
        return mel_to_linear_batch(self.tables, Ss, self.hparams.ref_level_db, power, inversion=inversion, nnls_iters=nnls_iters,
                                   backend=self.backend, device=self.device)

    def mel_distance_batch(self, preds, refs, feature="mcep", order=13, want_paths=False, keys=None):
        """DTW distance of every (predicted, ground-truth) pair of NORMALISED mels [T, num_mels] (what .mfbsp files and the prediction
        records hold): a list of dicts frames_pred, frames_ref, steps, cost, value (and path int32 [steps, 2] of (pred frame, ref
        frame) with want_paths).  feature "mcep": mel_cepstrum of the de-normalised dB mel, value = MCD in dB =
        (10 sqrt(2) / ln 10) cost / steps; "mel": the dB rows themselves, value = cost / steps / sqrt(num_mels), an RMS log-spectral
        distance in dB.  Both backends align the same float32 features (utils/mel_distance.py; on "hip" all pairs in one launch) and
        agree bit for bit.  `keys` name the pairs in error messages (default: their index)."""
        from . import mel_distance as md
        if feature not in ("mcep", "mel"):
            raise ValueError("feature must be 'mcep' or 'mel', got %r" % (feature,))
        if len(preds) != len(refs):
            raise ValueError("mel_distance_batch: %d predictions, %d references" % (len(preds), len(refs)))
        M = self.hparams.num_mels
        pairs = []
        for u, (pred, ref) in enumerate(zip(preds, refs)):
            name = keys[u] if keys is not None else "pair %d" % u
            feats = []
            for what, S in (("prediction", pred), ("reference", ref)):
                S = np.asarray(S)
                if S.ndim != 2 or S.shape[1] != M:
                    raise ValueError("%s: the %s has shape %r, need [T, num_mels=%d]" % (name, what, S.shape, M))
                if not 1 <= S.shape[0] <= md.DTW_MAX_FRAMES:
                    raise ValueError("%s: the %s has %d frames, need 1 .. %d" % (name, what, S.shape[0], md.DTW_MAX_FRAMES))
                if not np.isfinite(S).all():
                    raise ValueError("%s: the %s holds non-finite values" % (name, what))
                S_db = self.denormalize_mel(S.astype(np.float64))
                feats.append(md.mel_cepstrum(S_db, order) if feature == "mcep" else S_db.astype(np.float32))
            pairs.append(tuple(feats))
        if self.backend == "numpy":
            res = [md.dtw_numpy(a, b, want_paths) for a, b in pairs]
        else:
            res = md.dtw_hip(pairs, want_paths, self.device)
        scale = md.MCD_SCALE if feature == "mcep" else 1.0 / math.sqrt(M)
        out = []
        for (a, b), r in zip(pairs, res):
            o = dict(frames_pred=len(a), frames_ref=len(b), steps=int(r[1]), cost=float(r[0]), value=scale * float(r[0]) / int(r[1]))
            if want_paths:
                o["path"] = r[2]
            out.append(o)
        return out

    def f0_batch(self, ys, fmin=None, fmax=None, window_ms=None, threshold=None, silence_db=None, tracker="yin", jump_cost=None,
                 switch_cost=None, unvoiced_cost=None, lag_bias=None):
        """YIN pitch tracks of signals at hparams.sample_rate on the mel frame grid (utils/pitch.py): a list of dicts
        f0 (float32, Hz; 0 where no lag passes the threshold), voiced (bool), aperiodicity and power (float32), each [1 + n // hop].
        On "hip" the batch is one launch of csrc/yin.hip (cut at MAX_LAUNCH_SAMPLES), on "numpy" its float32 restatement: the same
        bits.  The defaults are pitch.FMIN / FMAX / WINDOW_MS / THRESHOLD / SILENCE_DB; they are arguments, not hparams.
        tracker="viterbi" (pitch.track_f0) chooses among the 8 deepest dips of every frame along the utterance instead (the costs
        default to pitch.JUMP_COST / SWITCH_COST / LAG_BIAS and the threshold) and adds `state` (uint8; 8 is unvoiced) to the dicts;
        utterances of more than pitch.F0_VITERBI_MAX_FRAMES frames are refused."""
        from . import pitch
        if tracker != "yin":
            kw = dict(fmin=pitch.FMIN if fmin is None else fmin, fmax=pitch.FMAX if fmax is None else fmax,
                      window_ms=pitch.WINDOW_MS if window_ms is None else window_ms,
                      threshold=pitch.THRESHOLD if threshold is None else threshold,
                      silence_db=pitch.SILENCE_DB if silence_db is None else silence_db,
                      jump_cost=pitch.JUMP_COST if jump_cost is None else jump_cost,
                      switch_cost=pitch.SWITCH_COST if switch_cost is None else switch_cost,
                      unvoiced_cost=unvoiced_cost, lag_bias=pitch.LAG_BIAS if lag_bias is None else lag_bias)
            res = pitch.track_f0(ys, self.hparams.sample_rate, self.tables.hop, tracker=tracker, backend=self.backend, device=self.device,
                                 with_state=True, **kw)
            return [dict(f0=f0, voiced=v, aperiodicity=ap, power=power, state=state) for f0, ap, power, v, state in res]
        kw = dict(fmin=pitch.FMIN if fmin is None else fmin, fmax=pitch.FMAX if fmax is None else fmax,
                  window_ms=pitch.WINDOW_MS if window_ms is None else window_ms,
                  threshold=pitch.THRESHOLD if threshold is None else threshold)
        silence_db = pitch.SILENCE_DB if silence_db is None else silence_db
        sr, hop = self.hparams.sample_rate, self.tables.hop
        pitch.yin_check(sr, hop, kw["fmin"], kw["fmax"], kw["window_ms"])
        if self.backend == "numpy":
            res = [pitch.yin_numpy(y, sr, hop, **kw) for y in ys]
        else:
            res = pitch.yin_hip(ys, sr, hop, device=self.device, **kw) if len(ys) else []
        return [dict(f0=f0, voiced=pitch.voicing(f0, power, silence_db), aperiodicity=ap, power=power) for f0, ap, power in res]

    def inv_melspectrogram(self, S, iters=60, alpha=0.99, power=1.0, seed=0, inversion="pinv", nnls_iters=MEL_NNLS_ITERS):
        """float32 [(T - 1) hop] from one dB mel spectrogram [num_mels, T], the layout melspectrogram returns"""
        return self.inv_melspectrogram_batch([np.asarray(S).T], iters, alpha, power, seed, inversion, nnls_iters)[0]


def _gpu_bound():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False
