"""Audio front end of the preprocessing drivers: the reference-named `Audio(hparams)` class (reference utils/audio.py) without
librosa.  The log-mel spectrogram runs in csrc/melspec.hip (backend "hip") or as a float32 scipy.fft restatement (backend
"numpy", for machines without a GPU); both follow librosa.stft's defaults: frames centred by reflect padding, a periodic Hann
window of `win` points zero-padded to n_fft, T = 1 + n // hop frames, Slaney's mel basis.  `trim` is O(n) host code (DESIGN.md
records the semantics chosen for it).  Resampling is not built: a wav whose rate differs from hparams.sample_rate is refused."""
import numpy as np

MAX_LAUNCH_SAMPLES = 1 << 23          # samples per kernel launch of melspectrogram_batch (32 MB of signal; one longer utterance
                                      # still goes out as a launch of its own)


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

    def device(self, device):
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = {k: torch.from_numpy(np.ascontiguousarray(getattr(self, k))).to(device)
                              for k in ("window", "twiddle", "band_start", "band_offset", "band_weight")}
        return self._dev[key]


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


def melspec_numpy(tables, y, ref_level_db, want_mag=False):
    """the same in float32 NumPy / scipy.fft: [T, num_mels] of one signal"""
    try:
        from scipy.fft import rfft
    except ImportError:                  # numpy's transform computes in float64; the result is rounded to float32 behind it
        rfft = np.fft.rfft
    t = tables
    y = np.ascontiguousarray(y, np.float32)
    T = frame_count(len(y), t.hop)
    yp = np.pad(y, t.n_fft // 2, mode="reflect")
    frames = np.lib.stride_tricks.as_strided(yp, (T, t.n_fft), (yp.strides[0] * t.hop, yp.strides[0]), writeable=False)
    mag = np.abs(rfft(frames * t.window[None, :], axis=1)).astype(np.float32)
    mel = mag @ t.basis.astype(np.float32).T
    db = (20.0 * np.log10(np.maximum(np.float32(1e-5), mel)) - np.float32(ref_level_db)).astype(np.float32)
    return (db, mag) if want_mag else db


class Audio:
    def __init__(self, hparams, backend=None, device="cuda"):
        self.hparams = hparams
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

    def load_wav(self, path):
        """float32 mono samples in [-1, 1) (int16 / 32768).  No resampling: the file's rate must be hparams.sample_rate."""
        from scipy.io import wavfile
        rate, data = wavfile.read(path)
        if data.ndim != 1:
            raise ValueError("%s: %d channels, need a mono file (rate %d Hz, hparams.sample_rate %d Hz)"
                             % (path, data.shape[1], rate, self.hparams.sample_rate))
        if rate != self.hparams.sample_rate:
            raise ValueError("%s: sample rate %d Hz differs from hparams.sample_rate %d Hz and resampling is not built"
                             % (path, rate, self.hparams.sample_rate))
        if data.dtype == np.int16:
            return data.astype(np.float32) / np.float32(32768.0)
        if data.dtype == np.int32:
            return (data.astype(np.float64) / 2147483648.0).astype(np.float32)
        if data.dtype == np.uint8:
            return (data.astype(np.float32) - np.float32(128.0)) / np.float32(128.0)
        return data.astype(np.float32)

    def save_wav(self, wav, path):
        from scipy.io import wavfile
        wavfile.write(path, self.hparams.sample_rate, wav)

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


def _gpu_bound():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False
