"""Objective distance between a predicted and a ground-truth mel spectrogram of different lengths: a dynamic-time-warping (DTW)
alignment of per-frame features and the mean local cost along the path (DESIGN.md 3.6 holds the definition).  The features are
either a cepstrum of the mel filterbank (`mel_cepstrum`: orthonormal DCT-II rows 1 .. order of the natural-log mel, c_0 dropped; the
value is then a mel-cepstral distortion in dB) or the dB mel rows themselves (an RMS log-spectral distance in dB).  The alignment
runs in csrc/dtw.hip (backend "hip", a batch of pairs in one launch) or in `dtw_numpy`, a float32 restatement with the kernel's
operations in the kernel's order: both consume the same float32 features and agree bit for bit on cost, steps and path.

This is NOT the MCD of the literature's WORLD / mel-generalised cepstra: it is a cepstrum of this project's mel filterbank, and its
values compare between runs of this tool only."""
import math

import numpy as np

DTW_MAX_FRAMES = 2048                 # satt_dtw_max_frames(): three diagonals of D and L in 48 KiB of LDS
DTW_MAX_K = 128
DTW_NT = 512                          # threads per workgroup of csrc/dtw.hip: row i belongs to thread i % DTW_NT
DTW_WORKSPACE_BYTES = 1 << 28         # direction bytes (Ta * Tb per pair) one launch of dtw_hip may ask for; a batch that needs more
                                      # goes out in several launches (64 pairs of 2048 x 2048 fit one)
MCD_SCALE = 10.0 * math.sqrt(2.0) / math.log(10.0)


def dtw_supported(Ta, Tb, K):
    """the predicate of satt_dtw_supported, evaluated here so that both backends refuse the same shapes"""
    return 1 <= Ta <= DTW_MAX_FRAMES and 1 <= Tb <= DTW_MAX_FRAMES and 1 <= K <= DTW_MAX_K


def mel_cepstrum(S_db, order):
    """float32 [T, order]: c_k = sqrt(2 / M) sum_m x_m cos(pi k (m + 0.5) / M), k = 1 .. order, of x = S_db ln(10) / 20 (the natural
    log of the mel amplitudes), evaluated in float64 and rounded once.  S_db: de-normalised dB mel [T, M].  c_0 is dropped: a
    constant level offset does not count."""
    S_db = np.asarray(S_db, np.float64)
    if S_db.ndim != 2:
        raise ValueError("mel_cepstrum: need [T, num_mels], got shape %r" % (S_db.shape,))
    M = S_db.shape[1]
    if not 1 <= order < M:
        raise ValueError("mel_cepstrum: order=%d is outside 1 .. num_mels - 1 = %d" % (order, M - 1))
    basis = math.sqrt(2.0 / M) * np.cos(np.pi * np.arange(1, order + 1)[:, None] * (np.arange(M)[None, :] + 0.5) / M)
    return ((S_db * (math.log(10.0) / 20.0)) @ basis.T).astype(np.float32)


def _check_pair(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1]:
        raise ValueError("dtw: need [Ta, K] and [Tb, K], got shapes %r and %r" % (a.shape, b.shape))
    if not dtw_supported(a.shape[0], b.shape[0], a.shape[1]):
        raise ValueError("dtw: Ta=%d Tb=%d K=%d is outside 1 <= Ta, Tb <= %d, 1 <= K <= %d"
                         % (a.shape[0], b.shape[0], a.shape[1], DTW_MAX_FRAMES, DTW_MAX_K))
    return a, b


def local_costs(a, b):
    """float32 [Ta, Tb]: sqrt(sum_k (a[i, k] - b[j, k])^2), k ascending in one chain, difference, product and sum each rounded"""
    acc = np.zeros((a.shape[0], b.shape[0]), np.float32)
    for k in range(a.shape[1]):
        d = a[:, k, None] - b[None, :, k]
        acc += d * d
    return np.sqrt(acc)


def dtw_numpy(a, b, want_path=False):
    """(cost float32, steps int[, path int32 [steps, 2]]) of one pair, float32 [Ta, K] against [Tb, K], with the operations of
    csrc/dtw.hip in its order.  Vectorised along the anti-diagonals i + j == d: arrays indexed by the row i hold the two diagonals
    before; the cells of row 0 and column 0 have one predecessor and are set apart."""
    a, b = _check_pair(a, b)
    Ta, Tb = a.shape[0], b.shape[0]
    C = local_costs(a, b).ravel()                                  # cell (i, j) at i Tb + j: a diagonal is a slice of stride Tb - 1
    D = [np.zeros(Ta, np.float32) for _ in range(3)]
    L = [np.zeros(Ta, np.int32) for _ in range(3)]
    dirs = np.zeros(Ta * Tb, np.uint8) if want_path else None
    for d in range(Ta + Tb - 1):
        lo, hi = max(0, d - (Tb - 1)), min(d, Ta - 1)
        Dc, D1, D2 = D[d % 3], D[(d - 1) % 3], D[(d - 2) % 3]
        Lc, L1, L2 = L[d % 3], L[(d - 1) % 3], L[(d - 2) % 3]
        if d == 0:
            Dc[0], Lc[0] = C[0], 1
            continue
        if lo == 0:                                                # (0, d): left only
            Dc[0], Lc[0] = D1[0] + C[d], L1[0] + 1
            if want_path:
                dirs[d] = 2
        if hi == d:                                                # (d, 0): up only
            Dc[d], Lc[d] = D1[d - 1] + C[d * Tb], L1[d - 1] + 1
            if want_path:
                dirs[d * Tb] = 1
        s, e = max(lo, 1), min(hi, d - 1)                          # the cells with three predecessors
        if s > e:
            continue
        first = s * Tb + d - s
        diag = slice(first, first + (e - s) * (Tb - 1) + 1, Tb - 1)      # (Tb >= 2 here: a single column has no such cell)
        best, length = D2[s - 1:e].copy(), L2[s - 1:e].copy()
        m1 = D1[s - 1:e] < best
        best[m1], length[m1] = D1[s - 1:e][m1], L1[s - 1:e][m1]
        m2 = D1[s:e + 1] < best
        best[m2], length[m2] = D1[s:e + 1][m2], L1[s:e + 1][m2]
        Dc[s:e + 1] = best + C[diag]
        Lc[s:e + 1] = length + 1
        if want_path:
            dirs[diag] = np.where(m2, 2, np.where(m1, 1, 0))
    last = (Ta + Tb - 2) % 3
    cost, steps = D[last][Ta - 1], int(L[last][Ta - 1])
    if not want_path:
        return cost, steps
    path = np.zeros((steps, 2), np.int32)
    i, j = Ta - 1, Tb - 1
    for s in range(steps - 1, -1, -1):
        path[s] = (i, j)
        if i == 0 and j == 0:
            break
        move = dirs[i * Tb + j]
        if i == 0:
            j -= 1
        elif j == 0:
            i -= 1
        elif move == 0:
            i, j = i - 1, j - 1
        elif move == 1:
            i -= 1
        else:
            j -= 1
    return cost, steps, path


def _dtw_launch(pairs, want_paths, device):
    import torch
    from .. import ops
    K = pairs[0][0].shape[1]
    ta = np.asarray([len(a) for a, _ in pairs], np.int64)
    tb = np.asarray([len(b) for _, b in pairs], np.int64)

    def offsets(counts):
        return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ao, bo = offsets(ta), offsets(tb)
    a = torch.from_numpy(np.concatenate([p[0] for p in pairs])).to(device)
    b = torch.from_numpy(np.concatenate([p[1] for p in pairs])).to(device)
    cost = torch.empty(len(pairs), dtype=torch.float32, device=device)
    steps = torch.empty(len(pairs), dtype=torch.int32, device=device)
    dirs = do = path = po = None
    if want_paths:
        do, po = offsets(ta * tb), offsets(ta + tb - 1)
        dirs = torch.empty(int(do[-1]), dtype=torch.uint8, device=device)
        path = torch.empty((int(po[-1]), 2), dtype=torch.int32, device=device)
        do_d, po_d = torch.from_numpy(do).to(device), torch.from_numpy(po).to(device)
    ops.dtw(a, b, torch.from_numpy(ao).to(device), torch.from_numpy(bo).to(device), int(ta.max()), int(tb.max()), cost, steps,
            dirs, do_d if want_paths else None, path, po_d if want_paths else None)
    cost, steps = cost.cpu().numpy(), steps.cpu().numpy()
    if not want_paths:
        return [(cost[u], int(steps[u])) for u in range(len(pairs))]
    path = path.cpu().numpy()
    return [(cost[u], int(steps[u]), path[po[u]:po[u] + steps[u]].copy()) for u in range(len(pairs))]


def dtw_hip(pairs, want_paths=False, device="cuda", workspace_bytes=None):
    """csrc/dtw.hip over `pairs`, a list of (a float32 [Ta, K], b float32 [Tb, K]) with one K: the list of (cost float32, steps int[,
    path int32 [steps, 2]]), in input order.  One launch for the batch; with paths it is cut only where the direction workspace
    (Ta * Tb bytes per pair) would exceed `workspace_bytes` (default DTW_WORKSPACE_BYTES; one pair always goes out)."""
    pairs = [_check_pair(a, b) for a, b in pairs]
    if not pairs:
        return []
    if len({a.shape[1] for a, _ in pairs}) != 1:
        raise ValueError("dtw: the pairs of a batch must share one feature width, got %r" % sorted({a.shape[1] for a, _ in pairs}))
    if not want_paths:
        return _dtw_launch(pairs, False, device)
    budget = DTW_WORKSPACE_BYTES if workspace_bytes is None else int(workspace_bytes)
    out, group, used = [], [], 0
    for a, b in pairs:
        need = len(a) * len(b)
        if group and used + need > budget:
            out += _dtw_launch(group, True, device)
            group, used = [], 0
        group.append((a, b))
        used += need
    return out + _dtw_launch(group, True, device)
