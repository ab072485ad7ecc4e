"""Shared yardstick of the DTW tests (test_dtw_cpu / test_dtw_gpu): a plain float64 per-cell dynamic programme (small sizes only),
the case builders, and the rounding bound both backends are held to.

gamma(Ta, Tb, K) = (Ta + Tb + K + 3) 2^-24 bounds the relative rounding a float32 path cost accumulates: at most Ta + Tb - 1
additions along the path, a K-term sum and a square root per local cost, each half an ulp (2^-24) of a non-negative partial result.
It is derived, not measured.  With P = the float64 cost re-summed along the backend's own path and D64 = the float64 optimum:
    |cost - P| <= gamma P          and          D64 <= P <= D64 (1 + 2 gamma)
(the second: the backend's path is optimal for costs that each lie within gamma of the float64 ones)."""
import numpy as np


def gamma(Ta, Tb, K):
    return (Ta + Tb + K + 3) * 2.0 ** -24


def costs64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2))


def dp64(a, b):
    """(D64, steps, path, local costs float64 [Ta, Tb]) by the definition, one cell at a time: predecessors in the order diagonal, up,
    left, a later one replacing an earlier one only when strictly smaller"""
    c = costs64(a, b)
    Ta, Tb = c.shape
    D = np.zeros((Ta, Tb))
    L = np.zeros((Ta, Tb), np.int64)
    back = {}
    for i in range(Ta):
        for j in range(Tb):
            if i == 0 and j == 0:
                D[0, 0], L[0, 0] = c[0, 0], 1
                continue
            best = None
            for pi, pj in ((i - 1, j - 1), (i - 1, j), (i, j - 1)):
                if pi >= 0 and pj >= 0 and (best is None or D[pi, pj] < D[best]):
                    best = (pi, pj)
            D[i, j], L[i, j], back[i, j] = D[best] + c[i, j], L[best] + 1, best
    cell, path = (Ta - 1, Tb - 1), []
    while cell != (0, 0):
        path.append(cell)
        cell = back[cell]
    path.append((0, 0))
    return D[-1, -1], int(L[-1, -1]), np.asarray(path[::-1], np.int32), c


def path_problems(path, Ta, Tb, steps):
    """what is wrong with a warping path ([] when nothing is): it starts at (0, 0), ends at (Ta-1, Tb-1), moves by (1, 1), (1, 0) or
    (0, 1) and has `steps` entries"""
    path = np.asarray(path)
    bad = []
    if steps < 1 or path.ndim != 2 or path.shape != (steps, 2):
        return ["shape %r, steps %d" % (path.shape, steps)]
    if tuple(path[0]) != (0, 0):
        bad.append("starts at %r" % (tuple(path[0]),))
    if tuple(path[-1]) != (Ta - 1, Tb - 1):
        bad.append("ends at %r" % (tuple(path[-1]),))
    moves = {tuple(m) for m in np.diff(path, axis=0)}
    if not moves <= {(1, 1), (1, 0), (0, 1)}:
        bad.append("moves %r" % sorted(moves))
    return bad


def check_against_float64(cost, steps, path, a, b, ref=None):
    """the two gamma bounds of the module docstring for one backend result; returns (|cost - P| / P, P / D64 - 1, gamma)"""
    Ta, Tb, K = len(a), len(b), a.shape[1]
    assert not path_problems(path, Ta, Tb, steps), path_problems(path, Ta, Tb, steps)
    D64, _, _, c = ref if ref is not None else dp64(a, b)
    P = 0.0
    for i, j in path:                              # summed in path order, as dp64 sums: rounded addition is monotone, so D64 <= P exactly
        P += float(c[i, j])
    g = gamma(Ta, Tb, K)
    e1 = abs(float(cost) - P) / P if P > 0 else abs(float(cost))
    e2 = P / D64 - 1.0 if D64 > 0 else P
    print("%d x %d x %d: |cost - P| / P = %.3e, P / D64 - 1 = %.3e (gamma %.3e)" % (Ta, Tb, K, e1, e2, g))
    assert e1 <= g, (e1, g)
    assert D64 <= P and e2 <= 2 * g, (D64, P, e2, g)
    return e1, e2, g


def warped_pair(Ta, Tb, K, seed=0):
    """a random sequence [Ta, K] and a time-warped, noised copy of it [Tb, K], float32"""
    rng = np.random.default_rng(seed + 1000 * Ta + 7 * Tb + K)
    a = (3.0 * rng.standard_normal((Ta, K))).astype(np.float32)
    idx = np.clip(np.round(np.linspace(0, Ta - 1, Tb) + rng.normal(0, 2, Tb)), 0, Ta - 1).astype(int)
    idx.sort()
    b = (a[idx] + 0.3 * rng.standard_normal((Tb, K))).astype(np.float32)
    return a, b


def tie_pair(Ta, Tb, K, seed=0):
    """small integers: local costs repeat, so the accumulated costs tie exactly and often"""
    rng = np.random.default_rng(seed + Ta + 3 * Tb)
    return rng.integers(0, 3, (Ta, K)).astype(np.float32), rng.integers(0, 3, (Tb, K)).astype(np.float32)


# Two hand-worked tie-break examples (K = 1, local cost |a_i - b_j|; dir: 0 diagonal, 1 up, 2 left).  Between them every kind of
# three-predecessor cell occurs: each predecessor strictly smallest, every two-way tie and the three-way tie.
#
# 1. a = 0 1 1, b = 0 0 1 1
#   c = 0 0 1 1      D = 0 0 1 2      dir = . 2 2 2      L = 1 2 3 4
#       1 1 0 0          1 1 0 0            1 0 0 2          2 2 3 4
#       1 1 0 0          2 2 0 0            1 0 1 0          3 3 4 4
# (1, 1): diagonal 0, up 0, left 1 - the tie of diagonal and up goes to the diagonal;  (1, 2): diagonal 0, up 1, left 1;
# (1, 3): diagonal 1, up 2, left 0 - left, strictly smaller;  (2, 1): diagonal 1, up 1, left 2 - the tie goes to the diagonal;
# (2, 2): diagonal 1, up 0, left 2 - up, strictly smaller;  (2, 3): diagonal 0, up 0, left 0 - the triple tie goes to the diagonal.
#
# 2. a = 0 2 1, b = 3 1 0 1: the corner has up == left < diagonal, the one tie in which "up before left" decides - and the two
#    predecessors carry different lengths, so that order shows in steps, in the direction and in the path.
#   c = 3 1 0 1      D = 3 4 4 5      dir = . 2 2 2      L = 1 2 3 4
#       1 1 2 1          4 4 6 5            1 0 0 0          2 2 3 4
#       2 0 1 0          6 4 5 5            1 0 0 1          3 3 3 5
# (1, 1): diagonal 3, up 4, left 4 - diagonal, 3 + 1;  (1, 2): diagonal 4, up 4, left 4 - the triple tie goes to the diagonal, 4 + 2,
# L = L(0, 1) + 1 = 3;  (1, 3): diagonal 4, up 5, left 6 - diagonal, 4 + 1, L = L(0, 2) + 1 = 4;
# (2, 1): diagonal 4, up 4, left 6 - the tie goes to the diagonal, 4 + 0, L = L(1, 0) + 1 = 3;
# (2, 2): diagonal 4, up 6, left 4 - the tie of diagonal and left goes to the diagonal, 4 + 1, L = L(1, 1) + 1 = 3;
# (2, 3): diagonal 6, up 5, left 5 - up == left < diagonal: UP, 5 + 0, L = L(1, 3) + 1 = 5 (left would give L(2, 2) + 1 = 4).
#
# D(i, j), L(i, j) and dir(i, j) of a whole pair are cost, steps and the last move of the pair cut to a[:i + 1], b[:j + 1].
def _column(*values):
    return np.asarray(values, np.float32)[:, None]


HAND_EXAMPLES = [
    dict(a=_column(0, 1, 1), b=_column(0, 0, 1, 1),
         D=np.asarray([[0, 0, 1, 2], [1, 1, 0, 0], [2, 2, 0, 0]], np.float32),
         dir=np.asarray([[0, 2, 2, 2], [1, 0, 0, 2], [1, 0, 1, 0]], np.uint8),
         L=np.asarray([[1, 2, 3, 4], [2, 2, 3, 4], [3, 3, 4, 4]], np.int32),
         path=np.asarray([[0, 0], [0, 1], [1, 2], [2, 3]], np.int32)),
    dict(a=_column(0, 2, 1), b=_column(3, 1, 0, 1),
         D=np.asarray([[3, 4, 4, 5], [4, 4, 6, 5], [6, 4, 5, 5]], np.float32),
         dir=np.asarray([[0, 2, 2, 2], [1, 0, 0, 0], [1, 0, 0, 1]], np.uint8),
         L=np.asarray([[1, 2, 3, 4], [2, 2, 3, 4], [3, 3, 3, 5]], np.int32),
         path=np.asarray([[0, 0], [0, 1], [0, 2], [1, 3], [2, 3]], np.int32)),
]
HAND_CELLS = [(e, i, j) for e in range(len(HAND_EXAMPLES)) for i in range(3) for j in range(4)]


def hand_prefix(e, i, j):
    """the pair of example e cut to the cell (i, j), and what D, L and dir hold there"""
    x = HAND_EXAMPLES[e]
    return (x["a"][:i + 1], x["b"][:j + 1]), (x["D"][i, j], int(x["L"][i, j]), int(x["dir"][i, j]))


MOVES = {(1, 1): 0, (1, 0): 1, (0, 1): 2}


def last_move(path):
    """the direction code of a path's last move (0 for the one-cell path)"""
    return MOVES[tuple(path[-1] - path[-2])] if len(path) > 1 else 0
