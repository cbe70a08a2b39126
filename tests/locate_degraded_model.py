"""A numpy model of rs_locate_device_degraded's contract (include/rs_mi355x.h "degraded locate"),
on the CPU oracle alone.  No tests here: tests/test_locate_degraded_cpu.py and
tests/test_gpu_locate_degraded.py import it.

With m originals missing, sel the selected recovery rows in increasing order, R = sel[:m] the
reference rows and K = sel[m:] the check rows:

    F    the originals completed from R: present rows as stored, missing rows from O.decode with
         recovery_present = the indicator of R
    D    O.encode(F) ^ recovery, as GF(2^16) elements per column
    T    [M, N]: T[j][p] = D_j of the unit stripe whose information position p holds the element 1
         (original p where it is present, else reference row R[rank of p among the missing]),
         through the same two oracle calls

and the result for a stripe is the locate's (tests/locate_model.py) over the rows of K and the
table T, with a located position p of a missing original named N + R[rank(p)].
"""
import numpy as np

import locate_model as LM
import oracle_lib as O
from test_update_cpu import elements

CLEAN, ROWS, UNKNOWN = LM.CLEAN, LM.ROWS, LM.UNKNOWN

_T = {}


def split(present, mask, M):
    """(present as bool [N], R, K) of a call's two masks (mask None = every row)."""
    present = np.asarray(present) != 0
    sel = np.arange(M) if mask is None else np.flatnonzero(np.asarray(mask) != 0)
    m = int((~present).sum())
    assert len(sel) >= m + 2, "the call needs two check rows at least"
    return present, sel[:m], sel[m:]


def complete(rate, orig, present, rec, R):
    """F [N, S]: absent rows of `orig` and rows of `rec` outside R are not used."""
    present = np.asarray(present) != 0
    if present.all():
        return orig.copy()
    rp = np.zeros(rec.shape[0], np.uint8)
    rp[R] = 1
    o = np.where(present[:, None], orig, 0).astype(np.uint8)
    r = np.where(rp[:, None] != 0, rec, 0).astype(np.uint8)
    out = O.decode(rate, o, present.astype(np.uint8), r, rp)
    return np.where(present[:, None], orig, out).astype(np.uint8)


def names(present, R, N):
    """[N]: what a located information position is called: p, or N + its reference row."""
    out = np.arange(N)
    out[~present] = N + np.asarray(R, np.int64)
    return out


def coefficients(rate, N, M, present, R):
    """T [M, N] (rows of R: zero), from the unit stripe in the coefficient kernels' layout (64 *
    ceil(N / 32) bytes per shard, element p of the shard of position p = 1).  Once per key."""
    present = np.asarray(present) != 0
    key = (rate, N, M, present.tobytes(), tuple(int(j) for j in R))
    if key not in _T:
        W = 64 * ((N + 31) // 32)
        p = np.arange(N)
        col = (p // 32) * 64 + p % 32
        uo, ur = np.zeros((N, W), np.uint8), np.zeros((M, W), np.uint8)
        uo[p[present], col[present]] = 1
        ur[np.asarray(R, np.int64), col[~present]] = 1
        F = complete(rate, uo, present, ur, R)
        coef = O.encode(rate, F, M) ^ ur
        T = coef[:, col].astype(np.int64) | coef[:, col + 32].astype(np.int64) << 8
        T[np.asarray(R, np.int64)] = 0  # (their D is zero by construction: not check rows)
        T.setflags(write=False)
        _T[key] = T
    return _T[key]


def locate(rate, orig, present, rec, mask=None):
    """(located, flags [M] uint8, F [N, S]) of one stripe under the contract."""
    N, M = orig.shape[0], rec.shape[0]
    present, R, K = split(present, mask, M)
    F = complete(rate, orig, present, rec, R)
    D = elements(O.encode(rate, F, M) ^ rec).astype(np.int64)
    flags = np.zeros(M, np.uint8)
    flags[K] = D[K].any(axis=1)
    n = int(flags.sum())
    if n == 0:
        return CLEAN, flags, F
    if n < len(K):
        return ROWS, flags, F
    T = coefficients(rate, N, M, present, R)
    j0, j1 = K[0], K[1]
    col = int(np.flatnonzero(D[j0])[0])
    cand = np.flatnonzero((T[j0] != 0) & (LM.gf_mul(T[j1], D[j0, col]) == LM.gf_mul(T[j0], D[j1, col])))
    for p in cand:
        if LM.explains(T, D, K, int(p)):
            return int(names(present, R, N)[p]), flags, F
    return UNKNOWN, flags, F
