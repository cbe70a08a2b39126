"""A numpy model of rs_locate_device's contract (include/rs_mi355x.h "locate"), on the CPU oracle
alone.  No tests here: tests/test_locate_cpu.py and tests/test_gpu_locate.py import it.

With D_j = recovery_j ^ encode(originals)_j (GF(2^16) elements per column) and G[j][i] = element j
of the encode of the unit stripe (original i = the element 1), the result for a stripe is

    CLEAN    no selected row has D_j != 0
    ROWS     some selected row has, some has not
    i        every selected row has, and D_j = G[j][i] * e for one e per column, for every selected j
    UNKNOWN  every selected row has, and no i does that

The model states the last two directly: any such i must reproduce the ratio D_j1 / D_j0 in a column
where D_j0 != 0 (j0, j1: two selected rows), so only the originals with that ratio are tried -- each
of them over every selected row and every column.
"""
import numpy as np

import oracle_lib as O
from test_update_cpu import elements

CLEAN, ROWS, UNKNOWN = -1, -2, -3

_G = {}
_TABLES = []


def tables():
    if not _TABLES:
        _TABLES.extend([O.table("exp", 65536).astype(np.int64), O.table("log", 65536).astype(np.int64)])
    return _TABLES


def gf_mul(a, b):
    """Element-wise product in GF(2^16) as Engine::mul forms it: a * exp(log b), 0 where either is 0."""
    exp, log = tables()
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    p = exp[(log[a] + log[b]) % 65535]
    return np.where((a == 0) | (b == 0), 0, p)


def coefficients(rate, N, M):
    """G [M, N] from the oracle's encode of the identity stripe in the coefficient kernels' layout
    (64 * ceil(N / 32) bytes per shard, element i of row i = 1).  Computed once per shape."""
    key = (rate, N, M)
    if key not in _G:
        W = 64 * ((N + 31) // 32)
        unit = np.zeros((N, W), np.uint8)
        i = np.arange(N)
        unit[i, (i // 32) * 64 + i % 32] = 1
        coef = O.encode(rate, unit, M)
        G = coef[:, (i // 32) * 64 + i % 32].astype(np.int64) | coef[:, (i // 32) * 64 + 32 + i % 32].astype(np.int64) << 8
        G.setflags(write=False)
        _G[key] = G
    return _G[key]


def syndromes(rate, orig, rec):
    """D [M, S / 2]: the stored recovery against the oracle's encode of the stored originals."""
    return elements(O.encode(rate, orig, rec.shape[0]) ^ rec).astype(np.int64)


def explains(G, D, sel, i):
    """Does original i alone explain D over the selected rows: one e per column with D_j = G[j][i] * e?"""
    j0 = sel[0]
    if G[j0, i] == 0:
        # e is free where G[j0][i] = 0, but then D_j0 = 0 everywhere: not a stripe whose rows all differ
        return False
    # cross-multiplied, so that no division is needed: D_j * G[j0][i] == D_j0 * G[j][i]
    left = gf_mul(D[sel], G[j0, i])
    right = gf_mul(D[j0][None, :], G[sel, i][:, None])
    return bool((left == right).all())


def locate(rate, orig, rec, mask=None, D=None):
    """(located, flags [M] uint8) of one stripe under the contract."""
    N, M = orig.shape[0], rec.shape[0]
    mask = np.ones(M, bool) if mask is None else np.asarray(mask) != 0
    sel = np.flatnonzero(mask)
    assert len(sel) >= 2
    if D is None:
        D = syndromes(rate, orig, rec)
    differs = D.any(axis=1) & mask
    flags = differs.astype(np.uint8)
    n = int(differs.sum())
    if n == 0:
        return CLEAN, flags
    if n < len(sel):
        return ROWS, flags
    G = coefficients(rate, N, M)
    j0, j1 = sel[0], sel[1]
    col = int(np.flatnonzero(D[j0])[0])
    cand = np.flatnonzero((G[j0] != 0) & (gf_mul(G[j1], D[j0, col]) == gf_mul(G[j0], D[j1, col])))
    for i in cand:
        if explains(G, D, sel, int(i)):
            return int(i), flags
    return UNKNOWN, flags
