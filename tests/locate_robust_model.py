"""A numpy model of rs_locate_device_robust's contract (include/rs_mi355x.h "robust locate"), on
the CPU oracle alone.  No tests here: tests/test_locate_robust_cpu.py and
tests/test_gpu_locate_robust.py import it.

With D_j and G as in tests/locate_model.py, c selected rows and t = max_outliers (2 (1 + t) <= c),
the result for a stripe is

    CLEAN / ROWS  as locate_model.locate: fewer than c selected rows differ; no outliers
    i, B          every selected row differs, and there are one e per column and a set B of at most
                  t selected rows with D_j = G[j][i] * e in every column for every selected j not in B
    UNKNOWN       every selected row differs and no such (i, e, B) exists; no outliers

Any e of an explanation is D_r / G[r][i] for each selected row r outside B (there are c - t >= 2 of
them), so trying every selected row as the reference finds every explanation.  Two forms:

    explanations / locate_direct  every i against every selected reference row
    locate                        the references are the first t + 1 selected rows (one of them is
                                  outside B); an i is tried in full only if its ratio G[j][i] /
                                  G[r][i] matches D_j / D_r, in the first column where D_r != 0, for
                                  t + 1 at least of the 2t + 1 other rows among the first 2t + 2 (of
                                  which at most t are in B)

Products are cross-multiplied (D_j * G[r][i] == D_r * G[j][i]) so that no division is needed; columns
in which no selected row differs hold e = 0 for every explanation and are left out.
"""
import numpy as np

import locate_model as LM

CLEAN, ROWS, UNKNOWN = LM.CLEAN, LM.ROWS, LM.UNKNOWN
MAX_OUTLIERS = 7


def _prepare(rate, orig, rec, t, mask, D):
    N, M = orig.shape[0], rec.shape[0]
    mask = np.ones(M, bool) if mask is None else np.asarray(mask) != 0
    sel = np.flatnonzero(mask)
    assert 0 <= t <= MAX_OUTLIERS and 2 * (1 + t) <= len(sel)
    if D is None:
        D = LM.syndromes(rate, orig, rec)
    differs = D.any(axis=1) & mask
    flags = differs.astype(np.uint8)
    n = int(differs.sum())
    status = None if n == len(sel) else (ROWS if n else CLEAN)
    return N, M, sel, D, flags, status


def _disagree(G, Dc, sel, r, cand):
    """[c, len(cand)] bool: selected row j disagrees with candidate original i in some column, e
    taken from reference row sel[r]."""
    Gs = G[np.ix_(sel, cand)]  # [c, k]
    left = LM.gf_mul(Dc[:, None, :], Gs[r][None, :, None])
    right = LM.gf_mul(Dc[r][None, None, :], Gs[:, :, None])
    return (left != right).any(axis=2)


def disagreements(G, D, sel):
    """Per selected reference row r, [c, N] bool: row j disagrees with original i, e from row r.
    (Independent of t: a test that tries several t forms it once.)"""
    Dc = D[sel][:, D[sel].any(axis=0)]
    every = np.arange(G.shape[1])
    return [_disagree(G, Dc, sel, r, every) for r in range(len(sel))]


def explanations(G, D, sel, t, bads=None):
    """Every distinct (i, B) with at most t selected rows B disagreeing, over every i and every
    selected reference row; B as a sorted tuple of row numbers."""
    found = set()
    for r, bad in enumerate(disagreements(G, D, sel) if bads is None else bads):
        for i in np.flatnonzero((bad.sum(axis=0) <= t) & (G[sel[r]] != 0)):
            found.add((int(i), tuple(int(j) for j in sel[bad[:, i]])))
    return found


def _answer(found, flags, M):
    outlier = np.zeros(M, np.uint8)
    if not found:
        return UNKNOWN, flags, outlier
    i, B = min(found)
    outlier[list(B)] = 1
    return i, flags, outlier


def locate_direct(rate, orig, rec, t, mask=None, D=None, bads=None):
    """(located, flags [M] uint8, outlier [M] uint8, explanations) of one stripe, the brute force.
    bads: disagreements() of the same stripe and mask, where the caller has them."""
    N, M, sel, D, flags, status = _prepare(rate, orig, rec, t, mask, D)
    if status is not None:
        return status, flags, np.zeros(M, np.uint8), set()
    found = explanations(LM.coefficients(rate, N, M), D, sel, t, bads)
    return _answer(found, flags, M) + (found,)


def locate(rate, orig, rec, t, mask=None, D=None):
    """(located, flags [M] uint8, outlier [M] uint8) of one stripe under the contract."""
    N, M, sel, D, flags, status = _prepare(rate, orig, rec, t, mask, D)
    if status is not None:
        return status, flags, np.zeros(M, np.uint8)
    G = LM.coefficients(rate, N, M)
    Dc = D[sel][:, D[sel].any(axis=0)]
    found = set()
    for r in range(t + 1):
        col = int(np.flatnonzero(Dc[r])[0])
        others = [j for j in range(2 * t + 2) if j != r]
        match = LM.gf_mul(G[sel[others]], Dc[r, col]) == LM.gf_mul(G[sel[r]][None, :], Dc[others, col][:, None])
        cand = np.flatnonzero((match.sum(axis=0) >= t + 1) & (G[sel[r]] != 0))
        if not len(cand):
            continue
        bad = _disagree(G, Dc, sel, r, cand)
        for k in np.flatnonzero(bad.sum(axis=0) <= t):
            found.add((int(cand[k]), tuple(int(j) for j in sel[bad[:, k]])))
    assert len(found) <= 1, found  # uniqueness (the header's fact 1)
    return _answer(found, flags, M)
