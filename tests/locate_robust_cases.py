"""The constructed stripes of the robust locate's tests (tests/test_locate_robust_cpu.py and
tests/test_gpu_locate_robust.py): the oracle's clean stripe with chosen bytes flipped, and what each
case is built to show.  No tests here.

A case is (name, t, originals, recovery, encode of the originals, intended), intended = (located,
[outlier rows]) or None where the shape is too small for the case to mean one thing (the model
decides).  sel = the selected rows, c their number; pair p = (sel[2p], sel[2p + 1]).
"""
import numpy as np

import locate_model as LM
import locate_robust_model as RM
import oracle_lib as O
import test_gpu_verify as V
import wide_cases as W
from test_gpu_locate import damage_original

CLEAN, ROWS, UNKNOWN = LM.CLEAN, LM.ROWS, LM.UNKNOWN
_ENC = {}


def t_max(c):
    """The largest max_outliers a call with c selected rows takes."""
    return min(RM.MAX_OUTLIERS, c // 2 - 1)


def encoded(key, orig, rate, M):
    """The oracle's encode of a damaged copy of the originals, computed once per key."""
    if key not in _ENC:
        enc = O.encode(rate, orig, M)
        enc.setflags(write=False)
        _ENC[key] = enc
    return _ENC[key]


def hit(rec, j, kind, form):
    """Damage recovery row j in place.  plain: one bit somewhere; lasthigh: the tail's last high
    byte; ezero: a byte of a column in which an original damaged by `form` has e = 0."""
    S = rec.shape[1]
    if kind == "plain":
        rec[j, (5 + 3 * j) % S] ^= 0x10
    elif kind == "lasthigh":
        rec[j, S - 1] ^= 0x20  # (not the bit of damage_original's lastbit: at 1:4 the two would cancel)
    else:
        assert kind == "ezero" and S > 2
        rec[j, S - 1 if form == "bit0" else 0] ^= 0x40


def wide_cases(rate, N, M, S):
    """The positional cases of a wide shard (tests/wide_cases.py), at t = 1 and 2, every row
    selected: clean; original N // 2 corrupt as a whole shard with t outlier rows whose only damage is
    in the last pack; original 0 corrupt in pack 0 alone with an outlier row damaged in the last pack,
    a column where e = 0; the whole shard again with t + 1 outliers, one in each of the first t + 1
    pairs, damaged in the last pack: UNKNOWN."""
    orig, rec = V.stripe(rate, N, M, S)
    packs = W.packs_of(S)
    rng = np.random.default_rng(N * 7 + M + S)
    out = [("none", 1, orig, rec, encoded((rate, N, M, S, "clean"), orig, rate, M), (CLEAN, []))]
    shard = orig.copy()
    shard[N // 2] ^= rng.integers(1, 256, S, dtype=np.uint8)
    shard_enc = encoded((rate, N, M, S, "wide shard"), shard, rate, M)
    narrow = orig.copy()
    W.damage_pack(narrow, 0, 0, rng)
    narrow_enc = encoded((rate, N, M, S, "wide pack 0"), narrow, rate, M)
    assert M >= 2 * 2 + 3

    def hit_rows(rows):
        r = rec.copy()
        for j in rows:
            W.damage_pack(r, j, packs - 1, rng)
        return r

    for t in (1, 2):
        rows = [0, M - 1][:t] if t == 1 else [1, M // 2]
        out.append((f"original {N // 2} shard, outliers {rows} pack {packs - 1} t={t}", t, shard, hit_rows(rows),
                    shard_enc, (N // 2, rows)))
        rows = [M // 2] if t == 1 else [0, M - 1]
        out.append((f"original 0 pack 0, ezero outliers {rows} pack {packs - 1} t={t}", t, narrow, hit_rows(rows),
                    narrow_enc, (0, rows)))
        rows = [2 * p + (p & 1) for p in range(t + 1)]
        out.append((f"original {N // 2} shard, {t + 1} outliers pack {packs - 1} t={t}", t, shard, hit_rows(rows),
                    shard_enc, (UNKNOWN, [])))
    return out


def cases(rate, N, M, S, mask=None, forms=("bit0", "lastbit"), ts=None, junk=False, wide=False):
    """Every case of the issue that the shape has rows for.  ts: the values of t the outlier cases
    run at (default 1, 2 and the largest allowed); junk: 0xC3 in the unselected rows; wide:
    wide_cases' instead."""
    if wide:
        assert mask is None
        return wide_cases(rate, N, M, S)
    orig, rec = V.stripe(rate, N, M, S)
    sel = np.arange(M) if mask is None else np.flatnonzero(np.asarray(mask) != 0)
    c, top = len(sel), t_max(len(sel))
    assert top >= 0
    if junk:
        rec = rec.copy()
        rec[np.setdiff1d(np.arange(M), sel)] = 0xC3
    want_t = lambda t: t <= top and (ts is None or t in ts)
    rng = np.random.default_rng(N * 7 + M + S)
    clean_enc = encoded((rate, N, M, S, "clean"), orig, rate, M)
    t0 = min(1, top)
    out = [("none", t0, orig, rec, clean_enc, (CLEAN, []))]

    def add(name, t, bad, enc, rows, kinds, form, intended="located", i=None):
        r = rec.copy()
        for j, kind in zip(rows, kinds):
            hit(r, int(j), kind, form)
        if intended == "located":
            intended = (i, sorted(int(j) for j in rows))
        out.append((f"{name} t={t}", t, bad, r, enc, intended))

    for i in sorted({0, N // 2, N - 1}):
        for form in forms:
            bad = orig.copy()
            damage_original(bad, i, form, rng)
            enc = encoded((rate, N, M, S, i, form), bad, rate, M)
            tag = f"original {i} {form}"
            for t in sorted({0, t0}):
                out.append((f"{tag} alone t={t}", t, bad, rec, enc, (i, [])))
            if want_t(1) and top >= 1:
                mid = sel[c // 2]
                for name, rows, kinds in (("outlier sel[0]", [sel[0]], ["plain"]), ("outlier sel[1]", [sel[1]], ["plain"]),
                                          ("outlier last", [sel[-1]], ["plain"]), ("outlier middle lasthigh", [mid], ["lasthigh"])):
                    add(f"{tag} {name}", 1, bad, enc, rows, kinds, form, i=i)
                if S > 2:
                    add(f"{tag} ezero sel[0]", 1, bad, enc, [sel[0]], ["ezero"], form, i=i)
                    add(f"{tag} ezero middle", 1, bad, enc, [mid], ["ezero"], form, i=i)
            if want_t(2) and top >= 2:
                for rows in ([sel[0], sel[2]], [sel[1], sel[3]], [sel[2], sel[3]]):
                    add(f"{tag} outliers {[int(j) for j in rows]}", 2, bad, enc, rows, ["plain"] * 2, form, i=i)
            # t + 1 outliers, one in each of the first t + 1 pairs: no pair is clean.  UNKNOWN is
            # certain from c >= 2t + 3 (two explanations within t + 2 and t + 1 of the stored word)
            for t in (1, 2):
                if want_t(t) and top >= t:
                    rows = [sel[2 * p + (p & 1)] for p in range(t + 1)]
                    add(f"{tag} {t + 1} outliers", t, bad, enc, rows, ["plain"] * (t + 1), form,
                        intended=(UNKNOWN, []) if c >= 2 * t + 3 else None)
            # the largest t, with exactly t outliers at the first row of the first t pairs
            if top >= 1 and (ts is None or top in ts):
                rows = [sel[2 * p] for p in range(top)]
                add(f"{tag} {top} outliers at pair heads", top, bad, enc, rows, ["plain"] * top, form, i=i)
    form = forms[0]
    if N >= 2:
        # two corrupt originals, in two columns and in one: UNKNOWN at t = 1 and at the largest t
        # that leaves two rows beyond the damage (c - 1 - t >= 2) -- unless some row matches by
        # coincidence, which is ROWS (tests/test_locate_cpu.py pins such a stripe)
        for name, second in (("two columns", (N - 1, S - 1, 0x20)), ("one column", (N // 2 if N > 2 else N - 1, 0, 0x33))):
            bad = orig.copy()
            bad[0, 0] ^= 0x10
            bad[second[0], second[1]] ^= second[2]
            enc = encoded((rate, N, M, S, "two", name), bad, rate, M)
            every = bool((enc[sel] != rec[sel]).any(axis=1).all())
            for t in sorted({t for t in (1, min(top, c - 3)) if 1 <= t <= top}):
                out.append((f"two originals, {name} t={t}", t, bad, rec, enc, (UNKNOWN if every else ROWS, [])))
    if top >= 1:
        r = rec.copy()  # every selected recovery row
        for j in sel:
            r[j, (int(j) * 7) % S] ^= 1 << (int(j) % 8)
        out.append(("every recovery row t=1", 1, orig, r, clean_enc, (UNKNOWN, []) if c >= 5 else None))
    r = rec.copy()  # recovery rows alone
    r[sel[0], 0] ^= 0x01
    r[sel[-1], S - 1] ^= 0x80
    out.append((f"recovery rows only t={t0}", t0, orig, r, clean_enc, (ROWS, [])))
    return out


def model(rate, case, mask=None):
    """(located, flags, outlier) of a case by the fast model, the intended status asserted first;
    the flags are also checked to be "the oracle's encode differs from the stored row"."""
    name, t, orig, rec, enc, intended = case
    M = rec.shape[0]
    sel = np.ones(M, bool) if mask is None else np.asarray(mask) != 0
    truth = ((enc != rec).any(axis=1) & sel).astype(np.uint8)
    got = RM.locate(rate, orig, rec, t, mask=mask, D=LM.elements(enc ^ rec).astype(np.int64))
    assert np.array_equal(got[1], truth), name
    if intended is not None:
        assert (got[0], np.flatnonzero(got[2]).tolist()) == (intended[0], intended[1]), \
            f"{name}: the model says {got[0]} with outliers {np.flatnonzero(got[2]).tolist()}, built for {intended}"
    return got
