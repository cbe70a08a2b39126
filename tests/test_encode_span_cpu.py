"""CPU: tests/span_cases.py against itself and against the oracle alone -- the table that
tests/test_gpu_encode_span.py and the masks of the verify and locate tests are drawn from."""
import numpy as np
import pytest

import oracle_lib as O
import span_cases as SC

SHAPES = sorted({(c.rate, c.N, c.M) for c in SC.CASES}
                | {s[:3] for s in SC.BATCH + SC.MASK_SHAPES + SC.MASK_SHAPES_MODE0})
IDS = ["%s-%d-%d" % s for s in SHAPES]


def has(sp, lo, hi):
    return any((a, b) == (lo, hi) for _, a, b in sp)


@pytest.mark.parametrize("rate,N,M", SHAPES, ids=IDS)
def test_spans_are_valid_and_distinct(rate, N, M):
    sp = SC.spans(rate, N, M)
    for name, lo, hi in sp:
        assert 0 <= lo < hi <= M, (name, lo, hi)
    assert len({(lo, hi) for _, lo, hi in sp}) == len(sp), sp
    assert len({name for name, _, _ in sp}) == len(sp), sp


@pytest.mark.parametrize("rate,N,M", SHAPES, ids=IDS)
def test_every_span_class_is_present(rate, N, M):
    """Stated from N, M and the rate alone (n and C recomputed here, not taken from the table)."""
    high = rate == "high"
    n = 1
    while n < (M if high else N):
        n *= 2
    C = ((N if high else M) + n - 1) // n
    assert SC.geometry(rate, N, M) == (n, n.bit_length() - 1, C)
    sp = SC.spans(rate, N, M)
    assert has(sp, 0, 1) and has(sp, M - 1, M) and has(sp, 0, M) and has(sp, 1, M - 1)
    h = (M // 2) | 1
    assert h % 2 == 1 and (h + 3) % 2 == 0  # first row odd, last row (h + 2) odd
    assert has(sp, h, h + 3)
    assert n // 2 + 1 <= M and has(sp, n // 2 - 1, n // 2 + 1)
    assert 1 < M // 3 and M - M // 4 < M - 1 and has(sp, M // 3, M - M // 4)  # a long run, lo > 1, hi < M - 1
    L = n.bit_length() - 1
    if L > 8:  # two pass levels (up to 2^16 rows): the second starts at bit ceil(L / 2)
        assert len(SC.pass_levels(L)) == 2 and SC.pass_levels(L)[1][0] == (L + 1) // 2
        b = 1 << ((L + 1) // 2)
        assert has(sp, b - 1, b + 1)
    else:
        assert SC.pass_levels(L) == [(0, L)]
    if high:
        # input chunks: M <= n, every recovery row in the one FFT -- no chunk span, none empty
        assert M <= n and all(hi <= n for _, _, hi in sp)
        assert not any(name.startswith(("edge", "chunk", "inside", "two")) for name, _, _ in sp)
        return
    if C < 2:
        return
    last = (C - 1) * n
    assert has(sp, n - 1, n + 1) and has(sp, last - 1, last + 1)
    assert has(sp, last, M) and (M - last < n) == (M % n != 0)
    if C >= 3:
        c = C // 2
        assert 1 <= c < C - 1 and has(sp, c * n, (c + 1) * n)
    assert has(sp, n + 1, n + 3) and has(sp, last + 1, last + 3)
    if n + n // 2 <= M:
        assert has(sp, n // 2, n + n // 2)
    # a span entirely outside chunk 0, and where the last chunk is partial one that ends inside it
    assert any(lo >= n for _, lo, _ in sp)
    if M % n:
        assert any(last < hi < M for _, _, hi in sp)


def test_routes_cover_partial_last_chunks():
    """Every multi-chunk LowRate route has a shape whose last output chunk is partial (128:1024 has
    none to offer), and HighRate k_chunks a partial last input chunk."""
    partial = set()
    for c in SC.CASES:
        n, _, C = SC.geometry(c.rate, c.N, c.M)
        if c.rate == "low" and C >= 2 and c.M % n:
            partial.add(c.route)
    multi = {c.route for c in SC.CASES if c.rate == "low" and SC.geometry(c.rate, c.N, c.M)[2] >= 2}
    assert multi - partial <= {"chunks-e2", "chunks-e4"} and "chunks-partial" in partial, (multi, partial)
    assert any(c.route == "chunks-partial" and c.rate == "high" and c.N % SC.geometry("high", c.N, c.M)[0]
               for c in SC.CASES)


def test_case_table_is_consistent():
    ids = [SC.case_id(c) for c in SC.CASES]
    assert len(set(ids)) == len(ids), ids
    assert {c.family for c in SC.CASES} == {"pass", "chunks", "staged", "lane", "quad", "unstaged", "half"}
    assert {c.family for c in SC.CASES if c.probe} == {"pass", "chunks", "staged", "lane", "unstaged"}
    for c in SC.CASES:
        n, L, C = SC.geometry(c.rate, c.N, c.M)
        on, everywhere = (c.mode & 3) != 0, (c.mode & 3) == 2
        for S, pad in c.layouts or SC.LAYOUTS:
            packs = SC.packs_of(S)
            assert S % 2 == 0 and S <= 66 or c.route == "chunks-pw2" and S <= 4096
            want = SC.launches(c, S)
            # the host's conditions, restated (rs_codec.cpp use_mono / use_chunks / use_half / try_*)
            e2 = not (c.mode & 8) and packs <= 128
            mono = on and 7 <= L <= 12 and packs <= 256 and (everywhere or (C == 1 and L <= 11))
            chunks = (on and not everywhere and not c.env and C >= 2 and 2 <= L <= 7 and not mono
                      and packs <= (512 if c.rate == "high" else 256) and (c.rate == "high" or not e2 or C <= 8))
            half = on and not everywhere and bool(c.mode & 128) and L == 12 and C == 1 and not mono
            staged = mono and C == 1 and L <= 11
            quad = staged and e2 and bool(c.mode & 2048) and L == 10
            lane = staged and e2 and not quad and 8 <= L <= (10 if c.mode & 32 else 9)
            family = ("quad" if quad else "lane" if lane else "staged" if staged else "unstaged" if mono
                      else "chunks" if chunks else "half" if half else "pass")
            assert family == c.family, (SC.case_id(c), S, family)
            if family == "pass":
                levels = len(SC.pass_levels(L))
                grid = c.env.get("RS_MI355X_CHUNK_PARALLEL") != "0"  # (automatic: few packs, small scratch)
                if levels == 1:
                    assert want == ("k_pass<", 2 if C > 1 and grid and c.rate == "high" else 1), SC.case_id(c)
                else:
                    assert want == ("k_pass<", 2 * levels - 1), SC.case_id(c)
            if c.route == "chunks-pw2":
                assert packs > 256 and want[0].endswith(", 4, true, 2>")


def test_locate_bounds_hold_for_the_mask_shapes():
    for rate, N, M, S in SC.MASK_SHAPES + [s[:4] for s in SC.MASK_SHAPES_MODE0]:
        assert N <= 4096 and N * M <= 1 << 24, (rate, N, M)
        assert sum(int(SC.span_mask(M, lo, hi).sum()) >= 2 for _, lo, hi in SC.spans(rate, N, M)) >= 4


@pytest.mark.parametrize("rate,N,M", SHAPES, ids=IDS)
def test_span_masks_keep_their_ends(rate, N, M):
    for _, lo, hi in SC.spans(rate, N, M):
        mask = SC.span_mask(M, lo, hi)
        sel = np.flatnonzero(mask)
        assert sel[0] == lo and sel[-1] == hi - 1
        inside = mask[lo:hi]
        assert not inside[2:-1:3].any() and int(inside.sum()) == (hi - lo) - len(inside[2:-1:3])


@pytest.mark.parametrize("rate,N,M", SHAPES, ids=IDS)
def test_expected_rows_are_the_oracles(rate, N, M):
    """What the GPU tests expect in d_recovery_out is rows [lo, hi) of the oracle's encode and
    poison elsewhere; the oracle's rows are pairwise different and differ from the poison and the
    junk, so a row stored one place off, not stored, or copied from d_recovery cannot pass."""
    S = 64
    orig, rec = SC.stripe(rate, N, M, S)
    assert np.array_equal(orig, O.generate_original(N, S, 0)) and np.array_equal(rec, O.encode(rate, orig, M))
    assert len(np.unique(rec, axis=0)) == M
    assert not (rec == SC.POISON).all(axis=1).any() and not (rec == SC.JUNK_R).all(axis=1).any()
    for name, lo, hi in SC.spans(rate, N, M):
        want = SC.expected_out(rec, lo, hi)
        assert np.array_equal(want[lo:hi], rec[lo:hi]), name
        assert (want[:lo] == SC.POISON).all() and (want[hi:] == SC.POISON).all()
        held = SC.held_recovery(rec, lo, hi)
        assert (held[lo:hi] == SC.JUNK_R).all() and np.array_equal(held[:lo], rec[:lo]) and np.array_equal(held[hi:], rec[hi:])
