"""Staged single-chunk encodes of 2^11 rows through the column kernel's encode entry
(rs_mono.hip k_mono), whose tables go into LDS by LDS-DMA (RS_MONO_LDS_DMA): layer 0 of
both in-wave phases takes turns with the layers above in the wave regions, 16 waves share
the largest LDS footprint, and the DMAs of phase 3 stay in flight across a remap and the
top phases.  tests/test_gpu_encode_staging.py covers 2^7 .. 2^10 rows; this file the
2^11-row plans it does not reach.

Every case is byte for byte against the CPU oracle and asserts from the profile records
that k_mono<11, ...> ran it: both rates, both pack formats, whole blocks (64 B) and a
tail pack with byte-wise I/O (72 B), zero-padded originals (1500 of 2048 rows), strided
rows, a batch of three stripes with padding between the stripes, and an alternation on
one stream between 2^11- and 2^10-row encodes with different originals -- a table read
that ran ahead of its DMA would see what the previous launch left in LDS.
"""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

RATE = {"high": 1, "low": 2}
MODE = {"high": 0, "low": 1}
# rs_mono_enable: column kernel on, lane kernel off (+ 64), 4-element packs only (+ 8) /
# 2-element packs wherever the staged kernel runs (+ 16)
FMT = {4: 1 | 8 | 64, 2: 1 | 16 | 64}

# (N originals, M recovery) of the HighRate case; the LowRate case swaps them, so both
# are one chunk of 2^11 rows
SHAPES = [(2048, 2048), (1500, 2048)]
SIZES = [64, 72]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def rs(torch):
    import reed_solomon_simd
    return reed_solomon_simd


_ORACLE = {}


def _case(rate, N, M, S, seed=0):
    """(originals, expected recovery rows) of a case, computed once and never written to."""
    key = (rate, N, M, S, seed)
    if key not in _ORACLE:
        orig = O.generate_original(N, S, (N * 7 + M * 3 + S + seed * 31) & 0xFF)
        want = O.encode(rate, orig, M)
        orig.setflags(write=False)
        want.setflags(write=False)
        _ORACLE[key] = (orig, want)
    return _ORACLE[key]


def _nm(rate, shape):
    return shape if rate == "high" else (shape[1], shape[0])


def _log2_rows(rate, N, M):
    return (max(M if rate == "high" else N, 1) - 1).bit_length()


def _kernel(rate, N, M, elems, batch=False):
    return "k_mono<%d, 1, %d, true, %s, false, %d>" % (_log2_rows(rate, N, M), MODE[rate],
                                                       "true" if batch else "false", elems)


def _dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared reference arrays are read-only)


def _route_of(torch, rs, fn):
    rs.profile_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        return [name for name, _, _ in rs.profile_collect()]
    finally:
        rs.profile_enable(False)


def _equal(got, want, what):
    got = np.asarray(got)
    diff = got != want
    if diff.any():
        rows = np.flatnonzero(diff.any(axis=1))
        cols = np.flatnonzero(diff.any(axis=0))
        raise AssertionError("%s: %d bytes differ in %d of %d rows; rows %s, byte columns %s" % (
            what, int(diff.sum()), rows.size, diff.shape[0], rows[:12].tolist(), cols[:12].tolist()))


def _encode(torch, rs, rate, N, M, S, d_o, elems, what):
    d_r = torch.full((M, S), 0xEE, dtype=torch.uint8, device="cuda")
    route = _route_of(torch, rs, lambda: rs.encode_device(N, M, S, d_o, d_r, rate_=RATE[rate]))
    assert route == [_kernel(rate, N, M, elems)], (what, route)
    return d_r.cpu().numpy()


@pytest.mark.parametrize("elems", [2, 4])
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("rate", ["high", "low"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d_%d" % s)
def test_encode_2048_rows_matches_oracle(torch, rs, shape, rate, S, elems):
    N, M = _nm(rate, shape)
    assert _log2_rows(rate, N, M) == 11
    orig, want = _case(rate, N, M, S)
    rs.mono_enable(FMT[elems])
    try:
        _equal(_encode(torch, rs, rate, N, M, S, _dev(torch, orig), elems, "encode"), want, "encode")
    finally:
        rs.mono_enable(1)


@pytest.mark.parametrize("elems", [2, 4])
def test_encode_2048_rows_strided(torch, rs, elems):
    """Rows that are column slices of wider matrices: the bytes between the rows stay untouched."""
    rate, S = "high", 72
    N, M = _nm(rate, (1500, 2048))
    orig, want = _case(rate, N, M, S)
    rs.mono_enable(FMT[elems])
    try:
        wo = torch.full((N, S + 64), 0x11, dtype=torch.uint8, device="cuda")
        wr = torch.full((M, S + 64), 0x22, dtype=torch.uint8, device="cuda")
        wo[:, 32:32 + S] = _dev(torch, orig)
        route = _route_of(torch, rs, lambda: rs.encode_device(N, M, S, wo[:, 32:32 + S], wr[:, 32:32 + S],
                                                              rate_=RATE[rate]))
        assert route == [_kernel(rate, N, M, elems)], route
        got = wr.cpu().numpy()
        _equal(got[:, 32:32 + S], want, "strided encode")
        assert np.all(got[:, :32] == 0x22) and np.all(got[:, 32 + S:] == 0x22), "bytes between the rows were written"
    finally:
        rs.mono_enable(1)


@pytest.mark.parametrize("elems", [2, 4])
@pytest.mark.parametrize("rate", ["high", "low"])
def test_encode_2048_rows_batch_of_three_with_stripe_padding(torch, rs, rate, elems):
    """Three stripes in one launch; each stripe's matrices are followed by rows that belong
    to no stripe, which the launch must leave alone."""
    S, PAD = 64, 3
    N, M = _nm(rate, (2048, 2048))
    cases = [_case(rate, N, M, S, seed) for seed in range(3)]
    rs.mono_enable(FMT[elems])
    try:
        big_o = torch.full((3, N + PAD, S), 0x11, dtype=torch.uint8, device="cuda")
        big_r = torch.full((3, M + PAD, S), 0xEE, dtype=torch.uint8, device="cuda")
        big_o[:, :N] = _dev(torch, np.stack([c[0] for c in cases]))
        route = _route_of(torch, rs, lambda: rs.encode_device_batch(N, M, S, big_o[:, :N], big_r[:, :M],
                                                                    rate_=RATE[rate]))
        assert route == [_kernel(rate, N, M, elems, batch=True)], route
        got = big_r.cpu().numpy()
        for b in range(3):
            _equal(got[b, :M], cases[b][1], "batch stripe %d" % b)
        assert np.all(got[:, M:] == 0xEE), "rows between the stripes were written"
    finally:
        rs.mono_enable(1)


@pytest.mark.parametrize("elems", [2, 4])
def test_alternating_2048_and_1024_rows_do_not_see_stale_tables(torch, rs, elems):
    """2048:2048 -> 1024:1024 -> 2048:2048 on one stream, different originals each time,
    outputs pre-filled with 0xEE: the 2^10-row launch leaves other tables where the
    2^11-row launch's regions lie, and the other way round."""
    S = 64
    steps = [("high", (2048, 2048), 1), ("high", (1024, 1024), 2), ("high", (2048, 2048), 3)]
    rs.mono_enable(FMT[elems])
    try:
        for i, (rate, shape, seed) in enumerate(steps):
            N, M = _nm(rate, shape)
            orig, want = _case(rate, N, M, S, seed)
            got = _encode(torch, rs, rate, N, M, S, _dev(torch, orig), elems, "step %d" % i)
            _equal(got, want, "step %d: %s %d:%d, %d-element packs" % (i, rate, N, M, elems))
    finally:
        rs.mono_enable(1)
