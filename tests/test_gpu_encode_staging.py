"""Staged single-chunk encodes of the column kernel (rs_mono.hip k_mono, encode entry):
every case is an encode through encode_device / encode_device_batch compared byte for
byte with the CPU oracle, and asserts from the profile records that k_mono ran it.

The encode entry takes its leading arguments preloaded in SGPRs (and, built with
RS_MONO_SPARE_BARRIERS=1, leaves out the barriers that open its two remaps and gives
the second remap a plane of its own), so the shapes are the smallest that reach each
branch of that code: 2^7 rows (one wave,
no shared region, no remap), 2^8 .. 2^10 rows (2, 4, 8 waves), zero-padded originals,
both pack formats, both rates, whole blocks, tail packs (byte-wise I/O), strided rows
and batches.  A read of LDS that ran ahead of the write it needs would see what the
previous launch left there -- often the same tables -- so the last tests alternate, in
one process and one stream, encodes whose tables differ, with a 2^11-row decode that
fills LDS with other contents in between, and check the first encode of a fresh process.
"""
import os
import subprocess
import sys

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
# are one chunk of 2^L rows
SHAPES = [(128, 128), (200, 256), (256, 256), (512, 512), (1024, 1024), (1000, 1024)]
SIZES = [64, 72, 1000, 1024]


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
        orig = O.generate_original(N, S, (N * 7 + M * 3 + S + seed) & 0xFF)
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
def test_staged_encode_matches_oracle(torch, rs, shape, rate, S, elems):
    N, M = _nm(rate, shape)
    orig, want = _case(rate, N, M, S)
    rs.mono_enable(FMT[elems])
    try:
        _equal(_encode(torch, rs, rate, N, M, S, _dev(torch, orig), elems, "encode"), want, "encode")
    finally:
        rs.mono_enable(1)


@pytest.mark.parametrize("elems", [2, 4])
@pytest.mark.parametrize("rate", ["high", "low"])
@pytest.mark.parametrize("shape,S", [((200, 256), 72), ((1000, 1024), 1000), ((1024, 1024), 64)],
                         ids=["200_256x72", "1000_1024x1000", "1024_1024x64"])
def test_staged_encode_strided_rows(torch, rs, shape, S, rate, elems):
    """Rows that are column slices of wider matrices: the bytes between the rows stay untouched."""
    N, M = _nm(rate, shape)
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
@pytest.mark.parametrize("shape,S", [((128, 128), 72), ((256, 256), 64), ((1000, 1024), 1024)],
                         ids=["128_128x72", "256_256x64", "1000_1024x1024"])
def test_staged_encode_batch_of_three(torch, rs, shape, S, rate, elems):
    N, M = _nm(rate, shape)
    cases = [_case(rate, N, M, S, seed) for seed in range(3)]
    rs.mono_enable(FMT[elems])
    try:
        b_o = _dev(torch, np.stack([c[0] for c in cases]))
        b_r = torch.full((3, M, S), 0xEE, dtype=torch.uint8, device="cuda")
        route = _route_of(torch, rs, lambda: rs.encode_device_batch(N, M, S, b_o, b_r, rate_=RATE[rate]))
        assert route == [_kernel(rate, N, M, elems, batch=True)], route
        got = b_r.cpu().numpy()
        for b in range(3):
            _equal(got[b], cases[b][1], "batch stripe %d" % b)
    finally:
        rs.mono_enable(1)


def _fill_lds_with_a_decode(torch, rs):
    """A 2^11-row decode (1024:1024, 100 originals lost): its tables and row info overwrite
    the LDS the encodes use."""
    N = M = 1024
    S = 64
    orig, rec = _case("high", N, M, S)
    lost = 100
    op = [0] * lost + [1] * (N - lost)
    rp = [1] * lost + [0] * (M - lost)
    d_out = torch.full((N, S), 0x33, dtype=torch.uint8, device="cuda")
    route = _route_of(torch, rs, lambda: rs.decode_device(N, M, S, _dev(torch, orig), op, _dev(torch, rec), rp, d_out))
    assert len(route) == 1 and route[0].startswith("k_mono<11, 1, 2, "), route
    _equal(d_out[:lost].cpu().numpy(), orig[:lost], "interleaved decode")


# pairs of encodes (rate, (N, M) of the HighRate form, elements per pack) whose tables differ
ALTERNATIONS = {
    "rates": (("high", (1024, 1024), 2), ("low", (1024, 1024), 2)),
    "rates_e4": (("high", (512, 512), 4), ("low", (512, 512), 4)),
    "sizes": (("high", (512, 512), 2), ("high", (1024, 1024), 2)),
    "sizes_one_wave": (("high", (128, 128), 2), ("high", (256, 256), 2)),
    "formats": (("high", (1024, 1024), 2), ("high", (1024, 1024), 4)),
    "formats_low": (("low", (256, 256), 4), ("low", (256, 256), 2)),
}


@pytest.mark.parametrize("decode_between", [False, True], ids=["back_to_back", "decode_between"])
@pytest.mark.parametrize("pair", sorted(ALTERNATIONS))
def test_alternating_encodes_do_not_see_stale_tables(torch, rs, pair, decode_between):
    S = 64
    try:
        for rnd in range(2):  # A, B, A, B
            for rate, shape, elems in ALTERNATIONS[pair]:
                N, M = _nm(rate, shape)
                orig, want = _case(rate, N, M, S)
                rs.mono_enable(FMT[elems])
                got = _encode(torch, rs, rate, N, M, S, _dev(torch, orig), elems, "round %d" % rnd)
                _equal(got, want, "%s round %d: %s %d:%d, %d-element packs" % (pair, rnd, rate, N, M, elems))
                if decode_between:
                    rs.mono_enable(1)
                    _fill_lds_with_a_decode(torch, rs)
    finally:
        rs.mono_enable(1)


_CHILD = r"""
import sys
sys.path[:0] = [%(pkg)r, %(tests)r]
import numpy as np
import torch
import oracle_lib as O
import reed_solomon_simd as rs

N = M = 1024
S = 1024
orig = O.generate_original(N, S, 5)
want = O.encode("high", orig, M)
d_o = torch.from_numpy(orig).cuda()
d_r = torch.full((M, S), 0xEE, dtype=torch.uint8, device="cuda")
rs.profile_enable(True)
rs.encode_device(N, M, S, d_o, d_r, rate_=1)  # the first launch of this process
torch.cuda.synchronize()
names = [n for n, _, _ in rs.profile_collect()]
assert names == ["k_mono<10, 1, 0, true, false, false, 2>"], names
assert np.array_equal(d_r.cpu().numpy(), want), "first encode of the process differs from the oracle"
print("first-encode ok")
"""


def test_first_encode_of_a_fresh_process(torch):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _CHILD % {"pkg": os.path.join(root, "reed-solomon-simd_amd"), "tests": os.path.join(root, "tests")}
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "first-encode ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
