"""The column kernel's dense encode entry (rs_mono.hip k_mono_dense): single-chunk encodes of
N = M = 2^L shards of whole 64-byte blocks, 4-byte aligned, where the host has decided that
every transform row is a row of both matrices (csrc/rs_mono_dense.hpp) and the kernel
addresses rows without range tests, stand-in rows, byte paths or 64-bit lane arithmetic.

Every case is byte for byte against the CPU oracle and against the same call through the
general entry (rs_mono_enable + 16384).  The profile records name the route k_mono<...> for
both entries, so the dense one is told by rs_mono_dense_launches: one launch more after a
dense call, none after a call through the general entry or after one that must fall back
(a 66-byte shard, a base off by 2, a narrowed recovery span).

Shapes: every L in 7..11, both rates, both pack formats, S = 64 and 128; at 1024:1024 also
512 bytes (2-element packs by default) and 1088 bytes (136 packs, past the 128-pack bound
of the 2-element format: 4-element packs by default); rows with a stride larger than S; a
batch of three stripes with rows between the stripes.
"""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

RATE = {"high": 1, "low": 2}
MODE = {"high": 0, "low": 1}
# rs_mono_enable: column kernel on, lane kernel off (+ 64), 4-element packs only (+ 8) /
# 2-element packs wherever the staged kernel runs (+ 16); None: the default format
FMT = {4: 1 | 8 | 64, 2: 1 | 16 | 64, None: 1 | 64}
DENSE_ON, DENSE_OFF = 8192, 16384


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
        orig = O.generate_original(N, S, (N * 5 + M * 3 + S + seed * 29) & 0xFF)
        want = O.encode(rate, orig, M)
        orig.setflags(write=False)
        want.setflags(write=False)
        _ORACLE[key] = (orig, want)
    return _ORACLE[key]


def _kernel(rate, n, elems, batch=False):
    return "k_mono<%d, 1, %d, true, %s, false, %d>" % (n.bit_length() - 1, MODE[rate], "true" if batch else "false", elems)


def _dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared reference arrays are read-only)


def _run(torch, rs, fn):
    """(kernel names, dense launches) of one call."""
    rs.profile_enable(True)
    try:
        before = rs.mono_dense_launches()
        fn()
        torch.cuda.synchronize()
        return [name for name, _, _ in rs.profile_collect()], rs.mono_dense_launches() - before
    finally:
        rs.profile_enable(False)


def _equal(got, want, what):
    got = np.asarray(got)
    diff = got != want
    if diff.any():
        rows = np.flatnonzero(diff.any(axis=-1).reshape(-1))
        raise AssertionError("%s: %d bytes differ in %d rows; rows %s" % (what, int(diff.sum()), rows.size,
                                                                         rows[:12].tolist()))


def _both_entries(torch, rs, fmt, call, kernel, dense_expected=1):
    """Run `call` (which returns the output tensor) through the dense and the general entry."""
    outs = []
    try:
        for switch, dense in ((DENSE_ON, dense_expected), (DENSE_OFF, 0)):
            rs.mono_enable(FMT[fmt] | switch)
            box = []
            names, launches = _run(torch, rs, lambda: box.append(call()))
            assert names == [kernel], (switch, names)
            assert launches == dense, "switch %d: %d dense launches, expected %d" % (switch, launches, dense)
            outs.append(box[0].cpu().numpy())
    finally:
        rs.mono_enable(1)
    return outs


@pytest.mark.parametrize("elems", [2, 4])
@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("rate", ["high", "low"])
@pytest.mark.parametrize("n", [128, 256, 512, 1024, 2048])
def test_dense_encode_matches_oracle_and_general_entry(torch, rs, n, rate, S, elems):
    orig, want = _case(rate, n, n, S)
    d_o = _dev(torch, orig)

    def call():
        d_r = torch.full((n, S), 0xEE, dtype=torch.uint8, device="cuda")
        rs.encode_device(n, n, S, d_o, d_r, rate_=RATE[rate])
        return d_r

    on, off = _both_entries(torch, rs, elems, call, _kernel(rate, n, elems))
    _equal(on, want, "dense entry")
    _equal(off, want, "general entry")
    assert on.tobytes() == off.tobytes()


@pytest.mark.parametrize("rate", ["high", "low"])
@pytest.mark.parametrize("S,elems", [(512, 2), (1088, 4)], ids=["512_e2", "1088_e4"])
def test_dense_encode_1024_default_pack_format(torch, rs, S, elems, rate):
    """The context's own choice of pack format: 2-element packs up to 128 packs of 4 elements
    (S = 1024), 4-element packs past that."""
    n = 1024
    orig, want = _case(rate, n, n, S)
    d_o = _dev(torch, orig)

    def call():
        d_r = torch.full((n, S), 0xEE, dtype=torch.uint8, device="cuda")
        rs.encode_device(n, n, S, d_o, d_r, rate_=RATE[rate])
        return d_r

    on, off = _both_entries(torch, rs, None, call, _kernel(rate, n, elems))
    _equal(on, want, "dense entry")
    assert on.tobytes() == off.tobytes()


@pytest.mark.parametrize("elems", [2, 4])
@pytest.mark.parametrize("rate,n", [("high", 1024), ("low", 256)])
def test_dense_encode_strided_rows(torch, rs, rate, n, elems):
    """Rows that are column slices of wider matrices: the bytes between the rows stay untouched."""
    S = 64
    orig, want = _case(rate, n, n, S)
    wo = torch.full((n, S + 64), 0x11, dtype=torch.uint8, device="cuda")
    wo[:, 32:32 + S] = _dev(torch, orig)

    def call():
        wr = torch.full((n, S + 192), 0x22, dtype=torch.uint8, device="cuda")
        rs.encode_device(n, n, S, wo[:, 32:32 + S], wr[:, 64:64 + S], rate_=RATE[rate])
        return wr

    on, off = _both_entries(torch, rs, elems, call, _kernel(rate, n, elems))
    _equal(on[:, 64:64 + S], want, "strided dense encode")
    assert np.all(on[:, :64] == 0x22) and np.all(on[:, 64 + S:] == 0x22), "bytes between the rows were written"
    assert on.tobytes() == off.tobytes()


@pytest.mark.parametrize("elems", [2, 4])
@pytest.mark.parametrize("rate,n,S", [("high", 256, 64), ("low", 128, 128), ("high", 1024, 64)])
def test_dense_encode_batch_of_three_with_stripe_padding(torch, rs, rate, n, S, elems):
    """Three stripes in one launch; rows between the stripes belong to no stripe and stay untouched."""
    PAD = 3
    cases = [_case(rate, n, n, S, seed) for seed in range(3)]
    big_o = torch.full((3, n + PAD, S), 0x11, dtype=torch.uint8, device="cuda")
    big_o[:, :n] = _dev(torch, np.stack([c[0] for c in cases]))

    def call():
        big_r = torch.full((3, n + PAD, S), 0xEE, dtype=torch.uint8, device="cuda")
        rs.encode_device_batch(n, n, S, big_o[:, :n], big_r[:, :n], rate_=RATE[rate])
        return big_r

    on, off = _both_entries(torch, rs, elems, call, _kernel(rate, n, elems, batch=True))
    for b in range(3):
        _equal(on[b, :n], cases[b][1], "batch stripe %d" % b)
    assert np.all(on[:, n:] == 0xEE), "rows between the stripes were written"
    assert on.tobytes() == off.tobytes()


@pytest.mark.parametrize("elems", [2, 4])
def test_tail_shard_falls_back(torch, rs, elems):
    """66-byte shards: one whole block and a tail pack -- the general entry, switch on or off."""
    n, S, rate = 256, 66, "high"
    orig, want = _case(rate, n, n, S)
    d_o = _dev(torch, orig)

    def call():
        d_r = torch.full((n, S), 0xEE, dtype=torch.uint8, device="cuda")
        rs.encode_device(n, n, S, d_o, d_r, rate_=RATE[rate])
        return d_r

    on, off = _both_entries(torch, rs, elems, call, _kernel(rate, n, elems), dense_expected=0)
    _equal(on, want, "66-byte shards")
    assert on.tobytes() == off.tobytes()


@pytest.mark.parametrize("elems", [2, 4])
@pytest.mark.parametrize("which", ["original", "recovery"])
def test_base_off_by_two_falls_back(torch, rs, which, elems):
    n, S, rate = 256, 64, "high"
    orig, want = _case(rate, n, n, S)
    flat_o = torch.zeros(n * S + 4, dtype=torch.uint8, device="cuda")
    o_off = 2 if which == "original" else 0
    r_off = 2 if which == "recovery" else 0
    d_o = flat_o[o_off:o_off + n * S].view(n, S)
    d_o.copy_(_dev(torch, orig))

    def call():
        flat_r = torch.full((n * S + 4,), 0xEE, dtype=torch.uint8, device="cuda")
        rs.encode_device(n, n, S, d_o, flat_r[r_off:r_off + n * S].view(n, S), rate_=RATE[rate])
        return flat_r

    on, off = _both_entries(torch, rs, elems, call, _kernel(rate, n, elems), dense_expected=0)
    _equal(on[r_off:r_off + n * S].reshape(n, S), want, "base off by 2")
    assert np.all(on[:r_off] == 0xEE) and np.all(on[r_off + n * S:] == 0xEE), "bytes around the matrix were written"
    assert on.tobytes() == off.tobytes()


@pytest.mark.parametrize("elems", [2, 4])
@pytest.mark.parametrize("rate", ["high", "low"])
def test_narrowed_recovery_span_falls_back(torch, rs, rate, elems):
    """A repair that misses recovery rows [10, 40) only re-encodes with the destination narrowed
    to that span: not every transform row is a row of the destination."""
    n, S, lo, hi = 256, 64, 10, 40
    orig, want = _case(rate, n, n, S)
    d_o = _dev(torch, orig)
    held = np.array(want)
    held[lo:hi] = 0x55
    d_r = _dev(torch, held)
    op, rp = np.ones(n, np.uint8), np.ones(n, np.uint8)
    rp[lo:hi] = 0

    def call():
        d_x = torch.full((n, S), 0xEE, dtype=torch.uint8, device="cuda")
        d_y = torch.full((n, S), 0xEE, dtype=torch.uint8, device="cuda")
        rs.repair_device(n, n, S, d_o, op, d_r, rp, d_x, d_y, rate_=RATE[rate])
        return d_y

    on, off = _both_entries(torch, rs, elems, call, _kernel(rate, n, elems), dense_expected=0)
    _equal(on[lo:hi], want[lo:hi], "narrowed span")
    assert np.all(on[:lo] == 0xEE) and np.all(on[hi:] == 0xEE), "rows outside the span were written"
    assert on.tobytes() == off.tobytes()
