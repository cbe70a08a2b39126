"""The split form of the column kernel's dense encode entry (rs_mono.hip k_mono_split):
1024:1024 in 2-element column packs, one stripe, the two byte planes of a pair of rows on
neighbouring lanes.

Every case is 1024:1024, byte for byte against the CPU oracle and against the same call
with the split form switched off (rs_mono_enable + 65536: the dense entry as before).  The
profile records keep the route's name for both, so the split form is told by
rs_mono_split_launches: one launch more per split call (and one dense launch, as the tests
of the dense entry expect), none where the route must not be taken -- a 66-byte shard, a
base off by 2, a narrowed recovery span, 512:512, a batch, the dense entry switched off.

Shapes: shards of 64, 128, 192 and 1024 bytes (1, 2, 3 and 16 blocks: 16 to 256
workgroups), both rates; rows with a stride larger than S; outputs pre-filled with 0xEE;
the first encode of a fresh process; split encodes with a decode between them (stale LDS).
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
# rs_mono_enable: column kernel on, lane kernel off (+ 64), 2-element packs wherever the
# staged kernel runs (+ 16)
E2 = 1 | 16 | 64
DENSE_OFF = 16384
SPLIT_ON, SPLIT_OFF = 32768, 65536
N = 1024


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


def _case(rate, n, S, seed=0):
    """(originals, expected recovery rows) of a case, computed once and never written to."""
    key = (rate, n, S, seed)
    if key not in _ORACLE:
        orig = O.generate_original(n, S, (n * 7 + S + seed * 31 + len(rate)) & 0xFF)
        want = O.encode(rate, orig, n)
        orig.setflags(write=False)
        want.setflags(write=False)
        _ORACLE[key] = (orig, want)
    return _ORACLE[key]


def _kernel(rate, n=N, batch=False):
    return "k_mono<%d, 1, %d, true, %s, false, 2>" % (n.bit_length() - 1, MODE[rate], "true" if batch else "false")


def _dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared reference arrays are read-only)


def _run(torch, rs, fn):
    """(kernel names, split launches, dense launches) of one call."""
    rs.profile_enable(True)
    try:
        s0, d0 = rs.mono_split_launches(), rs.mono_dense_launches()
        fn()
        torch.cuda.synchronize()
        return [name for name, _, _ in rs.profile_collect()], rs.mono_split_launches() - s0, rs.mono_dense_launches() - d0
    finally:
        rs.profile_enable(False)


def _equal(got, want, what):
    got = np.asarray(got)
    diff = got != want
    if diff.any():
        rows = np.flatnonzero(diff.any(axis=-1).reshape(-1))
        raise AssertionError("%s: %d bytes differ in %d rows; rows %s" % (what, int(diff.sum()), rows.size,
                                                                         rows[:12].tolist()))


def _on_and_off(torch, rs, call, kernel, split_expected=1, dense_expected=1, extra=0):
    """Run `call` (which returns the output tensor) with the split form on and off."""
    outs = []
    try:
        for switch, split in ((SPLIT_ON, split_expected), (SPLIT_OFF, 0)):
            rs.mono_enable(E2 | switch | extra)
            box = []
            names, s, d = _run(torch, rs, lambda: box.append(call()))
            assert names == [kernel], (switch, names)
            assert s == split, "switch %d: %d split launches, expected %d" % (switch, s, split)
            assert d == dense_expected, "switch %d: %d dense launches, expected %d" % (switch, d, dense_expected)
            outs.append(box[0].cpu().numpy())
    finally:
        rs.mono_enable(1)
    return outs


@pytest.mark.parametrize("S", [64, 128, 192, 1024])
@pytest.mark.parametrize("rate", ["high", "low"])
def test_split_encode_matches_oracle_and_dense_entry(torch, rs, rate, S):
    orig, want = _case(rate, N, S)
    d_o = _dev(torch, orig)

    def call():
        d_r = torch.full((N, S), 0xEE, dtype=torch.uint8, device="cuda")
        rs.encode_device(N, N, S, d_o, d_r, rate_=RATE[rate])
        return d_r

    on, off = _on_and_off(torch, rs, call, _kernel(rate))
    _equal(on, want, "split form")
    _equal(off, want, "dense entry")
    assert on.tobytes() == off.tobytes()


@pytest.mark.parametrize("rate", ["high", "low"])
def test_split_encode_strided_rows(torch, rs, rate):
    """Rows that are column slices of wider matrices (strides S + 64 and S + 192, multiples of
    4): the bytes between the rows stay untouched."""
    S = 128
    orig, want = _case(rate, N, S)
    wo = torch.full((N, S + 64), 0x11, dtype=torch.uint8, device="cuda")
    wo[:, 32:32 + S] = _dev(torch, orig)

    def call():
        wr = torch.full((N, S + 192), 0xEE, dtype=torch.uint8, device="cuda")
        rs.encode_device(N, N, S, wo[:, 32:32 + S], wr[:, 64:64 + S], rate_=RATE[rate])
        return wr

    on, off = _on_and_off(torch, rs, call, _kernel(rate))
    _equal(on[:, 64:64 + S], want, "strided split encode")
    assert np.all(on[:, :64] == 0xEE) and np.all(on[:, 64 + S:] == 0xEE), "bytes between the rows were written"
    assert on.tobytes() == off.tobytes()


def test_split_decode_split_alternation(torch, rs):
    """Both rates' split encodes with a 2^11-row decode between them: the decode's tables and
    row info overwrite the LDS the encode stages into."""
    S = 64
    lost = 100
    orig_h, rec_h = _case("high", N, S)
    op = [0] * lost + [1] * (N - lost)
    rp = [1] * lost + [0] * (N - lost)
    try:
        for rnd in range(2):
            for rate in ("high", "low"):
                orig, want = _case(rate, N, S)
                rs.mono_enable(E2 | SPLIT_ON)
                d_r = torch.full((N, S), 0xEE, dtype=torch.uint8, device="cuda")
                names, s, _ = _run(torch, rs, lambda: rs.encode_device(N, N, S, _dev(torch, orig), d_r, rate_=RATE[rate]))
                assert names == [_kernel(rate)] and s == 1, (names, s)
                _equal(d_r.cpu().numpy(), want, "round %d %s rate" % (rnd, rate))
                rs.mono_enable(1)
                d_out = torch.full((N, S), 0x33, dtype=torch.uint8, device="cuda")
                names, s, _ = _run(torch, rs, lambda: rs.decode_device(N, N, S, _dev(torch, orig_h), op,
                                                                       _dev(torch, rec_h), rp, d_out))
                assert len(names) == 1 and names[0].startswith("k_mono<11, 1, 2, ") and s == 0, (names, s)
                _equal(d_out[:lost].cpu().numpy(), orig_h[:lost], "decode between the encodes")
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
S = 128
orig = O.generate_original(N, S, 9)
want = O.encode("low", orig, M)
d_o = torch.from_numpy(orig).cuda()
d_r = torch.full((M, S), 0xEE, dtype=torch.uint8, device="cuda")
rs.mono_enable(1 | 16 | 64 | 32768)
rs.profile_enable(True)
rs.encode_device(N, M, S, d_o, d_r, rate_=2)  # the first launch of this process
torch.cuda.synchronize()
names = [n for n, _, _ in rs.profile_collect()]
assert names == ["k_mono<10, 1, 1, true, false, false, 2>"], names
assert rs.mono_split_launches() == 1 and rs.mono_dense_launches() == 1
assert np.array_equal(d_r.cpu().numpy(), want), "first split encode of the process differs from the oracle"
print("first-split-encode ok")
"""


def test_first_split_encode_of_a_fresh_process(torch):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _CHILD % {"pkg": os.path.join(root, "reed-solomon-simd_amd"), "tests": os.path.join(root, "tests")}
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "first-split-encode ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])


# ---- where the route must not be taken -------------------------------------------------

def test_tail_shard_is_not_split(torch, rs):
    """66-byte shards: one whole block and a tail pack -- the general entry."""
    S, rate = 66, "high"
    orig, want = _case(rate, N, S)
    d_o = _dev(torch, orig)

    def call():
        d_r = torch.full((N, S), 0xEE, dtype=torch.uint8, device="cuda")
        rs.encode_device(N, N, S, d_o, d_r, rate_=RATE[rate])
        return d_r

    on, off = _on_and_off(torch, rs, call, _kernel(rate), split_expected=0, dense_expected=0)
    _equal(on, want, "66-byte shards")
    assert on.tobytes() == off.tobytes()


@pytest.mark.parametrize("which", ["original", "recovery"])
def test_base_off_by_two_is_not_split(torch, rs, which):
    S, rate = 64, "high"
    orig, want = _case(rate, N, S)
    flat_o = torch.zeros(N * S + 4, dtype=torch.uint8, device="cuda")
    o_off = 2 if which == "original" else 0
    r_off = 2 if which == "recovery" else 0
    d_o = flat_o[o_off:o_off + N * S].view(N, S)
    d_o.copy_(_dev(torch, orig))

    def call():
        flat_r = torch.full((N * S + 4,), 0xEE, dtype=torch.uint8, device="cuda")
        rs.encode_device(N, N, S, d_o, flat_r[r_off:r_off + N * S].view(N, S), rate_=RATE[rate])
        return flat_r

    on, off = _on_and_off(torch, rs, call, _kernel(rate), split_expected=0, dense_expected=0)
    _equal(on[r_off:r_off + N * S].reshape(N, S), want, "base off by 2")
    assert np.all(on[:r_off] == 0xEE) and np.all(on[r_off + N * S:] == 0xEE), "bytes around the matrix were written"
    assert on.tobytes() == off.tobytes()


@pytest.mark.parametrize("rate", ["high", "low"])
def test_narrowed_recovery_span_is_not_split(torch, rs, rate):
    """A repair that misses recovery rows [10, 40) re-encodes with the destination narrowed to
    that span: not every transform row is a row of the destination."""
    S, lo, hi = 64, 10, 40
    orig, want = _case(rate, N, S)
    d_o = _dev(torch, orig)
    held = np.array(want)
    held[lo:hi] = 0x55
    d_r = _dev(torch, held)
    op, rp = np.ones(N, np.uint8), np.ones(N, np.uint8)
    rp[lo:hi] = 0

    def call():
        d_x = torch.full((N, S), 0xEE, dtype=torch.uint8, device="cuda")
        d_y = torch.full((N, S), 0xEE, dtype=torch.uint8, device="cuda")
        rs.repair_device(N, N, S, d_o, op, d_r, rp, d_x, d_y, rate_=RATE[rate])
        return d_y

    on, off = _on_and_off(torch, rs, call, _kernel(rate), split_expected=0, dense_expected=0)
    _equal(on[lo:hi], want[lo:hi], "narrowed span")
    assert np.all(on[:lo] == 0xEE) and np.all(on[hi:] == 0xEE), "rows outside the span were written"
    assert on.tobytes() == off.tobytes()


def test_512_rows_are_not_split(torch, rs):
    n, S, rate = 512, 64, "high"
    orig, want = _case(rate, n, S)
    d_o = _dev(torch, orig)

    def call():
        d_r = torch.full((n, S), 0xEE, dtype=torch.uint8, device="cuda")
        rs.encode_device(n, n, S, d_o, d_r, rate_=RATE[rate])
        return d_r

    on, off = _on_and_off(torch, rs, call, _kernel(rate, n), split_expected=0)
    _equal(on, want, "512:512")
    assert on.tobytes() == off.tobytes()


def test_batch_is_not_split(torch, rs):
    S, rate = 64, "high"
    cases = [_case(rate, N, S, seed) for seed in range(2)]
    big_o = _dev(torch, np.stack([c[0] for c in cases]))

    def call():
        big_r = torch.full((2, N, S), 0xEE, dtype=torch.uint8, device="cuda")
        rs.encode_device_batch(N, N, S, big_o, big_r, rate_=RATE[rate])
        return big_r

    on, off = _on_and_off(torch, rs, call, _kernel(rate, batch=True), split_expected=0)
    for b in range(2):
        _equal(on[b], cases[b][1], "batch stripe %d" % b)
    assert on.tobytes() == off.tobytes()


def test_dense_off_is_not_split(torch, rs):
    """rs_mono_enable + 16384 sends the call to the general entry, split bit or not."""
    S, rate = 64, "low"
    orig, want = _case(rate, N, S)
    d_o = _dev(torch, orig)

    def call():
        d_r = torch.full((N, S), 0xEE, dtype=torch.uint8, device="cuda")
        rs.encode_device(N, N, S, d_o, d_r, rate_=RATE[rate])
        return d_r

    on, off = _on_and_off(torch, rs, call, _kernel(rate), split_expected=0, dense_expected=0, extra=DENSE_OFF)
    _equal(on, want, "dense entry off")
    assert on.tobytes() == off.tobytes()
