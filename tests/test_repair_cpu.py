"""rs_repair_device* without a GPU: the symbols and their declarations, the argument and
pattern checks (all of which come before any device work), the Python wrappers' argument
checks, the INTEGRATION.md binding, and a pure-CPU statement of the identity the kernels rely
on: after the decode's last FFT the reveal multiply of an erased RECOVERY row gives the
encoder's recovery shard."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import oracle_lib as O
import test_integration_abi as ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rs_repair_device", "rs_repair_device_strided", "rs_repair_device_batch")


@pytest.fixture(scope="module")
def rs():
    # (imported by the tests that use it, not while pytest collects: tests/test_batch_masks_cpu.py)
    import reed_solomon_simd
    return reed_solomon_simd


def _plain(rs, ctx, N, M, S, d_o, op, d_r, rp, d_x, d_y, err=None):
    return rs._lib.rs_repair_device(ctx, 0, N, M, S, d_o, op, d_r, rp, d_x, d_y, None, err)


def _strided(rs, ctx, N, M, S, d_o, op, d_r, rp, d_x, d_y, err=None, strides=(0, 0, 0, 0)):
    return rs._lib.rs_repair_device_strided(ctx, 0, N, M, S, d_o, strides[0], op, d_r, strides[1], rp, d_x,
                                            strides[2], d_y, strides[3], None, err)


def _batch(rs, ctx, N, M, S, d_o, op, d_r, rp, d_x, d_y, err=None, strides=(0, 0, 0, 0), stripes=2):
    return rs._lib.rs_repair_device_batch(ctx, 0, N, M, S, stripes, d_o, strides[0], 0, op, d_r, strides[1], 0, rp,
                                          d_x, strides[2], 0, d_y, strides[3], 0, None, err)


FORMS = [_plain, _strided, _batch]


def test_symbols_are_exported_and_declared(rs):
    header = open(os.path.join(ROOT, "include", "rs_mi355x.h")).read()
    for name in NAMES:
        assert hasattr(rs._lib, name), name
        assert getattr(rs._lib, name).argtypes is not None, name  # the ctypes signature is declared
        m = re.search(r"rs_status\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, name
        assert "void *d_recovery_out" in m.group(1), name
        # between d_restored... and stream
        assert re.search(r"d_restored.*d_recovery_out.*void \*stream", m.group(1), re.S), name
    for name in NAMES[1:]:
        assert "recovery_out_stride" in re.search(r"%s\s*\(([^;]*)\)" % name, header).group(1)
    assert "recovery_out_stripe_stride" in re.search(r"rs_repair_device_batch\s*\(([^;]*)\)", header).group(1)


@pytest.mark.parametrize("call", FORMS)
def test_argument_checks_precede_any_device_work(rs, call):
    """A made-up non-null context is never dereferenced: every check comes first, in
    rs_decode_device_strided's order."""
    err = rs._RsError()
    e = ctypes.byref(err)
    op = bytes([1, 1, 0, 1])
    rp = bytes([1, 0, 0, 0])
    fake = ctypes.c_void_p(8)
    # null context, then each null pointer -- d_recovery_out included
    assert call(rs, None, 4, 4, 64, 8, op, 8, rp, 8, 8, e) == 101 and err.code == 101
    for args in ((0, op, 8, rp, 8, 8), (8, None, 8, rp, 8, 8), (8, op, 0, rp, 8, 8), (8, op, 8, None, 8, 8),
                 (8, op, 8, rp, 0, 8), (8, op, 8, rp, 8, 0)):
        assert call(rs, fake, 4, 4, 64, *args, e) == 101, args
    # rs_validate next: a bad shard size, then an unsupported count (src/rate.rs:91-106) --
    # ahead of the pattern (these masks are one shard short)
    short = bytes([0, 0, 0, 0])
    assert call(rs, fake, 4, 4, 63, 8, short, 8, rp, 8, 8, e) == 6 and err.shard_bytes == 63
    assert call(rs, fake, 4096, 61441, 64, 8, short, 8, rp, 8, 8, e) == 10
    # one shard short: NotEnoughShards with the counts
    assert call(rs, fake, 4, 4, 64, 8, bytes([1, 1, 0, 0]), 8, rp, 8, 8, e) == 7
    assert (err.original_count, err.original_received_count, err.recovery_received_count) == (4, 2, 1)
    # nothing missing: RS_OK, the context untouched
    assert call(rs, fake, 4, 4, 64, 8, bytes([1] * 4), 8, bytes([1] * 4), 8, 8, e) == 0 and err.code == 0


@pytest.mark.parametrize("call", FORMS[1:])
def test_bad_strides_are_rejected_after_validate_and_before_the_pattern(rs, call):
    err = rs._RsError()
    e = ctypes.byref(err)
    fake = ctypes.c_void_p(8)
    short = bytes([0, 0, 0, 0])  # (would be NotEnoughShards: the strides are checked first)
    rp = bytes([1, 0, 0, 0])
    for k in range(4):  # a row stride below the shard size, each matrix in turn
        strides = [0, 0, 0, 0]
        strides[k] = 32
        assert call(rs, fake, 4, 4, 64, 8, short, 8, rp, 8, 8, e, strides=tuple(strides)) == 101, k
    # rs_validate still comes before the strides
    assert call(rs, fake, 4, 4, 63, 8, short, 8, rp, 8, 8, e, strides=(0, 0, 0, 32)) == 6


def test_batch_of_no_stripes_is_a_no_op(rs):
    err = rs._RsError()
    fake = ctypes.c_void_p(8)
    assert _batch(rs, fake, 4, 4, 64, 8, bytes([1, 1, 0, 1]), 8, bytes([1, 0, 0, 0]), 8, 8, ctypes.byref(err),
                  stripes=0) == 0


class _Fake:
    """Stands in for a device tensor in the wrappers' argument checks."""

    is_cuda = True

    def __init__(self, *shape, dtype="torch.uint8"):
        self.shape = shape
        self.dtype = dtype

    def dim(self):
        return len(self.shape)

    def stride(self, k=None):
        return int(np.prod(self.shape[k + 1:]))

    def is_contiguous(self):
        return True

    def element_size(self):
        return 1

    def data_ptr(self):
        return 8  # (never dereferenced: a call that reaches the library fails on its null context)


def test_wrappers_reject_wrong_shapes_dtypes_and_masks(rs):
    N, M, S, B = 4, 6, 64, 3
    ctx = types.SimpleNamespace(handle=None)
    op, rp = [1] * N, [1] * (M - 1) + [0]
    good = lambda: [_Fake(N, S), _Fake(M, S), _Fake(N, S), _Fake(M, S)]
    names = ["d_original", "d_recovery", "d_restored", "d_recovery_out"]
    rows = [N, M, N, M]

    def single(t, op=op, rp=rp):
        return rs.repair_device(N, M, S, t[0], op, t[1], rp, t[2], t[3], ctx=ctx)

    for k in range(4):
        t = good()
        t[k] = _Fake(rows[k] - 1, S)  # too few rows
        with pytest.raises(ValueError, match=names[k] + ":"):
            single(t)
        t[k] = _Fake(rows[k], S + 2)  # wrong shard size
        with pytest.raises(ValueError, match=names[k] + ":"):
            single(t)
        t[k] = _Fake(rows[k], S, dtype="torch.int32")
        with pytest.raises(ValueError, match=names[k] + ": dtype"):
            single(t)
        t[k] = _Fake(2, rows[k], S)  # a batch where a matrix belongs
        with pytest.raises(ValueError, match=names[k] + ":"):
            single(t)
    with pytest.raises(ValueError, match="original_present"):
        single(good(), op=[1] * (N + 1))
    with pytest.raises(ValueError, match="recovery_present"):
        single(good(), rp=[1] * (M - 1))
    # well-formed arguments reach the library (whose first check refuses the null context)
    with pytest.raises(ValueError, match="rs_status 101"):
        single(good())

    goodb = lambda: [_Fake(B, N, S), _Fake(B, M, S), _Fake(B, N, S), _Fake(B, M, S)]

    def batch(t, op=op, rp=rp):
        return rs.repair_device_batch(N, M, S, t[0], op, t[1], rp, t[2], t[3], ctx=ctx)

    for k in range(4):
        t = goodb()
        t[k] = _Fake(rows[k], S)  # a matrix where a batch belongs
        with pytest.raises(ValueError, match=names[k] + ":"):
            batch(t)
        t[k] = _Fake(B, rows[k] - 1, S)
        with pytest.raises(ValueError, match=names[k] + ":"):
            batch(t)
        if k:
            t[k] = _Fake(B + 1, rows[k], S)
            with pytest.raises(ValueError, match="stripe count"):
                batch(t)
    with pytest.raises(ValueError, match="original_present"):
        batch(goodb(), op=np.ones((B, N), np.uint8))  # one pattern for the whole batch
    with pytest.raises(ValueError, match="recovery_present"):
        batch(goodb(), rp=[1] * (M + 1))


def test_integration_doc_binds_the_entry_points():
    bound = {name: args for name, args, _ in ABI._extern_fns()}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in bound, name
        assert "d_recovery_out: *mut c_void" in bound[name], name
        assert name in doc
    assert "recovery_out_stripe_stride: u64" in bound["rs_repair_device_batch"]


# ---------------------------------------------------------------------------
# the identity, on the CPU oracle's engine primitives

GF_ORDER, GF_MOD = 65536, 65535


def _pow2(x):
    return 1 << max(0, int(x - 1).bit_length())


def _to_work(shard):
    """A shard in a work row of whole 64-byte blocks (src/engine/shards.rs:38-74: the tail's low
    bytes at the block's start, its high bytes 32 further)."""
    S = shard.size
    whole, tail = S // 64 * 64, S % 64
    row = np.zeros((S + 63) // 64 * 64, np.uint8)
    row[:whole] = shard[:whole]
    row[whole:whole + tail // 2] = shard[whole:whole + tail // 2]
    row[whole + 32:whole + 32 + tail // 2] = shard[whole + tail // 2:]
    return row


def _from_work(row, S):
    whole, tail = S // 64 * 64, S % 64
    return np.concatenate([row[:whole], row[whole:whole + tail // 2], row[whole + 32:whole + 32 + tail // 2]])


def reveal_all(rate, orig, op, rec, rp):
    """The decode of rate_high.rs / rate_low.rs:172-254 on the oracle's engine primitives, with
    the reveal multiply applied to EVERY erased shard position; returns (restored originals,
    restored recovery shards) as {index: bytes}."""
    L = O.lib()
    N, S = orig.shape
    M = rec.shape[0]
    high = rate == "high" or (rate == "default" and L.orc_use_high_rate(N, M) == 1)
    blocks = (S + 63) // 64
    chunk = _pow2(M) if high else _pow2(N)
    rec_base, orig_base = (0, chunk) if high else (chunk, 0)
    end = chunk + (N if high else M)
    rows = _pow2(end)
    w = np.zeros((rows, blocks * 64), np.uint8)
    got = np.zeros(rows, bool)
    for i in range(N):
        if op[i]:
            w[orig_base + i] = _to_work(orig[i])
            got[orig_base + i] = True
    for i in range(M):
        if rp[i]:
            w[rec_base + i] = _to_work(rec[i])
            got[rec_base + i] = True
    er = np.zeros(GF_ORDER, np.uint16)
    if high:  # rate_high.rs:186-204: the padding [M, chunk) counts as erased
        er[:end] = ~got[:end]
        L.orc_eval_poly(O.ptr(er), end)
    else:  # rate_low.rs:186-204: everything past the last recovery position is erased
        er[:N] = ~got[:N]
        er[chunk:end] = ~got[chunk:end]
        er[end:] = 1
        L.orc_eval_poly(O.ptr(er), GF_ORDER)
    for i in range(rows):
        if i < end and got[i]:
            L.orc_mul(w[i].ctypes.data_as(ctypes.c_void_p), blocks, int(er[i]))
        else:
            w[i] = 0
    L.orc_ifft(O.ptr(w), blocks, 0, rows, end, 0)
    L.orc_formal_derivative(O.ptr(w), blocks, rows)
    L.orc_fft(O.ptr(w), blocks, 0, rows, end, 0)

    def reveal(p):
        L.orc_mul(w[p].ctypes.data_as(ctypes.c_void_p), blocks, GF_MOD - int(er[p]))
        return _from_work(w[p], S)

    return ({i: reveal(orig_base + i) for i in range(N) if not op[i]},
            {i: reveal(rec_base + i) for i in range(M) if not rp[i]})


IDENTITY_SHAPES = [
    # (rate, N, M, S): both rates, a tail size, multi-chunk shapes
    ("high", 5, 3, 64), ("low", 3, 5, 64), ("default", 1, 1, 64), ("default", 32, 32, 70),
    ("high", 100, 30, 64), ("low", 30, 100, 64), ("default", 100, 30, 130), ("default", 30, 100, 2),
    ("high", 64, 64, 8), ("low", 200, 256, 66),
]


@pytest.mark.parametrize("rate,N,M,S", IDENTITY_SHAPES)
def test_reveal_of_an_erased_recovery_row_is_the_recovery_shard(rate, N, M, S):
    orig = O.generate_original(N, S, 7)
    rec = O.encode(rate, orig, M)
    rng = np.random.default_rng(N * 1000 + M)
    lose_max = M  # at most M of the N + M shards may be missing

    def pat(n_o, n_r):
        op, rp = np.ones(N, np.uint8), np.ones(M, np.uint8)
        op[rng.choice(N, n_o, replace=False)] = 0
        rp[rng.choice(M, n_r, replace=False)] = 0
        return op, rp

    k = min(N, lose_max)
    pats = {
        "max": pat(k // 2, lose_max - k // 2),
        "half": pat(min(N, lose_max // 4), max(1, lose_max // 4)),
        "one recovery shard, every original present": pat(0, 1),
    }
    for what, (op, rp) in pats.items():
        assert int(op.sum()) + int(rp.sum()) >= N
        # (absent rows hold junk: the statement must not depend on them)
        got_o, got_r = reveal_all(rate, np.where(op[:, None] == 1, orig, 0xA5).astype(np.uint8), op,
                                  np.where(rp[:, None] == 1, rec, 0x5A).astype(np.uint8), rp)
        assert sorted(got_r) == np.flatnonzero(rp == 0).tolist()
        for i, row in got_r.items():
            assert np.array_equal(row, rec[i]), f"{rate} {N}:{M} x {S} {what}: recovery shard {i}"
        for i, row in got_o.items():
            assert np.array_equal(row, orig[i]), f"{rate} {N}:{M} x {S} {what}: original {i}"
        if (op == 0).any():  # and the originals agree with the oracle's own decode
            want = O.decode(rate, np.where(op[:, None] == 1, orig, 0).astype(np.uint8), op,
                            np.where(rp[:, None] == 1, rec, 0).astype(np.uint8), rp)
            for i, row in got_o.items():
                assert np.array_equal(row, want[i])
