"""rs_repair_device_batch_masks without a GPU: the symbol and its declaration, the argument and
pattern checks (all of which come before any device work), the Python wrapper's argument
checks, the INTEGRATION.md binding (tests/test_integration_abi.py compiles that binding against
the header), and the routing arithmetic the GPU tests' shapes rely on."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import test_gpu_batch_masks as GD
import test_gpu_repair_masks as G
import test_integration_abi as ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rs_repair_device_batch_masks"


@pytest.fixture(scope="module")
def rs():
    # (imported by the tests that use it, not while pytest collects: tests/test_batch_masks_cpu.py)
    import reed_solomon_simd
    return reed_solomon_simd


def _call(rs, ctx, N, M, S, stripes, d_o, op, d_r, rp, d_x, d_y, status=None, err=None, strides=(0, 0, 0, 0)):
    return rs._lib.rs_repair_device_batch_masks(ctx, 0, N, M, S, stripes, d_o, strides[0], 0, op, d_r, strides[1], 0,
                                                rp, d_x, strides[2], 0, d_y, strides[3], 0, status, None, err)


def test_symbol_is_exported_and_declared(rs):
    assert hasattr(rs._lib, NAME)
    assert rs._lib.rs_repair_device_batch_masks.argtypes is not None  # the ctypes signature is declared
    assert len(rs._lib.rs_repair_device_batch_masks.argtypes) == 23
    header = open(os.path.join(ROOT, "include", "rs_mi355x.h")).read()
    m = re.search(r"rs_status\s+%s\s*\(([^;]*)\)\s*;" % NAME, header)
    assert m
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    # ... d_restored and its strides, d_recovery_out and its two strides, stripe_status, stream, err
    assert args[-9:] == ["void *d_restored", "uint64_t restored_stride", "uint64_t restored_stripe_stride",
                         "void *d_recovery_out", "uint64_t recovery_out_stride",
                         "uint64_t recovery_out_stripe_stride", "uint8_t *stripe_status", "void *stream",
                         "rs_error *err"]
    assert len(args) == 23
    # the header's lists know the call
    assert NAME in header.split("Device-resident batch entry points")[1].split("Thread-safety")[0]
    not_yet = header.split("Not covered yet")[1].split("*/")[0]
    assert "per-stripe patterns (rs_decode_device_batch_masks)" not in not_yet


def test_argument_checks_precede_any_device_work(rs):
    """A made-up non-null context is never dereferenced: every check comes first."""
    err = rs._RsError()
    e = ctypes.byref(err)
    op = np.ones((2, 4), np.uint8).ctypes.data
    fake = ctypes.c_void_p(8)
    # null context, then each null pointer -- d_recovery_out included
    assert _call(rs, None, 4, 4, 64, 2, 8, op, 8, op, 8, 8, err=e) == 101 and err.code == 101
    for args in ((0, op, 8, op, 8, 8), (8, None, 8, op, 8, 8), (8, op, 0, op, 8, 8), (8, op, 8, None, 8, 8),
                 (8, op, 8, op, 0, 8), (8, op, 8, op, 8, 0)):
        assert _call(rs, fake, 4, 4, 64, 2, *args, err=e) == 101, args
    # rs_validate next: shard size, then shard counts (src/rate.rs:91-106) -- ahead of the strides
    assert _call(rs, fake, 4, 4, 63, 2, 8, op, 8, op, 8, 8, err=e, strides=(0, 0, 0, 32)) == 6
    assert err.shard_bytes == 63
    assert _call(rs, fake, 4096, 61441, 64, 2, 8, op, 8, op, 8, 8, err=e) == 10
    # the four row strides, each below the shard size in turn -- ahead of stripes == 0 and the patterns
    short = np.zeros((2, 4), np.uint8).ctypes.data  # (would be NotEnoughShards)
    for k in range(4):
        strides = [0, 0, 0, 0]
        strides[k] = 32
        assert _call(rs, fake, 4, 4, 64, 2, 8, short, 8, short, 8, 8, err=e, strides=tuple(strides)) == 101, k
        assert _call(rs, fake, 4, 4, 64, 0, 8, short, 8, short, 8, 8, err=e, strides=tuple(strides)) == 101, k
    # no stripes: nothing to do (the masks are not read)
    assert _call(rs, fake, 4, 4, 64, 0, 8, 8, 8, 8, 8, 8, err=e) == 0 and err.code == 0


def test_pattern_check_precedes_device_work(rs):
    """Stripe 1 of 3 is one shard short: all or nothing reports it (counts, stripe in `index`); the
    status form marks it.  The other stripes miss nothing, so neither touches the (made-up) context."""
    fake = ctypes.c_void_p(8)
    op = np.ones((3, 4), np.uint8)
    rp = np.ones((3, 4), np.uint8)
    op[1, :3] = 0
    rp[1, 2:] = 0
    err = rs._RsError()
    e = ctypes.byref(err)
    assert _call(rs, fake, 4, 4, 64, 3, 8, op.ctypes.data, 8, rp.ctypes.data, 8, 8, err=e) == 7
    assert (err.original_count, err.original_received_count, err.recovery_received_count, err.index) == (4, 1, 2, 1)
    status = (ctypes.c_uint8 * 3)(9, 9, 9)
    assert _call(rs, fake, 4, 4, 64, 3, 8, op.ctypes.data, 8, rp.ctypes.data, 8, 8, status, e) == 0
    assert list(status) == [0, 7, 0] and err.code == 0
    # every stripe undecodable
    none = np.zeros((3, 4), np.uint8)
    status = (ctypes.c_uint8 * 3)(9, 9, 9)
    assert _call(rs, fake, 4, 4, 64, 3, 8, none.ctypes.data, 8, none.ctypes.data, 8, 8, status, e) == 0
    assert list(status) == [7, 7, 7]
    assert _call(rs, fake, 4, 4, 64, 3, 8, none.ctypes.data, 8, none.ctypes.data, 8, 8, err=e) == 7 and err.index == 0


def test_batch_that_misses_nothing_is_a_no_op(rs):
    fake = ctypes.c_void_p(8)
    full = np.ones((3, 4), np.uint8)
    err = rs._RsError()
    assert _call(rs, fake, 4, 4, 64, 3, 8, full.ctypes.data, 8, full.ctypes.data, 8, 8, err=ctypes.byref(err)) == 0
    assert err.code == 0
    status = (ctypes.c_uint8 * 3)(9, 9, 9)
    assert _call(rs, fake, 4, 4, 64, 3, 8, full.ctypes.data, 8, full.ctypes.data, 8, 8, status) == 0
    assert list(status) == [0, 0, 0]


class _Fake:
    """Stands in for a device tensor in the wrapper's argument checks."""

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


def test_wrapper_rejects_wrong_shapes_dtypes_and_masks(rs):
    N, M, S, B = 4, 6, 64, 3
    ctx = types.SimpleNamespace(handle=None)
    good_o, good_r = np.ones((B, N), np.uint8), np.ones((B, M), np.uint8)
    good = lambda: [_Fake(B, N, S), _Fake(B, M, S), _Fake(B, N, S), _Fake(B, M, S)]
    names = ["d_original", "d_recovery", "d_restored", "d_recovery_out"]
    rows = [N, M, N, M]

    def call(t, op=good_o, rp=good_r, **kw):
        return rs.repair_device_batch_masks(N, M, S, t[0], op, t[1], rp, t[2], t[3], ctx=ctx, **kw)

    for k in range(4):
        t = good()
        t[k] = _Fake(rows[k], S)  # a matrix where a batch belongs
        with pytest.raises(ValueError, match=names[k] + ":"):
            call(t)
        t[k] = _Fake(B, rows[k] - 1, S)  # too few rows
        with pytest.raises(ValueError, match=names[k] + ":"):
            call(t)
        t[k] = _Fake(B, rows[k], S + 2)  # wrong shard size
        with pytest.raises(ValueError, match=names[k] + ":"):
            call(t)
        t[k] = _Fake(B, rows[k], S, dtype="torch.int32")
        with pytest.raises(ValueError, match=names[k] + ": dtype"):
            call(t)
        if k:
            t[k] = _Fake(B + 1, rows[k], S)
            with pytest.raises(ValueError, match="stripe count"):
                call(t)
    for op, rp, what in ((np.ones((B - 1, N), np.uint8), good_r, "original_present"),
                         (np.ones(N, np.uint8), good_r, "original_present"),  # 1-D: one pattern for the batch
                         (good_o, np.ones(M, np.uint8), "recovery_present"),
                         (good_o, np.ones((B, M + 1), np.uint8), "recovery_present"),
                         (good_o, [[1] * M] * (B + 1), "recovery_present")):
        with pytest.raises(ValueError, match=what):
            call(good(), op, rp)
    # well-formed arguments reach the library (whose first check refuses the null context)
    with pytest.raises(ValueError, match="rs_status 101"):
        call(good())
    with pytest.raises(ValueError, match="rs_status 101"):
        call(good(), status=True)


def test_integration_doc_binds_the_entry_point():
    bound = {name: args for name, args, _ in ABI._extern_fns()}
    assert NAME in bound
    for arg in ("d_recovery_out: *mut c_void", "recovery_out_stride: u64", "recovery_out_stripe_stride: u64",
                "stripe_status: *mut u8"):
        assert arg in bound[NAME], arg
    assert bound[NAME].index("recovery_out_stripe_stride") < bound[NAME].index("stripe_status")
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read().split("## 3.")[1]


def test_gpu_test_shapes_reach_the_kernel_forms_named(rs):
    """The routing arithmetic for the GPU tests' shapes: the fused route covers up to 2^11 work rows
    (16..64 padded to 2^7); 2- or 4-element packs from packs x stripes against half the CUs of an
    MI355X (128).  The shapes are those of the decode's test with the repair's kernel, plus the
    HighRate shape whose padding work rows lie in no map; the kinds cover every kind."""
    packs = lambda S: S // 64 * 8 + ((S % 64) // 2 + 3) // 4
    seen = set()
    for rate, N, M, S, B, k0, kernel in G.MIXED:
        nd = G.work_rows(rate, N, M)[2]
        if kernel is None:
            assert nd > 2048, (rate, N, M)
        else:
            assert kernel == "k_mono_repair_masks<%d, %d>" % (nd.bit_length() - 1, 2 if packs(S) * B <= 128 else 4)
        assert rs.use_high_rate(N, M) >= 0
        seen.update(G.mixed_kinds(B, k0))
    assert seen == set(G.KINDS)
    assert ({(r, N, M, S, B, (k or "").replace("k_mono_masks", "k_mono_repair_masks") or None)
             for r, N, M, S, B, _, k in GD.MIXED} <= {(r, N, M, S, B, k) for r, N, M, S, B, _, k in G.MIXED})
    chunk, end, nd = G.work_rows("high", 100, 300)
    assert (chunk, end, nd) == (512, 612, 1024) and 300 < chunk  # padding work rows [300, 512)
    # every pattern kind is decodable by construction, except the one that must not be
    rng = np.random.default_rng(0)
    for N, M in ((32, 32), (200, 56), (100, 1000), (100, 300)):
        for kind in G.KINDS:
            op, rp = G.pattern(kind, N, M, rng)
            assert (int(op.sum()) + int(rp.sum()) >= N) == (kind != "undecodable"), (kind, N, M)
