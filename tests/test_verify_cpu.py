"""rs_verify_device* without a GPU: the symbols and their declarations, the argument checks (all
of which come before any device work, in the header's order), the no-op cases, the Python
wrappers' argument checks and the INTEGRATION.md binding.
"""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import test_integration_abi as ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rs_verify_device", "rs_verify_device_batch", "rs_verify_set_fused")
HEADER = os.path.join(ROOT, "include", "rs_mi355x.h")


@pytest.fixture(scope="module")
def rs():
    # (imported by the tests that use it, not while pytest collects: tests/test_batch_masks_cpu.py)
    import reed_solomon_simd
    return reed_solomon_simd


def _single(rs, ctx, N, M, S, d_orig, d_rec, mask, d_flags, err=None, strides=(0, 0), stripes=None):
    return rs._lib.rs_verify_device(ctx, 0, N, M, S, d_orig, strides[0], d_rec, strides[1], mask, d_flags, None, err)


def _batch(rs, ctx, N, M, S, d_orig, d_rec, mask, d_flags, err=None, strides=(0, 0), stripes=2):
    return rs._lib.rs_verify_device_batch(ctx, 0, N, M, S, stripes, d_orig, strides[0], 0, d_rec, strides[1], 0, mask,
                                          d_flags, None, err)


FORMS = [_single, _batch]


def test_symbols_are_exported_and_declared(rs):
    header = open(HEADER).read()
    for name in NAMES:
        assert hasattr(rs._lib, name), name
        assert getattr(rs._lib, name).argtypes is not None, name  # the ctypes signature is declared
        assert re.search(r"rs_status\s+%s\s*\(([^;]*)\)\s*;" % name, header), name
    for name in NAMES[:2]:
        proto = re.search(r"rs_status\s+%s\s*\(([^;]*)\)\s*;" % name, header).group(1)
        assert re.search(r"const void \*d_original.*const void \*d_recovery.*const uint8_t \*recovery_check,\s*"
                         r"uint8_t \*d_mismatch,\s*void \*stream,\s*rs_error \*err", proto, re.S), name
    batch = re.search(r"rs_verify_device_batch\s*\(([^;]*)\)", header).group(1)
    for arg in ("uint64_t stripes", "original_stripe_stride", "recovery_stripe_stride"):
        assert arg in batch, arg
    assert re.search(r"rs_status\s+rs_verify_set_fused\s*\(\s*rs_context \*ctx,\s*int mode\s*\)", header)
    assert len(rs._lib.rs_verify_device.argtypes) == 13 and len(rs._lib.rs_verify_device_batch.argtypes) == 16
    assert len(rs._lib.rs_verify_set_fused.argtypes) == 2
    # the wrappers, and the default in both places
    for name in ("verify_device", "verify_device_batch", "verify_set_fused"):
        assert callable(getattr(rs, name)), name
    default = int(re.search(r"#define RS_VERIFY_FUSED_DEFAULT (\d+)", header).group(1))
    assert default in (0, 1) and rs.VERIFY_FUSED_DEFAULT == default
    # what the contract promises, in the header's words
    for phrase in ("every byte of d_mismatch is defined", "Nothing else is written", "are never read",
                   "never compared", "hipMemsetAsync"):
        assert phrase in header, phrase


@pytest.mark.parametrize("call", FORMS)
def test_argument_checks_precede_any_device_work(rs, call):
    """A made-up non-null context is never dereferenced: every check comes first, in the
    header's order."""
    err = rs._RsError()
    e = ctypes.byref(err)
    fake = ctypes.c_void_p(8)
    # 1. null context, d_original, d_recovery, d_mismatch
    assert call(rs, None, 4, 4, 64, 8, 8, None, 8, e) == 101 and err.code == 101
    assert call(rs, fake, 4, 4, 64, 0, 8, None, 8, e) == 101
    assert call(rs, fake, 4, 4, 64, 8, 0, None, 8, e) == 101
    assert call(rs, fake, 4, 4, 64, 8, 8, None, 0, e) == 101
    # ... ahead of rs_validate (a bad shard size here)
    assert call(rs, fake, 4, 4, 63, 8, 8, None, 0, e) == 101
    # 2. rs_validate: a bad shard size, an unsupported count (src/rate.rs:91-106) -- ahead of
    # the strides (bad here)
    assert call(rs, fake, 4, 4, 63, 8, 8, None, 8, e, strides=(32, 0)) == 6 and err.shard_bytes == 63
    assert call(rs, fake, 4096, 61441, 64, 8, 8, None, 8, e, strides=(0, 32)) == 10
    assert (err.original_count, err.recovery_count) == (4096, 61441)
    # 3. the two row strides, each in turn -- also when the mask selects nothing, and with
    # no stripes at all
    for strides in ((32, 0), (0, 32)):
        assert call(rs, fake, 4, 4, 64, 8, 8, None, 8, e, strides=strides) == 101 and err.code == 101, strides
        assert call(rs, fake, 4, 4, 64, 8, 8, bytes(4), 8, e, strides=strides) == 101, strides
    assert _batch(rs, fake, 4, 4, 64, 8, 8, None, 8, e, strides=(0, 63), stripes=0) == 101
    # a null err is allowed
    assert call(rs, fake, 4, 4, 64, 8, 8, None, 8, None, strides=(0, 32)) == 101
    assert call(rs, None, 4, 4, 64, 8, 8, None, 8, None) == 101


def test_no_stripes_is_ok_without_touching_anything(rs):
    err = rs._RsError()
    err.code = 55
    fake = ctypes.c_void_p(8)
    assert _batch(rs, fake, 4, 4, 64, 8, 8, None, 8, ctypes.byref(err), stripes=0) == 0 and err.code == 0
    assert _batch(rs, fake, 4, 4, 64, 8, 8, bytes(4), 8, None, stripes=0) == 0
    assert _batch(rs, fake, 4, 4, 64, 8, 8, b"\1\0\0\1", 8, None, strides=(64, 128), stripes=0) == 0


@pytest.mark.parametrize("call", FORMS)
def test_empty_mask_does_not_touch_the_context(rs, call):
    """A mask that selects no row: the made-up context is not dereferenced and no workspace is
    made -- all the call does is one memset of the flags on the stream.  Here the flag array is
    host memory the runtime does not know, so the memset is either refused (RS_ERR_DEVICE, with
    the runtime's message; also the answer of a machine without a GPU) or RS_OK; what it does on
    device memory is tests/test_gpu_verify.py's."""
    err = rs._RsError()
    fake = ctypes.c_void_p(8)
    flags = (ctypes.c_uint8 * 64)()
    st = call(rs, fake, 4, 4, 64, 8, 8, bytes(4), ctypes.addressof(flags), ctypes.byref(err))
    assert st in (0, 100) and err.code == st
    if st == 100:
        assert rs._lib.rs_last_device_error()


def test_set_fused_refuses_a_null_context(rs):
    assert rs._lib.rs_verify_set_fused(None, 0) == 101
    assert rs._lib.rs_verify_set_fused(None, 1) == 101


class _Fake:
    """Stands in for a device tensor in the wrappers' argument checks."""

    is_cuda = True
    device = "cuda:0"

    def __init__(self, *shape, dtype="torch.uint8", contiguous=True):
        self.shape = shape
        self.dtype = dtype
        self._contiguous = contiguous

    def dim(self):
        return len(self.shape)

    def stride(self, k=None):
        return int(np.prod(self.shape[k + 1:]))

    def is_contiguous(self):
        return self._contiguous

    def element_size(self):
        return 1

    def data_ptr(self):
        return 8  # (never dereferenced: a call that reaches the library fails on its null context)


def test_wrappers_reject_wrong_shapes_dtypes_and_masks(rs):
    N, M, S, B = 8, 6, 64, 3
    ctx = types.SimpleNamespace(handle=None)
    names = ["d_original", "d_recovery"]
    rows = [N, M]
    good = lambda: [_Fake(N, S), _Fake(M, S)]

    def single(t, mask=None, flags=_Fake(M)):
        return rs.verify_device(N, M, S, t[0], t[1], recovery_rows=mask, d_mismatch=flags, ctx=ctx)

    for k in range(2):
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
    with pytest.raises(ValueError, match="recovery_rows"):
        single(good(), mask=[1] * (M + 1))
    # the flags: exactly recovery_count bytes, uint8, contiguous (the library writes them densely)
    for bad in (_Fake(M - 1), _Fake(M + 1), _Fake(1, M), _Fake(M, dtype="torch.bool"), _Fake(M, contiguous=False)):
        with pytest.raises(ValueError, match="d_mismatch"):
            single(good(), flags=bad)
    with pytest.raises(ValueError, match="d_mismatch"):  # raw pointers: nothing says where to allocate
        rs.verify_device(N, M, S, 8, 8, ctx=ctx)
    with pytest.raises(rs.UnsupportedShardCount):  # the reference's own checks come first
        rs.verify_device(4096, 61441, S, _Fake(1, S), _Fake(1, S), d_mismatch=_Fake(1), ctx=ctx)
    # well-formed arguments reach the library (whose first check refuses the null context)
    with pytest.raises(ValueError, match="rs_status 101"):
        single(good())
    with pytest.raises(ValueError, match="rs_status 101"):
        single(good(), mask=[1, 0, 0, 1, 1, 0])
    with pytest.raises(ValueError, match="rs_status 101"):
        rs.verify_device(N, M, S, 8, 8, d_mismatch=8, ctx=ctx)  # raw pointers throughout

    goodb = lambda: [_Fake(B, N, S), _Fake(B, M, S)]

    def batch(t, mask=None, flags=_Fake(B, M)):
        return rs.verify_device_batch(N, M, S, t[0], t[1], recovery_rows=mask, d_mismatch=flags, ctx=ctx)

    for k in range(2):
        t = goodb()
        t[k] = _Fake(rows[k], S)  # a matrix where a batch belongs
        with pytest.raises(ValueError, match=names[k] + ":"):
            batch(t)
        t[k] = _Fake(B, rows[k] - 1, S)
        with pytest.raises(ValueError, match=names[k] + ":"):
            batch(t)
        t[k] = _Fake(B + 1, rows[k], S)
        with pytest.raises(ValueError, match="stripe count"):
            batch(t)
    with pytest.raises(ValueError, match="recovery_rows"):
        batch(goodb(), mask=np.ones((B, M), np.uint8))  # one mask for the whole batch
    for bad in (_Fake(M), _Fake(B, M + 1), _Fake(B + 1, M), _Fake(B * M)):
        with pytest.raises(ValueError, match="d_mismatch"):
            batch(goodb(), flags=bad)
    with pytest.raises(ValueError, match="rs_status 101"):
        batch(goodb())
    with pytest.raises(ValueError):
        rs.verify_set_fused(0, ctx=ctx)


def test_integration_doc_binds_the_entry_points():
    """The Rust lines of INTEGRATION.md name the three calls inside an `extern "C"` block that
    tests/test_integration_abi.py compiles against the header; the ctypes lines name them too,
    and the three-call scrub is there."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    bound = {f[0]: f for f in ABI._extern_fns()}
    for name in NAMES:
        assert name in bound, name
        ABI._prototype(*bound[name])  # every type maps
        assert re.search(r'_sig\("%s"|lib\.%s\b' % (name, name), doc), name  # the ctypes side
    args = bound["rs_verify_device_batch"][1]
    assert "recovery_check: *const u8" in args and "d_mismatch: *mut u8" in args
    scrub = doc[doc.index("rs.verify_device_batch("):]
    assert "repair_device_batch_masks(" in scrub[:1500]
