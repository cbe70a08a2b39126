"""rs_decode_device_batch_masks without a GPU: the symbol, its argument checks (which come
before any device work), the Python wrapper's mask-shape check, the header and the
INTEGRATION.md binding (tests/test_integration_abi.py compiles that binding against the
header), and the routing arithmetic the GPU tests' shapes rely on."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import test_gpu_batch_masks as G
import test_integration_abi as ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rs():
    # (imported by the tests that use it, not while pytest collects: a GPU run collects this
    # file too, and there torch is loaded before the library, as in every GPU test)
    import reed_solomon_simd
    return reed_solomon_simd


def _call(rs, ctx, N, M, S, stripes, d_o, op, d_r, rp, d_x, status=None, err=None):
    return rs._lib.rs_decode_device_batch_masks(ctx, 0, N, M, S, stripes, d_o, 0, 0, op, d_r, 0, 0, rp, d_x, 0, 0,
                                                status, None, err)


def test_entry_point_validates_before_any_device_work(rs):
    assert hasattr(rs._lib, "rs_decode_device_batch_masks")
    err = rs._RsError()
    op = np.ones((2, 4), np.uint8).ctypes.data
    # null context, then each null pointer (a made-up non-null context is never dereferenced:
    # the checks come first)
    assert _call(rs, None, 4, 4, 64, 2, 8, op, 8, op, 8, err=ctypes.byref(err)) == 101 and err.code == 101
    fake = ctypes.c_void_p(8)
    for args in ((0, op, 8, op, 8), (8, None, 8, op, 8), (8, op, 0, op, 8), (8, op, 8, None, 8), (8, op, 8, op, 0)):
        assert _call(rs, fake, 4, 4, 64, 2, *args, err=ctypes.byref(err)) == 101, args
    # rs_validate next: shard size, then shard counts (src/rate.rs:91-106)
    assert _call(rs, fake, 4, 4, 63, 2, 8, op, 8, op, 8, err=ctypes.byref(err)) == 6 and err.shard_bytes == 63
    assert _call(rs, fake, 4096, 61441, 64, 2, 8, op, 8, op, 8, err=ctypes.byref(err)) == 10
    # no stripes: nothing to do (the masks are not read)
    assert _call(rs, fake, 4, 4, 64, 0, 8, op, 8, op, 8, err=ctypes.byref(err)) == 0


def test_pattern_check_precedes_device_work(rs):
    """Stripe 1 of 3 is one shard short: all or nothing reports it (counts, stripe in `index`);
    the status form marks it.  Neither touches the (made-up) context when no stripe is left to decode."""
    fake = ctypes.c_void_p(8)
    op = np.ones((3, 4), np.uint8)
    rp = np.zeros((3, 4), np.uint8)
    op[1, :3] = 0
    rp[1, :2] = 1
    err = rs._RsError()
    code = _call(rs, fake, 4, 4, 64, 3, 8, op.ctypes.data, 8, rp.ctypes.data, 8, err=ctypes.byref(err))
    assert code == 7
    assert (err.original_count, err.original_received_count, err.recovery_received_count, err.index) == (4, 1, 2, 1)
    status = (ctypes.c_uint8 * 3)(9, 9, 9)
    assert _call(rs, fake, 4, 4, 64, 3, 8, op.ctypes.data, 8, rp.ctypes.data, 8, status, ctypes.byref(err)) == 0
    assert list(status) == [0, 7, 0]


class _FakeBatch:
    """Stands in for a [stripes, rows, shard_bytes] device tensor in the wrapper's argument checks."""

    dtype = "torch.uint8"
    is_cuda = True

    def __init__(self, *shape):
        self.shape = shape

    def dim(self):
        return len(self.shape)

    def stride(self, k):
        return int(np.prod(self.shape[k + 1:]))

    def element_size(self):
        return 1

    def data_ptr(self):
        return 8  # (never dereferenced: a call that got as far as the library fails on its null context)


def test_wrapper_rejects_masks_of_the_wrong_shape(rs):
    N, M, S, B = 4, 6, 64, 3
    t = (_FakeBatch(B, N, S), _FakeBatch(B, M, S), _FakeBatch(B, N, S))
    ctx = types.SimpleNamespace(handle=None)
    good_o, good_r = np.ones((B, N), np.uint8), np.ones((B, M), np.uint8)
    for op, rp, what in ((np.ones((B - 1, N), np.uint8), good_r, "original_present"),
                         (np.ones(N, np.uint8), good_r, "original_present"),
                         (good_o, np.ones((B, M + 1), np.uint8), "recovery_present"),
                         (good_o, [[1] * M] * (B + 1), "recovery_present")):
        with pytest.raises(ValueError, match=what):
            rs.decode_device_batch_masks(N, M, S, t[0], op, t[1], rp, t[2], ctx=ctx)
    # the shared-pattern entry keeps rejecting anything but one mask per side
    with pytest.raises(ValueError, match="original_present"):
        rs.decode_device_batch(N, M, S, t[0], np.ones((B, N), np.uint8), t[1], np.ones(M, np.uint8), t[2], ctx=ctx)


def test_header_and_integration_doc_declare_the_entry_point():
    header = open(os.path.join(ROOT, "include", "rs_mi355x.h")).read()
    assert re.search(r"rs_status\s+rs_decode_device_batch_masks\s*\(", header)
    bound = {name: args for name, args, _ in ABI._extern_fns()}
    assert "rs_decode_device_batch_masks" in bound
    assert "stripe_status: *mut u8" in bound["rs_decode_device_batch_masks"]
    assert "rs_decode_device_batch_masks" in open(os.path.join(ROOT, "INTEGRATION.md")).read().split("## 3.")[1]


def test_gpu_test_shapes_reach_the_kernel_forms_named(rs):
    """decode_dev's routing arithmetic for the GPU tests' shapes: the fused route covers up to
    2^11 work rows (16..64 padded to 2^7); 2- or 4-element packs from packs x stripes against
    half the CUs of an MI355X (128)."""
    packs = lambda S: S // 64 * 8 + ((S % 64) // 2 + 3) // 4
    for rate, N, M, S, B, k0, kernel in G.MIXED:
        nd = G.work_rows(rate, N, M)[2]
        if kernel is None:
            assert nd > 2048, (rate, N, M)
        else:
            assert kernel == "k_mono_masks<%d, %d>" % (nd.bit_length() - 1, 2 if packs(S) * B <= 128 else 4)
    for (L, rate), (N, M) in G.SWEEP_SHAPES.items():
        assert G.work_rows(rate, N, M)[2] == 1 << L, (L, rate, N, M)
        assert rs.use_high_rate(N, M) >= 0
    assert len(G._sweep_cases()) == 24 and {c[0] for c in G._sweep_cases()} == {7, 8, 9, 10, 11}
