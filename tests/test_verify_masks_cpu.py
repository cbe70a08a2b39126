"""rs_verify_device_batch_masks / rs_locate_device_batch_masks without a GPU: the symbols and their
declarations, the argument checks (all before any device work, in the header's order), the Python
wrappers' rejections, the INTEGRATION.md binding -- and the model: locate_model.locate applied
stripe by stripe, each with its own mask, gives the outcome every constructed batch of
tests/verify_masks_cases.py is built for, so that a failure on the GPU is the kernels'.
"""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import test_integration_abi as ABI
import verify_masks_cases as C
from test_verify_cpu import _Fake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rs_mi355x.h")
NAMES = ("rs_verify_device_batch_masks", "rs_locate_device_batch_masks")


@pytest.fixture(scope="module")
def rs():
    import reed_solomon_simd
    return reed_solomon_simd


def _verify(rs, ctx, N, M, S, d_orig, d_rec, mask, d_flags, err=None, strides=(0, 0), stripes=2):
    return rs._lib.rs_verify_device_batch_masks(ctx, 0, N, M, S, stripes, d_orig, strides[0], 0, d_rec, strides[1], 0,
                                                mask, d_flags, None, err)


def _locate(rs, ctx, N, M, S, d_orig, d_rec, mask, d_flags, err=None, strides=(0, 0), stripes=2, d_located=8,
            status=None):
    return rs._lib.rs_locate_device_batch_masks(ctx, 0, N, M, S, stripes, d_orig, strides[0], 0, d_rec, strides[1], 0,
                                                mask, d_located, d_flags, status, None, err)


def _mask(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a.ctypes.data_as(ctypes.c_void_p), a  # (the array is kept alive by the caller)


def test_symbols_are_exported_and_declared(rs):
    header = open(HEADER).read()
    for name in NAMES:
        assert hasattr(rs._lib, name), name
        assert getattr(rs._lib, name).argtypes is not None, name
        proto = re.search(r"rs_status\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert proto, name
        for arg in ("uint64_t stripes", "original_stripe_stride", "recovery_stripe_stride",
                    "const uint8_t *recovery_check", "uint8_t *d_mismatch", "void *stream", "rs_error *err"):
            assert arg in proto.group(1), (name, arg)
    assert "uint8_t *stripe_status" in re.search(r"rs_locate_device_batch_masks\s*\(([^;]*)\)\s*;", header).group(1)
    assert len(rs._lib.rs_verify_device_batch_masks.argtypes) == 16
    assert len(rs._lib.rs_locate_device_batch_masks.argtypes) == 18
    assert int(re.search(r"#define RS_LOCATE_SKIPPED \((-\d+)\)", header).group(1)) == rs.LOCATE_SKIPPED == -4
    for name in ("verify_device_batch_masks", "locate_device_batch_masks"):
        assert callable(getattr(rs, name)), name
    default = int(re.search(r"#define RS_VERIFY_MASKS_FUSED_DEFAULT (\d+)", header).group(1))
    assert default in (0, 1) and rs.VERIFY_MASKS_FUSED_DEFAULT == default


@pytest.mark.parametrize("call", [_verify, _locate])
def test_argument_checks_precede_any_device_work(rs, call):
    """A made-up non-null context is never dereferenced: every check comes first, in the
    header's order."""
    err = rs._RsError()
    e = ctypes.byref(err)
    fake = ctypes.c_void_p(8)
    m, keep = _mask(np.ones((2, 4)))
    # 1. null context, matrices, flags -- and the mask, which these calls do not default
    assert call(rs, None, 4, 4, 64, 8, 8, m, 8, e) == 101 and err.code == 101
    assert call(rs, fake, 4, 4, 64, 0, 8, m, 8, e) == 101
    assert call(rs, fake, 4, 4, 64, 8, 0, m, 8, e) == 101
    assert call(rs, fake, 4, 4, 64, 8, 8, m, 0, e) == 101
    err.code = 0
    assert call(rs, fake, 4, 4, 64, 8, 8, None, 8, e) == 101 and err.code == 101
    assert call(rs, fake, 4, 4, 63, 8, 8, None, 8, e) == 101  # ... ahead of rs_validate
    # 2. rs_validate, ahead of the strides (bad here)
    assert call(rs, fake, 4, 4, 63, 8, 8, m, 8, e, strides=(32, 0)) == 6 and err.shard_bytes == 63
    assert call(rs, fake, 4096, 61441, 64, 8, 8, m, 8, e, strides=(0, 32)) == 10
    # 3. the two row strides, each in turn, also with no stripes at all
    for strides in ((32, 0), (0, 32)):
        assert call(rs, fake, 4, 4, 64, 8, 8, m, 8, e, strides=strides) == 101 and err.code == 101, strides
        assert call(rs, fake, 4, 4, 64, 8, 8, m, 8, e, strides=strides, stripes=0) == 101, strides
    # 4. stripes == 0: RS_OK, nothing touched (the mask is not read: it has no row)
    err.code = 55
    assert call(rs, fake, 4, 4, 64, 8, 8, m, 8, e, stripes=0) == 0 and err.code == 0
    assert call(rs, fake, 4, 4, 64, 8, 8, m, 8, None, stripes=0) == 0
    assert call(rs, None, 4, 4, 64, 8, 8, m, 8, None) == 101  # a null err is allowed
    del keep


def test_locate_shape_bounds_and_stripe_counts(rs):
    """After the verify's checks: the locate's shape bounds, then every stripe's count in stripe
    order -- the first stripe with fewer than two rows is named in err->index, and nothing was
    written (the made-up pointers were never used)."""
    err = rs._RsError()
    e = ctypes.byref(err)
    fake = ctypes.c_void_p(8)
    m, keep = _mask(np.ones((2, 1)))
    assert _locate(rs, fake, 4, 1, 64, 8, 8, m, 8, e) == 101  # recovery_count < 2
    big, keep2 = _mask(np.ones((1, 4)))
    assert _locate(rs, fake, 4097, 4, 64, 8, 8, big, 8, e, stripes=1) == 101  # RS_LOCATE_MAX_ORIGINALS
    assert _locate(rs, fake, 4096, 4097, 64, 8, 8, big, 8, e, stripes=1) == 101  # RS_LOCATE_MAX_COEFFICIENTS
    assert _locate(rs, fake, 4, 1, 64, 8, 8, m, 8, e, stripes=0) == 0  # (stripes == 0 comes first)
    assert _locate(rs, None, 4, 4, 64, 8, 8, big, 0, e, d_located=8) == 101
    assert _locate(rs, fake, 4, 4, 64, 8, 8, big, 8, e, d_located=0) == 101  # null d_located
    masks = np.ones((5, 6), np.uint8)
    masks[3] = [0, 0, 1, 0, 0, 0]  # one row
    masks[4] = 0                   # none
    m5, keep3 = _mask(masks)
    err.index = 99
    assert _locate(rs, fake, 8, 6, 64, 8, 8, m5, 8, e, stripes=5) == 101 and err.code == 101 and err.index == 3
    masks[1, 1:] = 0
    assert _locate(rs, fake, 8, 6, 64, 8, 8, m5, 8, e, stripes=5) == 101 and err.index == 1
    assert _locate(rs, fake, 8, 6, 64, 8, 8, m5, 8, None, stripes=5) == 101
    del keep, keep2, keep3


def test_verify_of_an_all_empty_batch_does_not_touch_the_context(rs):
    """No stripe selects a row: the made-up context is not dereferenced -- all the call does is one
    memset of the flags on the stream (refused here: the flags are host memory, or there is no GPU)."""
    err = rs._RsError()
    fake = ctypes.c_void_p(8)
    flags = (ctypes.c_uint8 * 64)()
    m, keep = _mask(np.zeros((2, 4)))
    st = _verify(rs, fake, 4, 4, 64, 8, 8, m, ctypes.addressof(flags), ctypes.byref(err))
    assert st in (0, 100) and err.code == st
    del keep


def test_wrappers_reject_wrong_shapes(rs):
    N, M, S, B = 8, 6, 64, 3
    ctx = types.SimpleNamespace(handle=None)
    good = lambda: [_Fake(B, N, S), _Fake(B, M, S)]
    ones = np.ones((B, M), np.uint8)

    def verify(t, mask=ones, flags=_Fake(B, M)):
        return rs.verify_device_batch_masks(N, M, S, t[0], t[1], mask, d_mismatch=flags, ctx=ctx)

    def locate(t, mask=ones, located=_Fake(B, dtype="torch.int32"), flags=_Fake(B, M), status=False):
        return rs.locate_device_batch_masks(N, M, S, t[0], t[1], mask, d_located=located, d_mismatch=flags,
                                            status=status, ctx=ctx)

    for fn in (verify, locate):
        for bad in (np.ones(M, np.uint8), np.ones((B + 1, M), np.uint8), np.ones((B, M - 1), np.uint8),
                    np.ones((M, B), np.uint8), [1] * M):
            with pytest.raises(ValueError, match="recovery_rows"):
                fn(good(), mask=bad)
        for k, name in enumerate(("d_original", "d_recovery")):
            t = good()
            t[k] = _Fake((N, M)[k], S)  # a matrix where a batch belongs
            with pytest.raises(ValueError, match=name + ":"):
                fn(t)
            t[k] = _Fake(B + 1, (N, M)[k], S)
            with pytest.raises(ValueError, match="stripe count"):
                fn(t)
        for bad in (_Fake(M), _Fake(B, M + 1), _Fake(B * M), _Fake(B, M, dtype="torch.bool")):
            with pytest.raises(ValueError, match="d_mismatch"):
                fn(good(), flags=bad)
        with pytest.raises(ValueError, match="rs_status 101"):  # well-formed: the library's null-context check
            fn(good())
    for bad in (_Fake(B), _Fake(B + 1, dtype="torch.int32"), _Fake(B, 1, dtype="torch.int32")):
        with pytest.raises(ValueError, match="d_located"):
            locate(good(), located=bad)
    with pytest.raises(ValueError, match="two recovery rows"):
        rs.locate_device_batch_masks(N, 1, S, _Fake(B, N, S), _Fake(B, 1, S), np.ones((B, 1), np.uint8), ctx=ctx)
    with pytest.raises(rs.UnsupportedShardCount):
        rs.verify_device_batch_masks(4096, 61441, S, _Fake(1, 1, S), _Fake(1, 1, S), np.ones((1, 61441), np.uint8),
                                     ctx=ctx)


def test_integration_doc_binds_the_entry_points(tmp_path):
    """The Rust prototypes of INTEGRATION.md compile against the header, and the ctypes lines name
    both calls."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    types_ = dict(ABI.TYPES, **{"*mut i32": "int32_t *"})  # (as tests/test_locate_cpu.py: d_located)
    src = ["#include <stddef.h>", "#include <stdint.h>", f'#include "{HEADER}"', ""]
    for name in NAMES:
        m = re.search(r"fn\s+%s\s*\((.*?)\)\s*->\s*RsStatus;" % name, doc, flags=re.S)
        assert m, name
        params = []
        for a in filter(None, (x.strip() for x in " ".join(m.group(1).split()).split(","))):
            pname, ptype = (x.strip() for x in a.split(":", 1))
            params.append(f"{types_[ptype]} {pname}")
        assert "const uint8_t * recovery_check" in params and "uint8_t * d_mismatch" in params
        if name == NAMES[1]:
            assert "uint8_t * stripe_status" in params and "int32_t * d_located" in params
        src.append(f"rs_status {name}({', '.join(params)});")
        assert re.search(r"lib\.%s\b" % name, doc), name
    assert "RS_LOCATE_SKIPPED" in doc
    c = tmp_path / "masks.c"
    c.write_text("\n".join(src) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-c", str(c), "-o", str(tmp_path / "m.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_mask_sets_hold_what_the_issue_asks_for():
    for M in (5, 70, 100, 200, 1024, 4096):
        v = C.verify_masks(M)
        assert 5 <= len(v) <= 8
        assert v[0].all() and v[1].tolist() == [1] + [0] * (M - 1) and v[2].tolist() == [0] * (M - 1) + [1]
        assert np.flatnonzero(v[3]).tolist() == [0, M - 1]
        assert not v[4][1::3].any() and v[4].sum() == M - len(range(1, M, 3))
        assert not v[5].any()
        assert np.flatnonzero(v[6])[0] == 2 and np.flatnonzero(v.any(axis=0))[0] == 0
        l = C.locate_masks(M)
        assert 5 <= len(l) <= 8
        assert [int(r.sum() >= 2) for r in l] == [1, 0, 0, 1, 1, 1, 1, 1]  # stripes 1 and 2: one row, skipped


@pytest.mark.parametrize("rate,N,M,S,pad", C.FUSED + C.UNFUSED, ids=lambda v: str(v))
def test_model_gives_the_intended_outcome(rate, N, M, S, pad):
    """locate_model.locate per stripe, each with its own mask: the located word is the one the
    batch was built for and the flags are the constructed ones; for the verify's batch the model's
    flags are want[b] * mask[b]."""
    import locate_model as LM

    _, _, store, held, masks, intent, want = C.locate_batch(rate, N, M, S)
    assert sorted(set(intent.tolist())) == sorted({C.CLEAN, C.ROWS, C.UNKNOWN, C.SKIPPED, 0, N // 2, N - 1})
    for b in range(len(masks)):
        if intent[b] == C.SKIPPED:
            assert masks[b].sum() < 2 and not want[b].any()
            continue
        loc, flags = LM.locate(rate, store[b], held[b], masks[b])
        assert loc == intent[b], (b, loc, int(intent[b]))
        assert np.array_equal(flags, want[b]), b
    _, _, store, held, masks, want = C.verify_batch(rate, N, M, S)
    for b in range(len(masks)):
        truth = (LM.O.encode(rate, store[b], M) != held[b]).any(axis=1)
        assert np.array_equal(want[b], truth * masks[b]), b
        assert truth[masks[b] == 0].all(), b  # the junk differs
