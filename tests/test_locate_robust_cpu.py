"""rs_locate_device_robust* without a GPU: the symbols and their declarations, the argument checks
(all before any device work, in the header's order), the no-op case, the Python wrappers' argument
checks, the INTEGRATION.md binding, and the contract on the CPU oracle alone
(tests/locate_robust_model.py): the brute force over every original and every reference row against
the prefiltered form, on every constructed case of tests/locate_robust_cases.py.
"""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import locate_model as LM
import locate_robust_cases as RC
import locate_robust_model as RM
import test_integration_abi as ABI
from test_verify_cpu import _Fake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rs_locate_device_robust", "rs_locate_device_robust_batch")
HEADER = os.path.join(ROOT, "include", "rs_mi355x.h")


@pytest.fixture(scope="module")
def rs():
    # (imported by the tests that use it, not while pytest collects: tests/test_batch_masks_cpu.py)
    import reed_solomon_simd
    return reed_solomon_simd


def _single(rs, ctx, N, M, S, d_orig, d_rec, mask, t, d_loc, d_flags, d_out, err=None, strides=(0, 0), stripes=None):
    return rs._lib.rs_locate_device_robust(ctx, 0, N, M, S, d_orig, strides[0], d_rec, strides[1], mask, t, d_loc,
                                           d_flags, d_out, None, err)


def _batch(rs, ctx, N, M, S, d_orig, d_rec, mask, t, d_loc, d_flags, d_out, err=None, strides=(0, 0), stripes=2):
    return rs._lib.rs_locate_device_robust_batch(ctx, 0, N, M, S, stripes, d_orig, strides[0], 0, d_rec, strides[1], 0,
                                                 mask, t, d_loc, d_flags, d_out, None, err)


FORMS = [_single, _batch]


def test_symbols_are_exported_and_declared(rs):
    header = open(HEADER).read()
    for name in NAMES:
        assert hasattr(rs._lib, name), name
        assert getattr(rs._lib, name).argtypes is not None, name
        proto = re.search(r"rs_status\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert proto, name
        assert re.search(r"const void \*d_original.*const void \*d_recovery.*const uint8_t \*recovery_check,\s*"
                         r"uint32_t max_outliers,\s*int32_t \*d_located,\s*uint8_t \*d_mismatch,\s*"
                         r"uint8_t \*d_outlier,\s*void \*stream,\s*rs_error \*err", proto.group(1), re.S), name
    batch = re.search(r"rs_locate_device_robust_batch\s*\(([^;]*)\)", header).group(1)
    for arg in ("uint64_t stripes", "original_stripe_stride", "recovery_stripe_stride"):
        assert arg in batch, arg
    # the locate's arguments with two more
    assert len(rs._lib.rs_locate_device_robust.argtypes) == len(rs._lib.rs_locate_device.argtypes) + 2 == 16
    assert len(rs._lib.rs_locate_device_robust_batch.argtypes) == len(rs._lib.rs_locate_device_batch.argtypes) + 2 == 19
    for k, base in ((10, rs._lib.rs_locate_device_robust), (13, rs._lib.rs_locate_device_robust_batch)):
        assert base.argtypes[k] is ctypes.c_uint32
    for name in ("locate_device_robust", "locate_device_robust_batch"):
        assert callable(getattr(rs, name)), name
    m = re.search(r"#define RS_LOCATE_MAX_OUTLIERS (\d+)u", header)
    assert m and int(m.group(1)) == 7 == rs.LOCATE_MAX_OUTLIERS == RM.MAX_OUTLIERS
    # the contract and its three facts, in the header's words
    for phrase in ("every byte of d_mismatch, every word of d_located and", "every byte of d_outlier is defined",
                   "exactly what\n * rs_verify_device_batch writes", "1. Uniqueness.", "2. Trust.", "3. Compatibility.",
                   "s + 1 + t <= c", "Nothing is written but the three outputs", "ITS OWN reference row",
                   "writing the correction in place (a robust heal)"):
        assert phrase in header, phrase
    # ... and the plain locate no longer lists the case as not covered
    plain = header[header.index("---- locate: which original"):header.index("---- robust locate")]
    assert "Not covered:" in plain and "majority logic" not in plain


@pytest.mark.parametrize("call", FORMS)
def test_argument_checks_precede_any_device_work(rs, call):
    """A made-up non-null context is never dereferenced: every check comes first, in the
    header's order."""
    err = rs._RsError()
    e = ctypes.byref(err)
    fake = ctypes.c_void_p(8)
    # 1. the locate's checks, d_outlier among the null pointers
    assert call(rs, None, 4, 4, 64, 8, 8, None, 1, 8, 8, 8, e) == 101 and err.code == 101
    for k in range(5):
        p = [8] * 5
        p[k] = 0
        assert call(rs, fake, 4, 4, 64, p[0], p[1], None, 1, p[2], p[3], p[4], e) == 101, k
    err.code = 0  # ... ahead of rs_validate (a bad shard size here)
    assert call(rs, fake, 4, 4, 63, 8, 8, None, 1, 8, 8, 0, e) == 101 and err.code == 101
    # rs_validate ahead of the strides, the row counts and the shape bound (all bad here)
    assert call(rs, fake, 4, 1, 63, 8, 8, None, 9, 8, 8, 8, e, strides=(32, 0)) == 6 and err.shard_bytes == 63
    assert call(rs, fake, 4096, 61441, 64, 8, 8, bytes(61441), 9, 8, 8, 8, e, strides=(0, 32)) == 10
    assert (err.original_count, err.recovery_count) == (4096, 61441)
    # the two row strides ahead of the row count
    for strides in ((32, 0), (0, 32)):
        assert call(rs, fake, 4, 4, 64, 8, 8, None, 1, 8, 8, 8, e, strides=strides) == 101 and err.code == 101
        assert call(rs, fake, 4, 1, 64, 8, 8, None, 0, 8, 8, 8, e, strides=strides) == 101
    # fewer than two rows, whatever max_outliers
    assert call(rs, fake, 4, 1, 64, 8, 8, None, 0, 8, 8, 8, e) == 101
    assert call(rs, fake, 4, 4, 64, 8, 8, b"\0\1\0\0", 0, 8, 8, 8, e) == 101
    assert call(rs, fake, 4, 4, 64, 8, 8, bytes(4), 0, 8, 8, 8, e) == 101
    # 2. max_outliers > 7, or 2 (1 + max_outliers) > c -- ahead of the shape bound
    assert call(rs, fake, 4, 100, 64, 8, 8, None, 8, 8, 8, 8, e) == 101 and err.code == 101
    assert call(rs, fake, 4, 100, 64, 8, 8, None, 0xFFFFFFFF, 8, 8, 8, e) == 101
    assert call(rs, fake, 4, 4, 64, 8, 8, None, 2, 8, 8, 8, e) == 101  # 6 > 4
    assert call(rs, fake, 4, 15, 64, 8, 8, None, 7, 8, 8, 8, e) == 101  # 16 > 15
    assert call(rs, fake, 4, 6, 64, 8, 8, b"\1\1\0\1\0\0", 1, 8, 8, 8, e) == 101  # 4 > 3 selected
    assert call(rs, fake, 5000, 3, 64, 8, 8, None, 1, 8, 8, 8, e) == 101
    # 3. the locate's shape bound
    assert call(rs, fake, 4097, 4, 64, 8, 8, None, 1, 8, 8, 8, e) == 101 and err.code == 101
    assert call(rs, fake, 4096, 4097, 64, 8, 8, None, 1, 8, 8, 8, e) == 101
    # all of them with no stripes at all, too
    assert _batch(rs, fake, 4, 4, 64, 8, 8, None, 1, 8, 8, 8, e, strides=(0, 63), stripes=0) == 101
    assert _batch(rs, fake, 4, 4, 64, 8, 8, None, 2, 8, 8, 8, e, stripes=0) == 101
    assert _batch(rs, fake, 4097, 4, 64, 8, 8, None, 1, 8, 8, 8, e, stripes=0) == 101
    # a null err is allowed
    assert call(rs, fake, 4, 4, 64, 8, 8, None, 2, 8, 8, 8, None) == 101
    assert call(rs, None, 4, 4, 64, 8, 8, None, 1, 8, 8, 8, None) == 101


def test_no_stripes_is_ok_without_touching_anything(rs):
    err = rs._RsError()
    err.code = 55
    fake = ctypes.c_void_p(8)
    assert _batch(rs, fake, 4, 4, 64, 8, 8, None, 1, 8, 8, 8, ctypes.byref(err), stripes=0) == 0 and err.code == 0
    assert _batch(rs, fake, 4, 4, 64, 8, 8, b"\1\0\0\1", 0, 8, 8, 8, None, strides=(64, 128), stripes=0) == 0
    # the bounds themselves pass: 2 (1 + t) = c, t = 7, the largest shapes
    assert _batch(rs, fake, 4, 16, 64, 8, 8, None, 7, 8, 8, 8, None, stripes=0) == 0
    assert _batch(rs, fake, 4, 6, 64, 8, 8, b"\1\1\0\1\0\1", 1, 8, 8, 8, None, stripes=0) == 0
    assert _batch(rs, fake, 4096, 4096, 64, 8, 8, None, 7, 8, 8, 8, None, stripes=0) == 0


def test_wrappers_reject_wrong_arguments(rs):
    N, M, S, B = 8, 6, 64, 3
    ctx = types.SimpleNamespace(handle=None)
    loc = lambda *shape, **kw: _Fake(*shape, **dict({"dtype": "torch.int32"}, **kw))

    def single(t=1, mask=None, o=_Fake(N, S), r=_Fake(M, S), located=loc(1), flags=_Fake(M), outlier=_Fake(M)):
        return rs.locate_device_robust(N, M, S, o, r, recovery_rows=mask, max_outliers=t, d_located=located,
                                       d_mismatch=flags, d_outlier=outlier, ctx=ctx)

    # max_outliers outside the bound: above 7, negative, more than the selected rows allow
    for t in (8, -1, 1 << 32):
        with pytest.raises(ValueError, match="max_outliers: 0 .. 7"):
            single(t=t)
    with pytest.raises(ValueError, match="max_outliers: 3 outliers need 8 selected"):
        single(t=3)
    with pytest.raises(ValueError, match="max_outliers: 2 outliers need 6 selected"):
        single(t=2, mask=[1, 1, 1, 0, 1, 1])
    with pytest.raises(ValueError, match="recovery_rows: a locate needs two"):
        single(t=0, mask=[0, 0, 1, 0, 0, 0])
    with pytest.raises(ValueError, match="recovery_rows"):
        single(mask=[1] * (M + 1))
    # the matrices and the locate's two outputs, as locate_device
    with pytest.raises(ValueError, match="d_original:"):
        single(o=_Fake(N - 1, S))
    with pytest.raises(ValueError, match="d_recovery: dtype"):
        single(r=_Fake(M, S, dtype="torch.int32"))
    with pytest.raises(ValueError, match="d_located"):
        single(located=loc(2))
    with pytest.raises(ValueError, match="d_mismatch"):
        single(flags=_Fake(M + 1))
    # the outlier bytes: one per recovery row, uint8, contiguous
    for bad in (_Fake(M - 1), _Fake(M + 1), _Fake(1, M), _Fake(M, dtype="torch.bool"), _Fake(M, contiguous=False)):
        with pytest.raises(ValueError, match="d_outlier"):
            single(outlier=bad)
    with pytest.raises(ValueError, match="d_located"):  # raw pointers: nothing says where to allocate
        rs.locate_device_robust(N, M, S, 8, 8, ctx=ctx)
    with pytest.raises(ValueError, match="d_outlier"):
        rs.locate_device_robust(N, M, S, 8, 8, d_located=8, d_mismatch=8, ctx=ctx)
    with pytest.raises(rs.UnsupportedShardCount):  # the reference's own checks come first
        rs.locate_device_robust(4096, 61441, S, _Fake(1, S), _Fake(1, S), max_outliers=9, ctx=ctx)
    # well-formed arguments reach the library (whose first check refuses the null context)
    for kw in ({}, {"t": 0}, {"t": 2}, {"t": 1, "mask": [1, 0, 1, 1, 0, 1]}):
        with pytest.raises(ValueError, match="rs_status 101"):
            single(**kw)
    with pytest.raises(ValueError, match="rs_status 101"):
        rs.locate_device_robust(N, M, S, 8, 8, d_located=8, d_mismatch=8, d_outlier=8, ctx=ctx)

    def batch(t=1, o=_Fake(B, N, S), r=_Fake(B, M, S), located=loc(B), flags=_Fake(B, M), outlier=_Fake(B, M)):
        return rs.locate_device_robust_batch(N, M, S, o, r, max_outliers=t, d_located=located, d_mismatch=flags,
                                             d_outlier=outlier, ctx=ctx)

    with pytest.raises(ValueError, match="max_outliers"):
        batch(t=3)
    with pytest.raises(ValueError, match="d_recovery:"):
        batch(r=_Fake(M, S))
    with pytest.raises(ValueError, match="stripe count"):
        batch(o=_Fake(B + 1, N, S))
    for bad in (_Fake(M), _Fake(B, M + 1), _Fake(B + 1, M), _Fake(B * M)):
        with pytest.raises(ValueError, match="d_outlier"):
            batch(outlier=bad)
    with pytest.raises(ValueError, match="rs_status 101"):
        batch()


def test_integration_doc_binds_the_entry_points(tmp_path):
    """The Rust and ctypes lines of INTEGRATION.md name the two calls, and the Rust prototypes
    compile as redeclarations against the header."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    types_ = dict(ABI.TYPES, **{"*mut i32": "int32_t *"})
    protos = []
    for name in NAMES:
        m = re.search(r"fn\s+%s\s*\((.*?)\)\s*->\s*RsStatus;" % name, doc, flags=re.S)
        assert m, name
        params = []
        for a in filter(None, (x.strip() for x in " ".join(m.group(1).split()).split(","))):
            pname, ptype = (x.strip() for x in a.split(":", 1))
            params.append(f"{types_[ptype]} {pname}")
        for p in ("int32_t * d_located", "uint32_t max_outliers", "uint8_t * d_outlier"):
            assert p in params, (name, p)
        protos.append(f"rs_status {name}({', '.join(params)});")
        assert re.search(r'_sig\("%s"|lib\.%s\b' % (name, name), doc), name  # the ctypes side
    c = tmp_path / "locate_robust_bindings.c"
    c.write_text("\n".join(["#include <stdint.h>", f'#include "{HEADER}"'] + protos) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-c", str(c), "-o", str(tmp_path / "l.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + "\n" + c.read_text()
    scrub = doc[doc.index("rs.locate_device_robust_batch("):]
    assert "repair_device_batch_masks(" in scrub[:1200] and "outlier" in scrub[:1200]


def test_docs_describe_the_call():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.4g Robust locate"):]
    for phrase in ("Uniqueness", "Trust", "Compatibility", "k_locate_find_pairs", "k_locate_count", "k_locate_decide",
                   "VGPR"):
        assert phrase in section, phrase
    plain = design[design.index("### 4.4e Locate"):design.index("### 4.4f Heal")]
    assert "majority logic" not in plain
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "rs_locate_device_robust" in readme and "test_gpu_locate_robust.py" in readme


# ---------------------------------------------------------------------------
# the contract, on the CPU oracle alone

SHAPES = [("high", 70, 100, 64), ("low", 100, 70, 66), ("default", 128, 128, 64)]


@pytest.mark.parametrize("rate,N,M,S", SHAPES, ids=lambda v: str(v))
def test_direct_and_fast_models_agree(rate, N, M, S):
    """On every constructed case, at t = 0, 1, 2 each: the brute force over every original and
    every selected reference row finds at most one original (and one outlier set), and the
    prefiltered model returns the same three results; the intended status of each case holds."""
    located = 0
    for case in RC.cases(rate, N, M, S, ts=(1, 2)):
        name, _, orig, rec, enc, _ = case
        RC.model(rate, case)  # the intended status, at the case's own t
        D = LM.elements(enc ^ rec).astype(np.int64)
        bads = RM.disagreements(LM.coefficients(rate, N, M), D, np.arange(M)) if D.any(axis=1).all() else None
        for t in (0, 1, 2):
            want, flags, outlier, found = RM.locate_direct(rate, orig, rec, t, D=D, bads=bads)
            assert len({i for i, _ in found}) <= 1 and len(found) <= 1, (name, t, found)
            got = RM.locate(rate, orig, rec, t, D=D)
            assert got[0] == want and np.array_equal(got[1], flags) and np.array_equal(got[2], outlier), (name, t)
            assert int(outlier.sum()) <= t and (want >= 0 or not outlier.any()), (name, t)
            if t == 0:
                assert want == LM.locate(rate, orig, rec, D=D)[0], name
            located += want >= 0
    assert located > 50  # the cases do exercise the located outcome


@pytest.mark.parametrize("rate,N,M,S", SHAPES[:2], ids=lambda v: str(v))
def test_models_agree_under_a_mask_and_on_random_outliers(rate, N, M, S):
    """Every third row unselected with junk in it, and outliers at random selected rows: t outliers
    are named, t + 1 give no explanation."""
    mask = np.ones(M, np.uint8)
    mask[2::3] = 0
    for case in RC.cases(rate, N, M, S, mask=mask, forms=("bit0",), ts=(1, 2), junk=True):
        name, t, orig, rec, enc, _ = case
        got = RC.model(rate, case, mask=mask)
        want = RM.locate_direct(rate, orig, rec, t, mask=mask, D=LM.elements(enc ^ rec).astype(np.int64))
        assert got[0] == want[0] and np.array_equal(got[2], want[2]) and len(want[3]) <= 1, name
        assert not got[2][mask == 0].any(), name
    orig, rec = RC.V.stripe(rate, N, M, S)
    rng = np.random.default_rng(N)
    bad = orig.copy()
    bad[N // 3, 9] ^= 0x21
    enc = RC.encoded((rate, N, M, S, "random"), bad, rate, M)
    for t in (1, 2):
        for n in (t, t + 1):
            rows = np.sort(rng.choice(M, n, replace=False))
            r = rec.copy()
            r[rows, rng.integers(0, S, n)] ^= 0x04
            D = LM.elements(enc ^ r).astype(np.int64)
            got, want = RM.locate(rate, bad, r, t, D=D), RM.locate_direct(rate, bad, r, t, D=D)
            assert got[0] == want[0] == (N // 3 if n == t else RM.UNKNOWN), (t, rows)
            assert np.flatnonzero(got[2]).tolist() == np.flatnonzero(want[2]).tolist() == (rows.tolist() if n == t else [])
