"""rs_locate_device_degraded* without a GPU: the symbols and their declarations, the argument
checks (all of which come before any device work, in the header's order), the no-op case, the
Python wrappers' argument checks, the INTEGRATION.md binding, and the algebra the call rests on,
on the CPU oracle alone (tests/locate_degraded_model.py):

    D_j = recovery_j ^ encode(F)_j = T[j][p] * e   for one corrupt information shard p,

with F the originals completed from the reference rows R, j over the check rows K and T the
coefficient matrix over the information set (the present originals and the rows of R).
"""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import locate_degraded_model as DM
import locate_model as LM
import oracle_lib as O
import test_integration_abi as ABI
from test_verify_cpu import _Fake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rs_locate_device_degraded", "rs_locate_device_degraded_batch")
HEADER = os.path.join(ROOT, "include", "rs_mi355x.h")


@pytest.fixture(scope="module")
def rs():
    # (imported by the tests that use it, not while pytest collects: tests/test_batch_masks_cpu.py)
    import reed_solomon_simd
    return reed_solomon_simd


@pytest.fixture(scope="module", autouse=True)
def the_call_exists(rs):
    """Every test here states the contract of the two entry points, the model-only ones included:
    without the calls they have nothing to state."""
    for name in NAMES:
        assert hasattr(rs._lib, name), name


def _single(rs, ctx, N, M, S, d_orig, present, d_rec, mask, d_loc, d_flags, err=None, strides=(0, 0, 0), restored=0,
            stripes=None):
    return rs._lib.rs_locate_device_degraded(ctx, 0, N, M, S, d_orig, strides[0], present, d_rec, strides[1], mask,
                                             restored, strides[2], d_loc, d_flags, None, err)


def _batch(rs, ctx, N, M, S, d_orig, present, d_rec, mask, d_loc, d_flags, err=None, strides=(0, 0, 0), restored=0,
           stripes=2):
    return rs._lib.rs_locate_device_degraded_batch(ctx, 0, N, M, S, stripes, d_orig, strides[0], 0, present, d_rec,
                                                   strides[1], 0, mask, restored, strides[2], 0, d_loc, d_flags,
                                                   None, err)


FORMS = [_single, _batch]


def test_symbols_are_exported_and_declared(rs):
    header = open(HEADER).read()
    for name in NAMES:
        assert hasattr(rs._lib, name), name
        assert getattr(rs._lib, name).argtypes is not None, name  # the ctypes signature is declared
        proto = re.search(r"rs_status\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert proto, name
        assert re.search(r"const void \*d_original.*const uint8_t \*original_present.*const void \*d_recovery.*"
                         r"const uint8_t \*recovery_check,\s*void \*d_restored,\s*uint64_t restored_stride.*"
                         r"int32_t \*d_located,\s*uint8_t \*d_mismatch,\s*void \*stream,\s*rs_error \*err",
                         proto.group(1), re.S), name
    batch = re.search(r"rs_locate_device_degraded_batch\s*\(([^;]*)\)", header).group(1)
    for arg in ("uint64_t stripes", "original_stripe_stride", "recovery_stripe_stride", "restored_stripe_stride"):
        assert arg in batch, arg
    assert len(rs._lib.rs_locate_device_degraded.argtypes) == 17
    assert len(rs._lib.rs_locate_device_degraded_batch.argtypes) == 21
    for name in ("locate_device_degraded", "locate_device_degraded_batch"):
        assert callable(getattr(rs, name)), name
    # what the contract promises and what it does not, in the header's words
    section = header[header.index("---- degraded locate"):header.index("rs_status rs_locate_device_degraded(")]
    section = re.sub(r"\s*\n \*\s*", " ", section)
    for phrase in ("every byte of d_mismatch and every word of d_located", "NOT proven", "|K| - 1", "Select three check rows",
                   "Nothing is written but d_located", "byte-identical to rs_decode_device_batch",
                   "present rows are never written", "RS_ERR_NOT_ENOUGH_SHARDS", "k_locate_rename",
                   "k_coef_unit_degraded", "a degraded heal", "max_outliers", "a mask per stripe"):
        assert phrase in section, phrase
    # the four "Not covered" lists that name "stripes with missing originals" point here
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    assert flat.count("stripes with missing originals") == 4
    assert len(re.findall(r"stripes with missing originals \(rs_locate_device_degraded (?:above|below) locates in "
                          r"those\)", flat)) == 4


@pytest.mark.parametrize("call", FORMS)
def test_argument_checks_precede_any_device_work(rs, call):
    """A made-up non-null context is never dereferenced: every check comes first, in the
    header's order."""
    err = rs._RsError()
    e = ctypes.byref(err)
    fake = ctypes.c_void_p(8)
    p4, one = b"\1\1\1\1", b"\0\1\1\1"
    # 1. null context, d_original, original_present, d_recovery, d_located, d_mismatch
    assert call(rs, None, 4, 4, 64, 8, p4, 8, None, 8, 8, e) == 101 and err.code == 101
    assert call(rs, fake, 4, 4, 64, 0, p4, 8, None, 8, 8, e) == 101
    assert call(rs, fake, 4, 4, 64, 8, None, 8, None, 8, 8, e) == 101
    assert call(rs, fake, 4, 4, 64, 8, p4, 0, None, 8, 8, e) == 101
    assert call(rs, fake, 4, 4, 64, 8, p4, 8, None, 0, 8, e) == 101
    assert call(rs, fake, 4, 4, 64, 8, p4, 8, None, 8, 0, e) == 101
    # ... ahead of rs_validate (a bad shard size here)
    err.code = 0
    assert call(rs, fake, 4, 4, 63, 8, None, 8, None, 8, 8, e) == 101 and err.code == 101
    # 2. rs_validate: a bad shard size, an unsupported count -- ahead of the strides, the row
    # counts and the shape bound (all bad here)
    assert call(rs, fake, 4, 1, 63, 8, bytes(4), 8, None, 8, 8, e, strides=(32, 0, 0)) == 6 and err.shard_bytes == 63
    assert call(rs, fake, 4096, 61441, 64, 8, bytes(4096), 8, bytes(61441), 8, 8, e, strides=(0, 32, 0)) == 10
    assert (err.original_count, err.recovery_count) == (4096, 61441)
    # 3. the row strides, each in turn -- ahead of the row counts (nothing selected here);
    # restored_stride only when d_restored is given
    for strides in ((32, 0, 0), (0, 32, 0)):
        assert call(rs, fake, 4, 4, 64, 8, bytes(4), 8, bytes(4), 8, 8, e, strides=strides) == 101, strides
        assert err.code == 101
    assert call(rs, fake, 4, 4, 64, 8, bytes(4), 8, bytes(4), 8, 8, e, strides=(0, 0, 32), restored=8) == 101
    assert err.code == 101
    assert call(rs, fake, 4, 4, 64, 8, bytes(4), 8, bytes(4), 8, 8, e, strides=(0, 0, 32)) == 7  # (NULL: not read)
    # 4. c < m: not decodable, with the decode's counts
    err.code = 0
    assert call(rs, fake, 4, 4, 64, 8, b"\0\0\0\1", 8, b"\0\1\0\0", 8, 8, e) == 7 and err.code == 7
    assert (err.original_count, err.original_received_count, err.recovery_received_count) == (4, 1, 1)
    assert call(rs, fake, 6, 4, 64, 8, b"\0\0\0\0\0\1", 8, None, 8, 8, e) == 7
    assert (err.original_count, err.original_received_count, err.recovery_received_count) == (6, 1, 4)
    assert call(rs, fake, 5000, 1, 64, 8, bytes(5000), 8, None, 8, 8, e) == 7  # (... ahead of the shape bound)
    # 5. decodable, but fewer than two check rows: c = m and c = m + 1
    assert call(rs, fake, 4, 4, 64, 8, one, 8, b"\0\1\0\0", 8, 8, e) == 101 and err.code == 101  # c = m = 1
    assert call(rs, fake, 4, 4, 64, 8, one, 8, b"\0\1\0\1", 8, 8, e) == 101  # c = m + 1
    assert _batch(rs, fake, 4, 4, 64, 8, b"\0\0\1\1", 8, None, 8, 8, e, stripes=0) == 0  # c = m + 2: accepted
    assert call(rs, fake, 4, 4, 64, 8, b"\0\0\0\1", 8, None, 8, 8, e) == 101  # m = 3, c = 4
    assert call(rs, fake, 4, 4, 64, 8, bytes(4), 8, None, 8, 8, e) == 101  # m = c = 4
    assert call(rs, fake, 4, 4, 64, 8, p4, 8, b"\0\1\0\0", 8, 8, e) == 101  # m = 0: the locate's two rows
    assert call(rs, fake, 4, 1, 64, 8, p4, 8, None, 8, 8, e) == 101
    assert call(rs, fake, 5000, 3, 64, 8, b"\0" + b"\1" * 4999, 8, b"\1\1\0", 8, 8, e) == 101  # (ahead of the bound)
    # 6. the locate's shape bound
    assert call(rs, fake, 4097, 3, 64, 8, b"\0" + b"\1" * 4096, 8, None, 8, 8, e) == 101 and err.code == 101
    assert call(rs, fake, 4096, 4097, 64, 8, b"\0" + b"\1" * 4095, 8, None, 8, 8, e) == 101
    # all of them with no stripes at all, too
    assert _batch(rs, fake, 4, 4, 64, 8, one, 8, None, 8, 8, e, strides=(0, 63, 0), stripes=0) == 101
    assert _batch(rs, fake, 4, 4, 64, 8, one, 8, b"\0\0\0\1", 8, 8, e, stripes=0) == 101
    assert _batch(rs, fake, 4, 4, 64, 8, bytes(4), 8, b"\0\1\1\1", 8, 8, e, stripes=0) == 7
    assert _batch(rs, fake, 4097, 4, 64, 8, b"\0" + b"\1" * 4096, 8, None, 8, 8, e, stripes=0) == 101
    # a null err is allowed
    assert call(rs, fake, 4, 4, 64, 8, one, 8, None, 8, 8, None, strides=(0, 32, 0)) == 101
    assert call(rs, fake, 4, 4, 64, 8, bytes(4), 8, b"\0\1\1\1", 8, 8, None) == 7
    assert call(rs, None, 4, 4, 64, 8, one, 8, None, 8, 8, None) == 101


def test_no_stripes_is_ok_without_touching_anything(rs):
    err = rs._RsError()
    err.code = 55
    fake = ctypes.c_void_p(8)
    one = b"\0\1\1\1"
    assert _batch(rs, fake, 4, 4, 64, 8, one, 8, None, 8, 8, ctypes.byref(err), stripes=0) == 0 and err.code == 0
    assert _batch(rs, fake, 4, 4, 64, 8, one, 8, b"\1\1\0\1", 8, 8, None, strides=(64, 128, 192), restored=8,
                  stripes=0) == 0
    assert _batch(rs, fake, 4, 4, 64, 8, b"\1\1\1\1", 8, None, 8, 8, None, stripes=0) == 0  # m = 0
    # the largest shapes inside the bound pass the checks
    assert _batch(rs, fake, 4096, 4096, 64, 8, bytes(4094) + b"\1\1", 8, None, 8, 8, None, stripes=0) == 0
    assert _batch(rs, fake, 256, 65280, 64, 8, b"\0" + b"\1" * 255, 8, None, 8, 8, None, stripes=0) == 0


def test_wrappers_reject_wrong_shapes_dtypes_and_masks(rs):
    N, M, S, B = 8, 6, 64, 3
    ctx = types.SimpleNamespace(handle=None)
    names = ["d_original", "d_recovery", "d_restored"]
    rows = [N, M, N]
    good = lambda: [_Fake(N, S), _Fake(M, S), _Fake(N, S)]
    loc = lambda *shape, **kw: _Fake(*shape, **dict({"dtype": "torch.int32"}, **kw))
    present = [1, 0, 1, 1, 0, 1, 1, 1]  # m = 2

    def single(t, present=present, mask=None, located=loc(1), flags=_Fake(M)):
        return rs.locate_device_degraded(N, M, S, t[0], present, t[1], recovery_rows=mask, d_restored=t[2],
                                         d_located=located, d_mismatch=flags, ctx=ctx)

    for k in range(3):
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
        single(good(), present=[1] * (N + 1))
    with pytest.raises(ValueError, match="original_present"):
        single(good(), present=[1] * (N - 1))
    with pytest.raises(ValueError, match="recovery_rows"):
        single(good(), mask=[1] * (M + 1))
    # c = m and c = m + 1: decodable, nothing (or one row) left to check with
    for few in ([1, 1, 0, 0, 0, 0], [0, 1, 0, 1, 0, 1]):
        with pytest.raises(ValueError, match="recovery_rows: 2 missing originals"):
            single(good(), mask=few)
    with pytest.raises(ValueError, match="recovery_rows: 5 missing"):
        single(good(), present=[0, 0, 0, 0, 0, 1, 1, 1])  # m = 5, c = M = 6
    with pytest.raises(ValueError, match="recovery_rows: 0 missing"):
        single(good(), present=[1] * N, mask=[0, 0, 1, 0, 0, 0])  # m = 0: the locate's two rows
    # c < m is the library's NotEnoughShards with its counts (tests/test_gpu_locate_degraded.py): the
    # wrapper passes it on, and here the library's first check refuses the null context
    with pytest.raises(ValueError, match="rs_status 101"):
        single(good(), mask=[0, 0, 1, 0, 0, 0])
    # the result: exactly one int32 per stripe, contiguous; the flags as the verify's
    for bad in (loc(2), loc(1, 1), _Fake(1), loc(1, dtype="torch.int64"), loc(1, contiguous=False)):
        with pytest.raises(ValueError, match="d_located"):
            single(good(), located=bad)
    for bad in (_Fake(M - 1), _Fake(M + 1), _Fake(1, M), _Fake(M, dtype="torch.bool"), _Fake(M, contiguous=False)):
        with pytest.raises(ValueError, match="d_mismatch"):
            single(good(), flags=bad)
    with pytest.raises(ValueError, match="d_located"):  # raw pointers: nothing says where to allocate
        rs.locate_device_degraded(N, M, S, 8, present, 8, ctx=ctx)
    with pytest.raises(rs.UnsupportedShardCount):  # the reference's own checks come first
        rs.locate_device_degraded(4096, 61441, S, _Fake(1, S), [1], _Fake(1, S), d_located=loc(1),
                                  d_mismatch=_Fake(1), ctx=ctx)
    # well-formed arguments reach the library (whose first check refuses the null context)
    with pytest.raises(ValueError, match="rs_status 101"):
        single(good())
    with pytest.raises(ValueError, match="rs_status 101"):
        single(good(), mask=[1, 0, 1, 1, 1, 0])
    t = good()
    t[2] = None  # no d_restored
    with pytest.raises(ValueError, match="rs_status 101"):
        single(t)
    with pytest.raises(ValueError, match="rs_status 101"):
        rs.locate_device_degraded(N, M, S, 8, present, 8, d_located=8, d_mismatch=8, ctx=ctx)  # raw pointers

    goodb = lambda: [_Fake(B, N, S), _Fake(B, M, S), _Fake(B, N, S)]

    def batch(t, present=present, mask=None, located=loc(B), flags=_Fake(B, M)):
        return rs.locate_device_degraded_batch(N, M, S, t[0], present, t[1], recovery_rows=mask, d_restored=t[2],
                                               d_located=located, d_mismatch=flags, ctx=ctx)

    for k in range(3):
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
    with pytest.raises(ValueError, match="original_present"):
        batch(goodb(), present=np.ones((B, N), np.uint8))
    with pytest.raises(ValueError, match="recovery_rows: 2 missing originals"):
        batch(goodb(), mask=[1, 1, 1, 0, 0, 0])
    for bad in (loc(1), loc(B + 1), loc(B, 1), _Fake(B)):
        with pytest.raises(ValueError, match="d_located"):
            batch(goodb(), located=bad)
    for bad in (_Fake(M), _Fake(B, M + 1), _Fake(B + 1, M), _Fake(B * M)):
        with pytest.raises(ValueError, match="d_mismatch"):
            batch(goodb(), flags=bad)
    with pytest.raises(ValueError, match="rs_status 101"):
        batch(goodb())


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
        for want in ("int32_t * d_located", "const uint8_t * recovery_check", "const uint8_t * original_present",
                     "void * d_restored"):
            assert want in params, want
        protos.append(f"rs_status {name}({', '.join(params)});")
        assert re.search(r'_sig\("%s"|lib\.%s\b' % (name, name), doc), name  # the ctypes side
    c = tmp_path / "locate_degraded_bindings.c"
    c.write_text("\n".join(["#include <stdint.h>", f'#include "{HEADER}"'] + protos) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-c", str(c), "-o", str(tmp_path / "l.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + "\n" + c.read_text()


# ---------------------------------------------------------------------------
# the algebra, on the CPU oracle alone

# 70:100 and 100:70 under both rates, 128:128, 3:5
SHAPES = [("high", 70, 100), ("low", 70, 100), ("high", 100, 70), ("low", 100, 70), ("default", 128, 128),
          ("default", 3, 5)]


def _missing_counts(N, M):
    """m in {1, 3, M - 2}; M - 2 leaves the two check rows the call needs, and no stripe can miss
    more originals than it has."""
    return sorted({1, 3, min(M - 2, N)})


def _pattern(N, M, m, seed):
    """A scattered missing set of m originals that always has original 0 or N - 1 in it."""
    rng = np.random.default_rng(seed)
    present = np.ones(N, np.uint8)
    present[rng.permutation(N)[:m]] = 0
    if m < N and present[0] and present[N - 1]:
        present[np.flatnonzero(present == 0)[0]] = 1
        present[N - 1] = 0
    assert int((present == 0).sum()) == m
    return present


CASES = [(rate, N, M, m) for rate, N, M in SHAPES for m in _missing_counts(N, M)]


@pytest.mark.parametrize("rate,N,M,m", CASES, ids=lambda v: str(v))
def test_table_is_nonzero_and_ratios_distinct(rate, N, M, m):
    """What the search rests on: no T[j][p] of a check row is zero, and for the row pairs a call
    can start from -- the first two check rows, the first and last, the middle and last -- the N
    ratios T[j1][p] / T[j0][p] are pairwise distinct (no 2 x 2 minor vanishes).  With every row
    selected and with every third row out."""
    _, log = LM.tables()
    present = _pattern(N, M, m, N + M + m)
    masks = [None]
    third = np.ones(M, np.uint8)
    third[2::3] = 0
    if int(third.sum()) >= m + 2:
        masks.append(third)
    for mask in masks:
        pb, R, K = DM.split(present, mask, M)
        T = DM.coefficients(rate, N, M, pb, R)
        assert T.shape == (M, N) and (T[K] != 0).all()
        for j0, j1 in {(K[0], K[1]), (K[0], K[-1]), (K[len(K) // 2], K[-1])}:
            if j0 == j1:
                continue
            ratio = (log[T[j1]] - log[T[j0]]) % 65535
            assert len(np.unique(ratio)) == N, (j0, j1)


def _stripe(rate, N, M, S, seed=1):
    orig = O.generate_original(N, S, seed)
    return orig, O.encode(rate, orig, M)


@pytest.mark.parametrize("rate,N,M,m", CASES, ids=lambda v: str(v))
def test_model_outcomes(rate, N, M, m):
    """The outcomes of the contract on constructed stripes: a single corrupt information shard
    reproduces D_j = T[j][p] * e on every check row and is named i or N + j."""
    S = 66
    orig, rec = _stripe(rate, N, M, S)
    present = _pattern(N, M, m, N + M + m)
    pb, R, K = DM.split(present, None, M)
    junk = orig.copy()
    junk[~pb] = 0xA5  # absent rows are not used
    got, flags, F = DM.locate(rate, junk, present, rec)
    assert got == DM.CLEAN and not flags.any() and np.array_equal(F, orig)
    # a present original: one bit in byte 0, one bit in the tail's last high byte
    for i in np.flatnonzero(pb)[[0, -1]] if pb.any() else []:
        for col_byte, bit in ((0, 0x01), (S - 1, 0x80)):
            bad = junk.copy()
            bad[i, col_byte] ^= bit
            got, flags, F = DM.locate(rate, bad, present, rec)
            assert got == int(i) and np.array_equal(np.flatnonzero(flags), K)
    # a reference row: N + j, and the restored originals are wrong
    for j in {int(R[0]), int(R[-1])}:
        bad = rec.copy()
        bad[j, S // 2] ^= 0x10
        got, flags, F = DM.locate(rate, junk, present, bad)
        assert got == N + j and np.array_equal(np.flatnonzero(flags), K)
        assert not np.array_equal(F, orig)
    # a check row: ROWS, its flag alone
    bad = rec.copy()
    bad[K[-1], 0] ^= 1
    got, flags, F = DM.locate(rate, junk, present, bad)
    assert got == DM.ROWS and np.flatnonzero(flags).tolist() == [K[-1]] and np.array_equal(F, orig)
    # junk in an unselected row (with every third row out) is never flagged
    third = np.ones(M, np.uint8)
    third[2::3] = 0
    if int(third.sum()) >= m + 2:
        bad = rec.copy()
        bad[2::3] ^= 0x5A
        got, flags, F = DM.locate(rate, junk, present, bad, mask=third)
        assert got == DM.CLEAN and not flags.any()
    # two corrupt information shards, in different columns: each column names another position,
    # so no single one explains the stripe, and every check row differs in the first's column
    bad, badr = junk.copy(), rec.copy()
    if pb.any():
        bad[np.flatnonzero(pb)[0], 0] ^= 0x10
    else:
        badr[R[1], 0] ^= 0x10
    badr[R[0], 1] ^= 0x33
    got, flags, _ = DM.locate(rate, bad, present, badr)
    assert got == DM.UNKNOWN and np.array_equal(np.flatnonzero(flags), K)
    # a present original (or a second reference row) plus a check row
    badr = rec.copy()
    badr[K[0], 2] ^= 0x08
    if pb.any():
        badr2, bad = badr, junk.copy()
        bad[np.flatnonzero(pb)[-1], 0] ^= 0x10
    else:
        bad, badr2 = junk, badr
        badr2[R[-1], 0] ^= 0x10
    got, flags, _ = DM.locate(rate, bad, present, badr2)
    assert got == DM.UNKNOWN and np.array_equal(np.flatnonzero(flags), K)


@pytest.mark.parametrize("rate,N,M,m", CASES, ids=lambda v: str(v))
def test_single_corruption_reproduces_the_table(rate, N, M, m):
    """D_j = T[j][p] * e, stated directly: the syndrome of every check row over every column."""
    S = 64
    orig, rec = _stripe(rate, N, M, S, seed=2)
    present = _pattern(N, M, m, N + M + m)
    pb, R, K = DM.split(present, None, M)
    T = DM.coefficients(rate, N, M, pb, R)
    rng = np.random.default_rng(m)
    where = DM.names(pb, R, N)
    for p in {0, N // 2, N - 1}:
        e = rng.integers(0, 256, S, dtype=np.uint8)
        e[0] |= 1
        bo, br = orig.copy(), rec.copy()
        if where[p] < N:
            bo[p] ^= e
        else:
            br[where[p] - N] ^= e
        F = DM.complete(rate, bo, pb, br, R)
        D = DM.elements(O.encode(rate, F, M) ^ br).astype(np.int64)
        ee = DM.elements(e[None, :]).astype(np.int64)[0]
        assert np.array_equal(D[K], LM.gf_mul(T[K][:, p][:, None], ee[None, :]))
        assert D[K].any(axis=1).all()
        assert DM.locate(rate, bo, present, br)[0] == int(where[p])


@pytest.mark.parametrize("rate,N,M", SHAPES, ids=lambda v: str(v))
def test_nothing_missing_is_the_locate(rate, N, M):
    """m = 0: T equals the locate's coefficients and the outcomes are the locate's."""
    present = np.ones(N, np.uint8)
    assert np.array_equal(DM.coefficients(rate, N, M, present, []), LM.coefficients(rate, N, M))
    orig, rec = _stripe(rate, N, M, 64)
    bad = orig.copy()
    bad[N - 1, 5] ^= 4
    badr = rec.copy()
    badr[1, 0] ^= 1
    for o, r in ((orig, rec), (bad, rec), (orig, badr), (bad, badr)):
        got, flags, F = DM.locate(rate, o, present, r)
        want, wflags = LM.locate(rate, o, r)
        assert got == want and np.array_equal(flags, wflags) and np.array_equal(F, o)
