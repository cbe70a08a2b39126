"""rs_locate_device* without a GPU: the symbols and their declarations, the argument checks (all
of which come before any device work, in the header's order), the no-op case, the Python wrappers'
argument checks, the INTEGRATION.md binding, and the algebra the kernels rely on, on the CPU oracle
alone (tests/locate_model.py):

    D_j = recovery_j ^ encode(originals)_j = G[j][i] * e   for one corrupt original i,

so the ratio of two rows' syndromes names i -- provided no coefficient is zero and the ratios of
the N originals are pairwise distinct, which is checked here for every shape the issue lists.
"""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import locate_model as LM
import oracle_lib as O
import test_integration_abi as ABI
from test_verify_cpu import _Fake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rs_locate_device", "rs_locate_device_batch")
HEADER = os.path.join(ROOT, "include", "rs_mi355x.h")


@pytest.fixture(scope="module")
def rs():
    # (imported by the tests that use it, not while pytest collects: tests/test_batch_masks_cpu.py)
    import reed_solomon_simd
    return reed_solomon_simd


def _single(rs, ctx, N, M, S, d_orig, d_rec, mask, d_loc, d_flags, err=None, strides=(0, 0), stripes=None):
    return rs._lib.rs_locate_device(ctx, 0, N, M, S, d_orig, strides[0], d_rec, strides[1], mask, d_loc, d_flags,
                                    None, err)


def _batch(rs, ctx, N, M, S, d_orig, d_rec, mask, d_loc, d_flags, err=None, strides=(0, 0), stripes=2):
    return rs._lib.rs_locate_device_batch(ctx, 0, N, M, S, stripes, d_orig, strides[0], 0, d_rec, strides[1], 0, mask,
                                          d_loc, d_flags, None, err)


FORMS = [_single, _batch]


def test_symbols_are_exported_and_declared(rs):
    header = open(HEADER).read()
    for name in NAMES:
        assert hasattr(rs._lib, name), name
        assert getattr(rs._lib, name).argtypes is not None, name  # the ctypes signature is declared
        proto = re.search(r"rs_status\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert proto, name
        assert re.search(r"const void \*d_original.*const void \*d_recovery.*const uint8_t \*recovery_check,\s*"
                         r"int32_t \*d_located,\s*uint8_t \*d_mismatch,\s*void \*stream,\s*rs_error \*err",
                         proto.group(1), re.S), name
    batch = re.search(r"rs_locate_device_batch\s*\(([^;]*)\)", header).group(1)
    for arg in ("uint64_t stripes", "original_stripe_stride", "recovery_stripe_stride"):
        assert arg in batch, arg
    assert len(rs._lib.rs_locate_device.argtypes) == 14 and len(rs._lib.rs_locate_device_batch.argtypes) == 17
    for name in ("locate_device", "locate_device_batch"):
        assert callable(getattr(rs, name)), name
    # the three statuses, in both places
    for name, value in (("CLEAN", -1), ("ROWS", -2), ("UNKNOWN", -3)):
        m = re.search(r"#define RS_LOCATE_%s \((-\d+)\)" % name, header)
        assert m and int(m.group(1)) == value == getattr(rs, "LOCATE_" + name) == getattr(LM, name), name
    # the bound of the coefficient table covers what the issue requires
    assert int(re.search(r"#define RS_LOCATE_MAX_ORIGINALS (\d+)u", header).group(1)) >= 4096
    assert re.search(r"#define RS_LOCATE_MAX_COEFFICIENTS \(1u << (\d+)\)", header).group(1) == "24"
    # what the contract promises and what it does not, in the header's words
    for phrase in ("every byte of d_mismatch and every word of d_located", "exactly what rs_verify_device_batch writes",
                   "NOT proven", "matching by coincidence", "c - 1 corrupt shards", "Select three rows",
                   "Nothing is written but d_located", "Not covered:"):
        assert phrase in header, phrase


@pytest.mark.parametrize("call", FORMS)
def test_argument_checks_precede_any_device_work(rs, call):
    """A made-up non-null context is never dereferenced: every check comes first, in the
    header's order."""
    err = rs._RsError()
    e = ctypes.byref(err)
    fake = ctypes.c_void_p(8)
    # 1. null context, d_original, d_recovery, d_located, d_mismatch
    assert call(rs, None, 4, 4, 64, 8, 8, None, 8, 8, e) == 101 and err.code == 101
    assert call(rs, fake, 4, 4, 64, 0, 8, None, 8, 8, e) == 101
    assert call(rs, fake, 4, 4, 64, 8, 0, None, 8, 8, e) == 101
    assert call(rs, fake, 4, 4, 64, 8, 8, None, 0, 8, e) == 101
    assert call(rs, fake, 4, 4, 64, 8, 8, None, 8, 0, e) == 101
    # ... ahead of rs_validate (a bad shard size here)
    err.code = 0
    assert call(rs, fake, 4, 4, 63, 8, 8, None, 0, 8, e) == 101 and err.code == 101
    # 2. rs_validate: a bad shard size, an unsupported count -- ahead of the strides, the
    # row count and the shape bound (all bad here)
    assert call(rs, fake, 4, 1, 63, 8, 8, None, 8, 8, e, strides=(32, 0)) == 6 and err.shard_bytes == 63
    assert call(rs, fake, 4096, 61441, 64, 8, 8, bytes(61441), 8, 8, e, strides=(0, 32)) == 10
    assert (err.original_count, err.recovery_count) == (4096, 61441)
    # 3. the two row strides, each in turn -- ahead of the row count (one row, or a mask of one)
    for strides in ((32, 0), (0, 32)):
        assert call(rs, fake, 4, 4, 64, 8, 8, None, 8, 8, e, strides=strides) == 101 and err.code == 101, strides
        assert call(rs, fake, 4, 1, 64, 8, 8, None, 8, 8, e, strides=strides) == 101, strides
        assert call(rs, fake, 4, 4, 64, 8, 8, b"\0\1\0\0", 8, 8, e, strides=strides) == 101, strides
    # 4. fewer than two rows to compare: recovery_count < 2, a mask of one row, of none
    assert call(rs, fake, 4, 1, 64, 8, 8, None, 8, 8, e) == 101 and err.code == 101
    assert call(rs, fake, 4, 4, 64, 8, 8, b"\0\1\0\0", 8, 8, e) == 101
    assert call(rs, fake, 4, 4, 64, 8, 8, bytes(4), 8, 8, e) == 101
    assert call(rs, fake, 5000, 1, 64, 8, 8, None, 8, 8, e) == 101  # (... ahead of the shape bound)
    # 5. the bound of the coefficient table: original_count <= 4096, original_count x recovery_count <= 2^24
    assert call(rs, fake, 4097, 2, 64, 8, 8, None, 8, 8, e) == 101 and err.code == 101
    assert call(rs, fake, 4096, 4097, 64, 8, 8, None, 8, 8, e) == 101
    # all of them with no stripes at all, too
    assert _batch(rs, fake, 4, 4, 64, 8, 8, None, 8, 8, e, strides=(0, 63), stripes=0) == 101
    assert _batch(rs, fake, 4, 4, 64, 8, 8, b"\0\0\0\1", 8, 8, e, stripes=0) == 101
    assert _batch(rs, fake, 4097, 4, 64, 8, 8, None, 8, 8, e, stripes=0) == 101
    # a null err is allowed
    assert call(rs, fake, 4, 4, 64, 8, 8, None, 8, 8, None, strides=(0, 32)) == 101
    assert call(rs, None, 4, 4, 64, 8, 8, None, 8, 8, None) == 101


def test_no_stripes_is_ok_without_touching_anything(rs):
    err = rs._RsError()
    err.code = 55
    fake = ctypes.c_void_p(8)
    assert _batch(rs, fake, 4, 4, 64, 8, 8, None, 8, 8, ctypes.byref(err), stripes=0) == 0 and err.code == 0
    assert _batch(rs, fake, 4, 4, 64, 8, 8, b"\1\0\0\1", 8, 8, None, strides=(64, 128), stripes=0) == 0
    # the largest shapes inside the bound pass the checks
    assert _batch(rs, fake, 4096, 4096, 64, 8, 8, None, 8, 8, None, stripes=0) == 0
    assert _batch(rs, fake, 256, 65280, 64, 8, 8, None, 8, 8, None, stripes=0) == 0


def test_wrappers_reject_wrong_shapes_dtypes_and_masks(rs):
    N, M, S, B = 8, 6, 64, 3
    ctx = types.SimpleNamespace(handle=None)
    names = ["d_original", "d_recovery"]
    rows = [N, M]
    good = lambda: [_Fake(N, S), _Fake(M, S)]
    loc = lambda *shape, **kw: _Fake(*shape, **dict({"dtype": "torch.int32"}, **kw))

    def single(t, mask=None, located=loc(1), flags=_Fake(M)):
        return rs.locate_device(N, M, S, t[0], t[1], recovery_rows=mask, d_located=located, d_mismatch=flags, ctx=ctx)

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
    for few in ([0] * M, [0, 0, 1, 0, 0, 0]):  # a ratio needs two rows
        with pytest.raises(ValueError, match="recovery_rows: a locate needs two"):
            single(good(), mask=few)
    with pytest.raises(ValueError, match="recovery_rows: a locate needs two"):
        rs.locate_device(N, 1, S, _Fake(N, S), _Fake(1, S), d_located=loc(1), d_mismatch=_Fake(1), ctx=ctx)
    # the result: exactly one int32 per stripe, contiguous; the flags as the verify's
    for bad in (loc(2), loc(1, 1), _Fake(1), loc(1, dtype="torch.int64"), loc(1, contiguous=False)):
        with pytest.raises(ValueError, match="d_located"):
            single(good(), located=bad)
    for bad in (_Fake(M - 1), _Fake(M + 1), _Fake(1, M), _Fake(M, dtype="torch.bool"), _Fake(M, contiguous=False)):
        with pytest.raises(ValueError, match="d_mismatch"):
            single(good(), flags=bad)
    with pytest.raises(ValueError, match="d_located"):  # raw pointers: nothing says where to allocate
        rs.locate_device(N, M, S, 8, 8, ctx=ctx)
    with pytest.raises(rs.UnsupportedShardCount):  # the reference's own checks come first
        rs.locate_device(4096, 61441, S, _Fake(1, S), _Fake(1, S), d_located=loc(1), d_mismatch=_Fake(1), ctx=ctx)
    # well-formed arguments reach the library (whose first check refuses the null context)
    with pytest.raises(ValueError, match="rs_status 101"):
        single(good())
    with pytest.raises(ValueError, match="rs_status 101"):
        single(good(), mask=[1, 0, 0, 1, 1, 0])
    with pytest.raises(ValueError, match="rs_status 101"):
        rs.locate_device(N, M, S, 8, 8, d_located=8, d_mismatch=8, ctx=ctx)  # raw pointers throughout

    goodb = lambda: [_Fake(B, N, S), _Fake(B, M, S)]

    def batch(t, mask=None, located=loc(B), flags=_Fake(B, M)):
        return rs.locate_device_batch(N, M, S, t[0], t[1], recovery_rows=mask, d_located=located, d_mismatch=flags,
                                      ctx=ctx)

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
    compile as redeclarations against the header (d_located is a `*mut i32`)."""
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
        assert "int32_t * d_located" in params and "const uint8_t * recovery_check" in params
        protos.append(f"rs_status {name}({', '.join(params)});")
        assert re.search(r'_sig\("%s"|lib\.%s\b' % (name, name), doc), name  # the ctypes side
    c = tmp_path / "locate_bindings.c"
    c.write_text("\n".join(["#include <stdint.h>", f'#include "{HEADER}"'] + protos) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-c", str(c), "-o", str(tmp_path / "l.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + "\n" + c.read_text()
    scrub = doc[doc.index("rs.locate_device_batch("):]
    assert "repair_device_batch_masks(" in scrub[:1200] and "LOCATE_ROWS" in scrub[:1200]


# ---------------------------------------------------------------------------
# the algebra, on the CPU oracle alone

SHAPES = [("default", 100, 30), ("default", 30, 100), ("default", 1024, 1024), ("default", 3, 2), ("default", 2, 3),
          ("default", 300, 3), ("default", 2048, 2048), ("default", 4096, 4096), ("high", 1000, 100),
          ("low", 128, 1024)]


@pytest.mark.parametrize("rate,N,M", SHAPES, ids=lambda v: str(v))
def test_coefficients_are_nonzero_and_ratios_distinct(rate, N, M):
    """What the search for i rests on: no G[j][i] is zero (so every log is a real one), and for the
    row pairs a call can start from -- the first two rows, (0, M-1), (M/2, M-1) -- the N ratios
    G[j1][i] / G[j0][i] are pairwise distinct (no 2 x 2 minor vanishes)."""
    _, log = LM.tables()
    G = LM.coefficients(rate, N, M)
    assert G.shape == (M, N) and (G != 0).all()
    for j0, j1 in {(0, 1), (0, M - 1), (M // 2, M - 1)}:
        if j0 == j1:
            continue
        ratio = (log[G[j1]] - log[G[j0]]) % 65535
        assert len(np.unique(ratio)) == N, (j0, j1)


def _stripe(rate, N, M, S, seed=1):
    orig = O.generate_original(N, S, seed)
    return orig, O.encode(rate, orig, M)


OUTCOMES = [("default", 100, 30, 66), ("high", 1000, 100, 64), ("low", 128, 1024, 2), ("default", 3, 2, 190),
            ("default", 1, 2, 64), ("default", 128, 128, 64)]


@pytest.mark.parametrize("rate,N,M,S", OUTCOMES, ids=lambda v: str(v))
def test_model_outcomes(rate, N, M, S):
    """The four outcomes of the contract on constructed stripes."""
    orig, rec = _stripe(rate, N, M, S)
    rng = np.random.default_rng(N + M)
    assert LM.locate(rate, orig, rec)[0] == LM.CLEAN
    two = np.zeros(M, np.uint8)
    two[[0, M - 1]] = 1
    for i in sorted({0, N // 2, N - 1}):
        bad = orig.copy()
        bad[i, S - 1] ^= 0x80  # one bit in the last byte
        got, flags = LM.locate(rate, bad, rec)
        assert got == i and flags.all()
        assert LM.locate(rate, bad, rec, mask=two)[0] == i  # two rows are enough for one original
        bad[i] = rng.integers(0, 256, S, dtype=np.uint8)  # the whole shard
        assert LM.locate(rate, bad, rec)[0] == i
    # recovery rows alone
    bad = rec.copy()
    bad[M - 1, 0] ^= 1
    got, flags = LM.locate(rate, orig, bad)
    assert got == LM.ROWS and np.flatnonzero(flags).tolist() == [M - 1]
    # every recovery row (with two rows in all, the contract allows an i: see the header)
    if M >= 3:
        assert LM.locate(rate, orig, rec ^ 1)[0] == LM.UNKNOWN
    if N >= 2 and M >= 3:
        # two originals, in different columns and in one; an original and a recovery row
        bad = orig.copy()
        bad[0, 0] ^= 0x10
        bad[N - 1, S - 1] ^= 0x20
        D = LM.syndromes(rate, bad, rec)
        assert LM.locate(rate, bad, rec, D=D)[0] == (LM.UNKNOWN if D.any(axis=1).all() else LM.ROWS)
        bad = orig.copy()
        bad[0, 0] ^= 0x10
        bad[N // 2, 0] ^= 0x33
        D = LM.syndromes(rate, bad, rec)
        assert LM.locate(rate, bad, rec, D=D)[0] == (LM.UNKNOWN if D.any(axis=1).all() else LM.ROWS)
        bad, badr = orig.copy(), rec.copy()
        bad[N - 1, 0] ^= 0x04
        badr[1, S // 2] ^= 0x40
        assert LM.locate(rate, bad, badr)[0] == LM.UNKNOWN


@pytest.mark.parametrize("rate,N,M,S", [("default", 128, 128, 64), ("low", 128, 1024, 2)], ids=lambda v: str(v))
def test_a_matching_row_does_not_vouch_for_the_originals(rate, N, M, S):
    """The limit of RS_LOCATE_ROWS, pinned: original 0 off by 1 and original N-1 off by 2 in one
    column leave some recovery row matching by coincidence (G[j][0] = 2 * G[j][N-1] there: the
    coefficients of low positions lie in small subfields), so two corrupt originals come back as
    ROWS, not UNKNOWN -- "some row matches" rules out a single corrupt original, nothing stronger."""
    orig, rec = _stripe(rate, N, M, S)
    bad = orig.copy()
    bad[0, 0] ^= 1
    bad[N - 1, 0] ^= 2
    got, flags = LM.locate(rate, bad, rec)
    assert got == LM.ROWS
    assert 0 < flags.sum() < M
    # the rows that match are those where the two contributions cancel
    G = LM.coefficients(rate, N, M)
    cancel = LM.gf_mul(G[:, 0], 1) == LM.gf_mul(G[:, N - 1], 2)
    assert np.array_equal(flags == 0, cancel)
