"""rs_heal_device_degraded* without a GPU: the symbols and their declarations, the argument checks
(all of which come before any device work, in the header's order), the no-op case, the Python
wrappers' argument checks, the INTEGRATION.md binding, and the algebra the call rests on, on the
CPU oracle alone (tests/heal_degraded_model.py):

    clean shard q = stored shard q ^ e,   clean missing original p = F[p] ^ U[p][q] * e,

with q the located information position, e = D_j0 / T[j0][q] (j0 the first check row) and U the
coefficients of the decode from the reference rows.
"""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import heal_degraded_model as HDM
import locate_degraded_model as DM
import oracle_lib as O
import test_integration_abi as ABI
from test_verify_cpu import _Fake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rs_heal_device_degraded", "rs_heal_device_degraded_batch")
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


def _single(rs, ctx, N, M, S, d_orig, present, d_rec, mask, d_loc, d_flags, err=None, strides=(0, 0, 0), restored=8,
            mode=3, max_rows=0, action=8, stripes=None):
    return rs._lib.rs_heal_device_degraded(ctx, 0, N, M, S, d_orig, strides[0], present, d_rec, strides[1], mask,
                                           restored, strides[2], mode, max_rows, d_loc, d_flags, action, None, err)


def _batch(rs, ctx, N, M, S, d_orig, present, d_rec, mask, d_loc, d_flags, err=None, strides=(0, 0, 0), restored=8,
           mode=3, max_rows=0, action=8, stripes=2):
    return rs._lib.rs_heal_device_degraded_batch(ctx, 0, N, M, S, stripes, d_orig, strides[0], 0, present, d_rec,
                                                 strides[1], 0, mask, restored, strides[2], 0, mode, max_rows, d_loc,
                                                 d_flags, action, None, err)


FORMS = [_single, _batch]


def test_symbols_are_exported_and_declared(rs):
    header = open(HEADER).read()
    for name in NAMES:
        assert hasattr(rs._lib, name), name
        assert getattr(rs._lib, name).argtypes is not None, name  # the ctypes signature is declared
        proto = re.search(r"rs_status\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert proto, name
        assert re.search(r"[^t] void \*d_original.*const uint8_t \*original_present,\s*void \*d_recovery.*"
                         r"const uint8_t \*recovery_check,\s*void \*d_restored,\s*uint64_t restored_stride.*"
                         r"uint32_t mode,\s*uint32_t max_rows,\s*int32_t \*d_located,\s*uint8_t \*d_mismatch,\s*"
                         r"uint8_t \*d_action,\s*void \*stream,\s*rs_error \*err", proto.group(1), re.S), name
    batch = re.search(r"rs_heal_device_degraded_batch\s*\(([^;]*)\)", header).group(1)
    for arg in ("uint64_t stripes", "original_stripe_stride", "recovery_stripe_stride", "restored_stripe_stride"):
        assert arg in batch, arg
    assert len(rs._lib.rs_heal_device_degraded.argtypes) == 20
    assert len(rs._lib.rs_heal_device_degraded_batch.argtypes) == 24
    for name in ("heal_device_degraded", "heal_device_degraded_batch"):
        assert callable(getattr(rs, name)), name
    # what the contract promises and what it does not, in the header's words
    section = header[header.index("---- degraded heal"):header.index("rs_status rs_heal_device_degraded(")]
    section = re.sub(r"\s*\n \*\s*", " ", section)
    for phrase in ("d_restored is REQUIRED", "may alias d_original", "AS FOUND", "Every byte of d_action is defined",
                   "F_b[p] ^ U[p][i] * e", "recovery_j ^ e", "byte-identical to the clean stripe",
                   "RS_LOCATE_CLEAN with action 0", "delegates to rs_heal_device_batch", "c < m + 3",
                   "RS_ERR_NOT_ENOUGH_SHARDS", "three check rows", "k_heal_degraded", "k_coef_log_rows",
                   "builds BOTH tables again", "launches exactly what it did", "max_outliers", "a mask per stripe",
                   "filling unselected recovery rows", "the host pipeline, the object API and the sharded classes"):
        assert phrase in section, phrase
    assert "stripes with missing originals" not in section
    # the degraded locate's section keeps its words and points here
    locate = header[header.index("---- degraded locate"):header.index("rs_status rs_locate_device_degraded(")]
    assert "a degraded heal" in locate and "rs_heal_device_degraded" in locate


@pytest.mark.parametrize("call", FORMS)
def test_argument_checks_precede_any_device_work(rs, call):
    """A made-up non-null context is never dereferenced: every check comes first, in the
    header's order."""
    err = rs._RsError()
    e = ctypes.byref(err)
    fake = ctypes.c_void_p(8)
    p6, one = b"\1" * 6, b"\0\1\1\1\1\1"
    # 1. null context, d_original, original_present, d_recovery, d_restored, d_located, d_mismatch, d_action
    assert call(rs, None, 6, 6, 64, 8, p6, 8, None, 8, 8, e) == 101 and err.code == 101
    assert call(rs, fake, 6, 6, 64, 0, p6, 8, None, 8, 8, e) == 101
    assert call(rs, fake, 6, 6, 64, 8, None, 8, None, 8, 8, e) == 101
    assert call(rs, fake, 6, 6, 64, 8, p6, 0, None, 8, 8, e) == 101
    assert call(rs, fake, 6, 6, 64, 8, p6, 8, None, 8, 8, e, restored=0) == 101
    assert call(rs, fake, 6, 6, 64, 8, p6, 8, None, 0, 8, e) == 101
    assert call(rs, fake, 6, 6, 64, 8, p6, 8, None, 8, 0, e) == 101
    assert call(rs, fake, 6, 6, 64, 8, p6, 8, None, 8, 8, e, action=0) == 101
    # ... ahead of rs_validate (a bad shard size here): d_restored and d_action are among them
    for kw in ({"restored": 0}, {"action": 0}):
        err.code = 0
        assert call(rs, fake, 6, 6, 63, 8, p6, 8, None, 8, 8, e, **kw) == 101 and err.code == 101
    # 2. rs_validate: a bad shard size, an unsupported count -- ahead of the strides, the mode, the
    # row counts and the shape bound (all bad here)
    assert call(rs, fake, 6, 1, 63, 8, bytes(6), 8, None, 8, 8, e, strides=(32, 0, 0), mode=0) == 6
    assert err.shard_bytes == 63
    assert call(rs, fake, 4096, 61441, 64, 8, bytes(4096), 8, bytes(61441), 8, 8, e, strides=(0, 32, 0), mode=4) == 10
    assert (err.original_count, err.recovery_count) == (4096, 61441)
    # 3. the three row strides, each in turn -- ahead of the row counts (nothing selected here)
    for strides in ((32, 0, 0), (0, 32, 0), (0, 0, 32)):
        assert call(rs, fake, 6, 6, 64, 8, bytes(6), 8, bytes(6), 8, 8, e, strides=strides) == 101, strides
        assert err.code == 101
    assert call(rs, fake, 6, 6, 64, 8, bytes(6), 8, bytes(6), 8, 8, e) == 7  # (good strides: the row counts)
    # 4. mode == 0 or a bit outside the two -- after the strides, ahead of the row counts
    for mode in (0, 4, 7, 1 << 31):
        err.code = 0
        assert call(rs, fake, 6, 6, 64, 8, bytes(6), 8, bytes(6), 8, 8, e, mode=mode) == 101 and err.code == 101, mode
    for mode in (1, 2, 3):
        assert call(rs, fake, 6, 6, 64, 8, bytes(6), 8, bytes(6), 8, 8, e, mode=mode) == 7, mode
    # 5. c < m: not decodable, with the decode's counts
    err.code = 0
    assert call(rs, fake, 6, 6, 64, 8, b"\0\0\0\1\1\1", 8, b"\0\1\0\1\0\0", 8, 8, e) == 7 and err.code == 7
    assert (err.original_count, err.original_received_count, err.recovery_received_count) == (6, 3, 2)
    assert call(rs, fake, 8, 6, 64, 8, b"\0\0\0\0\0\0\0\1", 8, None, 8, 8, e) == 7
    assert (err.original_count, err.original_received_count, err.recovery_received_count) == (8, 1, 6)
    assert call(rs, fake, 5000, 1, 64, 8, bytes(5000), 8, None, 8, 8, e) == 7  # (... ahead of the shape bound)
    # 6. decodable, but fewer than three check rows: c = m, m + 1 and m + 2
    assert call(rs, fake, 6, 6, 64, 8, one, 8, b"\0\1\0\0\0\0", 8, 8, e) == 101 and err.code == 101  # c = m = 1
    assert call(rs, fake, 6, 6, 64, 8, one, 8, b"\0\1\0\1\0\0", 8, 8, e) == 101  # c = m + 1
    assert call(rs, fake, 6, 6, 64, 8, one, 8, b"\0\1\0\1\0\1", 8, 8, e) == 101  # c = m + 2: the locate's, not the heal's
    assert call(rs, fake, 6, 6, 64, 8, one, 8, b"\0\1\0\1\0\1", 8, 8, e, mode=2) == 101  # ... whatever the mode
    assert _batch(rs, fake, 6, 6, 64, 8, one, 8, b"\1\1\0\1\0\1", 8, 8, e, stripes=0) == 0  # c = m + 3: accepted
    assert _batch(rs, fake, 6, 6, 64, 8, b"\0\0\0\1\1\1", 8, None, 8, 8, e, stripes=0) == 0  # m = 3, c = 6
    assert call(rs, fake, 6, 6, 64, 8, b"\0\0\0\0\1\1", 8, None, 8, 8, e) == 101  # m = 4, c = 6
    assert call(rs, fake, 6, 6, 64, 8, bytes(6), 8, None, 8, 8, e) == 101  # m = c = 6
    assert call(rs, fake, 6, 6, 64, 8, p6, 8, b"\0\1\0\1\0\0", 8, 8, e) == 101  # m = 0: three rows all the same
    assert call(rs, fake, 5000, 4, 64, 8, b"\0" + b"\1" * 4999, 8, b"\1\1\1\0", 8, 8, e) == 101  # (ahead of the bound)
    # 7. the locate's shape bound
    assert call(rs, fake, 4097, 4, 64, 8, b"\0" + b"\1" * 4096, 8, None, 8, 8, e) == 101 and err.code == 101
    assert call(rs, fake, 4096, 4097, 64, 8, b"\0" + b"\1" * 4095, 8, None, 8, 8, e) == 101
    # all of them with no stripes at all, too
    assert _batch(rs, fake, 6, 6, 64, 8, one, 8, None, 8, 8, e, strides=(0, 63, 0), stripes=0) == 101
    assert _batch(rs, fake, 6, 6, 64, 8, one, 8, None, 8, 8, e, mode=0, stripes=0) == 101
    assert _batch(rs, fake, 6, 6, 64, 8, one, 8, b"\0\0\0\1\1\1", 8, 8, e, stripes=0) == 101
    assert _batch(rs, fake, 6, 6, 64, 8, bytes(6), 8, b"\0\1\1\1\1\1", 8, 8, e, stripes=0) == 7
    assert _batch(rs, fake, 4097, 4, 64, 8, b"\0" + b"\1" * 4096, 8, None, 8, 8, e, stripes=0) == 101
    assert _batch(rs, fake, 6, 6, 64, 8, one, 8, None, 8, 8, e, restored=0, stripes=0) == 101
    # a null err is allowed
    assert call(rs, fake, 6, 6, 64, 8, one, 8, None, 8, 8, None, strides=(0, 32, 0)) == 101
    assert call(rs, fake, 6, 6, 64, 8, bytes(6), 8, b"\0\1\1\1\1\1", 8, 8, None) == 7
    assert call(rs, None, 6, 6, 64, 8, one, 8, None, 8, 8, None) == 101


def test_no_stripes_is_ok_without_touching_anything(rs):
    err = rs._RsError()
    err.code = 55
    fake = ctypes.c_void_p(8)
    one = b"\0\1\1\1\1\1"
    assert _batch(rs, fake, 6, 6, 64, 8, one, 8, None, 8, 8, ctypes.byref(err), stripes=0) == 0 and err.code == 0
    assert _batch(rs, fake, 6, 6, 64, 8, one, 8, b"\1\1\0\1\1\0", 8, 8, None, strides=(64, 128, 192), stripes=0) == 0
    for mode in (1, 2, 3):
        assert _batch(rs, fake, 6, 6, 64, 8, one, 8, None, 8, 8, None, mode=mode, max_rows=1 << 31, stripes=0) == 0
    assert _batch(rs, fake, 6, 6, 64, 8, b"\1" * 6, 8, None, 8, 8, None, stripes=0) == 0  # m = 0
    # the largest shapes inside the bound pass the checks
    assert _batch(rs, fake, 4096, 4096, 64, 8, bytes(4093) + b"\1\1\1", 8, None, 8, 8, None, stripes=0) == 0
    assert _batch(rs, fake, 256, 65280, 64, 8, b"\0" + b"\1" * 255, 8, None, 8, 8, None, stripes=0) == 0


def test_wrappers_reject_wrong_shapes_dtypes_and_masks(rs):
    N, M, S, B = 8, 6, 64, 3
    ctx = types.SimpleNamespace(handle=None)
    names = ["d_original", "d_recovery", "d_restored"]
    rows = [N, M, N]
    good = lambda: [_Fake(N, S), _Fake(M, S), _Fake(N, S)]
    loc = lambda *shape, **kw: _Fake(*shape, **dict({"dtype": "torch.int32"}, **kw))
    present = [1, 0, 1, 1, 0, 1, 1, 1]  # m = 2

    def single(t, present=present, mask=None, located=loc(1), flags=_Fake(M), action=_Fake(1), mode=3, max_rows=0):
        return rs.heal_device_degraded(N, M, S, t[0], present, t[1], t[2], recovery_rows=mask, mode=mode,
                                       max_rows=max_rows, d_located=located, d_mismatch=flags, d_action=action,
                                       ctx=ctx)

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
    t = good()
    t[2] = None  # d_restored is required
    with pytest.raises(ValueError, match="d_restored: a degraded heal needs it"):
        single(t)
    for mode in (0, 4, 7):
        with pytest.raises(ValueError, match="mode:"):
            single(good(), mode=mode)
    for max_rows in (-1, 1 << 32):
        with pytest.raises(ValueError, match="max_rows:"):
            single(good(), max_rows=max_rows)
    with pytest.raises(ValueError, match="original_present"):
        single(good(), present=[1] * (N + 1))
    with pytest.raises(ValueError, match="original_present"):
        single(good(), present=[1] * (N - 1))
    with pytest.raises(ValueError, match="recovery_rows"):
        single(good(), mask=[1] * (M + 1))
    # c = m, m + 1 and m + 2: decodable, too few rows left to write on the evidence of
    for few in ([1, 1, 0, 0, 0, 0], [0, 1, 0, 1, 0, 1], [1, 1, 0, 1, 0, 1]):
        with pytest.raises(ValueError, match="recovery_rows: 2 missing originals"):
            single(good(), mask=few)
    with pytest.raises(ValueError, match="recovery_rows: 4 missing"):
        single(good(), present=[0, 0, 0, 0, 1, 1, 1, 1])  # m = 4, c = M = 6
    with pytest.raises(ValueError, match="recovery_rows: 0 missing"):
        single(good(), present=[1] * N, mask=[0, 0, 1, 0, 1, 0])  # m = 0: three rows all the same
    # c < m is the library's NotEnoughShards with its counts: the wrapper passes it on, and here
    # the library's first check refuses the null context
    with pytest.raises(ValueError, match="rs_status 101"):
        single(good(), mask=[0, 0, 1, 0, 0, 0])
    for bad in (loc(2), loc(1, 1), _Fake(1), loc(1, dtype="torch.int64"), loc(1, contiguous=False)):
        with pytest.raises(ValueError, match="d_located"):
            single(good(), located=bad)
    for bad in (_Fake(M - 1), _Fake(M + 1), _Fake(1, M), _Fake(M, dtype="torch.bool"), _Fake(M, contiguous=False)):
        with pytest.raises(ValueError, match="d_mismatch"):
            single(good(), flags=bad)
    for bad in (_Fake(2), _Fake(1, 1), loc(1), _Fake(1, contiguous=False)):
        with pytest.raises(ValueError, match="d_action"):
            single(good(), action=bad)
    with pytest.raises(ValueError, match="d_located"):  # raw pointers: nothing says where to allocate
        rs.heal_device_degraded(N, M, S, 8, present, 8, 8, ctx=ctx)
    with pytest.raises(rs.UnsupportedShardCount):  # the reference's own checks come first
        rs.heal_device_degraded(4096, 61441, S, _Fake(1, S), [1], _Fake(1, S), _Fake(1, S), d_located=loc(1),
                                d_mismatch=_Fake(1), d_action=_Fake(1), ctx=ctx)
    # well-formed arguments reach the library (whose first check refuses the null context)
    with pytest.raises(ValueError, match="rs_status 101"):
        single(good())
    with pytest.raises(ValueError, match="rs_status 101"):
        single(good(), mask=[1, 0, 1, 1, 1, 1], mode=1, max_rows=5)
    t = good()
    t[2] = t[0]  # d_restored = d_original
    with pytest.raises(ValueError, match="rs_status 101"):
        single(t)
    with pytest.raises(ValueError, match="rs_status 101"):
        rs.heal_device_degraded(N, M, S, 8, present, 8, 8, d_located=8, d_mismatch=8, d_action=8, ctx=ctx)

    goodb = lambda: [_Fake(B, N, S), _Fake(B, M, S), _Fake(B, N, S)]

    def batch(t, present=present, mask=None, located=loc(B), flags=_Fake(B, M), action=_Fake(B), mode=3):
        return rs.heal_device_degraded_batch(N, M, S, t[0], present, t[1], t[2], recovery_rows=mask, mode=mode,
                                             d_located=located, d_mismatch=flags, d_action=action, ctx=ctx)

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
    t = goodb()
    t[2] = None
    with pytest.raises(ValueError, match="d_restored: a degraded heal needs it"):
        batch(t)
    with pytest.raises(ValueError, match="mode:"):
        batch(goodb(), mode=0)
    with pytest.raises(ValueError, match="recovery_rows"):
        batch(goodb(), mask=np.ones((B, M), np.uint8))  # one mask for the whole batch
    with pytest.raises(ValueError, match="original_present"):
        batch(goodb(), present=np.ones((B, N), np.uint8))
    with pytest.raises(ValueError, match="recovery_rows: 2 missing originals"):
        batch(goodb(), mask=[1, 1, 1, 1, 0, 0])
    for bad in (loc(1), loc(B + 1), loc(B, 1), _Fake(B)):
        with pytest.raises(ValueError, match="d_located"):
            batch(goodb(), located=bad)
    for bad in (_Fake(M), _Fake(B, M + 1), _Fake(B + 1, M), _Fake(B * M)):
        with pytest.raises(ValueError, match="d_mismatch"):
            batch(goodb(), flags=bad)
    for bad in (_Fake(1), _Fake(B + 1), _Fake(B, 1), loc(B)):
        with pytest.raises(ValueError, match="d_action"):
            batch(goodb(), action=bad)
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
                     "void * d_original", "void * d_recovery", "void * d_restored", "uint32_t mode",
                     "uint32_t max_rows", "uint8_t * d_action"):
            assert want in params, want
        protos.append(f"rs_status {name}({', '.join(params)});")
        assert re.search(r'_sig\("%s"|lib\.%s\b' % (name, name), doc), name  # the ctypes side
    c = tmp_path / "heal_degraded_bindings.c"
    c.write_text("\n".join(["#include <stdint.h>", f'#include "{HEADER}"'] + protos) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-c", str(c), "-o", str(tmp_path / "h.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + "\n" + c.read_text()


# ---------------------------------------------------------------------------
# the algebra, on the CPU oracle alone

SHAPES = [("default", 3, 5), ("high", 12, 5), ("low", 5, 12), ("high", 70, 100), ("low", 100, 70),
          ("default", 200, 200)]
SIZES = (64, 72, 66)


def _pattern(N, m, seed):
    """A scattered missing set of m originals that always has original 0 or N - 1 in it."""
    rng = np.random.default_rng(seed)
    present = np.ones(N, np.uint8)
    present[rng.permutation(N)[:m]] = 0
    if m < N and present[0] and present[N - 1]:
        present[np.flatnonzero(present == 0)[0]] = 1
        present[N - 1] = 0
    assert int((present == 0).sum()) == m
    return present


def _faults(orig, rec, pb, R, S, rng):
    """(name, originals, recovery) of the constructed faults: one corrupt present original -- a
    whole shard, or the last high bit of the tail --, or one flipped bit in the last reference row."""
    out = []
    if pb.any():
        i = int(np.flatnonzero(pb)[len(np.flatnonzero(pb)) // 2])
        bad = orig.copy()
        bad[i] ^= rng.integers(1, 256, S, dtype=np.uint8)
        out.append(("shard", bad, rec))
        bad = orig.copy()
        bad[i, S - 1] ^= 0x80
        out.append(("tail bit", bad, rec))
    badr = rec.copy()
    badr[R[-1], S // 3] ^= 0x04
    out.append(("reference row", orig, badr))
    return out


CASES = [(rate, N, M, m) for rate, N, M in SHAPES for m in sorted({1, min(N, M - 3)})]


@pytest.mark.parametrize("rate,N,M,m", CASES, ids=lambda v: str(v))
def test_two_corrections_give_back_the_clean_stripe(rate, N, M, m):
    """The model heals every constructed case to the clean stripe byte for byte, separate and
    aliased; U has no zero; and a second heal of the result is CLEAN with action 0."""
    present = _pattern(N, m, N + M + m)
    pb, R, K = DM.split(present, None, M)
    U = HDM.restored_coefficients(rate, N, M, pb, R)
    assert U.shape == (m, N) and (U != 0).all()
    rng = np.random.default_rng(N * M + m)
    for S in SIZES:
        orig = O.generate_original(N, S, S)
        rec = O.encode(rate, orig, M)
        junk = orig.copy()
        junk[~pb] = 0xA5  # absent rows are not used
        for name, bo, br in _faults(junk, rec, pb, R, S, rng):
            loc, flags, action, o2, r2, x2 = HDM.heal(rate, bo, present, br, np.zeros_like(orig))
            assert loc >= 0 and np.array_equal(np.flatnonzero(flags), K), (S, name)
            assert action == (HDM.ORIGINAL if loc < N else HDM.RECOVERY), (S, name)
            assert np.array_equal(r2, rec), (S, name)
            assert np.array_equal(o2[pb], orig[pb]) and np.array_equal(o2[~pb], junk[~pb]), (S, name)
            assert np.array_equal(x2[~pb], orig[~pb]) and not x2[pb].any(), (S, name)
            # aliased: the restored rows land in the originals' matrix
            _, _, _, o3, r3, x3 = HDM.heal(rate, bo, present, br, bo)
            whole = np.where(pb[:, None], o3, x3)
            assert np.array_equal(whole, orig) and np.array_equal(r3, rec), (S, name)
            # again: CLEAN, action 0, the same bytes
            loc2, flags2, action2, o4, r4, x4 = HDM.heal(rate, whole, present, r3, whole)
            assert (loc2, action2) == (HDM.CLEAN, 0) and not flags2.any(), (S, name)
            assert np.array_equal(np.where(pb[:, None], o4, x4), orig) and np.array_equal(r4, rec), (S, name)


@pytest.mark.parametrize("rate,N,M,m", [c for c in CASES if c[1] >= 5], ids=lambda v: str(v))
def test_model_mode_bits_rows_and_unknown(rate, N, M, m):
    """What the call may write follows the mode bits; a ROWS stripe follows max_rows; anything
    else is left as the degraded locate leaves it."""
    S = 66
    present = _pattern(N, m, N + M + m)
    pb, R, K = DM.split(present, None, M)
    orig = O.generate_original(N, S, 3)
    rec = O.encode(rate, orig, M)
    zero = np.zeros_like(orig)
    # a located shard whose bit is off: action 0, the restored rows are F's (wrong), nothing else
    if pb.any():
        bad = orig.copy()
        bad[np.flatnonzero(pb)[0], 0] ^= 1
        loc, flags, action, o2, r2, x2 = HDM.heal(rate, bad, present, rec, zero, mode=HDM.RECOVERY)
        assert loc == int(np.flatnonzero(pb)[0]) and action == 0
        assert np.array_equal(o2, bad) and np.array_equal(r2, rec)
        assert np.array_equal(x2[~pb], DM.locate(rate, bad, present, rec)[2][~pb])
        assert not np.array_equal(x2[~pb], orig[~pb])
    badr = rec.copy()
    badr[R[0], 5] ^= 0x40
    loc, flags, action, o2, r2, x2 = HDM.heal(rate, orig, present, badr, zero, mode=HDM.ORIGINAL)
    assert loc == N + int(R[0]) and action == 0 and np.array_equal(r2, badr)
    assert not np.array_equal(x2[~pb], orig[~pb])
    loc, flags, action, o2, r2, x2 = HDM.heal(rate, orig, present, badr, zero, mode=HDM.RECOVERY)
    assert action == HDM.RECOVERY and np.array_equal(r2, rec) and np.array_equal(x2[~pb], orig[~pb])
    # check rows: rewritten within the threshold, with the bit
    badr = rec.copy()
    badr[K[0], 1] ^= 2
    badr[K[-1], S - 1] ^= 0x80
    for mode, max_rows, want in ((3, 2, HDM.RECOVERY), (2, 5, HDM.RECOVERY), (3, 1, 0), (1, 5, 0), (3, 0, 0)):
        loc, flags, action, o2, r2, x2 = HDM.heal(rate, orig, present, badr, zero, mode=mode, max_rows=max_rows)
        assert loc == HDM.ROWS and action == want and np.flatnonzero(flags).tolist() == [K[0], K[-1]]
        assert np.array_equal(r2, rec if want else badr) and np.array_equal(o2, orig)
        assert np.array_equal(x2[~pb], orig[~pb])
    # an information shard plus a check row: UNKNOWN, untouched
    badr = rec.copy()
    badr[R[-1], 0] ^= 0x10
    badr[K[1], 2] ^= 0x08
    loc, flags, action, o2, r2, x2 = HDM.heal(rate, orig, present, badr, zero, max_rows=M)
    assert loc == HDM.UNKNOWN and action == 0 and np.array_equal(r2, badr) and np.array_equal(o2, orig)
    assert np.array_equal(x2[~pb], DM.locate(rate, orig, present, badr)[2][~pb])
