"""rs_heal_device_robust* without a GPU: the symbols and their declarations, the argument checks
(all before any device work, in the header's order), the no-op case, the Python wrappers' argument
checks, the INTEGRATION.md binding, and the contract on the numpy model (tests/heal_robust_model.py)
over the constructed stripes of tests/locate_robust_cases.py:

    a located (i, B), both bits    both matrices byte-identical to the clean stripe
    any reference row outside B    the same e
    RS_HEAL_ORIGINAL alone         the next scan: ROWS, exactly B flagged
    RS_HEAL_RECOVERY alone         the next scan: the plain locate names i
    max_outliers = 0               tests/heal_model.py
"""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import heal_model as HM
import heal_robust_model as HRM
import locate_model as LM
import locate_robust_cases as RC
import locate_robust_model as RM
import oracle_lib as O
import test_integration_abi as ABI
from test_verify_cpu import _Fake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rs_heal_device_robust", "rs_heal_device_robust_batch")
HEADER = os.path.join(ROOT, "include", "rs_mi355x.h")
ORIGINAL, RECOVERY = HM.ORIGINAL, HM.RECOVERY
CLEAN, ROWS, UNKNOWN = LM.CLEAN, LM.ROWS, LM.UNKNOWN


@pytest.fixture(scope="module")
def rs():
    # (imported by the tests that use it, not while pytest collects: tests/test_batch_masks_cpu.py)
    import reed_solomon_simd
    return reed_solomon_simd


def _single(rs, ctx, N, M, S, d_orig, d_rec, mask, t, mode, d_loc, d_flags, d_out, d_act, err=None, strides=(0, 0),
            stripes=None, max_rows=1):
    return rs._lib.rs_heal_device_robust(ctx, 0, N, M, S, d_orig, strides[0], d_rec, strides[1], mask, t, mode,
                                         max_rows, d_loc, d_flags, d_out, d_act, None, err)


def _batch(rs, ctx, N, M, S, d_orig, d_rec, mask, t, mode, d_loc, d_flags, d_out, d_act, err=None, strides=(0, 0),
           stripes=2, max_rows=1):
    return rs._lib.rs_heal_device_robust_batch(ctx, 0, N, M, S, stripes, d_orig, strides[0], 0, d_rec, strides[1], 0,
                                               mask, t, mode, max_rows, d_loc, d_flags, d_out, d_act, None, err)


FORMS = [_single, _batch]


def test_symbols_are_exported_and_declared(rs):
    header = open(HEADER).read()
    for name in NAMES:
        assert hasattr(rs._lib, name), name
        assert getattr(rs._lib, name).argtypes is not None, name
        proto = re.search(r"rs_status\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert proto, name
        # the matrices are written: no const; max_outliers before mode, d_outlier before d_action
        assert re.search(r"[(,]\s*void \*d_original.*[(,]\s*void \*d_recovery.*const uint8_t \*recovery_check,\s*"
                         r"uint32_t max_outliers,\s*uint32_t mode,\s*uint32_t max_rows,\s*int32_t \*d_located,\s*"
                         r"uint8_t \*d_mismatch,\s*uint8_t \*d_outlier,\s*uint8_t \*d_action,\s*void \*stream,\s*"
                         r"rs_error \*err", proto.group(1), re.S), name
    batch = re.search(r"rs_heal_device_robust_batch\s*\(([^;]*)\)", header).group(1)
    for arg in ("uint64_t stripes", "original_stripe_stride", "recovery_stripe_stride"):
        assert arg in batch, arg
    # the heal's arguments with two more
    assert len(rs._lib.rs_heal_device_robust.argtypes) == len(rs._lib.rs_heal_device.argtypes) + 2 == 19
    assert len(rs._lib.rs_heal_device_robust_batch.argtypes) == len(rs._lib.rs_heal_device_batch.argtypes) + 2 == 22
    for k, fn in ((10, rs._lib.rs_heal_device_robust), (13, rs._lib.rs_heal_device_robust_batch)):
        assert fn.argtypes[k:k + 3] == [ctypes.c_uint32] * 3
    for name in ("heal_device_robust", "heal_device_robust_batch"):
        assert callable(getattr(rs, name)), name


def test_header_states_the_contract_and_the_caveats():
    header = open(HEADER).read()
    heal = header[header.index("---- robust heal:"):header.index("rs_status rs_heal_device_robust(")]
    for phrase in ("AS FOUND", "Every byte of d_action is defined", "it is a bit set", "RS_HEAL_ORIGINAL | RS_HEAL_RECOVERY",
                   "the first selected row\n *                     outside B", "not the\n *                     row padding",
                   "a zero coefficient contributes\n *                     nothing", "max_rows does not apply",
                   "every selected row agrees afterwards", "s + 1 + t <= c", "byte-identical to the clean stripe",
                   "RS_LOCATE_ROWS with exactly the rows of B flagged", "original i again",
                   "Nothing else is written anywhere", "an all-zero d_outlier", "With max_outliers == 0",
                   "CAVEATS", "does not prove\n * the originals intact", "not necessarily the true one",
                   "Keep t small against c", "d_outlier or d_action", "fewer than 3 with\n * RS_HEAL_ORIGINAL",
                   "stripes == 0: RS_OK", "must not overlap", "one k_heal_robust per group", "No\n * ordering hazard",
                   "Measured", "tools/heal_robust_time.py"):
        assert phrase in heal, phrase
    # neither "Not covered" list of the robust locate names the robust heal any more
    robust = header[header.index("---- robust locate"):header.index("#define RS_LOCATE_MAX_OUTLIERS")]
    not_covered = robust[robust.index("Not covered:"):]
    assert "robust heal" not in not_covered and "two or more" in not_covered
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.4g Robust locate"):design.index("### 4.4h Robust heal")]
    assert "robust heal" not in section[section.rindex("Not covered:"):]


@pytest.mark.parametrize("call", FORMS)
def test_argument_checks_precede_any_device_work(rs, call):
    """A made-up non-null context is never dereferenced: every check comes first, in the header's
    order.  (A batch call of no stripes returns RS_OK exactly when every check passes.)"""
    err = rs._RsError()
    e = ctypes.byref(err)
    fake = ctypes.c_void_p(8)
    # 1. null context, d_original, d_recovery, d_located, d_mismatch, d_outlier, d_action
    assert call(rs, None, 4, 4, 64, 8, 8, None, 1, 3, 8, 8, 8, 8, e) == 101 and err.code == 101
    for k in range(6):
        p = [8] * 6
        p[k] = 0
        assert call(rs, fake, 4, 4, 64, p[0], p[1], None, 1, 3, p[2], p[3], p[4], p[5], e) == 101, k
        assert _batch(rs, fake, 4, 4, 64, p[0], p[1], None, 1, 3, p[2], p[3], p[4], p[5], e, stripes=0) == 101, k
    err.code = 0  # ... ahead of rs_validate (a bad shard size here)
    assert call(rs, fake, 4, 4, 63, 8, 8, None, 1, 3, 8, 8, 0, 8, e) == 101 and err.code == 101
    assert call(rs, fake, 4, 4, 63, 8, 8, None, 1, 3, 8, 8, 8, 0, e) == 101 and err.code == 101
    # 2. rs_validate ahead of the strides, the mode, the row counts, max_outliers and the shape bound (all bad)
    assert call(rs, fake, 4, 1, 63, 8, 8, None, 9, 0, 8, 8, 8, 8, e, strides=(32, 0)) == 6 and err.shard_bytes == 63
    assert call(rs, fake, 4096, 61441, 64, 8, 8, bytes(61441), 9, 4, 8, 8, 8, 8, e, strides=(0, 32)) == 10
    assert (err.original_count, err.recovery_count) == (4096, 61441)
    # 3. the two row strides, each in turn
    for strides in ((32, 0), (0, 32)):
        assert call(rs, fake, 4, 4, 64, 8, 8, None, 1, 3, 8, 8, 8, 8, e, strides=strides) == 101 and err.code == 101
        assert _batch(rs, fake, 4, 4, 64, 8, 8, None, 1, 3, 8, 8, 8, 8, e, strides=strides, stripes=0) == 101
    # 4. the mode: none of the two bits, or a bit outside them
    for mode in (0, 4, 7, 8, 1 << 31):
        assert call(rs, fake, 4, 4, 64, 8, 8, None, 1, mode, 8, 8, 8, 8, e) == 101 and err.code == 101, mode
        assert _batch(rs, fake, 4, 4, 64, 8, 8, None, 0, mode, 8, 8, 8, 8, e, stripes=0) == 101, mode
    # 5. fewer than two rows; fewer than three where an original may be written (max_outliers = 0 fits both)
    for mode in (1, 2, 3):
        assert call(rs, fake, 4, 1, 64, 8, 8, None, 0, mode, 8, 8, 8, 8, e) == 101 and err.code == 101, mode
        assert call(rs, fake, 4, 4, 64, 8, 8, b"\0\1\0\0", 0, mode, 8, 8, 8, 8, e) == 101, mode
        assert call(rs, fake, 4, 4, 64, 8, 8, bytes(4), 0, mode, 8, 8, 8, 8, e) == 101, mode
    for mode in (1, 3):
        assert call(rs, fake, 4, 2, 64, 8, 8, None, 0, mode, 8, 8, 8, 8, e) == 101 and err.code == 101, mode
        assert _batch(rs, fake, 4, 4, 64, 8, 8, b"\1\0\0\1", 0, mode, 8, 8, 8, 8, e, stripes=0) == 101, mode
    assert _batch(rs, fake, 4, 2, 64, 8, 8, None, 0, 2, 8, 8, 8, 8, e, stripes=0) == 0 and err.code == 0
    assert _batch(rs, fake, 4, 4, 64, 8, 8, b"\1\0\0\1", 0, 2, 8, 8, 8, 8, e, stripes=0) == 0
    assert _batch(rs, fake, 4, 4, 64, 8, 8, b"\1\0\1\1", 0, 3, 8, 8, 8, 8, e, stripes=0) == 0
    # 6. max_outliers > 7, or 2 (1 + max_outliers) > c -- ahead of the shape bound
    assert call(rs, fake, 4, 100, 64, 8, 8, None, 8, 3, 8, 8, 8, 8, e) == 101 and err.code == 101
    assert call(rs, fake, 4, 100, 64, 8, 8, None, 0xFFFFFFFF, 3, 8, 8, 8, 8, e) == 101
    assert call(rs, fake, 4, 4, 64, 8, 8, None, 2, 3, 8, 8, 8, 8, e) == 101  # 6 > 4
    assert call(rs, fake, 4, 15, 64, 8, 8, None, 7, 3, 8, 8, 8, 8, e) == 101  # 16 > 15
    assert _batch(rs, fake, 4, 4, 64, 8, 8, b"\1\0\1\1", 1, 3, 8, 8, 8, 8, e, stripes=0) == 101  # 4 > 3 selected
    assert _batch(rs, fake, 4, 4, 64, 8, 8, b"\1\0\0\1", 1, 2, 8, 8, 8, 8, e, stripes=0) == 101  # 4 > 2
    assert call(rs, fake, 5000, 3, 64, 8, 8, None, 1, 3, 8, 8, 8, 8, e) == 101
    # 7. the locate's shape bound
    assert call(rs, fake, 4097, 4, 64, 8, 8, None, 1, 3, 8, 8, 8, 8, e) == 101 and err.code == 101
    assert call(rs, fake, 4096, 4097, 64, 8, 8, None, 1, 2, 8, 8, 8, 8, e) == 101
    assert _batch(rs, fake, 4097, 4, 64, 8, 8, None, 1, 3, 8, 8, 8, 8, e, stripes=0) == 101
    # a null err is allowed
    assert call(rs, fake, 4, 4, 64, 8, 8, None, 2, 3, 8, 8, 8, 8, None) == 101
    assert call(rs, fake, 4, 4, 64, 8, 8, None, 1, 4, 8, 8, 8, 8, None) == 101
    assert call(rs, None, 4, 4, 64, 8, 8, None, 1, 3, 8, 8, 8, 8, None) == 101


def test_no_stripes_is_ok_without_touching_anything(rs):
    err = rs._RsError()
    err.code = 55
    fake = ctypes.c_void_p(8)
    assert _batch(rs, fake, 4, 4, 64, 8, 8, None, 1, 3, 8, 8, 8, 8, ctypes.byref(err), stripes=0) == 0 and err.code == 0
    assert _batch(rs, fake, 4, 4, 64, 8, 8, b"\1\0\1\1", 0, 1, 8, 8, 8, 8, None, strides=(64, 128), stripes=0) == 0
    for max_rows in (0, 1, 0xFFFFFFFF):
        assert _batch(rs, fake, 4, 4, 64, 8, 8, None, 1, 2, 8, 8, 8, 8, None, stripes=0, max_rows=max_rows) == 0
    # the bounds themselves pass: 2 (1 + t) = c, t = 7, the largest shapes
    assert _batch(rs, fake, 4, 16, 64, 8, 8, None, 7, 3, 8, 8, 8, 8, None, stripes=0) == 0
    assert _batch(rs, fake, 4, 6, 64, 8, 8, b"\1\1\0\1\0\1", 1, 3, 8, 8, 8, 8, None, stripes=0) == 0
    assert _batch(rs, fake, 4096, 4096, 64, 8, 8, None, 7, 3, 8, 8, 8, 8, None, stripes=0) == 0


def test_wrappers_reject_wrong_arguments(rs):
    N, M, S, B = 8, 6, 64, 3
    ctx = types.SimpleNamespace(handle=None)
    loc = lambda *shape, **kw: _Fake(*shape, **dict({"dtype": "torch.int32"}, **kw))

    class _Host(_Fake):
        is_cuda = False

    def single(t=1, mask=None, mode=3, max_rows=1, o=_Fake(N, S), r=_Fake(M, S), located=loc(1), flags=_Fake(M),
               outlier=_Fake(M), action=_Fake(1)):
        return rs.heal_device_robust(N, M, S, o, r, recovery_rows=mask, max_outliers=t, mode=mode, max_rows=max_rows,
                                     d_located=located, d_mismatch=flags, d_outlier=outlier, d_action=action, ctx=ctx)

    # the heal's own: mode, max_rows, the rows an original is written on
    for mode in (0, 4, 7, -1):
        with pytest.raises(ValueError, match="mode:"):
            single(mode=mode)
    for max_rows in (-1, 1 << 32):
        with pytest.raises(ValueError, match="max_rows:"):
            single(max_rows=max_rows)
    for mode in (1, 2, 3):
        with pytest.raises(ValueError, match="recovery_rows: a locate needs two"):
            single(t=0, mask=[0, 0, 1, 0, 0, 0], mode=mode)
    for mode in (1, 3):
        with pytest.raises(ValueError, match="recovery_rows: HEAL_ORIGINAL .* three"):
            single(t=0, mask=[1, 0, 0, 0, 0, 1], mode=mode)
    with pytest.raises(ValueError, match="recovery_rows"):
        single(mask=[1] * (M + 1))
    # the robust locate's own: max_outliers above 7, negative, more than the selected rows allow
    for t in (8, -1, 1 << 32):
        with pytest.raises(ValueError, match="max_outliers: 0 .. 7"):
            single(t=t)
    with pytest.raises(ValueError, match="max_outliers: 3 outliers need 8 selected"):
        single(t=3)
    with pytest.raises(ValueError, match="max_outliers: 2 outliers need 6 selected"):
        single(t=2, mask=[1, 1, 1, 0, 1, 1])
    with pytest.raises(ValueError, match="max_outliers: 1 outliers need 4 selected"):
        single(t=1, mask=[1, 0, 0, 0, 0, 1], mode=2)
    # the matrices and the four outputs
    with pytest.raises(ValueError, match="d_original:"):
        single(o=_Fake(N - 1, S))
    with pytest.raises(ValueError, match="d_original:"):
        single(o=_Fake(2, N, S))
    with pytest.raises(ValueError, match="d_recovery: dtype"):
        single(r=_Fake(M, S, dtype="torch.int32"))
    for bad in (loc(2), loc(1, 1), _Fake(1), loc(1, contiguous=False)):
        with pytest.raises(ValueError, match="d_located"):
            single(located=bad)
    for bad in (_Fake(M - 1), _Fake(M + 1), _Fake(1, M), _Fake(M, dtype="torch.bool")):
        with pytest.raises(ValueError, match="d_mismatch"):
            single(flags=bad)
    for bad in (_Fake(M - 1), _Fake(M + 1), _Fake(1, M), _Fake(M, dtype="torch.bool"), _Fake(M, contiguous=False)):
        with pytest.raises(ValueError, match="d_outlier"):
            single(outlier=bad)
    for bad in (_Fake(2), _Fake(1, 1), _Fake(1, dtype="torch.int32"), _Fake(1, contiguous=False), _Host(1)):
        with pytest.raises(ValueError, match="d_action"):
            single(action=bad)
    with pytest.raises(ValueError, match="d_located"):  # raw pointers: nothing says where to allocate
        rs.heal_device_robust(N, M, S, 8, 8, ctx=ctx)
    with pytest.raises(ValueError, match="d_outlier"):
        rs.heal_device_robust(N, M, S, 8, 8, d_located=8, d_mismatch=8, ctx=ctx)
    with pytest.raises(ValueError, match="d_action"):
        rs.heal_device_robust(N, M, S, 8, 8, d_located=8, d_mismatch=8, d_outlier=8, ctx=ctx)
    with pytest.raises(rs.UnsupportedShardCount):  # the reference's own checks come first
        rs.heal_device_robust(4096, 61441, S, _Fake(1, S), _Fake(1, S), max_outliers=9, mode=0, ctx=ctx)
    # well-formed arguments reach the library (whose first check refuses the null context)
    for kw in ({}, {"t": 0}, {"t": 2}, {"t": 1, "mask": [1, 0, 1, 1, 0, 1]}, {"t": 0, "mask": [1, 0, 0, 0, 1, 0], "mode": 2},
               {"mode": 1, "max_rows": 0}):
        with pytest.raises(ValueError, match="rs_status 101"):
            single(**kw)
    with pytest.raises(ValueError, match="rs_status 101"):
        rs.heal_device_robust(N, M, S, 8, 8, d_located=8, d_mismatch=8, d_outlier=8, d_action=8, ctx=ctx)

    def batch(t=1, mask=None, mode=3, o=_Fake(B, N, S), r=_Fake(B, M, S), located=loc(B), flags=_Fake(B, M),
              outlier=_Fake(B, M), action=_Fake(B)):
        return rs.heal_device_robust_batch(N, M, S, o, r, recovery_rows=mask, max_outliers=t, mode=mode, max_rows=2,
                                           d_located=located, d_mismatch=flags, d_outlier=outlier, d_action=action,
                                           ctx=ctx)

    with pytest.raises(ValueError, match="max_outliers"):
        batch(t=3)
    with pytest.raises(ValueError, match="mode:"):
        batch(mode=0)
    with pytest.raises(ValueError, match="recovery_rows"):
        batch(mask=np.ones((B, M), np.uint8))  # one mask for the whole batch
    with pytest.raises(ValueError, match="d_recovery:"):
        batch(r=_Fake(M, S))
    with pytest.raises(ValueError, match="stripe count"):
        batch(o=_Fake(B + 1, N, S))
    for bad in (loc(1), loc(B + 1), loc(B, 1), _Fake(B)):
        with pytest.raises(ValueError, match="d_located"):
            batch(located=bad)
    for bad in (_Fake(M), _Fake(B, M + 1), _Fake(B + 1, M), _Fake(B * M)):
        with pytest.raises(ValueError, match="d_mismatch"):
            batch(flags=bad)
        with pytest.raises(ValueError, match="d_outlier"):
            batch(outlier=bad)
    for bad in (_Fake(1), _Fake(B + 1), _Fake(B, 1), loc(B), _Host(B)):
        with pytest.raises(ValueError, match="d_action"):
            batch(action=bad)
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
        for must in ("void * d_original", "void * d_recovery", "uint32_t max_outliers", "uint32_t mode",
                     "uint32_t max_rows", "int32_t * d_located", "uint8_t * d_outlier", "uint8_t * d_action",
                     "const uint8_t * recovery_check"):
            assert must in params, (name, must)
        protos.append(f"rs_status {name}({', '.join(params)});")
        assert re.search(r'_sig\("%s"|lib\.%s\b' % (name, name), doc), name  # the ctypes side
    c = tmp_path / "heal_robust_bindings.c"
    c.write_text("\n".join(["#include <stdint.h>", f'#include "{HEADER}"'] + protos) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-c", str(c), "-o", str(tmp_path / "h.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + "\n" + c.read_text()
    assert "rs.heal_device_robust_batch(" in doc and "max_outliers=2" in doc


def test_docs_describe_the_call():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4.4h Robust heal"):]
    for phrase in ("k_heal_robust", "k_locate_decide", "linearity", "hazard", "Measured", "per symbol", "VGPR"):
        assert phrase in section, phrase
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "rs_heal_device_robust" in readme and "test_gpu_heal_robust.py" in readme
    assert "heal_robust" in open(os.path.join(ROOT, "profiles", "README.md")).read()


# ---------------------------------------------------------------------------
# the contract, on the model

SHAPES = [("high", 70, 100, 64), ("low", 100, 70, 66), ("default", 128, 128, 64)]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("rate,N,M,S", SHAPES, ids=lambda v: str(v))
def test_model_on_the_case_table(rate, N, M, S):
    clean_orig, clean_rec = RC.V.stripe(rate, N, M, S)
    G = LM.coefficients(rate, N, M)
    healed = both = 0
    seen = set()
    for case in RC.cases(rate, N, M, S, ts=(1, 2)):
        name, case_t, orig, rec, enc, intended = case
        RC.model(rate, case)  # the intended status, at the case's own t
        D = LM.elements(enc ^ rec).astype(np.int64)
        for t in (0, 1, 2):
            what = f"{name} / t={t}"
            run = lambda mode, max_rows=M - 1: HRM.heal(rate, orig, rec, t, mode=mode, max_rows=max_rows, want=enc)
            located, flags, outlier, action, o2, r2 = run(3)
            assert (located, flags.tolist(), outlier.tolist()) == tuple(
                x.tolist() if hasattr(x, "tolist") else x for x in RM.locate(rate, orig, rec, t, D=D)), what
            B = np.flatnonzero(outlier).tolist()
            seen.add("i" if located >= 0 else located)
            # max_outliers = 0 is the heal, whatever the mode and the threshold
            if t == 0:
                assert not outlier.any(), what
                for mode, max_rows in ((1, M - 1), (2, M - 1), (3, M - 1), (3, 0), (3, 1), (2, 2)):
                    got = run(mode, max_rows)
                    assert _same(got[:2] + got[3:], HM.heal(rate, orig, rec, mode=mode, max_rows=max_rows)), (what, mode)
            if located >= 0:
                i = located
                assert action == ORIGINAL | (RECOVERY if B else 0), what
                if intended is not None and t == case_t:
                    assert (i, B) == (intended[0], intended[1]), what
                # every case built as "located (i, B)" (and any damage inside the bound): the clean stripe
                assert np.array_equal(o2, clean_orig) and np.array_equal(r2, clean_rec), what
                healed += 1
                both += bool(B)
                # the same e from every reference row outside B
                e = HRM.error(rate, N, M, D, i, next(j for j in range(M) if not outlier[j]))
                assert e.any(), what
                for r in np.flatnonzero(outlier == 0):
                    assert np.array_equal(HRM.error(rate, N, M, D, i, int(r)), e), (what, r)
                # an outlier's own row gives another e where the row was hit
                for r in B:
                    assert G[r, i] == 0 or not np.array_equal(HRM.error(rate, N, M, D, i, r), e), (what, r)
                # RS_HEAL_ORIGINAL alone: the rows of B stay as found, and the next scan flags exactly them
                l1, _, out1, a1, o1, r1 = run(ORIGINAL)
                assert (l1, out1.tolist(), a1) == (i, outlier.tolist(), ORIGINAL), what
                assert np.array_equal(o1, clean_orig) and np.array_equal(r1, rec), what
                nxt = RM.locate(rate, o1, r1, t, D=LM.elements(clean_rec ^ r1).astype(np.int64))
                assert nxt[0] == (ROWS if B else CLEAN) and np.flatnonzero(nxt[1]).tolist() == B, what
                assert not nxt[2].any(), what
                # RS_HEAL_RECOVERY alone: the original stays as found, and the plain locate names it
                l2, _, out2, a2, o2, r2 = run(RECOVERY)
                assert (l2, out2.tolist(), a2) == (i, outlier.tolist(), RECOVERY if B else 0), what
                assert np.array_equal(o2, orig) and np.array_equal(r2[B], clean_rec[B]), what
                keep = np.setdiff1d(np.arange(M), B)
                assert np.array_equal(r2[keep], rec[keep]), what
                assert LM.locate(rate, o2, r2, D=LM.elements(enc ^ r2).astype(np.int64))[0] == i, what
            elif located == ROWS:
                # as the heal, around max_rows
                n = int(flags.sum())
                assert 0 < n < M and not outlier.any(), what
                for mode, max_rows, rewritten in ((3, n, True), (2, n, True), (3, 0xFFFFFFFF, True), (3, n - 1, False),
                                                  (3, 0, False), (1, n, False)):
                    got = run(mode, max_rows)
                    assert _same(got[:2] + got[3:], HM.heal(rate, orig, rec, mode=mode, max_rows=max_rows)), (what, mode)
                    assert got[3] == (RECOVERY if rewritten else 0) and np.array_equal(got[4], orig), (what, mode)
                    rows = np.flatnonzero(flags)
                    assert np.array_equal(got[5][rows], enc[rows] if rewritten else rec[rows]), (what, mode)
                    assert np.array_equal(np.delete(got[5], rows, 0), np.delete(rec, rows, 0)), (what, mode)
            else:
                # UNKNOWN and CLEAN: untouched, whatever the mode
                assert located in (UNKNOWN, CLEAN) and not outlier.any(), what
                for mode in (1, 2, 3):
                    got = run(mode, 0xFFFFFFFF)
                    assert got[3] == 0 and np.array_equal(got[4], orig) and np.array_equal(got[5], rec), (what, mode)
    assert seen == {"i", CLEAN, ROWS, UNKNOWN} and healed > 50 and both > 20, (seen, healed, both)


@pytest.mark.parametrize("rate,N,M,S", SHAPES[:2], ids=lambda v: str(v))
def test_model_under_a_mask(rate, N, M, S):
    """Every third row unselected with junk in it: never flagged, named or written; the healed
    stripe is the clean one in the originals and in every selected row."""
    mask = np.ones(M, np.uint8)
    mask[2::3] = 0
    sel, unsel = np.flatnonzero(mask), np.flatnonzero(mask == 0)
    clean_orig, clean_rec = RC.V.stripe(rate, N, M, S)
    healed = 0
    for case in RC.cases(rate, N, M, S, mask=mask, forms=("lastbit",), ts=(1, 2), junk=True):
        name, t, orig, rec, enc, intended = case
        want = RC.model(rate, case, mask=mask)
        located, flags, outlier, action, o2, r2 = HRM.heal(rate, orig, rec, t, mask=mask, mode=3, max_rows=2, want=enc)
        assert (located, flags.tolist(), outlier.tolist()) == (want[0], want[1].tolist(), want[2].tolist()), name
        assert np.array_equal(r2[unsel], rec[unsel]) and (rec[unsel] == 0xC3).all(), name
        if located >= 0:
            healed += 1
            assert action == ORIGINAL | (RECOVERY if outlier.any() else 0), name
            assert np.array_equal(o2, clean_orig) and np.array_equal(r2[sel], clean_rec[sel]), name
            # r is the first SELECTED row outside B
            r = int(next(j for j in sel if not outlier[j]))
            D = LM.elements(enc ^ rec).astype(np.int64)
            e = HM.shard_bytes_of(HRM.error(rate, N, M, D, located, r)[None, :].astype(np.uint16), S)[0]
            assert np.array_equal(orig[located] ^ e, clean_orig[located]), name
        elif located in (UNKNOWN, CLEAN):
            assert action == 0 and np.array_equal(o2, orig) and np.array_equal(r2, rec), name
    assert healed > 10


def test_model_on_a_tiny_stripe():
    """3:4 x 64: four rows allow one outlier; the original and the outlier row come back clean."""
    rate, N, M, S = "default", 3, 4, 64
    orig, rec = RC.V.stripe(rate, N, M, S)
    bad, r = orig.copy(), rec.copy()
    bad[1, 5] ^= 0x40
    r[2, 9] ^= 0x01
    located, flags, outlier, action, o2, r2 = HRM.heal(rate, bad, r, 1)
    assert (located, np.flatnonzero(outlier).tolist(), action) == (1, [2], 3) and flags.all()
    assert np.array_equal(o2, orig) and np.array_equal(r2, rec)
