"""rs_heal_device* without a GPU: the symbols and their declarations, the argument checks (all of
which come before any device work, in the header's order), the no-op case, the Python wrappers'
argument checks, the INTEGRATION.md binding, and the contract's properties on the numpy model
(tests/heal_model.py, built on the CPU oracle and tests/locate_model.py):

    a located original i:  original_i ^ (D_j0 / G[j0][i])  is the clean shard when i alone was corrupt
    a ROWS stripe:         its flagged rows rewritten from the encode of the STORED originals --
                           which makes the stripe consistent, not the originals right (the caveat)
"""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import heal_model as HM
import locate_model as LM
import oracle_lib as O
import test_integration_abi as ABI
from test_verify_cpu import _Fake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rs_heal_device", "rs_heal_device_batch")
HEADER = os.path.join(ROOT, "include", "rs_mi355x.h")


@pytest.fixture(scope="module")
def rs():
    # (imported by the tests that use it, not while pytest collects: tests/test_batch_masks_cpu.py)
    import reed_solomon_simd
    return reed_solomon_simd


def _single(rs, ctx, N, M, S, d_orig, d_rec, mask, mode, d_loc, d_flags, d_act, err=None, strides=(0, 0),
            stripes=None, max_rows=1):
    return rs._lib.rs_heal_device(ctx, 0, N, M, S, d_orig, strides[0], d_rec, strides[1], mask, mode, max_rows, d_loc,
                                  d_flags, d_act, None, err)


def _batch(rs, ctx, N, M, S, d_orig, d_rec, mask, mode, d_loc, d_flags, d_act, err=None, strides=(0, 0), stripes=2,
           max_rows=1):
    return rs._lib.rs_heal_device_batch(ctx, 0, N, M, S, stripes, d_orig, strides[0], 0, d_rec, strides[1], 0, mask,
                                        mode, max_rows, d_loc, d_flags, d_act, None, err)


FORMS = [_single, _batch]


def test_symbols_are_exported_and_declared(rs):
    header = open(HEADER).read()
    for name in NAMES:
        assert hasattr(rs._lib, name), name
        assert getattr(rs._lib, name).argtypes is not None, name  # the ctypes signature is declared
        proto = re.search(r"rs_status\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert proto, name
        # the matrices are written: no const
        assert re.search(r"[(,]\s*void \*d_original.*[(,]\s*void \*d_recovery.*const uint8_t \*recovery_check,\s*"
                         r"uint32_t mode,\s*uint32_t max_rows,\s*int32_t \*d_located,\s*uint8_t \*d_mismatch,\s*"
                         r"uint8_t \*d_action,\s*void \*stream,\s*rs_error \*err", proto.group(1), re.S), name
    batch = re.search(r"rs_heal_device_batch\s*\(([^;]*)\)", header).group(1)
    for arg in ("uint64_t stripes", "original_stripe_stride", "recovery_stripe_stride"):
        assert arg in batch, arg
    assert len(rs._lib.rs_heal_device.argtypes) == 17 and len(rs._lib.rs_heal_device_batch.argtypes) == 20
    for name in ("heal_device", "heal_device_batch"):
        assert callable(getattr(rs, name)), name
    # the two mode bits, in the header, in Python and in the model
    for name, value in (("ORIGINAL", 1), ("RECOVERY", 2)):
        m = re.search(r"#define RS_HEAL_%s (\d+)u" % name, header)
        assert m and int(m.group(1)) == value == getattr(rs, "HEAL_" + name) == getattr(HM, name), name


def test_header_states_the_contract_and_the_caveat():
    header = open(HEADER).read()
    heal = header[header.index("---- heal:"):header.index("#define RS_HEAL_ORIGINAL")]
    for phrase in ("AS FOUND", "Every byte of d_action is defined", "not the row\n *                     padding",
                   "byte-identical", "0 never rewrites", "Nothing else is written anywhere",
                   # the caveat, plainly
                   "CAVEAT", "does not prove\n * the originals intact", "consistent with\n * CORRUPT originals",
                   "belong to the caller",
                   "fewer than 3 with RS_HEAL_ORIGINAL", "stripes == 0: RS_OK", "must not overlap",
                   "one k_heal per group", "Measured", "Not covered: a mask per stripe; stripes with missing originals"):
        assert phrase in heal, phrase
    # the locate no longer lists the write-back as missing
    locate = header[header.index("---- locate:"):header.index("#define RS_LOCATE_CLEAN")]
    assert "writing the correction e back" not in locate and "Not covered:" in locate


@pytest.mark.parametrize("call", FORMS)
def test_argument_checks_precede_any_device_work(rs, call):
    """A made-up non-null context is never dereferenced: every check comes first, in the
    header's order."""
    err = rs._RsError()
    e = ctypes.byref(err)
    fake = ctypes.c_void_p(8)
    # 1. null context, d_original, d_recovery, d_located, d_mismatch, d_action
    assert call(rs, None, 4, 4, 64, 8, 8, None, 3, 8, 8, 8, e) == 101 and err.code == 101
    assert call(rs, fake, 4, 4, 64, 0, 8, None, 3, 8, 8, 8, e) == 101
    assert call(rs, fake, 4, 4, 64, 8, 0, None, 3, 8, 8, 8, e) == 101
    assert call(rs, fake, 4, 4, 64, 8, 8, None, 3, 0, 8, 8, e) == 101
    assert call(rs, fake, 4, 4, 64, 8, 8, None, 3, 8, 0, 8, e) == 101
    assert call(rs, fake, 4, 4, 64, 8, 8, None, 3, 8, 8, 0, e) == 101
    # ... ahead of rs_validate (a bad shard size here)
    err.code = 0
    assert call(rs, fake, 4, 4, 63, 8, 8, None, 3, 8, 8, 0, e) == 101 and err.code == 101
    # 2. rs_validate: a bad shard size, an unsupported count -- ahead of the strides, the mode,
    # the row count and the shape bound (all bad here)
    assert call(rs, fake, 4, 1, 63, 8, 8, None, 0, 8, 8, 8, e, strides=(32, 0)) == 6 and err.shard_bytes == 63
    assert call(rs, fake, 4096, 61441, 64, 8, 8, bytes(61441), 4, 8, 8, 8, e, strides=(0, 32)) == 10
    assert (err.original_count, err.recovery_count) == (4096, 61441)
    # 3. the two row strides, each in turn -- ahead of the mode and the row count
    for strides in ((32, 0), (0, 32)):
        assert call(rs, fake, 4, 4, 64, 8, 8, None, 3, 8, 8, 8, e, strides=strides) == 101 and err.code == 101, strides
        assert call(rs, fake, 4, 4, 64, 8, 8, None, 0, 8, 8, 8, e, strides=strides) == 101, strides
        assert call(rs, fake, 4, 1, 64, 8, 8, None, 3, 8, 8, 8, e, strides=strides) == 101, strides
    # 4. the mode: none of the two bits, or a bit outside them -- ahead of the row count
    for mode in (0, 4, 7, 8, 1 << 31):
        assert call(rs, fake, 4, 4, 64, 8, 8, None, mode, 8, 8, 8, e) == 101 and err.code == 101, mode
        assert call(rs, fake, 4, 1, 64, 8, 8, None, mode, 8, 8, 8, e) == 101, mode
    # 5. fewer than two rows; fewer than three where an original may be written
    for mode in (1, 2, 3):
        assert call(rs, fake, 4, 1, 64, 8, 8, None, mode, 8, 8, 8, e) == 101 and err.code == 101, mode
        assert call(rs, fake, 4, 4, 64, 8, 8, b"\0\1\0\0", mode, 8, 8, 8, e) == 101, mode
        assert call(rs, fake, 4, 4, 64, 8, 8, bytes(4), mode, 8, 8, 8, e) == 101, mode
    for mode in (1, 3):  # two rows with RS_HEAL_ORIGINAL: rejected
        assert call(rs, fake, 4, 2, 64, 8, 8, None, mode, 8, 8, 8, e) == 101 and err.code == 101, mode
        assert call(rs, fake, 4, 4, 64, 8, 8, b"\1\0\0\1", mode, 8, 8, 8, e) == 101, mode
        assert _batch(rs, fake, 4, 4, 64, 8, 8, b"\1\0\0\1", mode, 8, 8, 8, e, stripes=0) == 101, mode
    assert call(rs, fake, 5000, 2, 64, 8, 8, None, 1, 8, 8, 8, e) == 101  # (... ahead of the shape bound)
    # two rows with RS_HEAL_RECOVERY alone: accepted
    assert _batch(rs, fake, 4, 2, 64, 8, 8, None, 2, 8, 8, 8, e, stripes=0) == 0 and err.code == 0
    assert _batch(rs, fake, 4, 4, 64, 8, 8, b"\1\0\0\1", 2, 8, 8, 8, e, stripes=0) == 0
    assert _batch(rs, fake, 4, 4, 64, 8, 8, b"\1\0\1\1", 3, 8, 8, 8, e, stripes=0) == 0
    # 6. the locate's shape bound
    assert call(rs, fake, 4097, 3, 64, 8, 8, None, 3, 8, 8, 8, e) == 101 and err.code == 101
    assert call(rs, fake, 4096, 4097, 64, 8, 8, None, 2, 8, 8, 8, e) == 101
    # all of them with no stripes at all, too
    assert _batch(rs, fake, 4, 4, 64, 8, 8, None, 3, 8, 8, 8, e, strides=(0, 63), stripes=0) == 101
    assert _batch(rs, fake, 4, 4, 64, 8, 8, None, 0, 8, 8, 8, e, stripes=0) == 101
    assert _batch(rs, fake, 4, 4, 64, 8, 8, b"\0\0\0\1", 2, 8, 8, 8, e, stripes=0) == 101
    assert _batch(rs, fake, 4097, 4, 64, 8, 8, None, 3, 8, 8, 8, e, stripes=0) == 101
    # a null err is allowed
    assert call(rs, fake, 4, 4, 64, 8, 8, None, 3, 8, 8, 8, None, strides=(0, 32)) == 101
    assert call(rs, fake, 4, 4, 64, 8, 8, None, 4, 8, 8, 8, None) == 101
    assert call(rs, None, 4, 4, 64, 8, 8, None, 3, 8, 8, 8, None) == 101


def test_no_stripes_is_ok_without_touching_anything(rs):
    err = rs._RsError()
    err.code = 55
    fake = ctypes.c_void_p(8)
    assert _batch(rs, fake, 4, 4, 64, 8, 8, None, 3, 8, 8, 8, ctypes.byref(err), stripes=0) == 0 and err.code == 0
    assert _batch(rs, fake, 4, 4, 64, 8, 8, b"\1\0\1\1", 1, 8, 8, 8, None, strides=(64, 128), stripes=0) == 0
    for max_rows in (0, 1, 0xFFFFFFFF):
        assert _batch(rs, fake, 4, 4, 64, 8, 8, None, 2, 8, 8, 8, None, stripes=0, max_rows=max_rows) == 0
    # the largest shapes inside the bound pass the checks
    assert _batch(rs, fake, 4096, 4096, 64, 8, 8, None, 3, 8, 8, 8, None, stripes=0) == 0
    assert _batch(rs, fake, 256, 65280, 64, 8, 8, None, 3, 8, 8, 8, None, stripes=0) == 0


def test_wrappers_reject_wrong_shapes_dtypes_modes_and_masks(rs):
    N, M, S, B = 8, 6, 64, 3
    ctx = types.SimpleNamespace(handle=None)
    names = ["d_original", "d_recovery"]
    rows = [N, M]
    good = lambda: [_Fake(N, S), _Fake(M, S)]
    loc = lambda *shape, **kw: _Fake(*shape, **dict({"dtype": "torch.int32"}, **kw))

    class _Host(_Fake):
        is_cuda = False

    def single(t, mask=None, mode=3, max_rows=1, located=loc(1), flags=_Fake(M), action=_Fake(1)):
        return rs.heal_device(N, M, S, t[0], t[1], recovery_rows=mask, mode=mode, max_rows=max_rows, d_located=located,
                              d_mismatch=flags, d_action=action, ctx=ctx)

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
    for mode in (0, 4, 7, -1):
        with pytest.raises(ValueError, match="mode:"):
            single(good(), mode=mode)
    for max_rows in (-1, 1 << 32):
        with pytest.raises(ValueError, match="max_rows:"):
            single(good(), max_rows=max_rows)
    with pytest.raises(ValueError, match="recovery_rows"):
        single(good(), mask=[1] * (M + 1))
    for few in ([0] * M, [0, 0, 1, 0, 0, 0]):
        for mode in (1, 2, 3):
            with pytest.raises(ValueError, match="recovery_rows: a locate needs two"):
                single(good(), mask=few, mode=mode)
    for mode in (1, 3):  # an original is written on three rows' evidence, no fewer
        with pytest.raises(ValueError, match="recovery_rows: HEAL_ORIGINAL .* three"):
            single(good(), mask=[1, 0, 0, 0, 0, 1], mode=mode)
        with pytest.raises(ValueError, match="recovery_rows: HEAL_ORIGINAL .* three"):
            rs.heal_device(N, 2, S, _Fake(N, S), _Fake(2, S), mode=mode, d_located=loc(1), d_mismatch=_Fake(2),
                           d_action=_Fake(1), ctx=ctx)
    # the outputs: exactly one int32 and one byte per stripe, contiguous, on the device
    for bad in (loc(2), loc(1, 1), _Fake(1), loc(1, dtype="torch.int64"), loc(1, contiguous=False)):
        with pytest.raises(ValueError, match="d_located"):
            single(good(), located=bad)
    for bad in (_Fake(M - 1), _Fake(M + 1), _Fake(1, M), _Fake(M, dtype="torch.bool"), _Fake(M, contiguous=False)):
        with pytest.raises(ValueError, match="d_mismatch"):
            single(good(), flags=bad)
    for bad in (_Fake(2), _Fake(1, 1), _Fake(1, dtype="torch.int32"), _Fake(1, dtype="torch.bool"),
                _Fake(1, contiguous=False), _Host(1)):
        with pytest.raises(ValueError, match="d_action"):
            single(good(), action=bad)
    with pytest.raises(ValueError, match="d_located"):  # raw pointers: nothing says where to allocate
        rs.heal_device(N, M, S, 8, 8, ctx=ctx)
    with pytest.raises(ValueError, match="d_action"):
        rs.heal_device(N, M, S, 8, 8, d_located=8, d_mismatch=8, ctx=ctx)
    with pytest.raises(rs.UnsupportedShardCount):  # the reference's own checks come first
        rs.heal_device(4096, 61441, S, _Fake(1, S), _Fake(1, S), mode=0, d_located=loc(1), d_mismatch=_Fake(1),
                       d_action=_Fake(1), ctx=ctx)
    # well-formed arguments reach the library (whose first check refuses the null context)
    with pytest.raises(ValueError, match="rs_status 101"):
        single(good())
    with pytest.raises(ValueError, match="rs_status 101"):
        single(good(), mask=[1, 0, 0, 1, 1, 0], mode=1, max_rows=0)
    with pytest.raises(ValueError, match="rs_status 101"):
        single(good(), mask=[1, 0, 0, 0, 1, 0], mode=2)  # two rows do for the recovery bit alone
    with pytest.raises(ValueError, match="rs_status 101"):
        rs.heal_device(N, M, S, 8, 8, d_located=8, d_mismatch=8, d_action=8, ctx=ctx)  # raw pointers throughout

    goodb = lambda: [_Fake(B, N, S), _Fake(B, M, S)]

    def batch(t, mask=None, mode=3, located=loc(B), flags=_Fake(B, M), action=_Fake(B)):
        return rs.heal_device_batch(N, M, S, t[0], t[1], recovery_rows=mask, mode=mode, max_rows=2, d_located=located,
                                    d_mismatch=flags, d_action=action, ctx=ctx)

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
    with pytest.raises(ValueError, match="mode:"):
        batch(goodb(), mode=0)
    for bad in (loc(1), loc(B + 1), loc(B, 1), _Fake(B)):
        with pytest.raises(ValueError, match="d_located"):
            batch(goodb(), located=bad)
    for bad in (_Fake(M), _Fake(B, M + 1), _Fake(B + 1, M), _Fake(B * M)):
        with pytest.raises(ValueError, match="d_mismatch"):
            batch(goodb(), flags=bad)
    for bad in (_Fake(1), _Fake(B + 1), _Fake(B, 1), loc(B), _Host(B)):
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
        for must in ("void * d_original", "void * d_recovery", "uint32_t mode", "uint32_t max_rows",
                     "int32_t * d_located", "uint8_t * d_action", "const uint8_t * recovery_check"):
            assert must in params, must
        protos.append(f"rs_status {name}({', '.join(params)});")
        assert re.search(r'_sig\("%s"|lib\.%s\b' % (name, name), doc), name  # the ctypes side
    c = tmp_path / "heal_bindings.c"
    c.write_text("\n".join(["#include <stdint.h>", f'#include "{HEADER}"'] + protos) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-c", str(c), "-o", str(tmp_path / "h.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + "\n" + c.read_text()
    assert "rs.heal_device_batch(" in doc and "HEAL_RECOVERY" in doc


# ---------------------------------------------------------------------------
# the contract's properties, on the model

def _stripe(rate, N, M, S, seed=1):
    orig = O.generate_original(N, S, seed)
    return orig, O.encode(rate, orig, M)


MODEL = [("default", 70, 100, 66), ("default", 100, 70, 64), ("default", 128, 128, 64)]


@pytest.mark.parametrize("rate,N,M,S", MODEL, ids=lambda v: str(v))
def test_model_heals_a_single_corrupt_original_to_the_clean_one(rate, N, M, S):
    orig, rec = _stripe(rate, N, M, S)
    rng = np.random.default_rng(N + M)
    third = (np.arange(M) % 3 != 1).astype(np.uint8)
    for i in sorted({0, N // 2, N - 1}):
        for whole in (False, True):
            bad = orig.copy()
            if whole:
                bad[i] = rng.integers(0, 256, S, dtype=np.uint8)
            else:
                bad[i, S - 1] ^= 0x80
            for mask in (None, third):
                located, flags, action, o2, r2 = HM.heal(rate, bad, rec, mask=mask, mode=3, max_rows=M - 1)
                assert located == i and action == HM.ORIGINAL
                assert np.array_equal(flags != 0, np.ones(M, bool) if mask is None else mask != 0)
                assert np.array_equal(o2, orig) and np.array_equal(r2, rec)
                assert LM.locate(rate, o2, r2, mask=mask)[0] == LM.CLEAN
            # the bit off: reported, untouched
            located, _, action, o2, r2 = HM.heal(rate, bad, rec, mode=HM.RECOVERY, max_rows=M - 1)
            assert located == i and action == 0 and np.array_equal(o2, bad) and np.array_equal(r2, rec)


@pytest.mark.parametrize("rate,N,M,S", MODEL, ids=lambda v: str(v))
def test_model_heals_a_rows_stripe_within_the_threshold(rate, N, M, S):
    orig, rec = _stripe(rate, N, M, S)
    bad = rec.copy()
    bad[0, 0] ^= 1
    bad[M - 1, S - 1] ^= 0x80
    for max_rows, mode, healed in ((2, 2, True), (2, 3, True), (M - 1, 2, True), (1, 3, False), (0, 3, False),
                                   (2, 1, False)):
        located, flags, action, o2, r2 = HM.heal(rate, orig, bad, mode=mode, max_rows=max_rows)
        assert located == LM.ROWS and np.flatnonzero(flags).tolist() == [0, M - 1]
        assert np.array_equal(o2, orig)
        if healed:
            assert action == HM.RECOVERY and np.array_equal(r2, rec)
            assert LM.locate(rate, o2, r2)[0] == LM.CLEAN
        else:
            assert action == 0 and np.array_equal(r2, bad)
    # a corrupt unselected row is neither flagged nor rewritten
    mask = np.ones(M, np.uint8)
    mask[0] = 0
    located, flags, action, o2, r2 = HM.heal(rate, orig, bad, mask=mask, mode=3, max_rows=1)
    assert located == LM.ROWS and action == HM.RECOVERY and np.flatnonzero(flags).tolist() == [M - 1]
    assert np.array_equal(r2[1:], rec[1:]) and np.array_equal(r2[0], bad[0])
    # UNKNOWN and CLEAN: untouched
    for o, r, status in ((orig, rec ^ 1, LM.UNKNOWN), (orig, rec, LM.CLEAN)):
        located, _, action, o2, r2 = HM.heal(rate, o, r, mode=3, max_rows=M - 1)
        assert located == status and action == 0 and np.array_equal(o2, o) and np.array_equal(r2, r)


def test_model_recovery_heal_can_bless_corrupt_originals():
    """The caveat, pinned on the case of the locate's header: at 128:128, original 0 off by 1 and
    the last original off by 2 in one column come back as ROWS (some recovery row matches by
    coincidence).  RS_HEAL_RECOVERY then rewrites the differing rows from the encode of those
    CORRUPT originals: the stripe is CLEAN afterwards and its originals are still wrong."""
    rate, N, M, S = "default", 128, 128, 64
    orig, rec = _stripe(rate, N, M, S)
    bad = orig.copy()
    bad[0, 0] ^= 1
    bad[N - 1, 0] ^= 2
    status, flags = LM.locate(rate, bad, rec)
    assert status == LM.ROWS and 0 < flags.sum() < M  # (the status first, as the locate's tests do)
    located, flags2, action, o2, r2 = HM.heal(rate, bad, rec, mode=HM.RECOVERY, max_rows=int(flags.sum()))
    assert located == LM.ROWS and np.array_equal(flags2, flags) and action == HM.RECOVERY
    assert LM.locate(rate, o2, r2)[0] == LM.CLEAN
    assert np.array_equal(o2, bad) and not np.array_equal(o2, orig)
    assert not np.array_equal(r2, rec) and np.array_equal(r2[flags == 0], rec[flags == 0])
    # one row below the count, and the threshold holds it back
    assert HM.heal(rate, bad, rec, mode=3, max_rows=int(flags.sum()) - 1)[2] == 0
