"""rs_heal_device_batch_masks without a GPU: the symbol and its declaration, the argument checks (all
before any device work, in the header's order), the all-or-nothing refusal, the Python wrapper's
rejections, the INTEGRATION.md binding -- and the model: heal_model.heal applied stripe by stripe,
each with its own mask, gives the outcome the batch of tests/heal_masks_cases.py is built for, so
that a failure on the GPU is the kernels'.
"""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import heal_masks_cases as H
import locate_model as LM
import test_integration_abi as ABI
import verify_masks_cases as C
from test_verify_cpu import _Fake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rs_mi355x.h")
NAME = "rs_heal_device_batch_masks"


@pytest.fixture(scope="module")
def rs():
    import reed_solomon_simd
    return reed_solomon_simd


def _heal(rs, ctx, N, M, S, d_orig, d_rec, mask, mode, d_loc, d_flags, d_act, err=None, strides=(0, 0), stripes=2,
          max_rows=1, status=None):
    return rs._lib.rs_heal_device_batch_masks(ctx, 0, N, M, S, stripes, d_orig, strides[0], 0, d_rec, strides[1], 0,
                                              mask, mode, max_rows, d_loc, d_flags, d_act, status, None, err)


def _mask(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a.ctypes.data_as(ctypes.c_void_p), a  # (the array is kept alive by the caller)


def test_symbol_is_exported_and_declared(rs):
    header = open(HEADER).read()
    assert hasattr(rs._lib, NAME) and getattr(rs._lib, NAME).argtypes is not None
    proto = re.search(r"rs_status\s+%s\s*\(([^;]*)\)\s*;" % NAME, header)
    assert proto
    args = [" ".join(a.split()) for a in proto.group(1).split(",")]
    assert args == ["rs_context *ctx", "rs_rate rate", "uint64_t original_count", "uint64_t recovery_count",
                    "uint64_t shard_bytes", "uint64_t stripes", "void *d_original", "uint64_t original_stride",
                    "uint64_t original_stripe_stride", "void *d_recovery", "uint64_t recovery_stride",
                    "uint64_t recovery_stripe_stride", "const uint8_t *recovery_check", "uint32_t mode",
                    "uint32_t max_rows", "int32_t *d_located", "uint8_t *d_mismatch", "uint8_t *d_action",
                    "uint8_t *stripe_status", "void *stream", "rs_error *err"]
    assert len(getattr(rs._lib, NAME).argtypes) == 21
    assert callable(rs.heal_device_batch_masks)
    # the header's lists know the call, and the heal's "Not covered" points at it
    assert NAME in header.split("Device-resident batch entry points")[1].split("Thread-safety")[0]
    section = header[header.index("---- heal with a mask per stripe"):header.index("rs_status " + NAME)]
    flat = re.sub(r"\s*\n \*\s*", " ", section)
    for phrase in ("NOT NULL", "exactly as if rs_heal_device had been called", "never read and never written",
                   "stripe's own count of differing selected rows", "CAVEAT of rs_heal_device",
                   "err->index", "RS_LOCATE_SKIPPED and d_action[b] = 0", "must not overlap",
                   "shared every way", "k_heal_masks directly after the group's k_locate_confirm_masks",
                   "a memset at the start of the call", "Measured", "tools/heal_masks_time.py", "Not covered:"):
        assert phrase in flat, phrase
    heal = header[header.index("---- heal:"):header.index("#define RS_HEAL_ORIGINAL")]
    assert NAME in heal[heal.rindex("Not covered:"):]
    locate = header[header.index("---- locate with a mask per stripe"):header.index("#define RS_LOCATE_SKIPPED")]
    assert "rs_heal_device*" not in locate[locate.rindex("Not covered:"):] and NAME in locate
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.4l" in design and NAME in design[design.index("4.4l"):]


def test_argument_checks_precede_any_device_work(rs):
    """A made-up non-null context is never dereferenced: every check comes first, in the
    header's order."""
    err = rs._RsError()
    e = ctypes.byref(err)
    fake = ctypes.c_void_p(8)
    m, keep = _mask(np.ones((2, 4)))
    # 1. null context, d_original, d_recovery, d_located, d_mismatch, d_action -- and the mask
    assert _heal(rs, None, 4, 4, 64, 8, 8, m, 3, 8, 8, 8, e) == 101 and err.code == 101
    assert _heal(rs, fake, 4, 4, 64, 0, 8, m, 3, 8, 8, 8, e) == 101
    assert _heal(rs, fake, 4, 4, 64, 8, 0, m, 3, 8, 8, 8, e) == 101
    assert _heal(rs, fake, 4, 4, 64, 8, 8, m, 3, 0, 8, 8, e) == 101
    assert _heal(rs, fake, 4, 4, 64, 8, 8, m, 3, 8, 0, 8, e) == 101
    assert _heal(rs, fake, 4, 4, 64, 8, 8, m, 3, 8, 8, 0, e) == 101
    err.code = 0
    assert _heal(rs, fake, 4, 4, 64, 8, 8, None, 3, 8, 8, 8, e) == 101 and err.code == 101
    assert _heal(rs, fake, 4, 4, 63, 8, 8, None, 3, 8, 8, 8, e) == 101  # ... ahead of rs_validate
    assert _heal(rs, fake, 4, 4, 63, 8, 8, m, 3, 8, 8, 0, e) == 101
    # 2. rs_validate, ahead of the strides, the mode and the shape bounds (all bad here)
    assert _heal(rs, fake, 4, 1, 63, 8, 8, m, 0, 8, 8, 8, e, strides=(32, 0)) == 6 and err.shard_bytes == 63
    assert _heal(rs, fake, 4096, 61441, 64, 8, 8, m, 4, 8, 8, 8, e, strides=(0, 32)) == 10
    assert (err.original_count, err.recovery_count) == (4096, 61441)
    # 3. the two row strides, each in turn -- ahead of the mode, also with no stripes at all
    for strides in ((32, 0), (0, 32)):
        assert _heal(rs, fake, 4, 4, 64, 8, 8, m, 3, 8, 8, 8, e, strides=strides) == 101 and err.code == 101, strides
        assert _heal(rs, fake, 4, 4, 64, 8, 8, m, 0, 8, 8, 8, e, strides=strides) == 101, strides
        assert _heal(rs, fake, 4, 4, 64, 8, 8, m, 3, 8, 8, 8, e, strides=strides, stripes=0) == 101, strides
    # 4. the mode: none of the two bits, or a bit outside them -- ahead of stripes == 0
    for mode in (0, 4, 7, 8, 1 << 31):
        assert _heal(rs, fake, 4, 4, 64, 8, 8, m, mode, 8, 8, 8, e) == 101 and err.code == 101, mode
        assert _heal(rs, fake, 4, 4, 64, 8, 8, m, mode, 8, 8, 8, e, stripes=0) == 101, mode
    # 5. stripes == 0: RS_OK, nothing touched -- ahead of the shape bounds (bad here) and the mask
    err.code = 55
    assert _heal(rs, fake, 4, 4, 64, 8, 8, m, 3, 8, 8, 8, e, stripes=0) == 0 and err.code == 0
    assert _heal(rs, fake, 4, 4, 64, 8, 8, m, 3, 8, 8, 8, None, stripes=0) == 0
    for mode in (1, 2, 3):
        assert _heal(rs, fake, 4, 1, 64, 8, 8, m, mode, 8, 8, 8, e, stripes=0) == 0, mode
    assert _heal(rs, fake, 4097, 4, 64, 8, 8, m, 3, 8, 8, 8, e, stripes=0) == 0
    assert _heal(rs, fake, 4096, 4097, 64, 8, 8, m, 2, 8, 8, 8, e, stripes=0) == 0
    # 6. recovery_count < need; the locate's shape bounds
    one, keep1 = _mask(np.ones((2, 1)))
    two, keep2 = _mask(np.ones((2, 2)))
    for mode in (1, 2, 3):
        assert _heal(rs, fake, 4, 1, 64, 8, 8, one, mode, 8, 8, 8, e) == 101 and err.code == 101, mode
    for mode in (1, 3):  # recovery_count 2 with the original bit: rejected, whatever the stripes select
        err.code, err.index = 0, 77
        assert _heal(rs, fake, 4, 2, 64, 8, 8, two, mode, 8, 8, 8, e) == 101 and err.code == 101, mode
    big, keep3 = _mask(np.ones((1, 4)))
    assert _heal(rs, fake, 4097, 4, 64, 8, 8, big, 3, 8, 8, 8, e, stripes=1) == 101  # RS_LOCATE_MAX_ORIGINALS
    assert _heal(rs, fake, 4096, 4097, 64, 8, 8, big, 2, 8, 8, 8, e, stripes=1) == 101  # RS_LOCATE_MAX_COEFFICIENTS
    assert _heal(rs, fake, 5000, 2, 64, 8, 8, two, 1, 8, 8, 8, e) == 101
    # ... and recovery_count 2 with the recovery bit alone is accepted past that point: the refusal
    # that follows is step 7's, and names the stripe
    short = np.ones((3, 2), np.uint8)
    short[2, 1] = 0
    m3, keep4 = _mask(short)
    err.index = 77
    assert _heal(rs, fake, 4, 2, 64, 8, 8, m3, 2, 8, 8, 8, e, stripes=3) == 101 and err.index == 2
    # a null err is allowed
    assert _heal(rs, None, 4, 4, 64, 8, 8, m, 3, 8, 8, 8, None) == 101
    assert _heal(rs, fake, 4, 4, 64, 8, 8, m, 4, 8, 8, 8, None) == 101
    assert _heal(rs, fake, 4, 2, 64, 8, 8, m3, 2, 8, 8, 8, None, stripes=3) == 101
    del keep, keep1, keep2, keep3, keep4


def test_all_or_nothing_names_the_first_stripe_that_cannot_be_healed(rs):
    """7. every stripe's count, in stripe order, against the heal's own rule -- three rows with the
    original bit, else two -- without touching the (made-up) context or any of the made-up pointers."""
    err = rs._RsError()
    e = ctypes.byref(err)
    fake = ctypes.c_void_p(8)
    M = 6
    masks = np.concatenate([H.heal_masks(M), H.heal_masks(M)[1:2]])  # a ninth stripe: one row again
    assert masks.sum(axis=1).tolist()[:4] == [M, 1, 2, 3]
    m, keep = _mask(masks)
    for mode in (1, 3):
        err.index = 99
        assert _heal(rs, fake, 8, M, 64, 8, 8, m, mode, 8, 8, 8, e, stripes=9) == 101 and err.code == 101
        assert err.index == 1
    keep[1] = 1  # stripe 1's mask widened: stripe 2, with two rows, is the first now
    for mode in (1, 3):
        err.index = 99
        assert _heal(rs, fake, 8, M, 64, 8, 8, m, mode, 8, 8, 8, e, stripes=9) == 101 and err.index == 2
    # the recovery bit alone: two rows do, so stripe 2 passes and the ninth stripe is named
    err.index = 99
    assert _heal(rs, fake, 8, M, 64, 8, 8, m, 2, 8, 8, 8, e, stripes=9) == 101 and err.index == 8
    keep[1] = H.heal_masks(M)[1]
    err.index = 99
    assert _heal(rs, fake, 8, M, 64, 8, 8, m, 2, 8, 8, 8, e, stripes=9) == 101 and err.index == 1
    assert _heal(rs, fake, 8, M, 64, 8, 8, m, 2, 8, 8, 8, None, stripes=9) == 101
    del keep


def test_wrapper_rejects_wrong_shapes_dtypes_modes_and_masks(rs):
    N, M, S, B = 8, 6, 64, 3
    ctx = types.SimpleNamespace(handle=None)
    good = lambda: [_Fake(B, N, S), _Fake(B, M, S)]
    ones = np.ones((B, M), np.uint8)
    loc = lambda *shape, **kw: _Fake(*shape, **dict({"dtype": "torch.int32"}, **kw))

    class _Host(_Fake):
        is_cuda = False

    def heal(t, mask=ones, mode=3, max_rows=2, located=loc(B), flags=_Fake(B, M), action=_Fake(B), status=False):
        return rs.heal_device_batch_masks(N, M, S, t[0], t[1], mask, mode=mode, max_rows=max_rows, d_located=located,
                                          d_mismatch=flags, d_action=action, status=status, ctx=ctx)

    for bad in (np.ones(M, np.uint8), np.ones((B + 1, M), np.uint8), np.ones((B, M - 1), np.uint8),
                np.ones((M, B), np.uint8), [1] * M, None):
        with pytest.raises(ValueError, match="recovery_rows"):
            heal(good(), mask=bad)
    for k, name in enumerate(("d_original", "d_recovery")):
        t = good()
        t[k] = _Fake((N, M)[k], S)  # a matrix where a batch belongs
        with pytest.raises(ValueError, match=name + ":"):
            heal(t)
        t[k] = _Fake(B, (N, M)[k] - 1, S)
        with pytest.raises(ValueError, match=name + ":"):
            heal(t)
        t[k] = _Fake(B, (N, M)[k], S, dtype="torch.int32")
        with pytest.raises(ValueError, match=name + ": dtype"):
            heal(t)
        t[k] = _Fake(B + 1, (N, M)[k], S)
        with pytest.raises(ValueError, match="stripe count"):
            heal(t)
    for mode in (0, 4, 7, -1):
        with pytest.raises(ValueError, match="mode:"):
            heal(good(), mode=mode)
    for max_rows in (-1, 1 << 32):
        with pytest.raises(ValueError, match="max_rows:"):
            heal(good(), max_rows=max_rows)
    for bad in (loc(1), loc(B + 1), loc(B, 1), _Fake(B), loc(B, contiguous=False)):
        with pytest.raises(ValueError, match="d_located"):
            heal(good(), located=bad)
    for bad in (_Fake(M), _Fake(B, M + 1), _Fake(B + 1, M), _Fake(B * M), _Fake(B, M, dtype="torch.bool")):
        with pytest.raises(ValueError, match="d_mismatch"):
            heal(good(), flags=bad)
    for bad in (_Fake(1), _Fake(B + 1), _Fake(B, 1), loc(B), _Host(B)):
        with pytest.raises(ValueError, match="d_action"):
            heal(good(), action=bad)
    for mode, count in ((1, 2), (3, 2), (2, 1)):  # recovery_count below what the mode needs
        with pytest.raises(ValueError, match="recovery_rows: this heal needs"):
            rs.heal_device_batch_masks(N, count, S, _Fake(B, N, S), _Fake(B, count, S), np.ones((B, count), np.uint8),
                                       mode=mode, ctx=ctx)
    with pytest.raises(rs.UnsupportedShardCount):  # the reference's own checks come first
        rs.heal_device_batch_masks(4096, 61441, S, _Fake(1, 1, S), _Fake(1, 1, S), np.ones((1, 61441), np.uint8),
                                   mode=0, ctx=ctx)
    # well-formed arguments reach the library (whose first check refuses the null context)
    for status in (False, True):
        with pytest.raises(ValueError, match="rs_status 101"):
            heal(good(), status=status)
    with pytest.raises(ValueError, match="rs_status 101"):
        heal(good(), mode=2, max_rows=0xFFFFFFFF)


def test_integration_doc_binds_the_entry_point(tmp_path):
    """The Rust prototype of INTEGRATION.md compiles against the header, and the ctypes and Python
    lines name the call."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    types_ = dict(ABI.TYPES, **{"*mut i32": "int32_t *"})  # (as tests/test_locate_cpu.py: d_located)
    m = re.search(r"fn\s+%s\s*\((.*?)\)\s*->\s*RsStatus;" % NAME, doc, flags=re.S)
    assert m
    params = []
    for a in filter(None, (x.strip() for x in " ".join(m.group(1).split()).split(","))):
        pname, ptype = (x.strip() for x in a.split(":", 1))
        params.append(f"{types_[ptype]} {pname}")
    for must in ("void * d_original", "void * d_recovery", "const uint8_t * recovery_check", "uint32_t mode",
                 "uint32_t max_rows", "int32_t * d_located", "uint8_t * d_mismatch", "uint8_t * d_action",
                 "uint8_t * stripe_status"):
        assert must in params, must
    assert len(params) == 21
    assert re.search(r"lib\.%s\b" % NAME, doc) and "rs.heal_device_batch_masks(" in doc
    c = tmp_path / "heal_masks.c"
    c.write_text("\n".join(["#include <stddef.h>", "#include <stdint.h>", f'#include "{HEADER}"',
                            f"rs_status {NAME}({', '.join(params)});"]) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-c", str(c), "-o", str(tmp_path / "m.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + "\n" + c.read_text()


def test_mask_set_holds_what_the_batch_is_built_on():
    for M in (5, 70, 100, 200, 1024, 4096):
        m = H.heal_masks(M)
        assert len(m) == 8 and m[0].all()
        assert np.flatnonzero(m[1]).tolist() == [0] and np.flatnonzero(m[2]).tolist() == [0, M - 1]
        assert np.flatnonzero(m[3]).tolist() == [0, M // 2, M - 1]
        assert not m[4][1::3].any() and m[4].sum() == M - len(range(1, M, 3))
        assert np.flatnonzero(m[5])[0] == 2 and m[5].sum() == M - 2
        assert np.flatnonzero(m[6] == 0).tolist() == [1]
        assert not m[7][[0, 2]].any() and m[7][1] == 1 and (M <= 8 or not m[7][M // 2::5].any())
        assert np.array_equal(m[7], C.locate_masks(M)[7])
        # need = 3 skips stripes 1 and 2, need = 2 stripe 1 alone
        assert [int(r.sum() >= 3) for r in m] == [1, 0, 0, 1, 1, 1, 1, 1]
        assert [int(r.sum() >= 2) for r in m] == [1, 0, 1, 1, 1, 1, 1, 1]


@pytest.mark.parametrize("rate,N,M,S,pad", C.FUSED + C.UNFUSED, ids=lambda v: str(v))
def test_model_gives_the_intended_outcome(rate, N, M, S, pad):
    """heal_model.heal per stripe, each with its own mask, both bits and max_rows = 2: (located,
    action) are the ones the batch is built for; the healed located stripes are byte-identical to
    the clean ones; stripe 6 has exactly two flagged rows and equals the oracle's recovery on its
    selected rows afterwards; a second model heal is CLEAN with action 0."""
    origs, recs, store, held, masks = H.heal_batch(rate, N, M, S)
    want_loc, want_act = H.heal_intent(N)
    loc, flags, act, o2, r2, codes = H.model(rate, N, M, S)
    assert loc.tolist() == want_loc.tolist(), (loc.tolist(), want_loc.tolist())
    assert act.tolist() == want_act.tolist()
    assert codes.tolist() == [0, 101, 101, 0, 0, 0, 0, 0]
    for b in (0, 3, 5):
        assert np.array_equal(o2[b], origs[b]) and np.array_equal(r2[b], held[b]), b
        assert flags[b].tolist() == masks[b].tolist(), b  # every selected row differed
    for b in (1, 2, 4, 7):
        assert np.array_equal(o2[b], store[b]) and np.array_equal(r2[b], held[b]), b
    assert not flags[[1, 2, 7]].any() and flags[4].tolist() == masks[4].tolist()
    sel6 = np.flatnonzero(masks[6])
    assert np.flatnonzero(flags[6]).tolist() == [sel6[0], sel6[-1]]
    assert np.array_equal(o2[6], origs[6]) and np.array_equal(r2[6][sel6], recs[6][sel6])
    assert np.array_equal(r2[6, 1], held[6, 1]) and not np.array_equal(held[6, 1], recs[6, 1])  # the junk stays
    # the junk of every stripe's unselected rows is where it was
    for b in range(len(masks)):
        assert np.array_equal(r2[b][masks[b] == 0], held[b][masks[b] == 0]), b
    # a second heal: nothing left to do on the healed stripes
    again = H.model(rate, N, M, S, store=o2, held=r2)
    assert again[0].tolist() == [C.CLEAN, C.SKIPPED, C.SKIPPED, C.CLEAN, C.UNKNOWN, C.CLEAN, C.CLEAN, C.CLEAN]
    assert not again[2].any() and np.array_equal(again[3], o2) and np.array_equal(again[4], r2)
    # the recovery bit alone: stripe 2 (two rows) is located and untouched, no original is written
    loc2, _, act2, o3, r3, codes2 = H.model(rate, N, M, S, mode=H.RECOVERY)
    assert loc2.tolist() == [0, C.SKIPPED, N // 2, N // 2, C.UNKNOWN, N - 1, C.ROWS, C.CLEAN]
    assert act2.tolist() == [0, 0, 0, 0, 0, 0, H.RECOVERY, 0] and codes2.tolist() == [0, 101, 0, 0, 0, 0, 0, 0]
    assert np.array_equal(o3, store) and np.array_equal(r3[6], r2[6])
    assert LM.ROWS == C.ROWS
