"""rs_update_device* without a GPU: the symbols and their declarations, the argument checks (all
of which come before any device work, in the header's order), the no-op cases, the Python
wrappers' argument checks, the INTEGRATION.md binding, and a pure-CPU statement of the identity
the kernels rely on,

    recovery_j(new) = recovery_j(old) ^ XOR_c G[j][index_c] * (old_c ^ new_c),

with G read from the oracle's encode of the unit stripe in the layout the coefficient kernels use
(64 * ceil(count / 32) bytes per shard, element c of row index[c] = 1) and the product taken as
Engine::mul does, x * exp(log g).
"""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import oracle_lib as O
import test_integration_abi as ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rs_update_device", "rs_update_device_batch", "rs_update_set_direct_max")
HEADER = os.path.join(ROOT, "include", "rs_mi355x.h")


@pytest.fixture(scope="module")
def rs():
    # (imported by the tests that use it, not while pytest collects: tests/test_batch_masks_cpu.py)
    import reed_solomon_simd
    return reed_solomon_simd


def _idx(*values):
    return (ctypes.c_uint64 * len(values))(*values)


def _single(rs, ctx, N, M, S, index, count, d_old, d_new, d_rec, mask, err=None, strides=(0, 0, 0), stripes=None):
    return rs._lib.rs_update_device(ctx, 0, N, M, S, index, count, d_old, strides[0], d_new, strides[1], d_rec,
                                    strides[2], mask, None, err)


def _batch(rs, ctx, N, M, S, index, count, d_old, d_new, d_rec, mask, err=None, strides=(0, 0, 0), stripes=2):
    return rs._lib.rs_update_device_batch(ctx, 0, N, M, S, stripes, index, count, d_old, strides[0], 0, d_new,
                                          strides[1], 0, d_rec, strides[2], 0, mask, None, err)


FORMS = [_single, _batch]


def test_symbols_are_exported_and_declared(rs):
    header = open(HEADER).read()
    for name in NAMES:
        assert hasattr(rs._lib, name), name
        assert getattr(rs._lib, name).argtypes is not None, name  # the ctypes signature is declared
        assert re.search(r"rs_status\s+%s\s*\(([^;]*)\)\s*;" % name, header), name
    for name in NAMES[:2]:
        proto = re.search(r"rs_status\s+%s\s*\(([^;]*)\)\s*;" % name, header).group(1)
        assert re.search(r"const uint64_t \*index,\s*uint64_t count.*const void \*d_old.*const void \*d_new.*"
                         r"void \*d_recovery.*const uint8_t \*recovery_update,\s*void \*stream", proto, re.S), name
    batch = re.search(r"rs_update_device_batch\s*\(([^;]*)\)", header).group(1)
    for arg in ("uint64_t stripes", "old_stripe_stride", "new_stripe_stride", "recovery_stripe_stride"):
        assert arg in batch, arg
    assert len(rs._lib.rs_update_device.argtypes) == 16 and len(rs._lib.rs_update_device_batch.argtypes) == 20
    # the wrappers, and one default in both places
    for name in ("update_device", "update_device_batch", "update_set_direct_max"):
        assert callable(getattr(rs, name)), name
    default = int(re.search(r"#define RS_UPDATE_DIRECT_MAX_DEFAULT (\d+)", header).group(1))
    assert rs.UPDATE_DIRECT_MAX_DEFAULT == default
    assert "must NOT overlap d_recovery" in header


@pytest.mark.parametrize("call", FORMS)
def test_argument_checks_precede_any_device_work(rs, call):
    """A made-up non-null context is never dereferenced: every check comes first, in the
    header's order."""
    err = rs._RsError()
    e = ctypes.byref(err)
    fake = ctypes.c_void_p(8)
    idx = _idx(1, 3)
    # 1. null context, d_new, d_recovery, and a null index list with count > 0
    assert call(rs, None, 4, 4, 64, idx, 2, 8, 8, 8, None, e) == 101 and err.code == 101
    assert call(rs, fake, 4, 4, 64, idx, 2, 8, 0, 8, None, e) == 101
    assert call(rs, fake, 4, 4, 64, idx, 2, 8, 8, 0, None, e) == 101
    assert call(rs, fake, 4, 4, 64, None, 2, 8, 8, 8, None, e) == 101
    # ... ahead of rs_validate (a bad shard size here)
    assert call(rs, fake, 4, 4, 63, None, 2, 8, 8, 8, None, e) == 101
    # 2. rs_validate: a bad shard size, an unsupported count (src/rate.rs:91-106) -- ahead of
    # the strides and of the index list (bad here)
    bad = _idx(9, 9)
    assert call(rs, fake, 4, 4, 63, bad, 2, 8, 8, 8, None, e, strides=(32, 0, 0)) == 6 and err.shard_bytes == 63
    assert call(rs, fake, 4096, 61441, 64, bad, 2, 8, 8, 8, None, e) == 10
    assert (err.original_count, err.recovery_count) == (4096, 61441)
    # 3. the row strides, each matrix in turn -- ahead of the index list
    for k in range(3):
        strides = [0, 0, 0]
        strides[k] = 32
        assert call(rs, fake, 4, 4, 64, bad, 2, 8, 8, 8, None, e, strides=tuple(strides)) == 101, k
    # (the old stride means nothing in the delta form)
    assert call(rs, fake, 4, 4, 64, bad, 2, None, 8, 8, None, e, strides=(32, 0, 0)) == 4
    # 4. the index list, in order: the first offender decides
    assert call(rs, fake, 4, 4, 64, _idx(1, 4, 1), 3, 8, 8, 8, None, e) == 4
    assert (err.code, err.original_count, err.index) == (4, 4, 4)
    assert call(rs, fake, 4, 4, 64, _idx(1, 2, 1, 7), 4, 8, 8, 8, None, e) == 2
    assert (err.code, err.index, err.original_count) == (2, 1, 0)
    assert call(rs, fake, 4, 4, 64, _idx(0, 1, 2, 3, 0), 5, 8, 8, 8, None, e) == 2 and err.index == 0
    # ... also when the mask selects nothing
    assert call(rs, fake, 4, 4, 64, _idx(5), 1, 8, 8, 8, bytes(4), e) == 4 and err.index == 5
    # a null err is allowed
    assert call(rs, fake, 4, 4, 64, _idx(5), 1, 8, 8, 8, None, None) == 4


@pytest.mark.parametrize("call", FORMS)
def test_no_op_cases_return_ok_without_touching_the_context(rs, call):
    err = rs._RsError()
    e = ctypes.byref(err)
    fake = ctypes.c_void_p(8)
    err.code = 55
    assert call(rs, fake, 4, 4, 64, None, 0, 8, 8, 8, None, e) == 0 and err.code == 0  # count == 0, no list at all
    assert call(rs, fake, 4, 4, 64, _idx(1), 0, None, 8, 8, None, e) == 0
    assert call(rs, fake, 4, 4, 64, _idx(1, 2), 2, None, 8, 8, bytes(4), e) == 0  # the mask selects no row
    if call is _batch:
        assert call(rs, fake, 4, 4, 64, _idx(1, 2), 2, None, 8, 8, None, e, stripes=0) == 0


def test_set_direct_max_refuses_a_null_context(rs):
    assert rs._lib.rs_update_set_direct_max(None, 4) == 101


class _Fake:
    """Stands in for a device tensor in the wrappers' argument checks."""

    is_cuda = True

    def __init__(self, *shape, dtype="torch.uint8"):
        self.shape = shape
        self.dtype = dtype

    def dim(self):
        return len(self.shape)

    def stride(self, k=None):
        return int(np.prod(self.shape[k + 1:]))

    def is_contiguous(self):
        return True

    def element_size(self):
        return 1

    def data_ptr(self):
        return 8  # (never dereferenced: a call that reaches the library fails on its null context)


def test_wrappers_reject_wrong_shapes_dtypes_and_masks(rs):
    N, M, S, B = 8, 6, 64, 3
    idx = [5, 0, 7]
    K = len(idx)
    ctx = types.SimpleNamespace(handle=None)
    names = ["d_old", "d_new", "d_recovery"]
    rows = [K, K, M]
    good = lambda: [_Fake(K, S), _Fake(K, S), _Fake(M, S)]

    def single(t, idx=idx, mask=None):
        return rs.update_device(N, M, S, idx, t[0], t[1], t[2], recovery_rows=mask, ctx=ctx)

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
    with pytest.raises(ValueError, match="recovery_rows"):
        single(good(), mask=[1] * (M + 1))
    with pytest.raises(ValueError, match="negative"):
        single(good(), idx=[5, -1, 7])
    with pytest.raises(rs.UnsupportedShardCount):  # the reference's own checks come first
        rs.update_device(4096, 61441, S, idx, None, _Fake(K, S), _Fake(61441, S), ctx=ctx)
    # well-formed arguments reach the library (whose first check refuses the null context),
    # in the delta form too
    with pytest.raises(ValueError, match="rs_status 101"):
        single(good())
    with pytest.raises(ValueError, match="rs_status 101"):
        single([None, _Fake(K, S), _Fake(M, S)], mask=[1, 0, 0, 1, 1, 0])

    goodb = lambda: [_Fake(B, K, S), _Fake(B, K, S), _Fake(B, M, S)]

    def batch(t, mask=None):
        return rs.update_device_batch(N, M, S, idx, t[0], t[1], t[2], recovery_rows=mask, ctx=ctx)

    for k in range(3):
        t = goodb()
        t[k] = _Fake(rows[k], S)  # a matrix where a batch belongs
        with pytest.raises(ValueError, match=names[k] + ":"):
            batch(t)
        t[k] = _Fake(B, rows[k] - 1, S)
        with pytest.raises(ValueError, match=names[k] + ":"):
            batch(t)
        if k != 1:
            t[k] = _Fake(B + 1, rows[k], S)
            with pytest.raises(ValueError, match="stripe count"):
                batch(t)
    with pytest.raises(ValueError, match="recovery_rows"):
        batch(goodb(), mask=np.ones((B, M), np.uint8))  # one mask for the whole batch
    with pytest.raises(ValueError, match="rs_status 101"):
        batch(goodb())
    with pytest.raises(ValueError):
        rs.update_set_direct_max(4, ctx=ctx)


def test_integration_doc_binds_the_entry_points(tmp_path):
    """The Rust and ctypes lines of INTEGRATION.md name the three calls, and the Rust prototypes
    compile as redeclarations against the header (the index list is a `*const u64`)."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    types_ = dict(ABI.TYPES, **{"*const u64": "const uint64_t *"})
    protos = []
    for name in NAMES:
        m = re.search(r"fn\s+%s\s*\((.*?)\)\s*->\s*RsStatus;" % name, doc, flags=re.S)
        assert m, name
        params = []
        for a in filter(None, (x.strip() for x in " ".join(m.group(1).split()).split(","))):
            pname, ptype = (x.strip() for x in a.split(":", 1))
            params.append(f"{types_[ptype]} {pname}")
        protos.append(f"rs_status {name}({', '.join(params)});")
        assert re.search(r'_sig\("%s"|lib\.%s\b' % (name, name), doc), name  # the ctypes side
    c = tmp_path / "update_bindings.c"
    c.write_text("\n".join(["#include <stdint.h>", f'#include "{HEADER}"'] + protos) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-c", str(c), "-o", str(tmp_path / "u.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + "\n" + c.read_text()


# ---------------------------------------------------------------------------
# the identity, on the CPU oracle alone

def elements(rows):
    """[rows, S] shard bytes -> [rows, S / 2] GF(2^16) elements (block and tail layout:
    src/engine/shards.rs:38-74)."""
    n, S = rows.shape
    full, t = S // 64, (S % 64) // 2
    out = np.zeros((n, S // 2), np.uint16)
    if full:
        b = rows[:, :full * 64].reshape(n, full, 64)
        out[:, :full * 32] = (b[:, :, :32].astype(np.uint16) | b[:, :, 32:].astype(np.uint16) << 8).reshape(n, -1)
    if t:
        tail = rows[:, full * 64:]
        out[:, full * 32:] = tail[:, :t].astype(np.uint16) | tail[:, t:].astype(np.uint16) << 8
    return out


def shard_bytes_of(el, S):
    n = el.shape[0]
    full, t = S // 64, (S % 64) // 2
    out = np.zeros((n, S), np.uint8)
    if full:
        e = el[:, :full * 32].reshape(n, full, 32)
        out[:, :full * 64] = np.concatenate([(e & 0xFF).astype(np.uint8), (e >> 8).astype(np.uint8)], axis=2).reshape(n, -1)
    if t:
        e = el[:, full * 32:]
        out[:, full * 64:] = np.concatenate([(e & 0xFF).astype(np.uint8), (e >> 8).astype(np.uint8)], axis=1)
    return out


def test_element_layout_round_trips():
    for S in (2, 64, 66, 72, 128, 190):
        rows = np.random.default_rng(S).integers(0, 256, (3, S), dtype=np.uint8)
        assert np.array_equal(shard_bytes_of(elements(rows), S), rows)


CASES = [("default", 100, 30, 64), ("default", 30, 100, 72), ("high", 1000, 100, 66), ("low", 128, 1024, 64),
         ("default", 1024, 1024, 128), ("default", 3, 2, 2), ("default", 1, 1, 64)]


@pytest.mark.parametrize("rate,N,M,S", CASES, ids=lambda v: str(v))
def test_identity_on_the_oracle(rate, N, M, S):
    exp, log = O.table("exp", 65536).astype(np.int64), O.table("log", 65536).astype(np.int64)
    # what the sentinel rests on: 0 has no log -- the table holds 65535 for it, which no
    # multiplier has, and as a log 65535 multiplies by ONE (Engine::mul), so a zero
    # coefficient must be skipped, not looked up
    assert log[0] == 65535 and not (log[1:] == 65535).any()
    assert exp[(log[0x1234] + 65535) % 65535] == 0x1234

    rng = np.random.default_rng(N * 3 + M)
    count = min(N, 33)  # two coefficient blocks where the shape has that many originals
    idx = rng.permutation(N)[:count]
    if count >= 2:
        idx[0], idx[-1] = N - 1, 0
        idx[1:-1] = [i for i in rng.permutation(np.arange(1, N - 1))[:count - 2]]
    # the unit stripe in the coefficient kernels' layout, through the encoder
    W = 64 * ((count + 31) // 32)
    unit = np.zeros((N, W), np.uint8)
    for c, i in enumerate(idx):
        unit[i, (c // 32) * 64 + c % 32] = 1
    coef = O.encode(rate, unit, M)
    G = np.stack([coef[:, (c // 32) * 64 + c % 32].astype(np.int64)
                  | coef[:, (c // 32) * 64 + 32 + c % 32].astype(np.int64) << 8 for c in range(count)], axis=1)
    # every other element of the coefficient encode is zero: the columns do not mix
    assert np.count_nonzero(elements(coef)) == np.count_nonzero(G)
    assert (G != 0).all(), "a zero coefficient (the issue found none in these cases)"

    orig = O.generate_original(N, S, 3)
    rec = O.encode(rate, orig, M)
    new = O.generate_original(count, S, 4)
    mod = orig.copy()
    mod[idx] = new
    want = O.encode(rate, mod, M)
    delta = elements(orig[idx] ^ new).astype(np.int64)  # [count, S / 2]
    acc = np.zeros((M, S // 2), np.int64)
    for c in range(count):
        lg = log[G[:, c]]  # [M]
        prod = exp[(log[delta[c]][None, :] + lg[:, None]) % 65535]  # x * exp(log g) ...
        prod[:, delta[c] == 0] = 0  # ... and 0 * g = 0
        prod[lg == 65535, :] = 0  # a zero coefficient adds nothing
        acc ^= prod
    got = rec ^ shard_bytes_of(acc.astype(np.uint16), S)
    assert np.array_equal(got, want)
