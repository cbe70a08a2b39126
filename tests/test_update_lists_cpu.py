"""rs_update_device_batch_lists without a GPU: the symbol and its declaration, the argument checks
(all before any device work, in the header's order, against a made-up context that is never
dereferenced), the no-op cases, the wrapper's rejections, the INTEGRATION.md binding, and the
identity the kernel relies on stated on the CPU oracle alone: with a different index list per
stripe,

    recovery_j(new) = recovery_j(old) ^ XOR_c G[j][index_c] * (old_c ^ new_c),

where G is the FULL coefficient matrix (the oracle's encode of the unit stripes of every original,
the table the locate keeps) read through the stripe's own indices.
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
from test_update_cpu import _Fake, elements, shard_bytes_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rs_update_device_batch_lists"
HEADER = os.path.join(ROOT, "include", "rs_mi355x.h")
ARGS = ["rs_context *ctx", "rs_rate rate", "uint64_t original_count", "uint64_t recovery_count",
        "uint64_t shard_bytes", "uint64_t stripes", "const uint64_t *index", "const uint32_t *count",
        "uint64_t max_count", "const void *d_old", "uint64_t old_stride", "uint64_t old_stripe_stride",
        "const void *d_new", "uint64_t new_stride", "uint64_t new_stripe_stride", "void *d_recovery",
        "uint64_t recovery_stride", "uint64_t recovery_stripe_stride", "const uint8_t *recovery_update",
        "void *stream", "rs_error *err"]


@pytest.fixture(scope="module")
def rs():
    import reed_solomon_simd
    return reed_solomon_simd


def _u64(*values):
    return (ctypes.c_uint64 * max(1, len(values)))(*values)


def _u32(*values):
    return (ctypes.c_uint32 * max(1, len(values)))(*values)


def call(rs, ctx, N, M, S, stripes, index, count, max_count, d_old, d_new, d_rec, mask, err=None,
         strides=(0, 0, 0)):
    m = None if mask is None else ctypes.cast(ctypes.c_char_p(bytes(mask)), ctypes.c_void_p)
    return getattr(rs._lib, NAME)(ctx, 0, N, M, S, stripes, index, count, max_count, d_old, strides[0], 0, d_new,
                                  strides[1], 0, d_rec, strides[2], 0, m, None, err)


def test_symbol_is_exported_and_declared(rs):
    header = open(HEADER).read()
    assert hasattr(rs._lib, NAME)
    fn = getattr(rs._lib, NAME)
    assert fn.argtypes is not None and len(fn.argtypes) == 21
    proto = re.search(r"rs_status\s+%s\s*\(([^;]*)\)\s*;" % NAME, header)
    assert proto, "not declared"
    args = [" ".join(a.split()) for a in proto.group(1).split(",")]
    assert args == ARGS
    assert callable(rs.update_device_batch_lists)
    # the patterns other tests read the header with still find the shared-list prototype first
    batch = re.search(r"rs_update_device_batch\s*\(([^;]*)\)", header).group(1)
    assert "uint64_t count" in batch and "max_count" not in batch


def test_argument_checks_precede_any_device_work(rs):
    err = rs._RsError()
    e = ctypes.byref(err)
    fake = ctypes.c_void_p(8)
    idx, cnt = _u64(1, 3, 0, 2, 0, 0), _u32(2, 2, 1)  # 3 stripes x max_count 2
    # 1. each null
    assert call(rs, None, 4, 4, 64, 3, idx, cnt, 2, 8, 8, 8, None, e) == 101 and err.code == 101
    assert call(rs, fake, 4, 4, 64, 3, idx, cnt, 2, 8, 0, 8, None, e) == 101
    assert call(rs, fake, 4, 4, 64, 3, idx, cnt, 2, 8, 8, 0, None, e) == 101
    assert call(rs, fake, 4, 4, 64, 3, idx, None, 2, 8, 8, 8, None, e) == 101
    assert call(rs, fake, 4, 4, 64, 3, None, cnt, 2, 8, 8, 8, None, e) == 101
    # ... ahead of rs_validate (a bad shard size here)
    assert call(rs, fake, 4, 4, 63, 3, None, cnt, 2, 8, 8, 8, None, e) == 101
    # (null lists are fine where nothing could be read from them -- and then rs_validate speaks)
    assert call(rs, fake, 4, 4, 63, 0, None, None, 2, 8, 8, 8, None, e) == 6
    assert call(rs, fake, 4, 4, 63, 3, None, cnt, 0, 8, 8, 8, None, e) == 6
    # 2. rs_validate, ahead of the strides and of the lists (bad here)
    bad, badc = _u64(9, 9, 9, 9, 9, 9), _u32(3, 3, 3)
    assert call(rs, fake, 4, 4, 63, 3, bad, badc, 2, 8, 8, 8, None, e, strides=(32, 0, 0)) == 6
    assert err.shard_bytes == 63
    assert call(rs, fake, 4096, 61441, 64, 3, bad, badc, 2, 8, 8, 8, None, e) == 10
    assert (err.original_count, err.recovery_count) == (4096, 61441)
    # 3. the row strides, each matrix in turn, ahead of the lists and of the empty batch
    for k in range(3):
        strides = [0, 0, 0]
        strides[k] = 32
        assert call(rs, fake, 4, 4, 64, 3, bad, badc, 2, 8, 8, 8, None, e, strides=tuple(strides)) == 101, k
        assert call(rs, fake, 4, 4, 64, 0, bad, badc, 2, 8, 8, 8, None, e, strides=tuple(strides)) == 101, k
    # (the old stride means nothing in the delta form: the lists are reached)
    assert call(rs, fake, 4, 4, 64, 3, bad, _u32(1, 1, 1), 2, None, 8, 8, None, e, strides=(32, 0, 0)) == 4
    # 4. stripes == 0 or max_count == 0: RS_OK ahead of the lists
    assert call(rs, fake, 4, 4, 64, 0, bad, badc, 2, 8, 8, 8, None, e) == 0
    assert call(rs, fake, 4, 4, 64, 3, bad, badc, 0, 8, 8, 8, None, e) == 0
    # 5. every stripe's list in stripe order, err->got = the stripe
    assert call(rs, fake, 4, 4, 64, 3, idx, _u32(2, 3, 9), 2, 8, 8, 8, None, e) == 101
    assert (err.code, err.got) == (101, 1)
    assert call(rs, fake, 4, 4, 64, 3, _u64(1, 3, 0, 4, 7, 7), _u32(2, 2, 2), 2, 8, 8, 8, None, e) == 4
    assert (err.code, err.original_count, err.index, err.got) == (4, 4, 4, 1)
    assert call(rs, fake, 4, 4, 64, 3, _u64(1, 3, 2, 2, 7, 7), _u32(2, 2, 2), 2, 8, 8, 8, None, e) == 2
    assert (err.code, err.index, err.got, err.original_count) == (2, 2, 1, 0)
    # ... slack entries past count[b] are not looked at, and the first offender decides
    assert call(rs, fake, 4, 4, 64, 3, _u64(1, 99, 2, 2, 7, 7), _u32(1, 2, 2), 2, 8, 8, 8, None, e) == 2
    assert err.got == 1
    assert call(rs, fake, 4, 4, 64, 3, _u64(5, 1, 2, 2, 7, 7), _u32(2, 2, 2), 2, 8, 8, 8, None, e) == 4
    assert (err.index, err.got) == (5, 0)
    # ... also when the masks select nothing
    assert call(rs, fake, 4, 4, 64, 3, _u64(1, 3, 2, 2, 0, 0), _u32(2, 2, 1), 2, 8, 8, 8, bytes(12), e) == 2
    # a null err is allowed
    assert call(rs, fake, 4, 4, 64, 3, _u64(1, 3, 2, 2, 0, 0), _u32(2, 2, 1), 2, 8, 8, 8, None, None) == 2


def test_the_same_index_in_two_stripes_is_accepted_and_no_ops_leave_the_context_alone(rs):
    """Every call here gets past the list checks and returns RS_OK without touching the made-up
    context: nothing selects a row, or every list is empty."""
    err = rs._RsError()
    e = ctypes.byref(err)
    fake = ctypes.c_void_p(8)
    same = _u64(1, 3, 3, 1, 1, 0)  # 1 and 3 in stripes 0 and 1, 1 again in stripe 2
    err.code = 55
    assert call(rs, fake, 4, 4, 64, 3, same, _u32(2, 2, 1), 2, 8, 8, 8, bytes(12), e) == 0 and err.code == 0
    assert call(rs, fake, 4, 4, 64, 3, same, _u32(0, 0, 0), 2, 8, 8, 8, None, e) == 0
    # the only stripe with a list selects nothing; the stripes that select rows have no list
    mask = bytes([1, 1, 1, 1]) + bytes(4) + bytes([0, 1, 0, 0])
    assert call(rs, fake, 4, 4, 64, 3, same, _u32(0, 2, 0), 2, None, 8, 8, mask, e) == 0
    assert call(rs, fake, 4, 4, 64, 0, None, None, 2, 8, 8, 8, None, e) == 0
    assert call(rs, fake, 4, 4, 64, 3, None, _u32(0, 0, 0), 0, 8, 8, 8, None, e) == 0


def test_wrapper_rejects_wrong_shapes_dtypes_and_masks(rs):
    N, M, S, B = 8, 6, 64, 3
    lists = [[5, 0, 7], [], [1]]
    K = 3
    ctx = types.SimpleNamespace(handle=None)
    names = ["d_old", "d_new", "d_recovery"]
    rows = [K, K, M]
    good = lambda: [_Fake(B, K, S), _Fake(B, K, S), _Fake(B, M, S)]

    def batch(t, lists=lists, mask=None):
        return rs.update_device_batch_lists(N, M, S, lists, t[0], t[1], t[2], recovery_rows=mask, ctx=ctx)

    for k in range(3):
        t = good()
        t[k] = _Fake(rows[k], S)  # a matrix where a batch belongs
        with pytest.raises(ValueError, match=names[k] + ":"):
            batch(t)
        t[k] = _Fake(B, rows[k] - 1, S)  # too few rows for the longest list
        with pytest.raises(ValueError, match=names[k] + ":"):
            batch(t)
        t[k] = _Fake(B, rows[k], S + 2)
        with pytest.raises(ValueError, match=names[k] + ":"):
            batch(t)
        t[k] = _Fake(B, rows[k], S, dtype="torch.int32")
        with pytest.raises(ValueError, match=names[k] + ": dtype"):
            batch(t)
        t[k] = _Fake(B + 1, rows[k], S)
        with pytest.raises(ValueError, match="stripe count"):
            batch(t)
    with pytest.raises(ValueError, match="recovery_rows"):
        batch(good(), mask=[1] * M)  # one mask where one per stripe belongs
    with pytest.raises(ValueError, match="recovery_rows"):
        batch(good(), mask=np.ones((B, M + 1), np.uint8))
    with pytest.raises(ValueError, match="negative"):
        batch(good(), lists=[[5, -1], [], [1]])
    with pytest.raises(rs.UnsupportedShardCount):  # the reference's own checks come first
        rs.update_device_batch_lists(4096, 61441, S, lists, None, _Fake(B, K, S), _Fake(B, 61441, S), ctx=ctx)
    # well-formed arguments reach the library (whose first check refuses the null context)
    with pytest.raises(ValueError, match="rs_status 101"):
        batch(good())
    with pytest.raises(ValueError, match="rs_status 101"):
        batch([None, _Fake(B, K, S), _Fake(B, M, S)], mask=np.ones((B, M), np.uint8))


def test_integration_doc_binds_the_entry_point(tmp_path):
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    types_ = dict(ABI.TYPES, **{"*const u64": "const uint64_t *", "*const u32": "const uint32_t *"})
    m = re.search(r"fn\s+%s\s*\((.*?)\)\s*->\s*RsStatus;" % NAME, doc, flags=re.S)
    assert m
    params = []
    for a in filter(None, (x.strip() for x in " ".join(m.group(1).split()).split(","))):
        pname, ptype = (x.strip() for x in a.split(":", 1))
        params.append(f"{types_[ptype]} {pname}")
    assert len(params) == 21
    assert re.search(r"lib\.%s\b" % NAME, doc)  # the ctypes side
    c = tmp_path / "update_lists_bindings.c"
    c.write_text("\n".join(["#include <stdint.h>", f'#include "{HEADER}"',
                            f"rs_status {NAME}({', '.join(params)});"]) + "\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-c", str(c), "-o", str(tmp_path / "u.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + "\n" + c.read_text()


# ---------------------------------------------------------------------------
# the identity, on the CPU oracle alone

def full_matrix(rate, N, M):
    """G[j][i] as integers [M, N]: the oracle's encode of the unit stripes, 32 originals per
    64-byte block (element i of row i = 1), as the locate's coefficient step lays them out."""
    W = 64 * ((N + 31) // 32)
    unit = np.zeros((N, W), np.uint8)
    for i in range(N):
        unit[i, (i // 32) * 64 + i % 32] = 1
    coef = O.encode(rate, unit, M)
    G = elements(coef).astype(np.int64)[:, :N]
    assert np.count_nonzero(elements(coef)) == np.count_nonzero(G)  # the columns do not mix
    return G


@pytest.mark.parametrize("rate,N,M,S", [("default", 3, 2, 2), ("default", 30, 100, 72), ("default", 100, 30, 64)],
                         ids=lambda v: str(v))
def test_identity_on_the_oracle_with_a_list_per_stripe(rate, N, M, S):
    exp, log = O.table("exp", 65536).astype(np.int64), O.table("log", 65536).astype(np.int64)
    assert log[0] == 65535  # the table's zero coefficients are the kernel's sentinel
    G = full_matrix(rate, N, M)
    LG = log[G]  # what the table holds: [M, N], pitch N
    rng = np.random.default_rng(N + M)
    lists = [[N - 1], [0], list(rng.permutation(N)[:min(N, 17)]), [], [N - 1]]
    for b, idx in enumerate(lists):
        orig = O.generate_original(N, S, b)
        rec = O.encode(rate, orig, M)
        new = O.generate_original(max(1, len(idx)), S, 50 + b)[:len(idx)]
        mod = orig.copy()
        mod[idx] = new
        want = O.encode(rate, mod, M) if idx else rec
        delta = elements(orig[idx] ^ new).astype(np.int64) if idx else np.zeros((0, S // 2), np.int64)
        acc = np.zeros((M, S // 2), np.int64)
        for c, i in enumerate(idx):
            lg = LG[:, i]
            prod = exp[(log[delta[c]][None, :] + lg[:, None]) % 65535]  # x * exp(log g), as Engine::mul
            prod[:, delta[c] == 0] = 0
            prod[lg == 65535, :] = 0  # a zero coefficient adds nothing
            acc ^= prod
        got = rec ^ shard_bytes_of(acc.astype(np.uint16), S)
        assert np.array_equal(got, want), (b, idx)
