"""GPU: rs_update_device* -- a partial-stripe write applied to the recovery shards in place.

The reference of every test is the CPU oracle's encode of the modified stripe, compared byte
for byte.  Both routes (the direct k_update launch and the re-encode of the delta stripe) are
forced through update_set_direct_max.  Unselected recovery rows, row padding and the inputs
are compared with what they held before the call, so a kernel that writes anything but the
selected recovery rows fails.
"""
import numpy as np
import pytest

import oracle_lib as O
import wide_cases as W

pytestmark = pytest.mark.gpu

RATE = {"default": 0, "high": 1, "low": 2}
DIRECT, REENCODE = 256, 0  # update_set_direct_max values that force a route for every count used here

# (rate, N, M, S); kernel forms of the existing encode in the issue's words
SHAPES = [
    ("default", 1, 1, 64),
    ("default", 3, 2, 2),
    ("default", 100, 30, 64),
    ("default", 30, 100, 72),      # tail
    ("high", 1000, 100, 66),       # k_chunks, tail, rows not 4-byte aligned
    ("low", 128, 1024, 64),
    ("default", 1024, 1024, 1024),  # column kernel
    ("default", 4096, 4096, 64),    # pass kernels (for the coefficient encode)
]
COUNTS = [1, 2, 31, 32, 33]  # 32: the column edge of the coefficient blocks


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def rs(torch):
    import reed_solomon_simd
    yield reed_solomon_simd
    reed_solomon_simd.update_set_direct_max(reed_solomon_simd.UPDATE_DIRECT_MAX_DEFAULT)


_STRIPES = {}


def stripe(rate, N, M, S, seed=0):
    """(originals, their recovery shards) from the oracle, computed once and never modified."""
    key = (rate, N, M, S, seed)
    if key not in _STRIPES:
        orig = O.generate_original(N, S, seed)
        rec = O.encode(rate, orig, M)
        orig.setflags(write=False)
        rec.setflags(write=False)
        _STRIPES[key] = (orig, rec)
    return _STRIPES[key]


def indices(N, count, rng):
    """`count` distinct originals: the first and the last (from count = 2 on) and random ones,
    handed over out of order."""
    if count == 1:
        return [N - 1]
    rest = rng.choice(np.arange(1, N - 1), count - 2, replace=False).tolist() if count > 2 else []
    idx = [N - 1] + rest + [0]  # last, random (unsorted), first
    assert len(set(idx)) == count
    return idx


def change(rate, N, M, S, idx, seed=0, positional=False):
    """(old rows, new rows, wanted recovery) for overwriting originals idx of the stripe.
    positional: the first new row differs from the old one in the last pack only and the second in
    pack 0 only (tests/wide_cases.py update_new_rows)."""
    orig, _ = stripe(rate, N, M, S, seed)
    new = O.generate_original(len(idx), S, seed + 17)
    if positional:
        new = W.update_new_rows(orig[idx], new)
    mod = orig.copy()
    mod[idx] = new
    return np.ascontiguousarray(orig[idx]), new, O.encode(rate, mod, M)


def dev(torch, a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def first_diff(got, want):
    r, b = np.argwhere(got != want)[0]
    return f"first difference at (row {int(r)}, byte {int(b)}): got {int(got[r, b]):#04x}, want {int(want[r, b]):#04x}"


def check(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        raise AssertionError(f"{what}: " + first_diff(got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])))


def run(torch, rs, rate, N, M, S, idx, route, form="delta", mask=None, seed=0, positional=False, pad=0):
    """One update on fresh device copies; returns the recovery matrix after it.  Also checks that
    the inputs and the unselected rows are as before, and with `pad` bytes of 0xC3 after every
    recovery row, that those are."""
    old, new, want = change(rate, N, M, S, idx, seed, positional)
    _, rec = stripe(rate, N, M, S, seed)
    rs.update_set_direct_max(route)
    d_rec, b_rec = view(torch, rec, 0, pad)
    if form == "delta":
        h_old, h_new = None, old ^ new
    else:
        h_old, h_new = old, new
    d_old = None if h_old is None else dev(torch, h_old)
    d_new = dev(torch, h_new)
    rs.update_device(N, M, S, idx, d_old, d_new, d_rec, recovery_rows=mask, rate_=RATE[rate])
    torch.cuda.synchronize()
    got = d_rec.cpu().numpy()
    what = f"{rate} {N}:{M} x {S} count {len(idx)} route {route} {form}"
    sel = np.ones(M, bool) if mask is None else np.asarray(mask) != 0
    check(got[sel], want[sel], what)
    check(got[~sel], rec[~sel], what + ": an unselected row was written")
    assert (padding_of(b_rec, rec, 0, pad) == 0xC3).all(), what + ": recovery padding written"
    check(d_new.cpu().numpy(), h_new, what + ": d_new was written")
    if d_old is not None:
        check(d_old.cpu().numpy(), h_old, what + ": d_old was written")
    return got


@pytest.mark.parametrize("rate,N,M,S", SHAPES, ids=lambda v: str(v))
def test_shapes_counts_and_routes(torch, rs, rate, N, M, S):
    rng = np.random.default_rng(N * 7 + M)
    counts = [c for c in COUNTS if c <= N] + ([N] if N <= 100 and N not in COUNTS else [])
    for k, count in enumerate(counts):
        idx = indices(N, count, rng)
        form = "delta" if k % 2 == 0 else "oldnew"
        a = run(torch, rs, rate, N, M, S, idx, DIRECT, form)
        b = run(torch, rs, rate, N, M, S, idx, REENCODE, form)
        check(a, b, f"{rate} {N}:{M} x {S} count {count}: the routes differ")


@pytest.mark.parametrize("route", [DIRECT, REENCODE])
@pytest.mark.parametrize("form", ["delta", "oldnew"])
@pytest.mark.parametrize("rate,N,M,S", [("default", 100, 30, 64), ("default", 30, 100, 72),
                                         ("default", 1024, 1024, 1024)])
def test_masks_and_forms(torch, rs, rate, N, M, S, form, route):
    rng = np.random.default_rng(5)
    idx = indices(N, 3, rng)
    one = np.zeros(M, np.uint8)
    one[M // 2] = 1
    third = np.zeros(M, np.uint8)
    third[rng.choice(M, max(1, M // 3), replace=False)] = 1
    for mask in (None, one, third, np.ones(M, np.uint8)):
        run(torch, rs, rate, N, M, S, idx, route, form, mask)


def view(torch, a, base, pad, fill=0xC3):
    """A device copy of `a` [rows, S] (or [B, rows, S]) inside a wider, `fill`ed buffer: `base`
    bytes in front, `pad` bytes after every row.  Returns (view, whole buffer)."""
    rows, S = a.shape[-2], a.shape[-1]
    lead = a.shape[:-2]
    n = int(np.prod(lead)) * rows if lead else rows
    buf = torch.full((base + n * (S + pad),), fill, dtype=torch.uint8, device="cuda")
    v = buf[base:].view(*lead, rows, S + pad)[..., :S]
    v.copy_(torch.from_numpy(np.array(a, copy=True)).cuda())
    return v, buf


def padding_of(buf, a, base, pad):
    """The bytes of `buf` outside the rows of the view made by view()."""
    S = a.shape[-1]
    h = buf.cpu().numpy()
    body = h[base:].reshape(-1, S + pad)
    return np.concatenate([h[:base], body[:, S:].reshape(-1)])


@pytest.mark.parametrize("route", [DIRECT, REENCODE])
@pytest.mark.parametrize("which", ["old", "new", "rec"])
@pytest.mark.parametrize("base,pad", [(0, 64), (1, 2)], ids=["padded", "unaligned"])
def test_strided_and_unaligned_matrices(torch, rs, base, pad, which, route):
    """Each matrix in turn padded (aligned: rows of S + 64) or unaligned (base + 1, stride S + 2);
    the padding and the lead byte stay as they were."""
    for rate, N, M, S in (("default", 30, 100, 72), ("default", 100, 30, 64)):
        idx = indices(N, 3, np.random.default_rng(9))
        old, new, want = change(rate, N, M, S, idx)
        _, rec = stripe(rate, N, M, S)
        lay = {w: ((base, pad) if w == which else (0, 0)) for w in ("old", "new", "rec")}
        d_old, b_old = view(torch, old, *lay["old"])
        d_new, b_new = view(torch, new, *lay["new"])
        d_rec, b_rec = view(torch, rec, *lay["rec"])
        mask = np.ones(M, np.uint8)
        mask[1::4] = 0
        rs.update_set_direct_max(route)
        rs.update_device(N, M, S, idx, d_old, d_new, d_rec, recovery_rows=mask)
        torch.cuda.synchronize()
        what = f"{N}:{M} x {S} {which} base {base} pad {pad} route {route}"
        got = d_rec.cpu().numpy()
        check(got[mask == 1], want[mask == 1], what)
        check(got[mask == 0], rec[mask == 0], what + ": an unselected row was written")
        assert (padding_of(b_rec, rec, *lay["rec"]) == 0xC3).all(), what + ": recovery padding written"
        check(d_old.cpu().numpy(), old, what + ": d_old written")
        check(d_new.cpu().numpy(), new, what + ": d_new written")
        assert (padding_of(b_old, old, *lay["old"]) == 0xC3).all() and (padding_of(b_new, new, *lay["new"]) == 0xC3).all()


@pytest.mark.parametrize("route", [DIRECT, REENCODE])
@pytest.mark.parametrize("form", ["delta", "oldnew"])
def test_batch_equals_single_calls(torch, rs, form, route):
    rate, N, M, S, B = "default", 30, 100, 72, 3
    idx = indices(N, 4, np.random.default_rng(3))
    mask = np.ones(M, np.uint8)
    mask[::5] = 0
    olds, news, wants, recs = [], [], [], []
    for b in range(B):
        o, n, w = change(rate, N, M, S, idx, seed=b)
        olds.append(o), news.append(n), wants.append(w), recs.append(stripe(rate, N, M, S, b)[1])
    olds, news, wants, recs = (np.stack(x) for x in (olds, news, wants, recs))
    if form == "delta":
        news, olds = olds ^ news, None

    def padded(a, extra):  # stripe padding: `extra` more rows per stripe than the call uses
        t = torch.full((B, a.shape[1] + extra, S), 0xC3, dtype=torch.uint8, device="cuda")
        t[:, :a.shape[1]] = torch.from_numpy(a).cuda()
        return t, t[:, :a.shape[1]]

    w_new, d_new = padded(news, 2)
    w_rec, d_rec = padded(recs, 1)
    d_old = None if olds is None else padded(olds, 3)[1]
    rs.update_set_direct_max(route)
    rs.update_device_batch(N, M, S, idx, d_old, d_new, d_rec, recovery_rows=mask)
    torch.cuda.synchronize()
    got = d_rec.cpu().numpy()
    check(got[:, mask == 1], wants[:, mask == 1], "batch")
    check(got[:, mask == 0], recs[:, mask == 0], "batch: an unselected row was written")
    assert (w_rec[:, M:].cpu().numpy() == 0xC3).all() and (w_new[:, len(idx):].cpu().numpy() == 0xC3).all()
    for b in range(B):  # the same as B single calls
        s_rec = dev(torch, recs[b])
        rs.update_device(N, M, S, idx, None if olds is None else dev(torch, olds[b]), dev(torch, news[b]), s_rec,
                         recovery_rows=mask)
        torch.cuda.synchronize()
        check(got[b], s_rec.cpu().numpy(), f"batch stripe {b} differs from the single call")


def profiled(torch, rs, fn):
    rs.profile_enable(True)
    try:
        rs.profile_collect()
        fn()
        torch.cuda.synchronize()
        return [name for name, _, _ in rs.profile_collect()]
    finally:
        rs.profile_enable(False)


def test_coefficient_table_is_reused_and_rebuilt(torch, rs):
    rate, N, M, S = "default", 1024, 1024, 1024
    rng = np.random.default_rng(11)
    A, B = indices(N, 2, rng), indices(N, 5, rng)
    _, rec = stripe(rate, N, M, S)
    rs.update_set_direct_max(DIRECT)
    rs.release_stream_scratch()  # cold: no table on this stream
    results, launches = [], []
    for idx in (A, B, A, A):
        old, new, want = change(rate, N, M, S, idx)
        d_rec, d_new = dev(torch, rec), dev(torch, old ^ new)
        launches.append(profiled(torch, rs, lambda: rs.update_device(N, M, S, idx, None, d_new, d_rec)))
        got = d_rec.cpu().numpy()
        check(got, want, f"index list {idx}")
        results.append(got)
    check(results[3], results[0], "the warm call differs from the cold one")
    for cold in launches[:3]:  # a new key: the coefficient step ran
        assert "k_coef_unit" in cold and "k_coef_log" in cold, cold
        assert sum(n.startswith("k_update") for n in cold) == 1, cold
    warm = launches[3]
    assert len(warm) == 1 and warm[0].startswith("k_update"), warm
    # the re-encode route launches no k_update at all
    rs.update_set_direct_max(REENCODE)
    d_rec, d_new = dev(torch, rec), dev(torch, old ^ new)
    names = profiled(torch, rs, lambda: rs.update_device(N, M, S, A, None, d_new, d_rec))
    assert names.count("k_rows_xor") == 2 and not any(n.startswith("k_update") for n in names), names


def test_updates_in_flight(torch, rs):
    """Two updates back to back on one stream (the second on top of the first, another index
    list: the table is rebuilt while the first call may still run), and two on two streams."""
    rate, N, M, S = "default", 100, 30, 64
    orig, rec = stripe(rate, N, M, S)
    A, B = [99, 7], [0, 50, 3]
    newA, newB = O.generate_original(2, S, 40), O.generate_original(3, S, 41)
    mod = orig.copy()
    mod[A] = newA
    mod[B] = newB
    want = O.encode(rate, mod, M)
    for route in (DIRECT, REENCODE):
        rs.update_set_direct_max(route)
        d_rec = dev(torch, rec)
        dA, dB = dev(torch, orig[A] ^ newA), dev(torch, orig[B] ^ newB)
        torch.cuda.synchronize()
        rs.update_device(N, M, S, A, None, dA, d_rec)
        rs.update_device(N, M, S, B, None, dB, d_rec)
        torch.cuda.synchronize()
        check(d_rec.cpu().numpy(), want, f"one stream, route {route}")
        # two streams, one stripe each
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        r1, r2 = dev(torch, rec), dev(torch, rec)
        torch.cuda.synchronize()
        rs.update_device(N, M, S, A, None, dA, r1, stream=s1)
        rs.update_device(N, M, S, B, None, dB, r2, stream=s2)
        torch.cuda.synchronize()
        mA, mB = orig.copy(), orig.copy()
        mA[A] = newA
        mB[B] = newB
        check(r1.cpu().numpy(), O.encode(rate, mA, M), f"stream 1, route {route}")
        check(r2.cpu().numpy(), O.encode(rate, mB, M), f"stream 2, route {route}")
        rs.release_stream_scratch(s1)
        rs.release_stream_scratch(s2)


def test_other_calls_are_undisturbed(torch, rs):
    """decode_device restores the NEW originals from the updated recovery shards, and an
    encode_device next to the update still gives the oracle's bytes."""
    rate, N, M, S = "default", 1024, 1024, 1024
    orig, rec = stripe(rate, N, M, S)
    idx = indices(N, 3, np.random.default_rng(21))
    old, new, want = change(rate, N, M, S, idx)
    for route in (DIRECT, REENCODE):
        rs.update_set_direct_max(route)
        d_rec, d_enc = dev(torch, rec), torch.zeros((M, S), dtype=torch.uint8, device="cuda")
        d_orig = dev(torch, orig)
        rs.encode_device(N, M, S, d_orig, d_enc)
        rs.update_device(N, M, S, idx, dev(torch, old), dev(torch, new), d_rec)
        rs.encode_device(N, M, S, d_orig, d_enc)
        torch.cuda.synchronize()
        check(d_enc.cpu().numpy(), rec, f"encode next to the update, route {route}")
        check(d_rec.cpu().numpy(), want, f"route {route}")
        op = np.ones(N, np.uint8)
        op[idx] = 0
        lost = orig.copy()
        lost[idx] = 0xA5
        d_out = torch.zeros((N, S), dtype=torch.uint8, device="cuda")
        rs.decode_device(N, M, S, dev(torch, lost), op, d_rec, np.ones(M, np.uint8), d_out)
        torch.cuda.synchronize()
        check(d_out.cpu().numpy()[idx], new, f"decode after the update, route {route}")
