"""GPU: rs_locate_device_robust* -- one corrupt original among up to max_outliers corrupt recovery rows.

Expected values are constructed, not computed by the code under test (tests/locate_robust_cases.py):
the oracle's clean stripe with chosen bytes flipped, the status each case is built to show asserted
on the numpy model of the contract first (tests/locate_robust_model.py).  `located`, the flags
(against the oracle's encode of the stored originals) and the WHOLE d_outlier array must equal the
model.  Every run also checks that nothing but the three outputs was written: the inputs equal their
host copies, the guards around the three outputs are intact, and all three, pre-filled with 0xFF,
come back fully defined.
"""
import numpy as np
import pytest

import locate_model as LM
import locate_robust_cases as RC
import locate_robust_model as RM
import oracle_lib as O
import test_gpu_locate as L
import test_gpu_verify as V
from test_gpu_locate import damage_original, guarded

pytestmark = pytest.mark.gpu

RATE = V.RATE
GUARD = V.GUARD
CLEAN, ROWS, UNKNOWN = LM.CLEAN, LM.ROWS, LM.UNKNOWN
# (rate, N, M): the staged single-chunk column kernel
COLUMN = [("high", 70, 100), ("low", 100, 70)]
LAYOUTS = L.LAYOUTS
# (rate, N, M, S, row padding): the lane kernel, 1024:1024 once, the multi-chunk encodes, and tiny
# stripes whose four selected rows allow one outlier (2:6 allows two)
OTHER = [("default", 200, 200, 72, 0), ("default", 1024, 1024, 64, 0), ("high", 1000, 100, 66, 0),
         ("low", 128, 1024, 64, 0), ("default", 1, 4, 64, 0), ("default", 3, 4, 2, 0), ("default", 2, 6, 190, 0)]


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
    reed_solomon_simd.mono_enable(True)


def check_outlier(out_buf, what):
    o = out_buf.cpu().numpy()
    assert (o[:GUARD] == 0xFF).all() and (o[-GUARD:] == 0xFF).all(), what + ": a byte outside d_outlier was written"
    assert (o[GUARD:-GUARD] <= 1).all(), what + ": an outlier byte is neither 0 nor 1"
    return o[GUARD:-GUARD]


def locate_one(torch, rs, rate, N, M, S, orig, rec, t, pad=0, mask=None, what="", stream=None):
    d_orig, d_rec = V.view(torch, orig, pad), V.view(torch, rec, pad)
    loc, loc_buf = guarded(torch, (1,), torch.int32)
    flags, flag_buf = guarded(torch, (M,), torch.uint8)
    out, out_buf = guarded(torch, (M,), torch.uint8)
    rs.locate_device_robust(N, M, S, d_orig, d_rec, recovery_rows=mask, max_outliers=t, d_located=loc,
                            d_mismatch=flags, d_outlier=out, rate_=RATE[rate], stream=stream)
    torch.cuda.synchronize()
    got, got_flags = L.check_outputs(loc_buf, flag_buf, what)
    outlier = check_outlier(out_buf, what)
    assert np.array_equal(d_orig.cpu().numpy(), orig), what + ": d_original was written"
    assert np.array_equal(d_rec.cpu().numpy(), rec), what + ": d_recovery was written"
    return int(got[0]), got_flags, outlier


def run_cases(torch, rs, rate, N, M, S, pad=0, mask=None, **kw):
    seen = set()
    for case in RC.cases(rate, N, M, S, mask=mask, **kw):
        name, t, orig, rec, _, _ = case
        what = f"{rate} {N}:{M} x {S} pad {pad} {name}"
        want, want_flags, want_out = RC.model(rate, case, mask=mask)
        got, flags, outlier = locate_one(torch, rs, rate, N, M, S, orig, rec, t, pad, mask, what)
        assert np.array_equal(flags, want_flags), \
            f"{what}: flagged rows {np.flatnonzero(flags).tolist()[:8]}, want {np.flatnonzero(want_flags).tolist()[:8]}"
        assert got == want, f"{what}: located {got}, want {want}"
        assert np.array_equal(outlier, want_out), \
            f"{what}: outliers {np.flatnonzero(outlier).tolist()}, want {np.flatnonzero(want_out).tolist()}"
        seen.add("i" if want >= 0 else want)
    return seen


@pytest.mark.parametrize("S,pad", LAYOUTS, ids=lambda v: str(v))
@pytest.mark.parametrize("rate,N,M", COLUMN, ids=lambda v: str(v))
def test_column_shapes(torch, rs, rate, N, M, S, pad):
    assert run_cases(torch, rs, rate, N, M, S, pad) == {"i", CLEAN, ROWS, UNKNOWN}


@pytest.mark.parametrize("rate,N,M,S,pad", OTHER, ids=lambda v: str(v))
def test_other_shapes(torch, rs, rate, N, M, S, pad):
    assert run_cases(torch, rs, rate, N, M, S, pad) >= {"i", CLEAN, ROWS}


def test_pass_kernels(torch, rs):
    """4096:4096 x 64 B, stripe by stripe through the pass kernels: bit0, t = 1 and 7."""
    assert run_cases(torch, rs, "default", 4096, 4096, 64, forms=("bit0",), ts=(1, 7)) == {"i", CLEAN, ROWS, UNKNOWN}


@pytest.mark.parametrize("rate,N,M,S,pad", [("high", 70, 100, 64, 0), ("default", 300, 500, 72, 8)], ids=lambda v: str(v))
def test_masks(torch, rs, rate, N, M, S, pad):
    """Exactly 2 (t + 1) selected rows; every third row unselected; junk (0xC3) in the unselected
    rows and the row padding; an outlier in an unselected row is never flagged, counted or named."""
    for t in (1, 2):
        mask = np.zeros(M, np.uint8)
        mask[[1, M // 3, M // 2, M - 2] + ([3, M - 5] if t == 2 else [])] = 1
        assert int(mask.sum()) == 2 * (t + 1)
        run_cases(torch, rs, rate, N, M, S, pad, mask=mask, forms=("bit0",), ts=(t,), junk=True)
    mask = np.ones(M, np.uint8)
    mask[2::3] = 0
    run_cases(torch, rs, rate, N, M, S, pad, mask=mask, forms=("lastbit",), ts=(1, 2), junk=True)
    # one corrupt original, one outlier at a selected row, and damage in unselected rows only
    orig, rec = V.stripe(rate, N, M, S)
    sel, unsel = np.flatnonzero(mask), np.flatnonzero(mask == 0)
    bad, r = orig.copy(), rec.copy()
    bad[N // 3, S // 2] ^= 0x08
    r[unsel[0], 0] ^= 0x01
    r[unsel[-1]] = 0xC3
    r[sel[5], 7] ^= 0x80
    for t, want, outliers in ((1, N // 3, [sel[5]]), (2, N // 3, [sel[5]]), (0, UNKNOWN, [])):
        model = RM.locate(rate, bad, r, t, mask=mask)
        assert (model[0], np.flatnonzero(model[2]).tolist()) == (want, outliers)
        got, flags, outlier = locate_one(torch, rs, rate, N, M, S, bad, r, t, pad, mask, f"unselected damage t={t}")
        assert got == want and np.array_equal(flags, mask) and np.flatnonzero(outlier).tolist() == outliers


def batch_case(rate, N, M, S, B, t):
    """B stripes (5..8) with a different outcome, a different i and different outliers in each."""
    rng = np.random.default_rng(B)
    kinds = [("orig", 0, "lastbit", [0]), ("none",), ("rec",), ("orig", N - 1, "bit0", [1, 3]), ("two",),
             ("orig", N // 2, "bit0", [0, 3, 4]), ("orig", N // 3, "lastbit", []), ("every",)][:B]
    origs, recs, wants = [], [], []
    for b, k in enumerate(kinds):
        o, r = (x.copy() for x in V.stripe(rate, N, M, S, seed=b))
        want = (CLEAN, [])
        if k[0] == "orig":
            damage_original(o, k[1], k[2], rng)
            for j in k[3]:
                RC.hit(r, j, "plain", k[2])
            want = (k[1], k[3]) if len(k[3]) <= t else (UNKNOWN, [])
        elif k[0] == "rec":
            r[M // 2, 3 % S] ^= 0x02
            want = (ROWS, [])
        elif k[0] == "two":
            o[0, 0] ^= 0x10
            o[N - 1, S - 1] ^= 0x20
            want = (UNKNOWN, [])
        elif k[0] == "every":
            r ^= 1
            want = (UNKNOWN, [])
        model = RM.locate(rate, o, r, t)
        assert (model[0], np.flatnonzero(model[2]).tolist()) == want, (b, k, model[0])
        origs.append(o), recs.append(r), wants.append(model)
    return np.stack(origs), np.stack(recs), [np.stack([w[k] for w in wants]) for k in range(3)]


@pytest.mark.parametrize("rate,N,M,S,B,pad", [("default", 1024, 1024, 72, 6, 0), ("high", 70, 100, 66, 8, 4),
                                              ("high", 1000, 100, 66, 5, 0), ("default", 4096, 4096, 64, 5, 0)],
                         ids=lambda v: str(v))
def test_batch(torch, rs, rate, N, M, S, B, pad):
    """A one-launch shape and stripe-by-stripe shapes, with stripe padding: the constructed
    results, which are also those of a loop of single calls."""
    t = 2
    origs, recs, (want, want_flags, want_out) = batch_case(rate, N, M, S, B, t)
    d_orig, d_rec = V.padded_batch(torch, origs, 2, pad), V.padded_batch(torch, recs, 3, pad)
    loc, loc_buf = guarded(torch, (B,), torch.int32)
    flags, flag_buf = guarded(torch, (B, M), torch.uint8)
    out, out_buf = guarded(torch, (B, M), torch.uint8)
    names = [r[0] for r in V.profiled(torch, rs, lambda: rs.locate_device_robust_batch(
        N, M, S, d_orig, d_rec, max_outliers=t, d_located=loc, d_mismatch=flags, d_outlier=out, rate_=RATE[rate]))]
    got, got_flags = L.check_outputs(loc_buf, flag_buf, "batch")
    got_out = check_outlier(out_buf, "batch").reshape(B, M)
    assert np.array_equal(d_orig.cpu().numpy(), origs) and np.array_equal(d_rec.cpu().numpy(), recs)
    assert got.tolist() == want.tolist(), (got, want)
    assert np.array_equal(got_flags.reshape(B, M), want_flags) and np.array_equal(got_out, want_out)
    # one launch of each kernel where the batch encode is one launch, else stripe by stripe; none of the locate's
    count = names.count("k_locate_find_pairs")
    assert count == names.count("k_locate_count") == names.count("k_locate_decide") == names.count("k_verify_rows"), names
    assert count == {1024: 1, 70: 1, 1000: B, 4096: B}[N], names
    assert "k_locate_find" not in names and "k_locate_confirm" not in names
    for b in range(B):
        single = locate_one(torch, rs, rate, N, M, S, origs[b], recs[b], t, pad, what=f"stripe {b}")
        assert single[0] == got[b] and np.array_equal(single[1], got_flags.reshape(B, M)[b])
        assert np.array_equal(single[2], got_out[b])
    # one mask for every stripe, and tensors the call allocates itself
    mask = np.ones(M, np.uint8)
    mask[M // 2] = 0
    l2, f2, o2 = rs.locate_device_robust_batch(N, M, S, d_orig, d_rec, recovery_rows=mask, max_outliers=1,
                                               rate_=RATE[rate])
    assert l2.shape == (B,) and str(l2.dtype) == "torch.int32" and f2.shape == o2.shape == (B, M) and o2.is_cuda
    model = [RM.locate(rate, origs[b], recs[b], 1, mask=mask) for b in range(B)]
    assert l2.cpu().numpy().tolist() == [m[0] for m in model]
    assert np.array_equal(f2.cpu().numpy(), np.stack([m[1] for m in model]))
    assert np.array_equal(o2.cpu().numpy(), np.stack([m[2] for m in model]))


@pytest.mark.parametrize("rate,N,M,S,B,pad", [("default", 1024, 1024, 72, 6, 0), ("high", 1000, 100, 66, 5, 0)],
                         ids=lambda v: str(v))
def test_max_outliers_zero_is_the_locate(torch, rs, rate, N, M, S, B, pad):
    """Compatibility: with max_outliers = 0, d_located and d_mismatch are locate_device_batch's on
    the same batch -- the locate's own batch, and the robust one with its outliers -- and d_outlier
    is all zero."""
    seen = set()
    for origs, recs in (L.batch_case(rate, N, M, S, B)[:2], batch_case(rate, N, M, S, B, 2)[:2]):
        d_orig, d_rec = V.padded_batch(torch, origs, 2, pad), V.padded_batch(torch, recs, 3, pad)
        want, want_flags = rs.locate_device_batch(N, M, S, d_orig, d_rec, rate_=RATE[rate])
        loc, loc_buf = guarded(torch, (B,), torch.int32)
        flags, flag_buf = guarded(torch, (B, M), torch.uint8)
        out, out_buf = guarded(torch, (B, M), torch.uint8)
        rs.locate_device_robust_batch(N, M, S, d_orig, d_rec, max_outliers=0, d_located=loc, d_mismatch=flags,
                                      d_outlier=out, rate_=RATE[rate])
        torch.cuda.synchronize()
        got, got_flags = L.check_outputs(loc_buf, flag_buf, "t = 0")
        assert got.tolist() == want.cpu().numpy().tolist()
        assert np.array_equal(got_flags.reshape(B, M), want_flags.cpu().numpy())
        assert not check_outlier(out_buf, "t = 0").any()
        seen |= {min(int(x), 0) for x in got}
    assert seen == {0, CLEAN, ROWS, UNKNOWN}  # every outcome was compared


def test_table_is_shared_with_the_locate_and_the_heal(torch, rs):
    """The table of a shape is built once, by whichever of the three calls comes first on the
    stream, and found by the others; the update's own table is a different one."""
    rate, N, M, S = "default", 300, 500, 72
    orig, rec = V.stripe(rate, N, M, S)
    bad, r = orig.copy(), rec.copy()
    bad[N - 1, 1] ^= 0x40
    r[7, 9] ^= 0x04
    d_bad, d_rec = V.view(torch, bad, 0), V.view(torch, r, 0)
    robust = lambda: rs.locate_device_robust(N, M, S, d_bad, d_rec, max_outliers=1)
    plain = lambda: rs.locate_device(N, M, S, d_bad, d_rec)
    heal = lambda: rs.heal_device(N, M, S, d_bad.clone(), d_rec.clone(), mode=rs.HEAL_ORIGINAL)
    coef = lambda fn: L.coef_launches(V.profiled(torch, rs, fn))
    rs.release_stream_scratch()
    first = V.profiled(torch, rs, robust)
    # two slabs of originals (256 + 44): a unit stripe and a log launch each, around the encodes
    assert L.coef_launches(first) == ["k_coef_unit_slab", "k_coef_log_slab"] * 2, first
    assert [x[0] for x in first][-4:] == ["k_verify_rows", "k_locate_find_pairs", "k_locate_count", "k_locate_decide"]
    assert coef(robust) == [] and coef(plain) == [] and coef(heal) == []
    mask = np.zeros(M, np.uint8)
    mask[[3, 4, 7, 400]] = 1
    assert coef(lambda: rs.locate_device_robust(N, M, S, d_bad, d_rec, recovery_rows=mask, max_outliers=1)) == []
    # the reverse: after a release the locate builds it and the robust locate finds it
    rs.release_stream_scratch()
    assert len(coef(plain)) == 4 and coef(robust) == [] and coef(heal) == []
    rs.release_stream_scratch()
    assert len(coef(heal)) == 4 and coef(robust) == []
    # an update of the same shape in between: its own table, built once, and ours stays
    d_new = torch.zeros((1, S), dtype=torch.uint8, device="cuda")
    d_new[0, 1] = 0x40
    d_upd = d_rec.clone()
    upd = lambda: rs.update_device(N, M, S, [N - 1], None, d_new, d_upd)
    assert coef(upd) == ["k_coef_unit", "k_coef_log"]
    assert coef(robust) == [] and coef(upd) == []
    got = [x.cpu().numpy() for x in robust()]
    assert int(got[0][0]) == N - 1 and got[1].all() and np.flatnonzero(got[2]).tolist() == [7]
    assert int(plain()[0].cpu()[0]) == UNKNOWN
    # another shape rebuilds
    o2, r2 = V.stripe("high", 70, 100, 64)
    other = lambda: rs.locate_device_robust(70, 100, 64, V.view(torch, o2, 0), V.view(torch, r2, 0), rate_=RATE["high"])
    assert coef(other) == ["k_coef_unit_slab", "k_coef_log_slab"] and len(coef(robust)) == 4
    rs.release_stream_scratch()


def test_calls_in_flight(torch, rs):
    """Two robust locates of different stripes (and different t) on one stream with an encode
    between them, and two on two streams."""
    rate, N, M, S = "default", 200, 200, 72
    orig, rec = V.stripe(rate, N, M, S)
    a, b, ra, rb = orig.copy(), orig.copy(), rec.copy(), rec.copy()
    a[7, 0] ^= 1
    ra[0, 5] ^= 0x10
    b[N - 2, S - 1] ^= 0x80
    rb[[3, 199], 9] ^= 0x20
    d_a, d_b, d_ra, d_rb = (V.view(torch, x, 0) for x in (a, b, ra, rb))
    d_enc = torch.zeros((M, S), dtype=torch.uint8, device="cuda")
    mask = np.ones(M, np.uint8)
    mask[1] = 0  # (a mask on the second call only: the selection travels between the two)
    want_b = np.zeros(M, np.uint8)
    want_b[[3, 199]] = 1

    def check(xa, xb):
        assert int(xa[0].cpu()[0]) == 7 and np.flatnonzero(xa[2].cpu().numpy()).tolist() == [0]
        assert int(xb[0].cpu()[0]) == N - 2 and np.array_equal(xb[2].cpu().numpy(), want_b)

    torch.cuda.synchronize()
    xa = rs.locate_device_robust(N, M, S, d_a, d_ra, max_outliers=1)
    rs.encode_device(N, M, S, d_a, d_enc)
    xb = rs.locate_device_robust(N, M, S, d_b, d_rb, recovery_rows=mask, max_outliers=3)
    xc = rs.locate_device_robust(N, M, S, d_a, d_enc, max_outliers=7)  # the encode of the corrupt originals agrees
    torch.cuda.synchronize()
    check(xa, xb)
    assert xa[1].cpu().numpy().all() and np.array_equal(xb[1].cpu().numpy(), mask)
    assert int(xc[0].cpu()[0]) == CLEAN and not xc[1].cpu().numpy().any() and not xc[2].cpu().numpy().any()
    assert np.array_equal(d_enc.cpu().numpy(), O.encode(rate, a, M))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    xa = rs.locate_device_robust(N, M, S, d_a, d_ra, max_outliers=1, stream=s1)
    xb = rs.locate_device_robust(N, M, S, d_b, d_rb, max_outliers=2, stream=s2)
    torch.cuda.synchronize()
    check(xa, xb)
    rs.release_stream_scratch(s1)
    rs.release_stream_scratch(s2)


def test_scrub(torch, rs):
    """Robust locate of a batch, read the three outputs, one repair_device_batch_masks with
    original i and the outlier rows (or the flagged rows of a ROWS stripe) absent: every stripe ends
    byte-identical to the clean one."""
    rate, N, M, S, B = "high", 70, 100, 66, 5
    pairs = [V.stripe(rate, N, M, S, seed=b) for b in range(B)]
    origs, recs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    bad_o, bad_r = origs.copy(), recs.copy()
    rng = np.random.default_rng(5)
    bad_o[0, 33] = rng.integers(0, 256, S, dtype=np.uint8)  # a whole shard, and its reference row
    bad_r[0, 0, 40] ^= 0x08
    bad_r[1, 17, 40] ^= 0x08  # recovery rows alone
    bad_r[1, 93, 3] ^= 0x80
    bad_o[3, N - 1, S - 1] ^= 0x80  # the tail's last high byte, and two whole rows
    bad_r[3, [2, 99]] = rng.integers(0, 256, (2, S), dtype=np.uint8)
    bad_o[4, 0, 0] ^= 0x01
    d_orig, d_rec = V.view(torch, bad_o, 0), V.view(torch, bad_r, 0)
    located, flags, outlier = (x.cpu().numpy() for x in rs.locate_device_robust_batch(
        N, M, S, d_orig, d_rec, max_outliers=2, rate_=RATE[rate]))
    assert located.tolist() == [33, ROWS, CLEAN, N - 1, 0]
    assert [np.flatnonzero(o).tolist() for o in outlier] == [[0], [], [], [2, 99], []]
    # (the plain locate gives up on stripes 0 and 3)
    assert rs.locate_device_batch(N, M, S, d_orig, d_rec, rate_=RATE[rate])[0].cpu().numpy().tolist() == \
        [UNKNOWN, ROWS, CLEAN, UNKNOWN, 0]
    orig_ok, rec_ok = np.ones((B, N), np.uint8), np.ones((B, M), np.uint8)
    for b, i in enumerate(located):
        if i >= 0:
            orig_ok[b, i] = 0
            rec_ok[b] = 1 - outlier[b]
        elif i == ROWS:
            rec_ok[b] = 1 - flags[b]
    rs.repair_device_batch_masks(N, M, S, d_orig, orig_ok, d_rec, rec_ok, d_orig, d_rec, rate_=RATE[rate])
    again = rs.locate_device_robust_batch(N, M, S, d_orig, d_rec, max_outliers=2, rate_=RATE[rate])
    assert (again[0].cpu().numpy() == CLEAN).all() and not again[2].cpu().numpy().any()
    assert np.array_equal(d_rec.cpu().numpy(), recs) and np.array_equal(d_orig.cpu().numpy(), origs)
