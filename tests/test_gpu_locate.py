"""GPU: rs_locate_device* -- which single original of a stripe is corrupt?

Expected values are constructed, not computed by the code under test: a clean stripe comes from the
CPU oracle, bytes are then flipped.  A single corrupt original i must come back as exactly i; every
other case must equal tests/locate_model.py, the numpy statement of the contract, and the status
each case is meant to show is asserted on the model first.  The flags must equal "the oracle's
encode of the stored originals differs from the stored recovery", per selected row.  Every run also
checks that nothing but the two outputs was written: the inputs equal their host copies, the guards
around d_located and the flags are as before, and both outputs, pre-filled with 0xFF, come back
fully defined.
"""
import numpy as np
import pytest

import locate_model as LM
import oracle_lib as O
import span_cases as SC
import test_gpu_verify as V
import wide_cases as W

pytestmark = pytest.mark.gpu

RATE = V.RATE
GUARD = V.GUARD
CLEAN, ROWS, UNKNOWN = LM.CLEAN, LM.ROWS, LM.UNKNOWN

# (rate, N, M): the encode is the staged single-chunk column kernel, or with mono_enable's defaults
# the lane kernel at 2^8 and 2^9 rows (the batch is one launch)
COLUMN = [("high", 70, 100), ("low", 100, 70), ("default", 200, 200), ("default", 300, 500),
          ("default", 1024, 1024), ("default", 2048, 2048)]
# (S, row padding): whole blocks; a tail; a tail with rows that are not 4-byte aligned (byte-wise)
LAYOUTS = [(64, 0), (72, 0), (66, 4)]
# (rate, N, M, S, row padding): the pass kernels, multi-chunk encodes, tiny stripes
OTHER = [("default", 4096, 4096, 64, 0), ("high", 1000, 100, 66, 0), ("low", 128, 1024, 64, 0),
         ("default", 3, 2, 2, 0), ("default", 1, 2, 64, 0), ("default", 2, 3, 190, 0)]
FORMS = ["bit0", "lastbit", "highhalf", "lastpack", "shard"]


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


def damage_original(orig, i, form, rng):
    """One error form in original i, in place."""
    S = orig.shape[1]
    full, th = S // 64, (S % 64) // 2
    if form == "bit0":
        orig[i, 0] ^= 0x01
    elif form == "lastbit":  # the tail's last high byte
        orig[i, S - 1] ^= 0x80
    elif form == "highhalf":  # the high half of a middle block only (a tail alone: its high bytes)
        lo, hi = ((full // 2) * 64 + 32, (full // 2) * 64 + 64) if full else (th, S)
        orig[i, lo:hi] ^= rng.integers(1, 256, hi - lo, dtype=np.uint8)
    elif form == "lastpack":  # the last pack only: its low bytes and its high bytes
        if th:
            e = 4 * ((th - 1) // 4)
            cols = list(range(full * 64 + e, full * 64 + th)) + list(range(full * 64 + th + e, S))
        else:
            cols = list(range(S - 36, S - 32)) + list(range(S - 4, S))
        orig[i, cols] ^= rng.integers(1, 256, len(cols), dtype=np.uint8)
    else:  # a whole random shard
        assert form == "shard"
        orig[i] ^= rng.integers(1, 256, S, dtype=np.uint8)


def cases(rate, N, M, S, wide=False):
    """[(name, originals, recovery, intended status or None)] of one stripe.  The intended status
    is what the case is built to show; None where the shape is too small for the case to mean one
    thing (two rows in all: "every row differs" may be one original's doing).  wide: the positional
    cases of tests/wide_cases.py instead, damage placed by pack number."""
    orig, rec = V.stripe(rate, N, M, S)
    if wide:
        return W.locate_cases(orig, rec, CLEAN, ROWS, UNKNOWN)
    rng = np.random.default_rng(N * 7 + M + S)
    out = [("none", orig, rec, CLEAN)]
    for i in sorted({0, N // 2, N - 1}):
        for form in FORMS:
            bad = orig.copy()
            damage_original(bad, i, form, rng)
            out.append((f"original {i} {form}", bad, rec, i))
    for name, rows in (("first", [0]), ("last", [M - 1]), ("two middle", sorted({M // 2, M // 3}))):
        bad = rec.copy()
        for k, j in enumerate(rows):
            bad[j, (5 + 32 * k) % S] ^= 0x10 << k
        out.append((f"recovery {name}", orig, bad, ROWS if len(rows) < M else None))
    if N >= 2:
        a, b = 0, N - 1
        bad = orig.copy()  # two originals in different columns
        bad[a, 0] ^= 0x10
        bad[b, S - 1] ^= 0x20
        out.append(("two originals, two columns", bad, rec, UNKNOWN if M >= 3 else None))
        bad = orig.copy()  # ... and in one column
        bad[a, 0] ^= 0x10
        bad[N // 2 if N > 2 else b, 0] ^= 0x33
        out.append(("two originals, one column", bad, rec, UNKNOWN if M >= 3 else None))
    bad, badr = orig.copy(), rec.copy()  # one original plus one recovery row
    bad[N - 1, 0] ^= 0x04
    badr[1, S // 2] ^= 0x40
    out.append(("original and recovery", bad, badr, UNKNOWN if M >= 3 else None))
    badr = rec.copy()  # every recovery row
    for j in range(M):
        badr[j, (j * 7) % S] ^= 1 << (j % 8)
    out.append(("every recovery row", orig, badr, UNKNOWN if M >= 3 else None))
    return out


def guarded(torch, shape, dtype):
    """A tensor of `shape` pre-filled with 0xFF bytes between two guards; (tensor, whole buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((2 * GUARD + n,), 0xFF if dtype == torch.uint8 else -1, dtype=dtype, device="cuda")
    return buf[GUARD:GUARD + n].view(*shape), buf


def check_outputs(loc_buf, flag_buf, what):
    """Guards intact, every word and byte defined; (located, flags) on the host."""
    l, f = loc_buf.cpu().numpy(), flag_buf.cpu().numpy()
    assert (l[:GUARD] == -1).all() and (l[-GUARD:] == -1).all(), what + ": a word outside d_located was written"
    assert (f[:GUARD] == 0xFF).all() and (f[-GUARD:] == 0xFF).all(), what + ": a byte outside the flags was written"
    assert (f[GUARD:-GUARD] <= 1).all(), what + ": a flag is neither 0 nor 1"
    assert (l[GUARD:-GUARD] >= UNKNOWN).all(), what + ": a result is not defined"
    return l[GUARD:-GUARD], f[GUARD:-GUARD]


def locate_one(torch, rs, rate, N, M, S, orig, rec, pad=0, mask=None, what="", stream=None):
    d_orig, d_rec = V.view(torch, orig, pad), V.view(torch, rec, pad)
    loc, loc_buf = guarded(torch, (1,), torch.int32)
    flags, flag_buf = guarded(torch, (M,), torch.uint8)
    rs.locate_device(N, M, S, d_orig, d_rec, recovery_rows=mask, d_located=loc, d_mismatch=flags, rate_=RATE[rate],
                     stream=stream)
    torch.cuda.synchronize()
    got, got_flags = check_outputs(loc_buf, flag_buf, what)
    assert np.array_equal(d_orig.cpu().numpy(), orig), what + ": d_original was written"
    assert np.array_equal(d_rec.cpu().numpy(), rec), what + ": d_recovery was written"
    return int(got[0]), got_flags


def run_cases(torch, rs, rate, N, M, S, pad=0, mask=None, only=None, wide=False):
    for name, orig, rec, intended in cases(rate, N, M, S, wide):
        if only and not any(name.startswith(o) for o in only):
            continue
        what = f"{rate} {N}:{M} x {S} pad {pad} {name}"
        # the flags: the oracle's encode of the stored originals against the stored recovery
        enc = O.encode(rate, orig, M)
        sel = np.ones(M, bool) if mask is None else np.asarray(mask) != 0
        truth = ((enc != rec).any(axis=1) & sel).astype(np.uint8)
        want, want_flags = LM.locate(rate, orig, rec, mask=mask, D=LM.elements(enc ^ rec).astype(np.int64))
        if intended is not None and mask is None:
            assert want == intended, f"{what}: the model says {want}, the case was built for {intended}"
        got, got_flags = locate_one(torch, rs, rate, N, M, S, orig, rec, pad, mask, what)
        assert np.array_equal(got_flags, truth) and np.array_equal(truth, want_flags), \
            f"{what}: flagged rows {np.flatnonzero(got_flags).tolist()[:8]}, want {np.flatnonzero(truth).tolist()[:8]}"
        assert got == want, f"{what}: located {got}, want {want}"


@pytest.mark.parametrize("S,pad", LAYOUTS, ids=lambda v: str(v))
@pytest.mark.parametrize("rate,N,M", COLUMN, ids=lambda v: str(v))
def test_column_shapes(torch, rs, rate, N, M, S, pad):
    run_cases(torch, rs, rate, N, M, S, pad)


@pytest.mark.parametrize("rate,N,M,S,pad", OTHER, ids=lambda v: str(v))
def test_other_shapes(torch, rs, rate, N, M, S, pad):
    run_cases(torch, rs, rate, N, M, S, pad)


def masks_of(M):
    two = np.zeros(M, np.uint8)
    two[[0, M - 1]] = 1  # exactly two rows: the first and the last
    adjacent = np.zeros(M, np.uint8)
    adjacent[[M // 2, M // 2 + 1]] = 1  # ... adjacent in the middle, row 0 unselected
    three = np.zeros(M, np.uint8)
    three[[1, M // 2, M - 2]] = 1
    most = np.ones(M, np.uint8)
    most[M // 3] = 0
    return [two, adjacent, three, most]


@pytest.mark.parametrize("rate,N,M,S,pad", [("high", 70, 100, 64, 0), ("default", 300, 500, 72, 8),
                                            ("default", 1024, 1024, 66, 4), ("high", 1000, 100, 66, 0),
                                            ("default", 4096, 4096, 64, 0)] + [s + (0,) for s in SC.MASK_SHAPES],
                         ids=lambda v: str(v))
def test_masks(torch, rs, rate, N, M, S, pad):
    """Each mask over the cases that mean something under it; then junk (0xC3) in the unselected
    rows and in the row padding changes neither output."""
    check_masks(torch, rs, rate, N, M, S, pad)


@pytest.mark.parametrize("rate,N,M,S,mode", SC.MASK_SHAPES_MODE0, ids=lambda v: str(v))
def test_masks_on_the_pass_kernels(torch, rs, rate, N, M, S, mode):
    """test_masks with the column kernels off: two pass levels over several chunks."""
    try:
        rs.mono_enable(mode)
        check_masks(torch, rs, rate, N, M, S, 0)
    finally:
        rs.mono_enable(True)


def check_span_masks(torch, rs, rate, N, M, S, pad):
    """The spans of tests/span_cases.py as masks (every third row inside a span unselected; the
    call takes no fewer than two rows), junk that differs in every unselected row: a corrupt
    original i in {0, N - 1} comes back as i, and the flags are the oracle's -- every selected
    row, as one corrupt original changes them all."""
    orig, rec = V.stripe(rate, N, M, S)
    rng = np.random.default_rng(N + 5 * M)
    for mask in V.span_masks(rate, N, M):
        sel = mask != 0
        if int(sel.sum()) < 2:
            continue
        junk = rec.copy()
        junk[~sel] ^= rng.integers(1, 256, (int((~sel).sum()), S), dtype=np.uint8)
        rows = np.flatnonzero(sel)
        what = f"{rate} {N}:{M} x {S} pad {pad} span mask [{rows[0]}, {rows[-1] + 1})"
        got, flags = locate_one(torch, rs, rate, N, M, S, orig, junk, pad, mask, what + " clean")
        assert got == CLEAN and not flags.any(), (what, got, np.flatnonzero(flags)[:8])
        for i in sorted({0, N - 1}):
            bad = orig.copy()
            bad[i, (7 * i + 3) % S] ^= 0x40
            enc = O.encode(rate, bad, M)
            truth = ((enc != junk).any(axis=1) & sel).astype(np.uint8)
            want, want_flags = LM.locate(rate, bad, junk, mask=mask, D=LM.elements(enc ^ junk).astype(np.int64))
            assert want == i and np.array_equal(truth, mask), f"{what}: the model says {want} for original {i}"
            got, flags = locate_one(torch, rs, rate, N, M, S, bad, junk, pad, mask, f"{what} original {i}")
            assert np.array_equal(flags, truth) and np.array_equal(truth, want_flags), \
                f"{what}: flagged rows {np.flatnonzero(flags).tolist()[:8]}, want {np.flatnonzero(truth).tolist()[:8]}"
            assert got == i, f"{what}: located {got}, want {i}"


def check_masks(torch, rs, rate, N, M, S, pad):
    orig, rec = V.stripe(rate, N, M, S)
    check_span_masks(torch, rs, rate, N, M, S, pad)
    for mask in masks_of(M):
        run_cases(torch, rs, rate, N, M, S, pad, mask=mask,
                  only=("none", "original 0 bit0", f"original {N // 2} shard", f"original {N - 1} lastbit",
                        "recovery", "two originals", "every recovery row"))
        # a corrupt selected row is ROWS, a corrupt unselected row is not seen
        sel, unsel = np.flatnonzero(mask), np.flatnonzero(mask == 0)
        bad = rec.copy()
        bad[sel[-1], S - 1] ^= 0x01
        got, flags = locate_one(torch, rs, rate, N, M, S, orig, bad, pad, mask, "selected row")
        assert got == ROWS and np.flatnonzero(flags).tolist() == [sel[-1]]
        junk = rec.copy()
        junk[unsel] = 0xC3
        got, flags = locate_one(torch, rs, rate, N, M, S, orig, junk, pad, mask, "junk rows")
        assert got == CLEAN and not flags.any()
        worse = orig.copy()
        worse[N // 3, S // 2] ^= 0x08
        got, flags = locate_one(torch, rs, rate, N, M, S, worse, junk, pad, mask, "junk rows, one original")
        assert got == N // 3 and np.array_equal(flags, mask)


def batch_case(rate, N, M, S, B, wide=False):
    """B stripes (up to 8) with a different outcome and a different i in each.  wide: the ROWS
    stripe's row is damaged in the last pack (tests/wide_cases.py), not in the first."""
    rng = np.random.default_rng(B)
    kinds = [("orig", 0, "lastbit"), ("none",), ("rec",), ("orig", N - 1, "shard"), ("two",), ("orig", N // 2, "lastpack"),
             ("orig", N // 3, "highhalf"), ("every",)][:B]
    origs, recs, wants = [], [], []
    for b, k in enumerate(kinds):
        o, r = (x.copy() for x in V.stripe(rate, N, M, S, seed=b))
        if k[0] == "orig":
            damage_original(o, k[1], k[2], rng)
            want = k[1]
        elif k[0] == "rec":
            if wide:
                W.damage_pack(r, M // 2, W.packs_of(S) - 1, rng)
            else:
                r[M // 2, 3 % S] ^= 0x02
            want = ROWS
        elif k[0] == "two":
            o[0, 0] ^= 0x10
            o[N - 1, S - 1] ^= 0x20
            want = UNKNOWN
        elif k[0] == "every":
            r ^= 1
            want = UNKNOWN
        else:
            want = CLEAN
        model, flags = LM.locate(rate, o, r)
        assert model == want, (b, k, model)
        origs.append(o), recs.append(r), wants.append((want, flags))
    return np.stack(origs), np.stack(recs), np.array([w[0] for w in wants]), np.stack([w[1] for w in wants])


@pytest.mark.parametrize("rate,N,M,S,B,pad", [("default", 1024, 1024, 72, 6, 0), ("high", 70, 100, 66, 8, 4),
                                              ("high", 1000, 100, 66, 5, 0), ("default", 4096, 4096, 64, 5, 0)],
                         ids=lambda v: str(v))
def test_batch(torch, rs, rate, N, M, S, B, pad, wide=False, groups=None):
    """A one-launch shape and stripe-by-stripe shapes, with stripe padding: the constructed
    results, which are also those of a loop of single calls.  (wide, groups:
    tests/test_gpu_wide_shards.py's -- batch_case's wide form, and the number of groups the batch
    must run in.)"""
    origs, recs, want, want_flags = batch_case(rate, N, M, S, B, wide)
    d_orig, d_rec = V.padded_batch(torch, origs, 2, pad), V.padded_batch(torch, recs, 3, pad)
    loc, loc_buf = guarded(torch, (B,), torch.int32)
    flags, flag_buf = guarded(torch, (B, M), torch.uint8)
    names = [r[0] for r in V.profiled(torch, rs, lambda: rs.locate_device_batch(
        N, M, S, d_orig, d_rec, d_located=loc, d_mismatch=flags, rate_=RATE[rate]))]
    got, got_flags = check_outputs(loc_buf, flag_buf, "batch")
    assert np.array_equal(d_orig.cpu().numpy(), origs) and np.array_equal(d_rec.cpu().numpy(), recs)
    assert got.tolist() == want.tolist(), (got, want)
    assert np.array_equal(got_flags.reshape(B, M), want_flags)
    # one launch of each kernel where the batch encode is one launch, else stripe by stripe
    count = names.count("k_locate_find")
    assert count == names.count("k_locate_confirm") == names.count("k_verify_rows"), names
    assert count == {1024: 1, 1000: B}.get(N, count) and count in (1, B), names
    assert groups is None or count == groups, names
    for b in range(B):
        single, single_flags = locate_one(torch, rs, rate, N, M, S, origs[b], recs[b], pad, what=f"stripe {b}")
        assert single == got[b] and np.array_equal(single_flags, got_flags.reshape(B, M)[b])
    # one mask for every stripe, and tensors the call allocates itself
    mask = np.ones(M, np.uint8)
    mask[M // 2] = 0
    l2, f2 = rs.locate_device_batch(N, M, S, d_orig, d_rec, recovery_rows=mask, rate_=RATE[rate])
    assert l2.shape == (B,) and str(l2.dtype) == "torch.int32" and f2.shape == (B, M) and l2.is_cuda
    model = [LM.locate(rate, origs[b], recs[b], mask=mask) for b in range(B)]
    assert l2.cpu().numpy().tolist() == [m[0] for m in model]
    assert np.array_equal(f2.cpu().numpy(), np.stack([m[1] for m in model]))


def coef_launches(recs):
    return [r[0] for r in recs if r[0].startswith("k_coef_")]


def test_table_is_built_once_per_shape(torch, rs):
    """The table of a shape is built by the first call on a stream and reused; another shape or
    release_stream_scratch rebuilds it; the update's own table is a different one."""
    rate, N, M, S = "default", 300, 500, 72
    orig, rec = V.stripe(rate, N, M, S)
    bad = orig.copy()
    bad[N - 1, 1] ^= 0x40
    d_bad, d_rec = V.view(torch, bad, 0), V.view(torch, rec, 0)
    call = lambda: rs.locate_device(N, M, S, d_bad, d_rec)
    rs.release_stream_scratch()
    first = V.profiled(torch, rs, call)
    # two slabs of originals (256 + 44): a unit stripe and a log launch each, around the encodes
    assert coef_launches(first) == ["k_coef_unit_slab", "k_coef_log_slab"] * 2, first
    assert [r[0] for r in first][-3:] == ["k_verify_rows", "k_locate_find", "k_locate_confirm"]
    second = V.profiled(torch, rs, call)
    assert coef_launches(second) == [] and int(call()[0].cpu()[0]) == N - 1
    # a masked call and a batch of the same shape use the same table
    mask = np.zeros(M, np.uint8)
    mask[[3, 4, 400]] = 1
    assert coef_launches(V.profiled(torch, rs, lambda: rs.locate_device(N, M, S, d_bad, d_rec, recovery_rows=mask))) == []
    # an update of the same shape in between: its own table, built once, and ours stays
    d_new = torch.zeros((1, S), dtype=torch.uint8, device="cuda")
    d_new[0, 1] = 0x40  # the delta that turns `bad` back into `orig`, applied to a copy of the recovery
    d_upd = d_rec.clone()
    upd = lambda: rs.update_device(N, M, S, [N - 1], None, d_new, d_upd)
    assert coef_launches(V.profiled(torch, rs, upd)) == ["k_coef_unit", "k_coef_log"]
    assert coef_launches(V.profiled(torch, rs, call)) == []
    assert coef_launches(V.profiled(torch, rs, upd)) == []  # (applied twice: d_upd is the recovery again)
    torch.cuda.synchronize()
    assert np.array_equal(d_upd.cpu().numpy(), rec)
    got, _ = rs.locate_device(N, M, S, d_bad, d_rec)
    assert int(got.cpu()[0]) == N - 1
    # another shape (the other rate of the same counts is one) rebuilds, and so does coming back
    o2, r2 = V.stripe("high", 70, 100, 64)
    other = lambda: rs.locate_device(70, 100, 64, V.view(torch, o2, 0), V.view(torch, r2, 0), rate_=RATE["high"])
    assert coef_launches(V.profiled(torch, rs, other)) == ["k_coef_unit_slab", "k_coef_log_slab"]
    assert len(coef_launches(V.profiled(torch, rs, call))) == 4
    rs.release_stream_scratch()
    assert len(coef_launches(V.profiled(torch, rs, call))) == 4
    assert int(call()[0].cpu()[0]) == N - 1


def test_locates_in_flight(torch, rs):
    """Two locates of different stripes on one stream with an encode between them, and two on two
    streams."""
    rate, N, M, S = "default", 200, 200, 72
    orig, rec = V.stripe(rate, N, M, S)
    a, b = orig.copy(), orig.copy()
    a[7, 0] ^= 1
    b[N - 2, S - 1] ^= 0x80
    d_a, d_b, d_rec = V.view(torch, a, 0), V.view(torch, b, 0), V.view(torch, rec, 0)
    d_enc = torch.zeros((M, S), dtype=torch.uint8, device="cuda")
    mask = np.ones(M, np.uint8)
    mask[0] = 0  # (a mask on the second call only: the selection travels between the two)
    torch.cuda.synchronize()
    la, fa = rs.locate_device(N, M, S, d_a, d_rec)
    rs.encode_device(N, M, S, d_a, d_enc)
    lb, fb = rs.locate_device(N, M, S, d_b, d_rec, recovery_rows=mask)
    lc, fc = rs.locate_device(N, M, S, d_a, d_enc)  # the encode of the corrupt originals agrees with them
    torch.cuda.synchronize()
    assert (int(la.cpu()[0]), int(lb.cpu()[0]), int(lc.cpu()[0])) == (7, N - 2, CLEAN)
    assert fa.cpu().numpy().all() and np.array_equal(fb.cpu().numpy(), mask) and not fc.cpu().numpy().any()
    assert np.array_equal(d_enc.cpu().numpy(), O.encode(rate, a, M))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    la, _ = rs.locate_device(N, M, S, d_a, d_rec, stream=s1)
    lb, _ = rs.locate_device(N, M, S, d_b, d_rec, stream=s2)
    torch.cuda.synchronize()
    assert (int(la.cpu()[0]), int(lb.cpu()[0])) == (7, N - 2)
    rs.release_stream_scratch(s1)
    rs.release_stream_scratch(s2)


def test_scrub(torch, rs):
    """Locate a batch, read the results, one repair_device_batch_masks with original i or the
    flagged rows marked absent: every stripe ends byte-identical to the clean one."""
    rate, N, M, S, B = "high", 70, 100, 66, 5
    pairs = [V.stripe(rate, N, M, S, seed=b) for b in range(B)]
    origs, recs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    bad_o, bad_r = origs.copy(), recs.copy()
    rng = np.random.default_rng(5)
    bad_o[0, 33] = rng.integers(0, 256, S, dtype=np.uint8)  # a whole shard
    bad_r[1, 17, 40] ^= 0x08
    bad_r[1, 93, 3] ^= 0x80
    bad_o[3, N - 1, S - 1] ^= 0x80  # the tail's last high byte
    bad_o[4, 0, 0] ^= 0x01
    d_orig, d_rec = V.view(torch, bad_o, 0), V.view(torch, bad_r, 0)
    located, flags = (t.cpu().numpy() for t in rs.locate_device_batch(N, M, S, d_orig, d_rec, rate_=RATE[rate]))
    assert located.tolist() == [33, ROWS, CLEAN, N - 1, 0]
    orig_ok, rec_ok = np.ones((B, N), np.uint8), np.ones((B, M), np.uint8)
    for b, i in enumerate(located):
        if i >= 0:
            orig_ok[b, i] = 0
        elif i == ROWS:
            rec_ok[b] = 1 - flags[b]
    assert np.flatnonzero(1 - rec_ok[1]).tolist() == [17, 93]
    rs.repair_device_batch_masks(N, M, S, d_orig, orig_ok, d_rec, rec_ok, d_orig, d_rec, rate_=RATE[rate])
    again, _ = rs.locate_device_batch(N, M, S, d_orig, d_rec, rate_=RATE[rate])
    assert (again.cpu().numpy() == CLEAN).all()
    assert np.array_equal(d_rec.cpu().numpy(), recs) and np.array_equal(d_orig.cpu().numpy(), origs)
