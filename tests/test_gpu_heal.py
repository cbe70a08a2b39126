"""GPU: rs_heal_device* -- the locate that also writes the correction, in place.

Expected values are constructed, not computed by the code under test: clean stripes come from the
CPU oracle, bytes are then flipped, and what the call must report and leave behind is
tests/heal_model.py, the numpy statement of the contract.  Where a case is one corrupt original the
healed matrix must also equal the CLEAN originals byte for byte, and where recovery rows were
flipped they must equal the oracle's encode.  Every run compares the WHOLE device buffer of both
matrices with the expected one -- the guards before and after, the junk in the row padding, the
stripe padding and every row that must not change -- and checks that the three outputs, pre-filled
with 0xFF between guards, come back fully defined.
"""
import numpy as np
import pytest

import heal_model as HM
import locate_model as LM
import oracle_lib as O
import test_gpu_locate as L
import test_gpu_verify as V
import wide_cases as W

pytestmark = pytest.mark.gpu

RATE = V.RATE
GUARD = 64  # bytes around a matrix (the base stays 4-byte aligned)
CLEAN, ROWS, UNKNOWN = LM.CLEAN, LM.ROWS, LM.UNKNOWN
ORIGINAL, RECOVERY = HM.ORIGINAL, HM.RECOVERY

# (rate, N, M): the column kernel, and with mono_enable's defaults the lane kernel at 2^8 rows
COLUMN = [("high", 70, 100), ("low", 100, 70), ("default", 200, 200)]
# (S, row padding): whole blocks; a tail; a tail with rows that are not 4-byte aligned (byte-wise)
LAYOUTS = [(64, 0), (72, 0), (66, 4)]
# (rate, N, M, S, row padding): the column kernel at its headline size, the pass kernels,
# multi-chunk encodes, tiny stripes
OTHER = [("default", 1024, 1024, 72, 0), ("default", 4096, 4096, 64, 0), ("high", 1000, 100, 66, 0),
         ("low", 128, 1024, 64, 0), ("default", 1, 3, 64, 0), ("default", 2, 3, 190, 0)]


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
    reed_solomon_simd.verify_set_fused(reed_solomon_simd.VERIFY_FUSED_DEFAULT)
    reed_solomon_simd.mono_enable(True)


class Dev:
    """A matrix [rows, S] or a batch [B, rows, S] on the device inside ONE buffer of junk: GUARD
    bytes, the rows with `pad` bytes after each and `extra` rows after each stripe, GUARD bytes.
    `t` is the strided view the library gets; check() compares the whole buffer."""

    def __init__(self, torch, a, pad=0, extra=0):
        a = np.asarray(a)
        self.batch = a.ndim == 3
        rows, S = a.shape[-2:]
        B = a.shape[0] if self.batch else 1
        self.inner = (B, rows + extra, S + pad)
        self.rows, self.S = rows, S
        n = int(np.prod(self.inner))
        self.junk = np.random.default_rng(rows * 3 + S + pad).integers(0, 256, 2 * GUARD + n, dtype=np.uint8)
        self.buf = torch.from_numpy(self.expect(a)).cuda()
        v = self.buf[GUARD:GUARD + n].view(*self.inner)[:, :rows, :S]
        self.t = v if self.batch else v[0]

    def expect(self, a):
        """The whole buffer when the matrix holds `a`."""
        h = self.junk.copy()
        h[GUARD:len(h) - GUARD].reshape(self.inner)[:, :self.rows, :self.S] = np.asarray(a).reshape(
            (self.inner[0], self.rows, self.S))
        return h

    def check(self, a, what):
        got, want = self.buf.cpu().numpy(), self.expect(a)
        if not np.array_equal(got, want):
            at = int(np.flatnonzero(got != want)[0]) - GUARD
            b, r, c = np.unravel_index(max(at, 0), self.inner) if 0 <= at < int(np.prod(self.inner)) else (-1, -1, -1)
            raise AssertionError(f"{what}: first wrong byte at offset {at} (stripe {b}, row {r}, column {c}; rows "
                                 f"{self.rows} x {self.S}): {got[at + GUARD]:#x}, want {want[at + GUARD]:#x}")


class Out:
    """The three outputs, pre-filled with 0xFF between guards."""

    def __init__(self, torch, B, M, batch):
        self.B, self.M = B, M
        self.loc, self.loc_buf = L.guarded(torch, (B,), torch.int32)
        self.flags, self.flag_buf = L.guarded(torch, (B, M) if batch else (M,), torch.uint8)
        self.act, self.act_buf = L.guarded(torch, (B,), torch.uint8)

    def read(self, what):
        """Guards intact, every word and byte defined; (located [B], flags [B, M], action [B])."""
        loc, flags = L.check_outputs(self.loc_buf, self.flag_buf, what)
        a = self.act_buf.cpu().numpy()
        g = L.GUARD
        assert (a[:g] == 0xFF).all() and (a[-g:] == 0xFF).all(), what + ": a byte outside d_action was written"
        assert np.isin(a[g:-g], (0, ORIGINAL, RECOVERY)).all(), what + f": an action is not defined: {a[g:-g]}"
        return loc, flags.reshape(self.B, self.M), a[g:-g]


def heal_one(torch, rs, rate, N, M, S, orig, rec, pad=0, mask=None, mode=3, max_rows=0, what="", stream=None,
             model=None):
    """One heal of one stripe on fresh device copies, checked against the model in full (`model`:
    HM.heal of the same arguments, where the caller has it); the model's (located, flags, action,
    originals after, recovery after)."""
    d_orig, d_rec = Dev(torch, orig, pad), Dev(torch, rec, pad)
    out = Out(torch, 1, M, False)
    rs.heal_device(N, M, S, d_orig.t, d_rec.t, recovery_rows=mask, mode=mode, max_rows=max_rows, d_located=out.loc,
                   d_mismatch=out.flags, d_action=out.act, rate_=RATE[rate], stream=stream)
    torch.cuda.synchronize()
    loc, flags, act = out.read(what)
    w_loc, w_flags, w_act, w_orig, w_rec = model or HM.heal(rate, orig, rec, mask=mask, mode=mode, max_rows=max_rows)
    assert int(loc[0]) == w_loc, f"{what}: located {loc[0]}, want {w_loc}"
    assert np.array_equal(flags[0], w_flags), \
        f"{what}: flagged rows {np.flatnonzero(flags[0]).tolist()[:8]}, want {np.flatnonzero(w_flags).tolist()[:8]}"
    assert int(act[0]) == w_act, f"{what}: action {act[0]}, want {w_act}"
    d_orig.check(w_orig, what + ": d_original")
    d_rec.check(w_rec, what + ": d_recovery")
    return w_loc, w_flags, w_act, w_orig, w_rec


def run_cases(torch, rs, rate, N, M, S, pad=0, mode=3, only=None, wide=False, again=False):
    """wide: the positional cases of tests/wide_cases.py; again: every stripe the heal wrote is healed
    a second time from what the first heal left, which must be CLEAN with action 0."""
    clean_orig, clean_rec = V.stripe(rate, N, M, S)
    for name, orig, rec, intended in L.cases(rate, N, M, S, wide):
        if only and not any(name.startswith(o) for o in only):
            continue
        what = f"{rate} {N}:{M} x {S} pad {pad} mode {mode} {name}"
        loc, flags, act, o2, r2 = heal_one(torch, rs, rate, N, M, S, orig, rec, pad, mode=mode, max_rows=M - 1,
                                           what=what)
        if intended is not None:
            assert loc == intended, f"{what}: the model says {loc}, the case was built for {intended}"
        # what the model left behind (which the device matched), against the clean stripe
        if intended is not None and intended >= 0 and mode & ORIGINAL:
            assert act == ORIGINAL and np.array_equal(o2, clean_orig) and np.array_equal(r2, rec), what
        elif name.startswith("recovery ") and mode & RECOVERY and loc == ROWS:
            assert act == RECOVERY and np.array_equal(r2, O.encode(rate, orig, M)) and np.array_equal(r2, clean_rec)
            assert np.array_equal(o2, orig), what
        elif loc in (UNKNOWN, CLEAN):
            assert act == 0 and np.array_equal(o2, orig) and np.array_equal(r2, rec), what
        if again and act:
            loc, flags, act, _, _ = heal_one(torch, rs, rate, N, M, S, o2, r2, pad, mode=mode, max_rows=M - 1,
                                             what=what + ", healed again")
            assert (loc, act) == (CLEAN, 0) and not flags.any(), f"{what}: a second heal gives {loc}, action {act}"


@pytest.mark.parametrize("S,pad", LAYOUTS, ids=lambda v: str(v))
@pytest.mark.parametrize("rate,N,M", COLUMN, ids=lambda v: str(v))
def test_column_shapes(torch, rs, rate, N, M, S, pad):
    run_cases(torch, rs, rate, N, M, S, pad)


@pytest.mark.parametrize("rate,N,M,S,pad", OTHER, ids=lambda v: str(v))
def test_other_shapes(torch, rs, rate, N, M, S, pad):
    big = N * M >= 1 << 20  # the large shapes once: one case of each outcome
    run_cases(torch, rs, rate, N, M, S, pad,
              only=("none", "original 0 lastbit", f"original {N - 1} shard", "recovery two", "two originals, two")
              if big else None)


def test_two_rows_take_the_recovery_bit_alone(torch, rs):
    """3:2 x 2: two recovery rows in all, so RS_HEAL_ORIGINAL is refused and RS_HEAL_RECOVERY runs."""
    rate, N, M, S = "default", 3, 2, 2
    with pytest.raises(ValueError, match="three"):
        rs.heal_device(N, M, S, *(V.view(torch, x, 0) for x in V.stripe(rate, N, M, S)), mode=3)
    run_cases(torch, rs, rate, N, M, S, 0, mode=RECOVERY)
    orig, rec = V.stripe(rate, N, M, S)
    bad = rec.copy()
    bad[1, 1] ^= 0x80
    _, _, act, _, r2 = heal_one(torch, rs, rate, N, M, S, orig, bad, mode=RECOVERY, max_rows=1, what="3:2 one row")
    assert act == RECOVERY and np.array_equal(r2, rec)


@pytest.mark.parametrize("rate,N,M,S,pad", [("high", 70, 100, 66, 4), ("default", 200, 200, 72, 0),
                                            ("high", 1000, 100, 66, 0)], ids=lambda v: str(v))
def test_mode_bits_and_threshold(torch, rs, rate, N, M, S, pad):
    orig, rec = V.stripe(rate, N, M, S)
    two = rec.copy()
    two[M // 3, 5] ^= 0x10
    two[M - 1, S - 1] ^= 0x80
    one = orig.copy()
    one[N - 1, S - 1] ^= 0x80
    run = lambda o, r, mode, max_rows, what: heal_one(torch, rs, rate, N, M, S, o, r, pad, mode=mode,
                                                       max_rows=max_rows, what=what)
    # RS_HEAL_ORIGINAL alone leaves a ROWS stripe untouched
    loc, _, act, _, r2 = run(orig, two, ORIGINAL, M - 1, "ROWS, original bit alone")
    assert (loc, act) == (ROWS, 0) and np.array_equal(r2, two)
    # RS_HEAL_RECOVERY alone leaves a located stripe untouched
    loc, _, act, o2, _ = run(one, rec, RECOVERY, M - 1, "located, recovery bit alone")
    assert (loc, act) == (N - 1, 0) and np.array_equal(o2, one)
    # two differing rows: untouched with max_rows = 1 and 0, rewritten with 2 and above
    for max_rows, healed in ((1, False), (0, False), (2, True), (M, True), (0xFFFFFFFF, True)):
        loc, flags, act, _, r2 = run(orig, two, 3, max_rows, f"two rows, max_rows {max_rows}")
        assert loc == ROWS and flags.sum() == 2
        assert (act, np.array_equal(r2, rec), np.array_equal(r2, two)) == \
            ((RECOVERY, True, False) if healed else (0, False, True)), max_rows
    # max_rows = 0 never rewrites, not even one row; it does not hold an original back
    bad = rec.copy()
    bad[0, 0] ^= 1
    assert run(orig, bad, 3, 0, "one row, max_rows 0")[2] == 0
    loc, _, act, o2, _ = run(one, rec, 3, 0, "located, max_rows 0")
    assert (loc, act) == (N - 1, ORIGINAL) and np.array_equal(o2, orig)


def masks_of(M):
    three = np.zeros(M, np.uint8)
    three[[1, M // 2, M - 2]] = 1  # exactly three rows, row 0 unselected
    third = (np.arange(M) % 3 != 1).astype(np.uint8)  # every third row unselected
    most = np.ones(M, np.uint8)
    most[M // 3] = 0  # all but one
    return [three, third, most]


@pytest.mark.parametrize("rate,N,M,S,pad", [("high", 70, 100, 64, 0), ("low", 100, 70, 66, 4),
                                            ("default", 200, 200, 72, 0), ("high", 1000, 100, 66, 0)],
                         ids=lambda v: str(v))
def test_masks(torch, rs, rate, N, M, S, pad):
    """Unselected rows hold junk: never flagged, never written (the whole-buffer compare), whatever
    the stripe's outcome; a corrupt unselected recovery row stays corrupt."""
    orig, rec = V.stripe(rate, N, M, S)
    rng = np.random.default_rng(M)
    for mask in masks_of(M):
        sel, unsel = np.flatnonzero(mask), np.flatnonzero(mask == 0)
        junk = rec.copy()
        junk[unsel] ^= rng.integers(1, 256, (len(unsel), S), dtype=np.uint8)
        what = f"{rate} {N}:{M} mask of {len(sel)}"
        run = lambda o, r, name, max_rows=M - 1: heal_one(torch, rs, rate, N, M, S, o, r, pad, mask=mask, mode=3,
                                                          max_rows=max_rows, what=f"{what} {name}")
        loc, flags, act, _, _ = run(orig, junk, "clean")
        assert (loc, act) == (CLEAN, 0) and not flags.any()
        for i in sorted({0, N - 1}):
            bad = orig.copy()
            L.damage_original(bad, i, "lastpack", rng)
            loc, flags, act, o2, r2 = run(bad, junk, f"original {i}")
            assert (loc, act) == (i, ORIGINAL) and np.array_equal(flags, mask)
            assert np.array_equal(o2, orig) and np.array_equal(r2, junk)
        # a selected row and an unselected one corrupt: the one is rewritten, the other stays
        bad = junk.copy()
        bad[sel[-1], S - 1] ^= 0x01
        bad[sel[0], 0] ^= 0x80
        loc, flags, act, o2, r2 = run(orig, bad, "rows")
        assert (loc, act) == (ROWS, RECOVERY) and np.flatnonzero(flags).tolist() == [sel[0], sel[-1]]
        assert np.array_equal(r2, junk) and not np.array_equal(r2[unsel], rec[unsel])
        assert run(orig, bad, "rows over the threshold", max_rows=1)[2] == 0
        # every selected row wrong in its own way: UNKNOWN, untouched
        worse = junk.copy()
        worse[sel] ^= 1
        loc, _, act, _, r2 = run(orig, worse, "every selected row")
        assert (loc, act) == (UNKNOWN, 0) and np.array_equal(r2, worse)


def batch_case(rate, N, M, S, B, max_rows, wide=False):
    """B stripes with a different outcome in each: [originals], [recovery], [intended status].
    wide: recovery rows are damaged in the last pack, the middle pack and pack 0
    (tests/wide_cases.py), not all in the first block."""
    rng = np.random.default_rng(B)
    kinds = ["orig0", "clean", "row", "origN", "over", "unknown", "rows", "origmid"][:B]
    origs, recs, wants = [], [], []
    for b, k in enumerate(kinds):
        o, r = (x.copy() for x in V.stripe(rate, N, M, S, seed=b))
        want = CLEAN
        if k.startswith("orig"):
            want = {"orig0": 0, "origN": N - 1, "origmid": N // 2}[k]
            L.damage_original(o, want, {"orig0": "lastbit", "origN": "shard", "origmid": "highhalf"}[k], rng)
        elif k in ("row", "rows", "over"):
            packs = W.packs_of(S)
            for n, j in enumerate([M - 1, 0, M // 2][:{"row": 1, "rows": max_rows, "over": max_rows + 1}[k]]):
                if wide:
                    W.damage_pack(r, j, [packs - 1, packs // 2, 0][n], rng)
                else:
                    r[j, (3 + 7 * n) % S] ^= 0x02 << n
            want = ROWS
        elif k == "unknown":
            o[0, 0] ^= 0x10
            o[N - 1, S - 1] ^= 0x20
            want = UNKNOWN
        origs.append(o), recs.append(r), wants.append(want)
    return np.stack(origs), np.stack(recs), wants


@pytest.mark.parametrize("rate,N,M,S,B,pad", [("high", 70, 100, 66, 8, 4), ("default", 1024, 1024, 72, 6, 0),
                                              ("high", 1000, 100, 66, 5, 0), ("low", 128, 1024, 64, 4, 0),
                                              ("default", 4096, 4096, 64, 4, 0)], ids=lambda v: str(v))
def test_batch(torch, rs, rate, N, M, S, B, pad, wide=False, groups=None):
    """A different outcome in every stripe, with stripe padding.  One launch of each kernel where
    the batch encode is one launch; stripe by stripe elsewhere, which is the case that catches a
    k_heal reading another stripe's scratch.  Byte-identical to the model, to a loop of single
    calls, and healed a second time: CLEAN, action 0, nothing written.  (wide, groups:
    tests/test_gpu_wide_shards.py's -- batch_case's wide form, and the number of groups the batch
    must run in where the shape alone does not say.)"""
    max_rows = 2
    origs, recs, intended = batch_case(rate, N, M, S, B, max_rows, wide)
    model = [HM.heal(rate, origs[b], recs[b], mode=3, max_rows=max_rows) for b in range(B)]
    assert [m[0] for m in model] == intended
    w_orig, w_rec = np.stack([m[3] for m in model]), np.stack([m[4] for m in model])
    w_act = [m[2] for m in model]
    assert w_act == [ORIGINAL if i >= 0 else RECOVERY if i == ROWS and int(m[1].sum()) <= max_rows else 0
                     for i, m in zip(intended, model)]
    d_orig, d_rec = Dev(torch, origs, pad, extra=2), Dev(torch, recs, pad, extra=3)
    out = Out(torch, B, M, True)
    call = lambda o: rs.heal_device_batch(N, M, S, d_orig.t, d_rec.t, mode=3, max_rows=max_rows, d_located=o.loc,
                                          d_mismatch=o.flags, d_action=o.act, rate_=RATE[rate])
    # (the table first, by a plain locate of copies: the launches below are then the call's own)
    d_o2, d_r2 = V.padded_batch(torch, origs, 2, pad), V.padded_batch(torch, recs, 3, pad)
    locate = lambda: rs.locate_device_batch(N, M, S, d_o2, d_r2, rate_=RATE[rate])
    locate()
    names = [r[0] for r in V.profiled(torch, rs, lambda: call(out))]
    loc, flags, act = out.read("batch")
    assert loc.tolist() == intended and act.tolist() == w_act, (loc, act)
    assert np.array_equal(flags, np.stack([m[1] for m in model]))
    d_orig.check(w_orig, "batch: d_original")
    d_rec.check(w_rec, "batch: d_recovery")
    # the launches: the locate's list plus exactly one k_heal per group, after its confirm
    want_groups, groups = groups, names.count("k_locate_confirm")
    assert groups == ({70: 1, 1024: 1}.get(N, B) if want_groups is None else want_groups), names
    assert names.count("k_heal") == groups == names.count("k_locate_find") == names.count("k_verify_rows"), names
    assert all(names[k + 1] == "k_heal" for k, n in enumerate(names) if n == "k_locate_confirm"), names
    plain = [r[0] for r in V.profiled(torch, rs, locate)]
    assert not any(n.startswith("k_coef_") for n in names + plain), (names, plain)  # the heal's table is the locate's
    assert [n for n in names if n != "k_heal"] == plain, (names, plain)
    # a loop of single calls (each checked against the model in full by heal_one)
    for b in range(B):
        heal_one(torch, rs, rate, N, M, S, origs[b], recs[b], pad, mode=3, max_rows=max_rows,
                 what=f"stripe {b} alone", model=model[b])
    # idempotence: healed stripes are CLEAN with action 0, the others as before, nothing written
    again = Out(torch, B, M, True)
    call(again)
    torch.cuda.synchronize()
    loc2, flags2, act2 = again.read("second heal")
    for b in range(B):
        if w_act[b]:
            assert loc2[b] == CLEAN and act2[b] == 0 and not flags2[b].any(), b
        else:
            assert loc2[b] == loc[b] and act2[b] == 0 and np.array_equal(flags2[b], flags[b]), b
    d_orig.check(w_orig, "second heal: d_original")
    d_rec.check(w_rec, "second heal: d_recovery")


def test_with_the_rest_of_the_library(torch, rs):
    """After a heal: both verify routes show no flag for the healed stripes, a locate on the
    stream finds its table, the update's table is undisturbed, and a decode from a healed stripe
    with an original dropped restores the clean original."""
    rate, N, M, S, B = "high", 70, 100, 66, 4
    pairs = [V.stripe(rate, N, M, S, seed=b) for b in range(B)]
    origs, recs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    bad_o, bad_r = origs.copy(), recs.copy()
    bad_o[0, 33] = np.random.default_rng(5).integers(0, 256, S, dtype=np.uint8)
    bad_r[1, 17, 40] ^= 0x08
    bad_r[1, 93, 3] ^= 0x80
    bad_o[3, N - 1, S - 1] ^= 0x80
    d_orig, d_rec = V.view(torch, bad_o, 0), V.view(torch, bad_r, 0)
    # the update's table, built before the heal
    d_new = torch.zeros((1, S), dtype=torch.uint8, device="cuda")
    d_upd = V.view(torch, recs[2], 0)
    upd = lambda: rs.update_device(N, M, S, [5], None, d_new, d_upd, rate_=RATE[rate])
    rs.release_stream_scratch()
    assert L.coef_launches(V.profiled(torch, rs, upd)) == ["k_coef_unit", "k_coef_log"]
    heal = lambda: rs.heal_device_batch(N, M, S, d_orig, d_rec, mode=3, max_rows=2, rate_=RATE[rate])
    first = V.profiled(torch, rs, heal)
    assert L.coef_launches(first) == ["k_coef_unit_slab", "k_coef_log_slab"]
    assert [r[0] for r in first][-4:] == ["k_verify_rows", "k_locate_find", "k_locate_confirm", "k_heal"]
    assert np.array_equal(d_orig.cpu().numpy(), origs) and np.array_equal(d_rec.cpu().numpy(), recs)
    for fused in (1, 0):
        rs.verify_set_fused(fused)
        assert not rs.verify_device_batch(N, M, S, d_orig, d_rec, rate_=RATE[rate]).cpu().numpy().any(), fused
    rs.verify_set_fused(rs.VERIFY_FUSED_DEFAULT)
    after = V.profiled(torch, rs, lambda: rs.locate_device_batch(N, M, S, d_orig, d_rec, rate_=RATE[rate]))
    assert L.coef_launches(after) == [] and [r[0] for r in after][-1] == "k_locate_confirm"
    assert L.coef_launches(V.profiled(torch, rs, heal)) == []  # ... and the reverse
    assert L.coef_launches(V.profiled(torch, rs, upd)) == []  # the update's own table is still there
    torch.cuda.synchronize()
    assert np.array_equal(d_upd.cpu().numpy(), recs[2])  # (a zero delta)
    # decode stripe 0 with the healed original dropped
    d_out = torch.zeros((N, S), dtype=torch.uint8, device="cuda")
    op = [1] * N
    op[33] = 0
    rp = [1] + [0] * (M - 1)
    rs.decode_device(N, M, S, d_orig[0].contiguous(), op, d_rec[0].contiguous(), rp, d_out, rate_=RATE[rate])
    torch.cuda.synchronize()
    assert np.array_equal(d_out[33].cpu().numpy(), origs[0, 33])


def test_heals_in_flight(torch, rs):
    """Two heals back to back on one stream with an encode between them, then two on two streams
    on separate buffers; one synchronize, then everything is checked."""
    rate, N, M, S = "default", 200, 200, 72
    orig, rec = V.stripe(rate, N, M, S)
    a, b = orig.copy(), rec.copy()
    a[7, 0] ^= 1
    b[M - 2, S - 1] ^= 0x80
    b[3, 9] ^= 0x04

    def launch(stream_a=None, stream_b=None):
        da, dra = Dev(torch, a, 0), Dev(torch, rec, 0)
        db, drb = Dev(torch, orig, 0), Dev(torch, b, 0)
        oa, ob = Out(torch, 1, M, False), Out(torch, 1, M, False)
        d_enc = torch.zeros((M, S), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rs.heal_device(N, M, S, da.t, dra.t, mode=3, max_rows=2, d_located=oa.loc, d_mismatch=oa.flags,
                       d_action=oa.act, stream=stream_a)
        rs.encode_device(N, M, S, da.t, d_enc, stream=stream_a)  # of the healed originals: the stream orders it
        rs.heal_device(N, M, S, db.t, drb.t, mode=3, max_rows=2, d_located=ob.loc, d_mismatch=ob.flags,
                       d_action=ob.act, stream=stream_b)
        return da, dra, db, drb, oa, ob, d_enc

    for streams in ((None, None), (torch.cuda.Stream(), torch.cuda.Stream())):
        da, dra, db, drb, oa, ob, d_enc = launch(*streams)
        torch.cuda.synchronize()
        la, fa, aa = oa.read("first heal")
        lb, fb, ab = ob.read("second heal")
        assert (int(la[0]), int(aa[0])) == (7, ORIGINAL) and fa.all()
        assert (int(lb[0]), int(ab[0])) == (ROWS, RECOVERY) and np.flatnonzero(fb[0]).tolist() == [3, M - 2]
        da.check(orig, "first heal: d_original"), dra.check(rec, "first heal: d_recovery")
        db.check(orig, "second heal: d_original"), drb.check(rec, "second heal: d_recovery")
        assert np.array_equal(d_enc.cpu().numpy(), rec)
        for s in streams:
            if s is not None:
                rs.release_stream_scratch(s)


def test_wrappers_reject_before_any_call(torch, rs):
    N, M, S = 8, 6, 64
    o = torch.zeros((N, S), dtype=torch.uint8, device="cuda")
    r = torch.zeros((M, S), dtype=torch.uint8, device="cuda")
    dev = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype, device="cuda")
    with pytest.raises(ValueError, match="d_original: dtype"):
        rs.heal_device(N, M, S, o.to(torch.int32), r)
    with pytest.raises(ValueError, match="d_recovery:"):
        rs.heal_device(N, M, S, o, dev(M - 1, S))
    with pytest.raises(ValueError, match="d_action"):
        rs.heal_device(N, M, S, o, r, d_action=torch.zeros(1, dtype=torch.uint8))  # on the host
    with pytest.raises(ValueError, match="d_action"):
        rs.heal_device(N, M, S, o, r, d_action=dev(2))
    with pytest.raises(ValueError, match="d_action"):
        rs.heal_device(N, M, S, o, r, d_action=dev(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="d_located"):
        rs.heal_device(N, M, S, o, r, d_located=dev(1))
    with pytest.raises(ValueError, match="d_mismatch"):
        rs.heal_device(N, M, S, o, r, d_mismatch=dev(M + 1))
    with pytest.raises(ValueError, match="mode:"):
        rs.heal_device(N, M, S, o, r, mode=0)
    with pytest.raises(ValueError, match="stripe count"):
        rs.heal_device_batch(N, M, S, dev(2, N, S), dev(3, M, S))
    with pytest.raises(ValueError, match="d_action"):
        rs.heal_device_batch(N, M, S, dev(2, N, S), dev(2, M, S), d_action=dev(3))
    # tensors the call allocates itself
    loc, flags, act = rs.heal_device_batch(N, M, S, dev(2, N, S), dev(2, M, S), mode=3, max_rows=1)
    assert loc.shape == (2,) and flags.shape == (2, M) and act.shape == (2,) and str(act.dtype) == "torch.uint8"
    assert act.is_cuda and loc.cpu().tolist() == [CLEAN, CLEAN] and act.cpu().tolist() == [0, 0]
