"""GPU: rs_heal_device_robust* -- the robust locate that also writes the correction, in place.

Expected values are constructed, not computed by the code under test: the stripes are those of
tests/locate_robust_cases.py (the oracle's clean stripe with chosen bytes flipped), and what the call
must report and leave behind is tests/heal_robust_model.py, the numpy statement of the contract.
Where a case is built as "original i with outlier rows B" the healed matrices must also equal the
CLEAN stripe byte for byte.  Every run compares `located`, the flags, the WHOLE d_outlier, the action
and the WHOLE device buffer of both matrices with the expected ones -- the guards before and after,
the junk in the row padding, the stripe padding and every row that must not change -- and checks that
the four outputs, pre-filled with 0xFF between guards, come back fully defined.
"""
import numpy as np
import pytest

import heal_model as HM
import heal_robust_model as HRM
import locate_model as LM
import locate_robust_cases as RC
import locate_robust_model as RM
import oracle_lib as O
import test_gpu_heal as H
import test_gpu_locate as L
import test_gpu_verify as V

pytestmark = pytest.mark.gpu

RATE = V.RATE
Dev = H.Dev
CLEAN, ROWS, UNKNOWN = LM.CLEAN, LM.ROWS, LM.UNKNOWN
ORIGINAL, RECOVERY = HM.ORIGINAL, HM.RECOVERY
# (rate, N, M): the staged single-chunk column kernel
COLUMN = [("high", 70, 100), ("low", 100, 70)]
# (S, row padding): whole blocks; a tail; a tail with rows that are not 4-byte aligned (byte-wise)
LAYOUTS = L.LAYOUTS
# (rate, N, M, S, row padding, forms, ts): the lane kernel, 1024:1024, the pass kernels, the multi-chunk
# encodes, and stripes of four (one outlier) and six (two) recovery rows; the large shapes with one
# error form and the t the issue names
OTHER = [("default", 200, 200, 72, 0, None, None), ("default", 1024, 1024, 72, 0, ("lastbit",), (1, 7)),
         ("default", 4096, 4096, 64, 0, ("bit0",), (1, 7)), ("high", 1000, 100, 66, 0, ("lastbit",), (1, 2)),
         ("low", 128, 1024, 64, 0, ("bit0",), (1, 7)), ("default", 1, 4, 64, 0, None, None),
         ("default", 3, 4, 2, 0, None, None), ("default", 2, 6, 190, 0, None, None)]


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


class Out:
    """The four outputs, pre-filled with 0xFF between guards."""

    def __init__(self, torch, B, M, batch):
        self.B, self.M = B, M
        self.loc, self.loc_buf = L.guarded(torch, (B,), torch.int32)
        self.flags, self.flag_buf = L.guarded(torch, (B, M) if batch else (M,), torch.uint8)
        self.outlier, self.outlier_buf = L.guarded(torch, (B, M) if batch else (M,), torch.uint8)
        self.act, self.act_buf = L.guarded(torch, (B,), torch.uint8)

    def kw(self):
        return dict(d_located=self.loc, d_mismatch=self.flags, d_outlier=self.outlier, d_action=self.act)

    def read(self, what):
        """Guards intact, every word and byte defined; (located [B], flags [B, M], outlier [B, M],
        action [B])."""
        loc, flags = L.check_outputs(self.loc_buf, self.flag_buf, what)
        g = L.GUARD
        o, a = self.outlier_buf.cpu().numpy(), self.act_buf.cpu().numpy()
        assert (o[:g] == 0xFF).all() and (o[-g:] == 0xFF).all(), what + ": a byte outside d_outlier was written"
        assert (o[g:-g] <= 1).all(), what + ": an outlier byte is neither 0 nor 1"
        assert (a[:g] == 0xFF).all() and (a[-g:] == 0xFF).all(), what + ": a byte outside d_action was written"
        assert (a[g:-g] <= 3).all(), what + f": an action is not defined: {a[g:-g]}"
        return loc, flags.reshape(self.B, self.M), o[g:-g].reshape(self.B, self.M), a[g:-g]


def compare(got, want, what):
    """(located, flags, outlier, action) of one stripe against the model's."""
    loc, flags, outlier, act = got
    w_loc, w_flags, w_out, w_act = want
    assert int(loc) == w_loc, f"{what}: located {loc}, want {w_loc}"
    assert np.array_equal(flags, w_flags), \
        f"{what}: flagged rows {np.flatnonzero(flags).tolist()[:8]}, want {np.flatnonzero(w_flags).tolist()[:8]}"
    assert np.array_equal(outlier, w_out), \
        f"{what}: outliers {np.flatnonzero(outlier).tolist()}, want {np.flatnonzero(w_out).tolist()}"
    assert int(act) == w_act, f"{what}: action {act}, want {w_act}"


def heal_one(torch, rs, rate, N, M, S, orig, rec, t, pad=0, mask=None, mode=3, max_rows=0, what="", stream=None,
             model=None, want=None):
    """One robust heal of one stripe on fresh device copies, checked against the model in full
    (`model`: HRM.heal of the same arguments, where the caller has it; `want`: the oracle's encode
    of `orig`); the model's (located, flags, outlier, action, originals after, recovery after)."""
    d_orig, d_rec = Dev(torch, orig, pad), Dev(torch, rec, pad)
    out = Out(torch, 1, M, False)
    rs.heal_device_robust(N, M, S, d_orig.t, d_rec.t, recovery_rows=mask, max_outliers=t, mode=mode, max_rows=max_rows,
                          rate_=RATE[rate], stream=stream, **out.kw())
    torch.cuda.synchronize()
    loc, flags, outlier, act = out.read(what)
    model = model or HRM.heal(rate, orig, rec, t, mask=mask, mode=mode, max_rows=max_rows, want=want)
    compare((loc[0], flags[0], outlier[0], act[0]), model[:4], what)
    d_orig.check(model[4], what + ": d_original")
    d_rec.check(model[5], what + ": d_recovery")
    return model


def run_cases(torch, rs, rate, N, M, S, pad=0, mask=None, **kw):
    """Every constructed case, both bits, max_rows = M - 1; the outcomes seen."""
    clean_orig, clean_rec = V.stripe(rate, N, M, S)
    sel = np.arange(M) if mask is None else np.flatnonzero(mask)
    seen = set()
    for case in RC.cases(rate, N, M, S, mask=mask, **kw):
        name, t, orig, rec, enc, intended = case
        what = f"{rate} {N}:{M} x {S} pad {pad} {name}"
        located, flags, outlier = RC.model(rate, case, mask=mask)  # (the intended status asserted)
        m = heal_one(torch, rs, rate, N, M, S, orig, rec, t, pad, mask, 3, M - 1, what, want=enc)
        assert (m[0], m[1].tolist(), m[2].tolist()) == (located, flags.tolist(), outlier.tolist()), what
        # what the model left behind (which the device matched), against the clean stripe
        if intended is not None and intended[0] >= 0:
            assert m[3] == ORIGINAL | (RECOVERY if intended[1] else 0), what
            assert np.array_equal(m[4], clean_orig) and np.array_equal(m[5][sel], clean_rec[sel]), what
            assert np.array_equal(np.delete(m[5], sel, 0), np.delete(rec, sel, 0)), what
        elif located == ROWS:
            assert m[3] == RECOVERY and np.array_equal(m[4], orig) and np.array_equal(m[5][sel], enc[sel]), what
        elif located in (UNKNOWN, CLEAN):
            assert m[3] == 0 and np.array_equal(m[4], orig) and np.array_equal(m[5], rec), what
        seen.add(("i", bool(outlier.any())) if located >= 0 else located)
    return seen


@pytest.mark.parametrize("S,pad", LAYOUTS, ids=lambda v: str(v))
@pytest.mark.parametrize("rate,N,M", COLUMN, ids=lambda v: str(v))
def test_column_shapes(torch, rs, rate, N, M, S, pad):
    assert run_cases(torch, rs, rate, N, M, S, pad) == {("i", True), ("i", False), CLEAN, ROWS, UNKNOWN}


@pytest.mark.parametrize("rate,N,M,S,pad,forms,ts", OTHER, ids=lambda v: str(v))
def test_other_shapes(torch, rs, rate, N, M, S, pad, forms, ts):
    kw = {} if forms is None else {"forms": forms, "ts": ts}
    assert run_cases(torch, rs, rate, N, M, S, pad, **kw) >= {("i", True), ("i", False), CLEAN, ROWS}


@pytest.mark.parametrize("rate,N,M,S,pad", [("high", 70, 100, 66, 4), ("default", 200, 200, 72, 0),
                                            ("high", 1000, 100, 66, 0)], ids=lambda v: str(v))
def test_mode_bits_and_threshold(torch, rs, rate, N, M, S, pad):
    orig, rec = V.stripe(rate, N, M, S)
    one, hit = orig.copy(), rec.copy()
    one[N - 1, S - 1] ^= 0x80
    hit[0, 5] ^= 0x10  # sel[0], the plain heal's reference row
    hit[M - 1, S - 1] ^= 0x20
    enc = O.encode(rate, one, M)
    run = lambda o, r, t, mode, max_rows, what, **kw: heal_one(torch, rs, rate, N, M, S, o, r, t, pad, mode=mode,
                                                               max_rows=max_rows, what=what, **kw)
    # each bit alone on a located stripe with two outliers: the other half stays as found
    loc, _, outlier, act, o2, r2 = run(one, hit, 2, ORIGINAL, 0, "located, original bit alone", want=enc)
    assert (loc, np.flatnonzero(outlier).tolist(), act) == (N - 1, [0, M - 1], ORIGINAL)
    assert np.array_equal(o2, orig) and np.array_equal(r2, hit)
    loc, _, outlier, act, o2, r2 = run(one, hit, 2, RECOVERY, 0, "located, recovery bit alone", want=enc)
    assert (loc, np.flatnonzero(outlier).tolist(), act) == (N - 1, [0, M - 1], RECOVERY)
    assert np.array_equal(o2, one) and np.array_equal(r2, rec)
    # ... the recovery bit alone with no outlier: action 0; both bits, max_rows 0: both written
    assert run(one, rec, 2, RECOVERY, M, "located alone, recovery bit alone", want=enc)[3] == 0
    loc, _, _, act, o2, r2 = run(one, hit, 2, 3, 0, "located, both bits, max_rows 0", want=enc)
    assert act == 3 and np.array_equal(o2, orig) and np.array_equal(r2, rec)
    # RS_HEAL_ORIGINAL alone leaves a ROWS stripe untouched
    loc, _, _, act, _, r2 = run(orig, hit, 1, ORIGINAL, M - 1, "ROWS, original bit alone", want=rec)
    assert (loc, act) == (ROWS, 0) and np.array_equal(r2, hit)
    # two differing rows: untouched with max_rows = 1 and 0, rewritten with 2 and above
    for max_rows, healed in ((1, False), (0, False), (2, True), (0xFFFFFFFF, True)):
        loc, flags, outlier, act, _, r2 = run(orig, hit, 1, 3, max_rows, f"two rows, max_rows {max_rows}", want=rec)
        assert loc == ROWS and flags.sum() == 2 and not outlier.any()
        assert (act, np.array_equal(r2, rec), np.array_equal(r2, hit)) == \
            ((RECOVERY, True, False) if healed else (0, False, True)), max_rows


@pytest.mark.parametrize("rate,N,M,S,B,pad", [("default", 1024, 1024, 72, 6, 0), ("high", 1000, 100, 66, 5, 0)],
                         ids=lambda v: str(v))
def test_max_outliers_zero_is_the_heal(torch, rs, rate, N, M, S, B, pad):
    """Compatibility: with max_outliers = 0 the outputs and both matrices are heal_device_batch's on
    the same batch -- the heal's own batch, and the robust one with its outliers -- and d_outlier
    is all zero."""
    seen = set()
    for origs, recs in (H.batch_case(rate, N, M, S, B, 2)[:2], batch_case(rate, N, M, S, B, 2, 2)[:2]):
        d_o1, d_r1 = Dev(torch, origs, pad, extra=2), Dev(torch, recs, pad, extra=3)
        d_o2, d_r2 = Dev(torch, origs, pad, extra=2), Dev(torch, recs, pad, extra=3)
        want = rs.heal_device_batch(N, M, S, d_o1.t, d_r1.t, mode=3, max_rows=2, rate_=RATE[rate])
        out = Out(torch, B, M, True)
        rs.heal_device_robust_batch(N, M, S, d_o2.t, d_r2.t, max_outliers=0, mode=3, max_rows=2, rate_=RATE[rate],
                                    **out.kw())
        torch.cuda.synchronize()
        loc, flags, outlier, act = out.read("t = 0")
        assert loc.tolist() == want[0].cpu().numpy().tolist() and act.tolist() == want[2].cpu().numpy().tolist()
        assert np.array_equal(flags, want[1].cpu().numpy()) and not outlier.any()
        assert np.array_equal(d_o2.buf.cpu().numpy(), d_o1.buf.cpu().numpy())
        assert np.array_equal(d_r2.buf.cpu().numpy(), d_r1.buf.cpu().numpy())
        seen |= {(min(int(x), 0), int(a)) for x, a in zip(loc, act)}
    # every outcome was compared: healed originals, rows under and over the threshold, UNKNOWN, CLEAN
    assert seen == {(0, ORIGINAL), (CLEAN, 0), (ROWS, RECOVERY), (ROWS, 0), (UNKNOWN, 0)}


@pytest.mark.parametrize("rate,N,M,S,pad", [("high", 70, 100, 64, 0), ("default", 300, 500, 72, 8)], ids=lambda v: str(v))
def test_masks(torch, rs, rate, N, M, S, pad):
    """Exactly 2 (t + 1) selected rows; every third row unselected; junk (0xC3) in the unselected
    rows and the row padding; a corrupt unselected row stays corrupt and is never flagged, named
    or written (the whole-buffer compare)."""
    for t in (1, 2):
        mask = np.zeros(M, np.uint8)
        mask[[1, M // 3, M // 2, M - 2] + ([3, M - 5] if t == 2 else [])] = 1
        assert int(mask.sum()) == 2 * (t + 1)
        seen = run_cases(torch, rs, rate, N, M, S, pad, mask=mask, forms=("bit0",), ts=(t,), junk=True)
        assert seen >= {("i", True), ("i", False), CLEAN, ROWS}
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
    healed = r.copy()
    healed[sel[5]] = rec[sel[5]]
    enc = O.encode(rate, bad, M)
    for t, want, outliers in ((1, N // 3, [sel[5]]), (2, N // 3, [sel[5]]), (0, UNKNOWN, [])):
        loc, flags, outlier, act, o2, r2 = heal_one(torch, rs, rate, N, M, S, bad, r, t, pad, mask, 3, M,
                                                    f"unselected damage t={t}", want=enc)
        assert (loc, np.flatnonzero(outlier).tolist()) == (want, outliers) and np.array_equal(flags, mask)
        assert act == (3 if want >= 0 else 0)
        assert np.array_equal(o2, orig if want >= 0 else bad) and np.array_equal(r2, healed if want >= 0 else r)
        assert not np.array_equal(r2[unsel], rec[unsel])


def batch_case(rate, N, M, S, B, t, max_rows):
    """B stripes (5..8) with a different outcome in each: located with outliers (at sel[0] too),
    located alone, ROWS under and over max_rows, UNKNOWN (t + 1 outliers, two originals), CLEAN.
    [originals], [recovery], [HRM.heal of each stripe at mode 3]."""
    rng = np.random.default_rng(B)
    kinds = [("orig", 0, "lastbit", [0]), ("none",), ("rows", max_rows), ("orig", N - 1, "bit0", [1, 3][:t]),
             ("rows", max_rows + 1), ("orig", N // 2, "bit0", list(range(t + 1))), ("orig", N // 3, "lastbit", []),
             ("two",)][:B]
    origs, recs, models = [], [], []
    for b, k in enumerate(kinds):
        o, r = (x.copy() for x in V.stripe(rate, N, M, S, seed=b))
        want = (CLEAN, [], 0)
        if k[0] == "orig":
            L.damage_original(o, k[1], k[2], rng)
            for j in k[3]:
                RC.hit(r, j, "plain", k[2])
            want = (k[1], k[3], ORIGINAL | (RECOVERY if k[3] else 0)) if len(k[3]) <= t else (UNKNOWN, [], 0)
        elif k[0] == "rows":
            for n, j in enumerate([M - 1, 0, M // 2][:k[1]]):
                r[j, (3 + 7 * n) % S] ^= 0x02 << n
            want = (ROWS, [], RECOVERY if k[1] <= max_rows else 0)
        elif k[0] == "two":
            o[0, 0] ^= 0x10
            o[N - 1, S - 1] ^= 0x20
            want = (UNKNOWN, [], 0)
        model = HRM.heal(rate, o, r, t, mode=3, max_rows=max_rows)
        assert (model[0], np.flatnonzero(model[2]).tolist(), model[3]) == want, (b, k, model[0], model[3])
        if model[3]:  # whatever was healed is the clean stripe again
            assert all(np.array_equal(x, y) for x, y in zip(model[4:], V.stripe(rate, N, M, S, seed=b))), (b, k)
        origs.append(o), recs.append(r), models.append(model)
    return np.stack(origs), np.stack(recs), models


@pytest.mark.parametrize("rate,N,M,S,B,pad", [("high", 70, 100, 66, 8, 4), ("default", 1024, 1024, 72, 6, 0),
                                              ("high", 1000, 100, 66, 5, 0), ("low", 128, 1024, 64, 5, 0),
                                              ("default", 4096, 4096, 64, 5, 0)], ids=lambda v: str(v))
def test_batch(torch, rs, rate, N, M, S, B, pad):
    """A different outcome in every stripe, with stripe padding.  One launch of each kernel where
    the batch encode is one launch; stripe by stripe elsewhere, which is the case that catches a
    k_heal_robust reading another stripe's scratch.  Byte-identical to the model, to a loop of
    single calls, and healed a second time: CLEAN, action 0, nothing written."""
    t, max_rows = 2, 2
    origs, recs, model = batch_case(rate, N, M, S, B, t, max_rows)
    w_orig, w_rec = np.stack([m[4] for m in model]), np.stack([m[5] for m in model])
    d_orig, d_rec = Dev(torch, origs, pad, extra=2), Dev(torch, recs, pad, extra=3)
    out = Out(torch, B, M, True)
    call = lambda o: rs.heal_device_robust_batch(N, M, S, d_orig.t, d_rec.t, max_outliers=t, mode=3, max_rows=max_rows,
                                                 rate_=RATE[rate], **o.kw())
    # (the table first, by a robust locate of copies: the launches below are then the call's own)
    d_o2, d_r2 = V.padded_batch(torch, origs, 2, pad), V.padded_batch(torch, recs, 3, pad)
    locate = lambda: rs.locate_device_robust_batch(N, M, S, d_o2, d_r2, max_outliers=t, rate_=RATE[rate])
    locate()
    names = [r[0] for r in V.profiled(torch, rs, lambda: call(out))]
    loc, flags, outlier, act = out.read("batch")
    for b in range(B):
        compare((loc[b], flags[b], outlier[b], act[b]), model[b][:4], f"batch stripe {b}")
    d_orig.check(w_orig, "batch: d_original")
    d_rec.check(w_rec, "batch: d_recovery")
    # the launches: the robust locate's list plus exactly one k_heal_robust per group, after its decide
    groups = names.count("k_locate_decide")
    assert groups == {70: 1, 1024: 1}.get(N, B), names
    assert names.count("k_heal_robust") == groups == names.count("k_locate_find_pairs") == names.count("k_verify_rows")
    assert all(names[k + 1] == "k_heal_robust" for k, n in enumerate(names) if n == "k_locate_decide"), names
    plain = [r[0] for r in V.profiled(torch, rs, locate)]
    assert not any(n.startswith("k_coef_") for n in names + plain), (names, plain)  # the table is the robust locate's
    assert [n for n in names if n != "k_heal_robust"] == plain, (names, plain)
    assert "k_heal" not in names and "k_locate_confirm" not in names
    # a loop of single calls (each checked against the model in full by heal_one)
    for b in range(B):
        heal_one(torch, rs, rate, N, M, S, origs[b], recs[b], t, pad, mode=3, max_rows=max_rows,
                 what=f"stripe {b} alone", model=model[b])
    # idempotence: healed stripes are CLEAN with action 0, the others as before, nothing written
    again = Out(torch, B, M, True)
    call(again)
    torch.cuda.synchronize()
    loc2, flags2, outlier2, act2 = again.read("second heal")
    assert not outlier2.any() and not act2.any()
    for b in range(B):
        if model[b][3]:
            assert loc2[b] == CLEAN and not flags2[b].any(), b
        else:
            assert loc2[b] == loc[b] and np.array_equal(flags2[b], flags[b]), b
    d_orig.check(w_orig, "second heal: d_original")
    d_rec.check(w_rec, "second heal: d_recovery")
    # one mask for every stripe, and tensors the call allocates itself
    mask = np.ones(M, np.uint8)
    mask[M // 2] = 0
    d_o3, d_r3 = Dev(torch, origs, pad, extra=2), Dev(torch, recs, pad, extra=3)
    got = rs.heal_device_robust_batch(N, M, S, d_o3.t, d_r3.t, recovery_rows=mask, max_outliers=1, mode=3, max_rows=1,
                                      rate_=RATE[rate])
    assert got[0].shape == (B,) and str(got[0].dtype) == "torch.int32" and got[1].shape == got[2].shape == (B, M)
    assert got[3].shape == (B,) and str(got[3].dtype) == "torch.uint8" and got[3].is_cuda
    masked = [HRM.heal(rate, origs[b], recs[b], 1, mask=mask, mode=3, max_rows=1) for b in range(B)]
    for b in range(B):
        compare([x.cpu().numpy()[b] for x in got], masked[b][:4], f"masked batch stripe {b}")
    d_o3.check(np.stack([m[4] for m in masked]), "masked batch: d_original")
    d_r3.check(np.stack([m[5] for m in masked]), "masked batch: d_recovery")


def test_with_the_rest_of_the_library(torch, rs):
    """After a robust heal: a second call reports CLEAN and writes nothing, both verify routes show
    no flag, the table is shared both ways with the locate, the heal and the robust locate, the
    update's table is undisturbed, and a decode from a healed stripe restores the clean original."""
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
    d_orig, d_rec = Dev(torch, bad_o, 0), Dev(torch, bad_r, 0)
    # the update's table, built before the heal
    d_new = torch.zeros((1, S), dtype=torch.uint8, device="cuda")
    d_upd = V.view(torch, recs[2], 0)
    upd = lambda: rs.update_device(N, M, S, [5], None, d_new, d_upd, rate_=RATE[rate])
    rs.release_stream_scratch()
    assert L.coef_launches(V.profiled(torch, rs, upd)) == ["k_coef_unit", "k_coef_log"]
    heal = lambda: rs.heal_device_robust_batch(N, M, S, d_orig.t, d_rec.t, max_outliers=2, mode=3, max_rows=2,
                                               rate_=RATE[rate])
    result = []
    first = V.profiled(torch, rs, lambda: result.extend(heal()))
    assert L.coef_launches(first) == ["k_coef_unit_slab", "k_coef_log_slab"]
    assert [r[0] for r in first][-5:] == ["k_verify_rows", "k_locate_find_pairs", "k_locate_count", "k_locate_decide",
                                          "k_heal_robust"]
    located, flags, outlier, action = (x.cpu().numpy() for x in result)
    assert located.tolist() == [33, ROWS, CLEAN, N - 1, 0] and action.tolist() == [3, RECOVERY, 0, 3, ORIGINAL]
    assert [np.flatnonzero(o).tolist() for o in outlier] == [[0], [], [], [2, 99], []]
    d_orig.check(origs, "healed: d_original")
    d_rec.check(recs, "healed: d_recovery")
    # a second call: CLEAN, action 0, an all-zero d_outlier, nothing written
    out = Out(torch, B, M, True)
    rs.heal_device_robust_batch(N, M, S, d_orig.t, d_rec.t, max_outliers=2, mode=3, max_rows=2, rate_=RATE[rate],
                                **out.kw())
    torch.cuda.synchronize()
    loc2, flags2, outlier2, act2 = out.read("second heal")
    assert (loc2 == CLEAN).all() and not flags2.any() and not outlier2.any() and not act2.any()
    d_orig.check(origs, "second heal: d_original")
    d_rec.check(recs, "second heal: d_recovery")
    for fused in (1, 0):
        rs.verify_set_fused(fused)
        assert not rs.verify_device_batch(N, M, S, d_orig.t, d_rec.t, rate_=RATE[rate]).cpu().numpy().any(), fused
    rs.verify_set_fused(rs.VERIFY_FUSED_DEFAULT)
    # the table: found by the three other calls after the robust heal built it, and the reverse
    coef = lambda fn: L.coef_launches(V.profiled(torch, rs, fn))
    plain = lambda: rs.locate_device_batch(N, M, S, d_orig.t, d_rec.t, rate_=RATE[rate])
    robust = lambda: rs.locate_device_robust_batch(N, M, S, d_orig.t, d_rec.t, max_outliers=1, rate_=RATE[rate])
    plain_heal = lambda: rs.heal_device_batch(N, M, S, d_orig.t, d_rec.t, mode=3, max_rows=2, rate_=RATE[rate])
    assert coef(plain) == [] and coef(robust) == [] and coef(plain_heal) == [] and coef(heal) == []
    for builder in (plain, robust, plain_heal):
        rs.release_stream_scratch()
        assert len(coef(builder)) == 2 and coef(heal) == [], builder
        assert coef(upd) == ["k_coef_unit", "k_coef_log"] and coef(upd) == []  # (released with the stream's scratch)
    assert coef(heal) == []  # ... and the update's own table in between does not disturb ours
    torch.cuda.synchronize()
    assert np.array_equal(d_upd.cpu().numpy(), recs[2])  # (a zero delta)
    d_orig.check(origs, "after the other calls: d_original")
    d_rec.check(recs, "after the other calls: d_recovery")
    # decode stripe 0 with the healed original dropped, from the healed outlier row alone
    d_out = torch.zeros((N, S), dtype=torch.uint8, device="cuda")
    op = [1] * N
    op[33] = 0
    rp = [1] + [0] * (M - 1)
    rs.decode_device(N, M, S, d_orig.t[0].contiguous(), op, d_rec.t[0].contiguous(), rp, d_out, rate_=RATE[rate])
    torch.cuda.synchronize()
    assert np.array_equal(d_out[33].cpu().numpy(), origs[0, 33])
    rs.release_stream_scratch()


def test_heals_in_flight(torch, rs):
    """Two robust heals back to back on one stream with an encode between them, then two on two
    streams on separate buffers; one synchronize, then everything is checked."""
    rate, N, M, S = "default", 200, 200, 72
    orig, rec = V.stripe(rate, N, M, S)
    a, ra, b, rb = orig.copy(), rec.copy(), orig.copy(), rec.copy()
    a[7, 0] ^= 1
    ra[0, 5] ^= 0x10
    b[N - 2, S - 1] ^= 0x80
    rb[[3, 199], 9] ^= 0x20
    mask = np.ones(M, np.uint8)
    mask[1] = 0  # (a mask on the second call only: the selection travels between the two)

    def launch(stream_a=None, stream_b=None):
        da, dra, db, drb = Dev(torch, a, 0), Dev(torch, ra, 0), Dev(torch, b, 0), Dev(torch, rb, 0)
        oa, ob = Out(torch, 1, M, False), Out(torch, 1, M, False)
        d_enc = torch.zeros((M, S), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rs.heal_device_robust(N, M, S, da.t, dra.t, max_outliers=1, mode=3, stream=stream_a, **oa.kw())
        rs.encode_device(N, M, S, da.t, d_enc, stream=stream_a)  # of the healed originals: the stream orders it
        rs.heal_device_robust(N, M, S, db.t, drb.t, recovery_rows=mask, max_outliers=3, mode=3, stream=stream_b,
                              **ob.kw())
        return da, dra, db, drb, oa, ob, d_enc

    for streams in ((None, None), (torch.cuda.Stream(), torch.cuda.Stream())):
        da, dra, db, drb, oa, ob, d_enc = launch(*streams)
        torch.cuda.synchronize()
        la, fa, xa, aa = oa.read("first heal")
        lb, fb, xb, ab = ob.read("second heal")
        assert (int(la[0]), int(aa[0])) == (7, 3) and fa.all() and np.flatnonzero(xa[0]).tolist() == [0]
        assert (int(lb[0]), int(ab[0])) == (N - 2, 3) and np.array_equal(fb[0], mask)
        assert np.flatnonzero(xb[0]).tolist() == [3, 199]
        da.check(orig, "first heal: d_original"), dra.check(rec, "first heal: d_recovery")
        db.check(orig, "second heal: d_original"), drb.check(rec, "second heal: d_recovery")
        assert np.array_equal(d_enc.cpu().numpy(), rec)
        for s in streams:
            if s is not None:
                rs.release_stream_scratch(s)


def test_scrub(torch, rs):
    """The three-call scrub (robust locate, read, repair_device_batch_masks) and the robust heal of
    the same batch end byte-identical to each other and to the clean batch."""
    rate, N, M, S, B = "high", 70, 100, 66, 5
    pairs = [V.stripe(rate, N, M, S, seed=b) for b in range(B)]
    origs, recs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    bad_o, bad_r = origs.copy(), recs.copy()
    rng = np.random.default_rng(5)
    bad_o[0, 33] = rng.integers(0, 256, S, dtype=np.uint8)
    bad_r[0, 0, 40] ^= 0x08
    bad_r[1, 17, 40] ^= 0x08
    bad_r[1, 93, 3] ^= 0x80
    bad_o[3, N - 1, S - 1] ^= 0x80
    bad_r[3, [2, 99]] = rng.integers(0, 256, (2, S), dtype=np.uint8)
    bad_o[4, 0, 0] ^= 0x01
    # the scrub
    d_orig, d_rec = V.view(torch, bad_o, 0), V.view(torch, bad_r, 0)
    located, flags, outlier = (x.cpu().numpy() for x in rs.locate_device_robust_batch(
        N, M, S, d_orig, d_rec, max_outliers=2, rate_=RATE[rate]))
    assert located.tolist() == [33, ROWS, CLEAN, N - 1, 0]
    orig_ok, rec_ok = np.ones((B, N), np.uint8), np.ones((B, M), np.uint8)
    for b, i in enumerate(located):
        if i >= 0:
            orig_ok[b, i] = 0
            rec_ok[b] = 1 - outlier[b]
        elif i == ROWS:
            rec_ok[b] = 1 - flags[b]
    rs.repair_device_batch_masks(N, M, S, d_orig, orig_ok, d_rec, rec_ok, d_orig, d_rec, rate_=RATE[rate])
    # the heal
    h_orig, h_rec = Dev(torch, bad_o, 0), Dev(torch, bad_r, 0)
    out = Out(torch, B, M, True)
    rs.heal_device_robust_batch(N, M, S, h_orig.t, h_rec.t, max_outliers=2, mode=3, max_rows=2, rate_=RATE[rate],
                                **out.kw())
    torch.cuda.synchronize()
    loc, f, x, act = out.read("heal")
    assert loc.tolist() == located.tolist() and np.array_equal(f, flags) and np.array_equal(x, outlier)
    assert act.tolist() == [3, RECOVERY, 0, 3, ORIGINAL]
    h_orig.check(origs, "heal: d_original")
    h_rec.check(recs, "heal: d_recovery")
    assert np.array_equal(d_orig.cpu().numpy(), h_orig.t.cpu().numpy())
    assert np.array_equal(d_rec.cpu().numpy(), h_rec.t.cpu().numpy())
    assert np.array_equal(d_orig.cpu().numpy(), origs) and np.array_equal(d_rec.cpu().numpy(), recs)


def test_wrappers_reject_before_any_call(torch, rs):
    N, M, S = 8, 6, 64
    o = torch.zeros((N, S), dtype=torch.uint8, device="cuda")
    r = torch.zeros((M, S), dtype=torch.uint8, device="cuda")
    dev = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype, device="cuda")
    with pytest.raises(ValueError, match="d_original: dtype"):
        rs.heal_device_robust(N, M, S, o.to(torch.int32), r)
    with pytest.raises(ValueError, match="d_recovery:"):
        rs.heal_device_robust(N, M, S, o, dev(M - 1, S))
    with pytest.raises(ValueError, match="d_action"):
        rs.heal_device_robust(N, M, S, o, r, d_action=torch.zeros(1, dtype=torch.uint8))  # on the host
    with pytest.raises(ValueError, match="d_outlier"):
        rs.heal_device_robust(N, M, S, o, r, d_outlier=dev(M + 1))
    with pytest.raises(ValueError, match="d_located"):
        rs.heal_device_robust(N, M, S, o, r, d_located=dev(1))
    with pytest.raises(ValueError, match="mode:"):
        rs.heal_device_robust(N, M, S, o, r, mode=0)
    with pytest.raises(ValueError, match="max_outliers"):
        rs.heal_device_robust(N, M, S, o, r, max_outliers=3)
    with pytest.raises(ValueError, match="stripe count"):
        rs.heal_device_robust_batch(N, M, S, dev(2, N, S), dev(3, M, S))
    # tensors the call allocates itself
    loc, flags, outlier, act = rs.heal_device_robust_batch(N, M, S, dev(2, N, S), dev(2, M, S), max_outliers=2, max_rows=1)
    assert loc.shape == (2,) and flags.shape == outlier.shape == (2, M) and act.shape == (2,)
    assert act.is_cuda and loc.cpu().tolist() == [CLEAN, CLEAN] and act.cpu().tolist() == [0, 0]
    assert not outlier.cpu().numpy().any() and not flags.cpu().numpy().any()
