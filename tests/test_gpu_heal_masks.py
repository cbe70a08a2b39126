"""GPU: rs_heal_device_batch_masks -- a heal of a batch in which every stripe has its own
recovery-row mask.

The batch is tests/heal_masks_cases.py's: 8 stripes, each built for a different outcome (an original
healed at 0, N / 2 and N - 1 -- the last with e from row 2 --, UNKNOWN from two corrupt originals, a
ROWS stripe with two rows to rewrite, CLEAN, and two stripes with fewer than three selected rows,
which a heal of originals skips), whose intended outcome tests/test_heal_masks_cpu.py has checked
against heal_model.heal stripe by stripe.  The rows a stripe's mask leaves out hold junk.  The three
outputs and BOTH matrices, whole (guards, row padding, stripe padding, junk), must equal the model's
and those of a loop of heal_device calls; all or nothing must refuse the batch and write nothing.
"""
import numpy as np
import pytest

import heal_masks_cases as H
import verify_masks_cases as C
from test_gpu_verify import GUARD, guarded_flags, padded_batch, profiled, view

pytestmark = pytest.mark.gpu
RATE = C.RATE
BOTH = H.ORIGINAL | H.RECOVERY
SHAPE = ("default", 200, 200, 72)  # the column kernel, a tail
OFF = ("high", 1000, 100, 66)      # off it: a group is one stripe; byte-wise rows


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


def guarded_located(torch, n):
    buf = torch.full((n + 8,), -1, dtype=torch.int32, device="cuda")  # (0xFF bytes throughout)
    return buf[4:4 + n], buf


def whole(v):
    """The buffer a padded_batch / view tensor lives in, on the host: padding and all."""
    return (v if v._base is None else v._base).cpu().numpy()


def expected_whole(v, a):
    """What whole(v) must hold when the matrices are `a` and every padding byte is untouched."""
    base = v if v._base is None else v._base
    w = np.full(tuple(base.shape), 0xC3, np.uint8)
    w[tuple(slice(0, n) for n in a.shape)] = a
    return w


def heal(torch, rs, rate, N, M, S, store, held, masks, mode=BOTH, max_rows=2, pad=0, extra=(0, 0), stream=None):
    """One status-mode call on fresh device copies over 0xFF-poisoned, guarded outputs; checks the
    guards; (located, flags, action, codes, d_orig, d_rec, launch records)."""
    B = len(masks)
    d_orig = padded_batch(torch, np.array(store), extra[0], pad)
    d_rec = padded_batch(torch, np.array(held), extra[1], pad)
    flags, fbuf = guarded_flags(torch, (B, M))
    action, abuf = guarded_flags(torch, (B,))
    located, lbuf = guarded_located(torch, B)
    out = {}

    def call():
        out["r"] = rs.heal_device_batch_masks(N, M, S, d_orig, d_rec, masks, mode=mode, max_rows=max_rows,
                                              d_located=located, d_mismatch=flags, d_action=action, status=True,
                                              stream=stream, rate_=RATE[rate])

    recs = profiled(torch, rs, call)
    for buf in (fbuf.cpu().numpy(), abuf.cpu().numpy()):
        assert (buf[:GUARD] == 0xFF).all() and (buf[-GUARD:] == 0xFF).all(), "a byte outside an output was written"
    lh = lbuf.cpu().numpy()
    assert (lh[:4] == -1).all() and (lh[-4:] == -1).all(), "a word outside d_located was written"
    return located.cpu().numpy(), flags.cpu().numpy(), action.cpu().numpy(), out["r"][3], d_orig, d_rec, recs


def check(got, want, what):
    """The five results and the status codes of a call against the model's; the matrices whole."""
    loc, flags, act, codes, d_orig, d_rec, _ = got
    wloc, wflags, wact, o2, r2, wcodes = want
    assert codes.tolist() == wcodes.tolist(), (what, codes)
    assert loc.tolist() == wloc.tolist(), (what, loc.tolist(), wloc.tolist())
    assert act.tolist() == wact.tolist(), (what, act.tolist(), wact.tolist())
    for b in range(len(loc)):
        assert np.array_equal(flags[b], wflags[b]), (what, b, np.flatnonzero(flags[b])[:8], np.flatnonzero(wflags[b])[:8])
    assert np.array_equal(whole(d_orig), expected_whole(d_orig, o2)), what + ": the originals"
    assert np.array_equal(whole(d_rec), expected_whole(d_rec, r2)), what + ": the recovery shards"


@pytest.mark.parametrize("rate,N,M,S,pad", C.FUSED + C.UNFUSED, ids=lambda v: str(v))
def test_shapes(torch, rs, rate, N, M, S, pad):
    """Status mode, both bits, max_rows = 2, stripe padding of 2 and 3 rows: everything equals the
    per-stripe model, and the outcome is the one each stripe is built for."""
    _, _, store, held, masks = H.heal_batch(rate, N, M, S)
    got = heal(torch, rs, rate, N, M, S, store, held, masks, pad=pad, extra=(2, 3))
    check(got, H.model(rate, N, M, S), f"{rate} {N}:{M} x {S} pad {pad}")
    want_loc, want_act = H.heal_intent(N)
    assert got[0].tolist() == want_loc.tolist() and got[2].tolist() == want_act.tolist()
    assert got[3].tolist() == [0, 101, 101, 0, 0, 0, 0, 0]
    names = [r[0] for r in got[6]]
    column = (rate, N, M, S, pad) in C.FUSED
    assert names.count("k_heal_masks") == (1 if column else 6), names
    assert not any(n.startswith("k_mono_verify") for n in names) and "k_heal" not in names, names


@pytest.mark.parametrize("rate,N,M,S", [SHAPE, OFF], ids=lambda v: str(v))
def test_a_loop_of_single_heals_gives_the_same(torch, rs, rate, N, M, S):
    """Every non-skipped stripe through heal_device (the shared-mask kernels) on copies: the same
    located, flags, action and matrices."""
    _, _, store, held, masks = H.heal_batch(rate, N, M, S)
    loc, flags, act, _, d_orig, d_rec, _ = heal(torch, rs, rate, N, M, S, store, held, masks)
    o2, r2 = d_orig.cpu().numpy(), d_rec.cpu().numpy()
    for b in range(len(masks)):
        if masks[b].sum() < 3:
            assert loc[b] == rs.LOCATE_SKIPPED and act[b] == 0 and not flags[b].any()
            assert np.array_equal(o2[b], store[b]) and np.array_equal(r2[b], held[b])
            continue
        o1, r1 = view(torch, store[b], 0), view(torch, held[b], 0)
        l1, f1, a1 = rs.heal_device(N, M, S, o1, r1, recovery_rows=masks[b], mode=BOTH, max_rows=2, rate_=RATE[rate])
        assert int(l1.cpu().numpy()[0]) == loc[b] and int(a1.cpu().numpy()[0]) == act[b], b
        assert np.array_equal(f1.cpu().numpy(), flags[b]), b
        assert np.array_equal(o1.cpu().numpy(), o2[b]) and np.array_equal(r1.cpu().numpy(), r2[b]), b


@pytest.mark.parametrize("rate,N,M,S", [SHAPE, OFF], ids=lambda v: str(v))
def test_unselected_rows_are_neither_read_nor_written(torch, rs, rate, N, M, S):
    """Other junk in the rows the masks leave out: the same outputs, the same matrices apart from
    that junk, which stays where it is (a corrupt unselected row stays corrupt, unflagged)."""
    _, recs, store, held, masks = H.heal_batch(rate, N, M, S)
    other = np.array(held)
    out = masks == 0
    other[out] ^= 0x5A
    a = heal(torch, rs, rate, N, M, S, store, held, masks)
    b = heal(torch, rs, rate, N, M, S, store, other, masks)
    for k in range(4):
        assert np.array_equal(a[k], b[k]), k
    assert not (a[1] & (masks == 0)).any()
    assert np.array_equal(a[4].cpu().numpy(), b[4].cpu().numpy())
    ra, rb = a[5].cpu().numpy(), b[5].cpu().numpy()
    assert np.array_equal(ra[~out], rb[~out])
    assert np.array_equal(ra[out], np.array(held)[out]) and np.array_equal(rb[out], other[out])
    assert not np.array_equal(rb[6, 1], recs[6, 1])  # stripe 6's row 1: still not the right row


@pytest.mark.parametrize("mode,max_rows", [(H.ORIGINAL, 2), (H.RECOVERY, 2), (BOTH, 0), (BOTH, 1), (BOTH, 2),
                                           (BOTH, 0xFFFFFFFF)])
def test_mode_bits_and_threshold(torch, rs, mode, max_rows):
    """Each mode bit alone (with the recovery bit alone stripe 2's two rows do: it is located and
    left untouched), and max_rows around stripe 6's two differing rows."""
    for rate, N, M, S in (SHAPE, OFF):
        _, _, store, held, masks = H.heal_batch(rate, N, M, S)
        want = H.model(rate, N, M, S, mode=mode, max_rows=max_rows)
        got = heal(torch, rs, rate, N, M, S, store, held, masks, mode=mode, max_rows=max_rows)
        check(got, want, f"{rate} {N}:{M} x {S} mode {mode} max_rows {max_rows}")
        healed6 = bool(mode & H.RECOVERY) and max_rows >= 2
        assert got[0][6] == C.ROWS and got[2][6] == (H.RECOVERY if healed6 else 0)
        assert got[2][[0, 3, 5]].tolist() == [mode & H.ORIGINAL] * 3
        if mode == H.RECOVERY:
            assert got[0][2] == N // 2 and got[2][2] == 0 and got[3].tolist() == [0, 101, 0, 0, 0, 0, 0, 0]
            assert np.array_equal(got[4].cpu().numpy(), store)


def test_four_element_packs(torch, rs):
    rate, N, M, S = SHAPE
    _, _, store, held, masks = H.heal_batch(rate, N, M, S)
    try:
        for enable in (1 + 8, 1):
            rs.mono_enable(enable)
            check(heal(torch, rs, rate, N, M, S, store, held, masks), H.model(rate, N, M, S), f"mono_enable({enable})")
    finally:
        rs.mono_enable(True)


@pytest.mark.parametrize("rate,N,M,S", [SHAPE, OFF], ids=lambda v: str(v))
def test_all_or_nothing_refuses_and_writes_nothing(torch, rs, rate, N, M, S):
    _, _, store, held, masks = H.heal_batch(rate, N, M, S)
    d_orig, d_rec = padded_batch(torch, np.array(store), 2), padded_batch(torch, np.array(held), 3)
    flags, fbuf = guarded_flags(torch, masks.shape)
    action, abuf = guarded_flags(torch, (len(masks),))
    located, lbuf = guarded_located(torch, len(masks))
    torch.cuda.synchronize()
    for mode, widen, stripe in ((BOTH, False, 1), (BOTH, True, 2), (H.RECOVERY, False, 1)):
        m = np.array(masks)
        if widen:
            m[1] = 1
        with pytest.raises(ValueError, match=f"stripe {stripe} ") as e:
            rs.heal_device_batch_masks(N, M, S, d_orig, d_rec, m, mode=mode, max_rows=2, d_located=located,
                                       d_mismatch=flags, d_action=action, rate_=RATE[rate])
        assert e.value.stripe == stripe
    torch.cuda.synchronize()
    assert (fbuf.cpu().numpy() == 0xFF).all() and (abuf.cpu().numpy() == 0xFF).all() and (lbuf.cpu().numpy() == -1).all()
    assert np.array_equal(whole(d_orig), expected_whole(d_orig, store))
    assert np.array_equal(whole(d_rec), expected_whole(d_rec, held))


@pytest.mark.parametrize("rate,N,M,S", [SHAPE, OFF], ids=lambda v: str(v))
def test_a_batch_in_which_no_stripe_can_be_healed(torch, rs, rate, N, M, S):
    """Every group is without a confirm and a k_heal_masks: d_action is still defined (0), every
    stripe SKIPPED, every flag 0, nothing else written."""
    _, _, store, held, masks = H.heal_batch(rate, N, M, S)
    few = np.tile(masks[2], (len(masks), 1))
    few[1::2] = masks[1]
    loc, flags, act, codes, d_orig, d_rec, recs = heal(torch, rs, rate, N, M, S, store, held, few, extra=(2, 3))
    assert loc.tolist() == [C.SKIPPED] * len(masks) and not act.any() and not flags.any()
    assert codes.tolist() == [101] * len(masks)
    assert np.array_equal(whole(d_orig), expected_whole(d_orig, store))
    assert np.array_equal(whole(d_rec), expected_whole(d_rec, held))
    assert not any(r[0] in ("k_heal_masks", "k_locate_confirm_masks", "k_verify_rows_masks") for r in recs), recs


@pytest.mark.parametrize("rate,N,M,S", [SHAPE, OFF, ("default", 4096, 4096, 64)], ids=lambda v: str(v))
def test_launches_of_a_warm_call(torch, rs, rate, N, M, S):
    """The locate-masks call's own launches plus exactly one k_heal_masks per group with a stripe
    to heal, each directly after that group's k_locate_confirm_masks; no k_heal, no decode, no table."""
    _, _, store, held, masks = H.heal_batch(rate, N, M, S)
    heal(torch, rs, rate, N, M, S, store, held, masks)  # (warm: the table is built)
    names = [r[0] for r in heal(torch, rs, rate, N, M, S, store, held, masks)[6]]
    skipped = np.array(masks)
    skipped[masks.sum(axis=1) < 3] = masks[1]  # the locate skips what the heal skips
    d_orig, d_rec = view(torch, store, 0), view(torch, held, 0)
    locate = [r[0] for r in profiled(torch, rs, lambda: rs.locate_device_batch_masks(
        N, M, S, d_orig, d_rec, skipped, status=True, rate_=RATE[rate]))]
    assert [n for n in names if n != "k_heal_masks"] == locate, (names, locate)
    at = [k for k, n in enumerate(names) if n == "k_heal_masks"]
    assert len(at) == (1 if (rate, N, M, S) == SHAPE else 6), names
    assert all(names[k - 1] == "k_locate_confirm_masks" for k in at), names
    assert names.count("k_locate_confirm_masks") == len(at)
    assert not any(n == "k_heal" or n.startswith("k_coef_") or "repair" in n or "decode" in n for n in names), names


def coef_launches(recs):
    return [r[0] for r in recs if r[0].startswith("k_coef_")]


def test_table_is_shared_with_the_plain_locate(torch, rs):
    rate, N, M, S = "default", 200, 200, 64
    _, _, store, held, masks = H.heal_batch(rate, N, M, S)
    d_orig, d_rec = view(torch, store, 0), view(torch, held, 0)
    rs.release_stream_scratch()
    call = lambda: rs.heal_device_batch_masks(N, M, S, d_orig, d_rec, masks, mode=BOTH, max_rows=2, status=True)
    plain = lambda: rs.locate_device_batch(N, M, S, d_orig, d_rec)
    assert coef_launches(profiled(torch, rs, call)) == ["k_coef_unit_slab", "k_coef_log_slab"]
    assert coef_launches(profiled(torch, rs, call)) == []
    assert coef_launches(profiled(torch, rs, plain)) == []
    rs.release_stream_scratch()
    assert coef_launches(profiled(torch, rs, plain)) == ["k_coef_unit_slab", "k_coef_log_slab"]
    assert coef_launches(profiled(torch, rs, call)) == []
    rs.release_stream_scratch()


def test_one_mask_for_every_stripe_is_the_shared_mask_call(torch, rs):
    rate, N, M, S = SHAPE
    _, _, store, held, masks = H.heal_batch(rate, N, M, S)
    for mask in (masks[4], masks[3], masks[0]):
        rec = np.array(held)
        rec[:, mask == 0] = 0xEE
        ours = (view(torch, store, 0), view(torch, rec, 0))
        theirs = (view(torch, store, 0), view(torch, rec, 0))
        a = rs.heal_device_batch_masks(N, M, S, ours[0], ours[1], np.tile(mask, (len(masks), 1)), mode=BOTH,
                                       max_rows=2, rate_=RATE[rate])
        b = rs.heal_device_batch(N, M, S, theirs[0], theirs[1], recovery_rows=mask, mode=BOTH, max_rows=2,
                                 rate_=RATE[rate])
        for x, y in zip(a + ours, b + theirs):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())
        assert a[2].cpu().numpy().any()  # (something was healed)


@pytest.mark.parametrize("rate,N,M,S", [SHAPE, OFF], ids=lambda v: str(v))
def test_second_call_finds_nothing_to_do_and_the_verify_is_clean(torch, rs, rate, N, M, S):
    origs, recs, store, held, masks = H.heal_batch(rate, N, M, S)
    _, _, _, _, d_orig, d_rec, _ = heal(torch, rs, rate, N, M, S, store, held, masks)
    o2, r2 = d_orig.cpu().numpy(), d_rec.cpu().numpy()
    loc, flags, act, codes, d_orig, d_rec, _ = heal(torch, rs, rate, N, M, S, o2, r2, masks)
    assert loc.tolist() == [C.CLEAN, C.SKIPPED, C.SKIPPED, C.CLEAN, C.UNKNOWN, C.CLEAN, C.CLEAN, C.CLEAN]
    assert not act.any() and codes.tolist() == [0, 101, 101, 0, 0, 0, 0, 0]
    assert np.array_equal(d_orig.cpu().numpy(), o2) and np.array_equal(d_rec.cpu().numpy(), r2)
    got = rs.verify_device_batch_masks(N, M, S, d_orig, d_rec, masks, rate_=RATE[rate]).cpu().numpy()
    assert not got[[0, 3, 5, 6, 7]].any()
    # the scrub's end: the healed stripes equal the clean batch on the originals and on every selected row
    for b in (0, 3, 5, 6):
        sel = masks[b] != 0
        assert np.array_equal(o2[b], origs[b]) and np.array_equal(r2[b][sel], recs[b][sel]), b


def test_calls_in_flight_keep_their_own_masks(torch, rs):
    """Two calls with DIFFERENT masks back to back on one stream, then on two streams with an
    encode between them: each ends as it does when run alone."""
    rate, N, M, S = SHAPE
    _, _, store, held, masks = H.heal_batch(rate, N, M, S)
    B = len(masks)
    masks2 = np.array(masks)
    masks2[[0, 5]] = masks[[5, 0]]  # stripes 0 and 5 swap masks: other flags, other reference rows
    masks2[1] = masks[3]            # and a skipped stripe is healed
    alone = [heal(torch, rs, rate, N, M, S, store, held, m) for m in (masks, masks2)]
    check(alone[1], H.model(rate, N, M, S, masks=masks2), "masks2 alone")
    assert not np.array_equal(alone[0][1], alone[1][1])

    def fresh():
        return dict(o=view(torch, store, 0), r=view(torch, held, 0),
                    l=torch.full((B,), -1, dtype=torch.int32, device="cuda"),
                    f=torch.full((B, M), 0xFF, dtype=torch.uint8, device="cuda"),
                    a=torch.full((B,), 0xFF, dtype=torch.uint8, device="cuda"))

    def launch(t, m, stream=None):
        rs.heal_device_batch_masks(N, M, S, t["o"], t["r"], m, mode=BOTH, max_rows=2, d_located=t["l"],
                                   d_mismatch=t["f"], d_action=t["a"], status=True, stream=stream, rate_=RATE[rate])

    def same(t, ref):
        for x, y in zip((t["l"], t["f"], t["a"], t["o"], t["r"]), (ref[0], ref[1], ref[2], ref[4], ref[5])):
            assert np.array_equal(x.cpu().numpy(), y if isinstance(y, np.ndarray) else y.cpu().numpy())

    ta, tb = fresh(), fresh()
    torch.cuda.synchronize()
    h1, h2 = np.array(masks), np.array(masks2)
    launch(ta, h1)
    h1[:] = 1  # the host mask is the caller's again when the call returns
    launch(tb, h2)
    h2[:] = 0
    torch.cuda.synchronize()
    same(ta, alone[0]), same(tb, alone[1])
    ta, tb = fresh(), fresh()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    d_enc = torch.zeros((M, S), dtype=torch.uint8, device="cuda")
    d_src = view(torch, store[7], 0)
    torch.cuda.synchronize()
    launch(ta, masks, s1)
    rs.encode_device(N, M, S, d_src, d_enc, rate_=RATE[rate])
    launch(tb, masks2, s2)
    torch.cuda.synchronize()
    same(ta, alone[0]), same(tb, alone[1])
    assert np.array_equal(d_enc.cpu().numpy(), C.O.encode(rate, store[7], M))
    rs.release_stream_scratch(s1)
    rs.release_stream_scratch(s2)
