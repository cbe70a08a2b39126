"""GPU: rs_locate_device_batch_masks -- a locate of a batch in which every stripe has its own
recovery-row mask.

The batches are tests/verify_masks_cases.py's: 8 stripes, each built for a different outcome (a
located original at 0, N / 2 and N - 1, UNKNOWN from two corrupt originals, ROWS, CLEAN, and two
stripes with one selected row, which a locate skips), whose intended outcome
tests/test_verify_masks_cpu.py has checked against locate_model.locate stripe by stripe.  The rows a
stripe's mask leaves out hold junk.  `located` and the flags must equal the model's and those of a
loop of locate_device calls; all or nothing must refuse the batch and write nothing.
"""
import numpy as np
import pytest

import verify_masks_cases as C
from test_gpu_verify import GUARD, guarded_flags, padded_batch, profiled, view

pytestmark = pytest.mark.gpu
RATE = C.RATE


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


def run(torch, rs, rate, N, M, S, pad, batch=None):
    """One status-mode call on fresh, stripe-padded device copies, checked against the constructed
    outcome and for stray writes; (located, flags, codes, records, device matrices).  batch: (stored
    originals, stored recovery, masks, intended located, expected flags) in place of
    C.locate_batch's."""
    store, held, masks, intent, want = batch or C.locate_batch(rate, N, M, S)[2:]
    B = len(masks)
    d_orig, d_rec = padded_batch(torch, np.array(store), 2, pad), padded_batch(torch, np.array(held), 3, pad)
    flags, buf = guarded_flags(torch, (B, M))
    located, lbuf = guarded_located(torch, B)
    out = {}

    def call():
        out["r"] = rs.locate_device_batch_masks(N, M, S, d_orig, d_rec, masks, d_located=located, d_mismatch=flags,
                                                status=True, rate_=RATE[rate])

    recs = profiled(torch, rs, call)
    what = f"{rate} {N}:{M} x {S} pad {pad}"
    h, lh = buf.cpu().numpy(), lbuf.cpu().numpy()
    assert (h[:GUARD] == 0xFF).all() and (h[-GUARD:] == 0xFF).all(), what + ": a byte outside the flags was written"
    assert (lh[:4] == -1).all() and (lh[-4:] == -1).all(), what + ": a word outside d_located was written"
    assert np.array_equal(d_orig.cpu().numpy(), store) and np.array_equal(d_rec.cpu().numpy(), held), what
    got, loc, codes = flags.cpu().numpy(), located.cpu().numpy(), out["r"][2]
    assert (got <= 1).all()
    assert codes.tolist() == [101 if i == C.SKIPPED else 0 for i in intent], (what, codes)
    assert loc.tolist() == intent.tolist(), (what, loc.tolist(), intent.tolist())
    for b in range(B):
        assert np.array_equal(got[b], want[b]), (what, b, np.flatnonzero(got[b])[:8], np.flatnonzero(want[b])[:8])
    return loc, got, codes, recs, (d_orig, d_rec)


def check_against_singles(torch, rs, rate, N, M, S, d_orig, d_rec, masks, loc, got):
    for b in range(len(masks)):
        if masks[b].sum() < 2:
            assert loc[b] == rs.LOCATE_SKIPPED and not got[b].any()
            continue
        l1, f1 = rs.locate_device(N, M, S, d_orig[b], d_rec[b], recovery_rows=masks[b], rate_=RATE[rate])
        assert int(l1.cpu().numpy()[0]) == loc[b], b
        assert np.array_equal(f1.cpu().numpy(), got[b]), b


@pytest.mark.parametrize("rate,N,M,S,pad", C.FUSED + C.UNFUSED, ids=lambda v: str(v))
def test_shapes(torch, rs, rate, N, M, S, pad):
    masks = C.locate_batch(rate, N, M, S)[4]
    loc, got, _, recs, (d_orig, d_rec) = run(torch, rs, rate, N, M, S, pad)
    check_against_singles(torch, rs, rate, N, M, S, d_orig, d_rec, masks, loc, got)
    names = [r[0] for r in recs]
    assert not any(n.startswith("k_mono_verify") for n in names), names
    column = (rate, N, M, S, pad) in C.FUSED
    groups = 1 if column else len(masks)
    assert names.count("k_locate_find_masks") == groups, names
    if column:  # the unfused verify's launches, then exactly one find and one confirm
        assert names[-3:] == ["k_verify_rows_masks", "k_locate_find_masks", "k_locate_confirm_masks"], names
        # (one encode and one compare per run of located stripes: the skipped stripes 1 and 2 split the batch)
        assert names.count("k_verify_rows_masks") == 2 and names.count("k_locate_confirm_masks") == 1
    else:  # stripe by stripe: the skipped stripes cost a find and nothing else
        live = int((masks.sum(axis=1) >= 2).sum())
        assert names.count("k_verify_rows_masks") == live and names.count("k_locate_confirm_masks") == live, names


def test_four_element_packs(torch, rs):
    try:
        rs.mono_enable(1 + 8)
        run(torch, rs, "default", 200, 200, 72, 0)
    finally:
        rs.mono_enable(True)


@pytest.mark.parametrize("rate,N,M,S", [("default", 200, 200, 72), ("high", 1000, 100, 66)], ids=lambda v: str(v))
def test_all_or_nothing_refuses_and_writes_nothing(torch, rs, rate, N, M, S):
    _, _, store, held, masks, _, _ = C.locate_batch(rate, N, M, S)
    d_orig, d_rec = view(torch, store, 0), view(torch, held, 0)
    flags, buf = guarded_flags(torch, masks.shape)
    located, lbuf = guarded_located(torch, len(masks))
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="stripe 1 ") as e:
        rs.locate_device_batch_masks(N, M, S, d_orig, d_rec, masks, d_located=located, d_mismatch=flags,
                                     rate_=RATE[rate])
    assert e.value.stripe == 1
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0xFF).all() and (lbuf.cpu().numpy() == -1).all()


def coef_launches(recs):
    return [r[0] for r in recs if r[0].startswith("k_coef_")]


def test_table_is_shared_with_the_plain_locate(torch, rs):
    """The first locate of a shape on a stream builds the table; a warm masks call builds none, and
    neither does a plain locate_device_batch after it (nor a masks call after a plain one)."""
    rate, N, M, S = "default", 200, 200, 64
    _, _, store, held, masks, _, _ = C.locate_batch(rate, N, M, S)
    d_orig, d_rec = view(torch, store, 0), view(torch, held, 0)
    rs.release_stream_scratch()
    call = lambda: rs.locate_device_batch_masks(N, M, S, d_orig, d_rec, masks, status=True)
    plain = lambda: rs.locate_device_batch(N, M, S, d_orig, d_rec)
    assert coef_launches(profiled(torch, rs, call)) == ["k_coef_unit_slab", "k_coef_log_slab"]
    assert coef_launches(profiled(torch, rs, call)) == []
    assert coef_launches(profiled(torch, rs, plain)) == []
    rs.release_stream_scratch()
    assert coef_launches(profiled(torch, rs, plain)) == ["k_coef_unit_slab", "k_coef_log_slab"]
    assert coef_launches(profiled(torch, rs, call)) == []
    rs.release_stream_scratch()


def test_one_mask_for_every_stripe_is_the_shared_mask_call(torch, rs):
    rate, N, M, S = "default", 200, 200, 72
    _, _, store, held, masks, _, _ = C.locate_batch(rate, N, M, S)
    d_orig = view(torch, store, 0)
    for mask in (masks[4], masks[3], masks[0]):
        rec = np.array(held)
        rec[:, mask == 0] = 0xEE
        d_rec = view(torch, rec, 0)
        a = rs.locate_device_batch_masks(N, M, S, d_orig, d_rec, np.tile(mask, (len(masks), 1)), rate_=RATE[rate])
        b = rs.locate_device_batch(N, M, S, d_orig, d_rec, recovery_rows=mask, rate_=RATE[rate])
        for x, y in zip(a, b):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())


def test_calls_in_flight_keep_their_own_masks(torch, rs):
    """Two calls with DIFFERENT masks back to back on one stream, then on two streams with an
    encode between them: each equals its own truth (a loop of locate_device calls, run afterwards)."""
    rate, N, M, S = "default", 200, 200, 72
    _, _, store, held, masks, intent, want = C.locate_batch(rate, N, M, S)
    B = len(masks)
    d_orig, d_rec = view(torch, store, 0), view(torch, held, 0)
    masks2 = masks.copy()
    masks2[[0, 5]] = masks[[5, 0]]  # stripes 0 and 5 swap masks: other flags, other reference rows
    masks2[1] = masks[3]            # and a skipped stripe is located
    la, lb = (torch.full((B,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    fa, fb = (torch.full((B, M), 0xFF, dtype=torch.uint8, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    h1, h2 = masks.copy(), masks2.copy()
    rs.locate_device_batch_masks(N, M, S, d_orig, d_rec, h1, d_located=la, d_mismatch=fa, status=True, rate_=RATE[rate])
    h1[:] = 1
    rs.locate_device_batch_masks(N, M, S, d_orig, d_rec, h2, d_located=lb, d_mismatch=fb, status=True, rate_=RATE[rate])
    h2[:] = 0
    torch.cuda.synchronize()
    assert la.cpu().numpy().tolist() == intent.tolist() and np.array_equal(fa.cpu().numpy(), want)
    check_against_singles(torch, rs, rate, N, M, S, d_orig, d_rec, masks2, lb.cpu().numpy(), fb.cpu().numpy())
    assert not np.array_equal(fa.cpu().numpy(), fb.cpu().numpy())
    keep = (lb.cpu().numpy().copy(), fb.cpu().numpy().copy())
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    la.fill_(-1), lb.fill_(-1), fa.fill_(0xFF), fb.fill_(0xFF)
    d_enc = torch.zeros((M, S), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rs.locate_device_batch_masks(N, M, S, d_orig, d_rec, masks, d_located=la, d_mismatch=fa, status=True,
                                 rate_=RATE[rate], stream=s1)
    rs.encode_device(N, M, S, d_orig[1], d_enc, rate_=RATE[rate])
    rs.locate_device_batch_masks(N, M, S, d_orig, d_rec, masks2, d_located=lb, d_mismatch=fb, status=True,
                                 rate_=RATE[rate], stream=s2)
    torch.cuda.synchronize()
    assert la.cpu().numpy().tolist() == intent.tolist() and np.array_equal(fa.cpu().numpy(), want)
    assert np.array_equal(lb.cpu().numpy(), keep[0]) and np.array_equal(fb.cpu().numpy(), keep[1])
    assert np.array_equal(d_enc.cpu().numpy(), C.O.encode(rate, store[1], M))
    rs.release_stream_scratch(s1)
    rs.release_stream_scratch(s2)


def test_scrub(torch, rs):
    """locate_device_batch_masks, read the results, ONE repair_device_batch_masks: the rows each
    stripe had lost, the located originals and the flagged rows are absent.  The batch ends
    byte-identical to the clean one (but for the UNKNOWN stripe, which is left out of the batch: it
    needs more than one original replaced and is the caller's)."""
    rate, N, M, S = "high", 70, 100, 72
    origs, recs, store, held, masks, intent, _ = C.locate_batch(rate, N, M, S)
    keep = [b for b in range(len(masks)) if intent[b] != C.UNKNOWN]
    origs, recs, store, held, masks = (np.array(a[keep]) for a in (origs, recs, store, held, masks))
    d_orig, d_rec = view(torch, store, 0), view(torch, held, 0)
    located, flags, codes = rs.locate_device_batch_masks(N, M, S, d_orig, d_rec, masks, status=True, rate_=RATE[rate])
    located, flags = located.cpu().numpy(), flags.cpu().numpy()
    orig_ok = np.ones((len(keep), N), np.uint8)
    rec_ok = masks * (1 - flags)  # a lost row is absent, and so is a row that differs ...
    for b, i in enumerate(located):
        if i >= 0:  # ... unless an original explains it: the selected rows are right, the original is not
            orig_ok[b, i] = 0
            rec_ok[b] = masks[b]
    assert (codes != 0).sum() == 2 and (located == rs.LOCATE_SKIPPED).sum() == 2
    rs.repair_device_batch_masks(N, M, S, d_orig, orig_ok, d_rec, rec_ok, d_orig, d_rec, rate_=RATE[rate])
    torch.cuda.synchronize()
    assert np.array_equal(d_orig.cpu().numpy(), origs) and np.array_equal(d_rec.cpu().numpy(), recs)
