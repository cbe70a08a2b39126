"""GPU: rs_verify_device_batch_masks -- a verify of a batch in which every stripe has its own
recovery-row mask.

The batches are tests/verify_masks_cases.py's (tests/test_verify_masks_cpu.py checks them against
the oracle and the model): 7 stripes whose masks select every row, row 0 only, the last row only,
two rows far apart, all but every third row, nothing, and rows 2.. ; the rows a stripe's mask leaves
out hold junk that differs from stripe to stripe.  Both routes are forced through verify_set_fused
and must give the constructed flags, which must also be those of a loop of verify_device calls.
Every run checks that nothing but the flags was written (the helpers of tests/test_gpu_verify.py).
"""
import numpy as np
import pytest

import verify_masks_cases as C
from test_gpu_verify import GUARD, check_untouched, guarded_flags, padded_batch, profiled, view

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
    reed_solomon_simd.verify_set_fused(reed_solomon_simd.VERIFY_FUSED_DEFAULT)
    reed_solomon_simd.mono_enable(True)


def run(torch, rs, rate, N, M, S, pad, fused, batch=None):
    """One call on fresh, stripe-padded device copies; (flags, launch records).  batch: (stored
    originals, stored recovery, masks, expected flags) in place of C.verify_batch's."""
    store, held, masks, want = batch or C.verify_batch(rate, N, M, S)[2:]
    B = len(masks)
    d_orig, d_rec = padded_batch(torch, np.array(store), 2, pad), padded_batch(torch, np.array(held), 3, pad)
    flags, buf = guarded_flags(torch, (B, M))
    rs.verify_set_fused(fused)
    recs = profiled(torch, rs, lambda: rs.verify_device_batch_masks(N, M, S, d_orig, d_rec, masks, d_mismatch=flags,
                                                                    rate_=RATE[rate]))
    what = f"{rate} {N}:{M} x {S} pad {pad} fused {fused}"
    got = check_untouched(buf, flags, d_orig, store, d_rec, held, what)
    for b in range(B):
        assert np.array_equal(got[b], want[b]), f"{what}: stripe {b} flagged {np.flatnonzero(got[b]).tolist()[:8]}, " \
                                                f"want {np.flatnonzero(want[b]).tolist()[:8]}"
    return got, recs, (d_orig, d_rec)


def loop_of_singles(torch, rs, rate, N, M, S, d_orig, d_rec, masks):
    out = []
    for b in range(len(masks)):
        f = torch.full((M,), 0xFF, dtype=torch.uint8, device="cuda")
        rs.verify_device(N, M, S, d_orig[b], d_rec[b], recovery_rows=masks[b], d_mismatch=f, rate_=RATE[rate])
        out.append(f)
    torch.cuda.synchronize()
    return np.stack([f.cpu().numpy() for f in out])


@pytest.mark.parametrize("rate,N,M,S,pad", C.FUSED, ids=lambda v: str(v))
def test_fused_shapes(torch, rs, rate, N, M, S, pad):
    """Both pack widths, fused and unfused: the constructed flags, those of a loop of verify_device
    calls, and the two routes agree.  A fused call is exactly one k_mono_verify_masks launch."""
    masks = C.verify_batch(rate, N, M, S)[4]
    try:
        for enable, elems in ((1, 2), (1 + 8, 4)):
            rs.mono_enable(enable)
            a, recs, (d_orig, d_rec) = run(torch, rs, rate, N, M, S, pad, fused=1)
            names = [r[0] for r in recs]
            assert len(names) == 1 and names[0].startswith("k_mono_verify_masks<") and \
                names[0].endswith(f", {elems}>"), names
            assert not any(n.startswith("k_mono_verify<") or n.startswith("k_verify_rows") for n in names)
            assert np.array_equal(a, loop_of_singles(torch, rs, rate, N, M, S, d_orig, d_rec, masks))
            b, recs, _ = run(torch, rs, rate, N, M, S, pad, fused=0)
            names = [r[0] for r in recs]
            # one batch encode and one compare per run of stripes that select something: the empty
            # stripe 5, none of whose memory may be read, splits this batch in two
            assert names[-1] == "k_verify_rows_masks" and names.count("k_verify_rows_masks") == 2, names
            assert not any(n.startswith("k_mono_verify") for n in names), names
            assert np.array_equal(a, b)
    finally:
        rs.mono_enable(True)


@pytest.mark.parametrize("rate,N,M,S,pad", C.UNFUSED, ids=lambda v: str(v))
def test_unfused_shapes(torch, rs, rate, N, M, S, pad):
    """Shapes whose encode is not the staged column kernel: whatever verify_set_fused says the work
    goes stripe by stripe, each stripe with its own span, and the empty stripe costs no launch."""
    masks = C.verify_batch(rate, N, M, S)[4]
    for fused in (1, 0):
        got, recs, (d_orig, d_rec) = run(torch, rs, rate, N, M, S, pad, fused)
        names = [r[0] for r in recs]
        assert names[-1] == "k_verify_rows_masks" and not any(n.startswith("k_mono_verify") for n in names), names
        assert names.count("k_verify_rows_masks") == int((masks.sum(axis=1) > 0).sum()), names
    assert np.array_equal(got, loop_of_singles(torch, rs, rate, N, M, S, d_orig, d_rec, masks))


@pytest.mark.parametrize("fused", [1, 0])
def test_padding_is_not_compared(torch, rs, fused):
    """Row and stripe padding that differs from anything an encode would leave there (0xC3 beside
    the originals, 0x5A beside the recovery rows): no row is flagged."""
    rate, N, M, S, pad = "high", 70, 100, 72, 8
    origs, recs, _, _, masks, _ = C.verify_batch(rate, N, M, S)
    d_orig = padded_batch(torch, np.array(origs), 1, pad)
    whole = torch.full((len(masks), M + 1, S + pad), 0x5A, dtype=torch.uint8, device="cuda")
    d_rec = whole[:, :M, :S]
    d_rec.copy_(torch.from_numpy(np.array(recs)).cuda())
    rs.verify_set_fused(fused)
    every = np.ones_like(masks)
    got = rs.verify_device_batch_masks(N, M, S, d_orig, d_rec, every, rate_=RATE[rate]).cpu().numpy()
    assert not got.any(), np.argwhere(got)[:8]


@pytest.mark.parametrize("fused", [1, 0])
def test_all_empty_batch_launches_nothing(torch, rs, fused):
    rate, N, M, S = "default", 200, 200, 64
    _, _, store, held, masks, _ = C.verify_batch(rate, N, M, S)
    d_orig, d_rec = view(torch, store, 0), view(torch, held, 0)
    flags, buf = guarded_flags(torch, masks.shape)
    rs.verify_set_fused(fused)
    recs = profiled(torch, rs, lambda: rs.verify_device_batch_masks(N, M, S, d_orig, d_rec, np.zeros_like(masks),
                                                                    d_mismatch=flags))
    assert recs == []
    h = buf.cpu().numpy()
    assert (h[:GUARD] == 0xFF).all() and (h[-GUARD:] == 0xFF).all() and not h[GUARD:-GUARD].any()


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("rate,N,M,S", [("default", 200, 200, 72), ("high", 1000, 100, 66)], ids=lambda v: str(v))
def test_one_mask_for_every_stripe_is_the_shared_mask_call(torch, rs, rate, N, M, S, fused):
    _, _, store, held, masks, _ = C.verify_batch(rate, N, M, S)
    d_orig = view(torch, store, 0)
    rs.verify_set_fused(fused)
    for mask in (masks[4], masks[3], masks[0]):
        rec = np.array(held)
        rec[:, mask == 0] = 0xEE  # junk where the shared mask leaves rows out
        rec[2, np.flatnonzero(mask)[-1], 3] ^= 0x20
        d_rec = view(torch, rec, 0)
        tiled = np.tile(mask, (len(masks), 1))
        a = rs.verify_device_batch_masks(N, M, S, d_orig, d_rec, tiled, rate_=RATE[rate]).cpu().numpy()
        b = rs.verify_device_batch(N, M, S, d_orig, d_rec, recovery_rows=mask, rate_=RATE[rate]).cpu().numpy()
        assert np.array_equal(a, b) and a[2, np.flatnonzero(mask)[-1]] == 1


@pytest.mark.parametrize("fused", [1, 0])
def test_calls_in_flight_keep_their_own_masks(torch, rs, fused):
    """Two calls with DIFFERENT masks back to back on one stream (the second call's masks must not
    reach the first call's kernel through the staging), then on two streams with an encode between."""
    rate, N, M, S = "default", 200, 200, 72
    _, recs, store, held, masks, want = C.verify_batch(rate, N, M, S)
    B = len(masks)
    d_orig, d_rec = view(torch, store, 0), view(torch, held, 0)
    # the second call: the masks rotated by one stripe, over data whose junk follows the first call's masks
    masks2 = np.roll(masks, 1, axis=0)
    truth = np.stack([(C.O.encode(rate, store[b], M) != held[b]).any(axis=1) for b in range(B)]).astype(np.uint8)
    want2 = truth * masks2
    assert not np.array_equal(want, want2)
    rs.verify_set_fused(fused)
    fa, fb = (torch.full((B, M), 0xFF, dtype=torch.uint8, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    h1, h2 = masks.copy(), masks2.copy()
    rs.verify_device_batch_masks(N, M, S, d_orig, d_rec, h1, d_mismatch=fa, rate_=RATE[rate])
    h1[:] = 1  # the host masks may be reused as soon as the call returns
    rs.verify_device_batch_masks(N, M, S, d_orig, d_rec, h2, d_mismatch=fb, rate_=RATE[rate])
    h2[:] = 0
    torch.cuda.synchronize()
    assert np.array_equal(fa.cpu().numpy(), want) and np.array_equal(fb.cpu().numpy(), want2)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    fa.fill_(0xFF), fb.fill_(0xFF)
    d_enc = torch.zeros((M, S), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rs.verify_device_batch_masks(N, M, S, d_orig, d_rec, masks, d_mismatch=fa, rate_=RATE[rate], stream=s1)
    rs.encode_device(N, M, S, d_orig[0], d_enc, rate_=RATE[rate])
    rs.verify_device_batch_masks(N, M, S, d_orig, d_rec, masks2, d_mismatch=fb, rate_=RATE[rate], stream=s2)
    torch.cuda.synchronize()
    assert np.array_equal(fa.cpu().numpy(), want) and np.array_equal(fb.cpu().numpy(), want2)
    assert np.array_equal(d_enc.cpu().numpy(), C.O.encode(rate, store[0], M))
    rs.release_stream_scratch(s1)
    rs.release_stream_scratch(s2)
