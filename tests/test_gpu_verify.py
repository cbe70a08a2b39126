"""GPU: rs_verify_device* -- do the recovery shards of a stripe still agree with its originals?

Ground truth is constructed, not computed by the code under test: a stripe's recovery shards come
from the CPU oracle, chosen bytes are then flipped, and the expected flags are exactly the set of
rows touched (for a corrupted original: the rows where the oracle's encode of the corrupted
originals differs from the stored recovery).  Both routes -- the fused column kernel
(k_mono_verify) and the encode into scratch followed by k_verify_rows -- are forced through
verify_set_fused and must give those flags.  Every run also checks that nothing but the flags was
written: the inputs equal their host copies, the guard bytes around the flag array are as before,
and flags pre-filled with 0xFF come back 0 or 1.
"""
import numpy as np
import pytest

import oracle_lib as O
import span_cases as SC
import wide_cases as W

pytestmark = pytest.mark.gpu

RATE = {"default": 0, "high": 1, "low": 2}
GUARD = 16

# (rate, N, M): the encode is the staged single-chunk column kernel (2^7 .. 2^11 transform rows)
FUSED = [("high", 70, 100), ("low", 100, 70), ("default", 200, 200), ("default", 300, 500),
         ("default", 1024, 1024), ("default", 2048, 2048)]
# (S, row padding): whole blocks; a tail; a tail with rows that are not 4-byte aligned (byte-wise)
LAYOUTS = [(64, 0), (72, 0), (66, 4)]
# (rate, N, M, S): everything else the encode does
UNFUSED = [("default", 1, 1, 64), ("default", 3, 2, 2), ("high", 1000, 100, 66), ("low", 128, 1024, 64),
           ("default", 4096, 4096, 64)]
CORRUPTIONS = ["none", "first", "last", "middle", "every", "original"]


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


_STRIPES = {}
_WANT_ORIGINAL = {}


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


def corrupt(kind, rate, N, M, S, seed=0):
    """(originals, recovery, expected flags) of the stripe after one corruption.  A tuple is one of
    tests/wide_cases.py's positional kinds: damage placed by pack number."""
    orig, rec = stripe(rate, N, M, S, seed)
    if isinstance(kind, tuple):
        key = (kind, rate, N, M, S, seed)
        if key not in _WANT_ORIGINAL:
            _WANT_ORIGINAL[key] = W.verify_corrupt(kind, orig, rec, lambda o: O.encode(rate, o, M))
        return tuple(a.copy() for a in _WANT_ORIGINAL[key])
    orig, rec = orig.copy(), rec.copy()
    want = np.zeros(M, np.uint8)
    if kind == "first":  # one bit in row 0, byte 0
        rec[0, 0] ^= 0x01
        want[0] = 1
    elif kind == "last":  # one bit in the last byte of the last row (the tail's last high byte)
        rec[M - 1, S - 1] ^= 0x80
        want[M - 1] = 1
    elif kind == "middle":  # a low half and a high half of a middle block, in two middle rows
        if S >= 64:
            base = (S // 64 // 2) * 64
            lo, hi = base + 5, base + 32 + 17
        else:  # a tail alone: its low bytes, then its high bytes
            lo, hi = 0, S // 2
        a, b = M // 2, M // 3
        rec[a, lo] ^= 0x10
        rec[b, hi] ^= 0x02
        want[[a, b]] = 1
    elif kind == "every":
        for j in range(M):
            rec[j, (j * 7) % S] ^= 1 << (j % 8)
        want[:] = 1
    elif kind == "original":  # the stored recovery no longer belongs to these originals
        orig[N // 2, S // 3] ^= 0x04
        key = (rate, N, M, S, seed)
        if key not in _WANT_ORIGINAL:
            _WANT_ORIGINAL[key] = (O.encode(rate, orig, M) != rec).any(axis=1).astype(np.uint8)
        want = _WANT_ORIGINAL[key].copy()
        assert want.any()
    else:
        assert kind == "none"
    return orig, rec, want


def view(torch, a, pad, fill=0xC3):
    """A device copy of `a` [rows, S] or [B, rows, S] with `pad` junk bytes after every row."""
    if pad == 0:
        return torch.from_numpy(np.array(a, copy=True)).cuda()
    buf = torch.full(a.shape[:-1] + (a.shape[-1] + pad,), fill, dtype=torch.uint8, device="cuda")
    v = buf[..., :a.shape[-1]]
    v.copy_(torch.from_numpy(np.array(a, copy=True)).cuda())
    return v


def guarded_flags(torch, shape):
    """A flag tensor of `shape` pre-filled with 0xFF between two guards; (flags, whole buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((2 * GUARD + n,), 0xFF, dtype=torch.uint8, device="cuda")
    return buf[GUARD:GUARD + n].view(*shape), buf


def check_untouched(buf, flags, d_orig, orig, d_rec, rec, what):
    h = buf.cpu().numpy()
    assert (h[:GUARD] == 0xFF).all() and (h[-GUARD:] == 0xFF).all(), what + ": a byte outside the flags was written"
    got = flags.cpu().numpy()
    assert (got <= 1).all(), what + ": a flag is neither 0 nor 1"
    assert np.array_equal(d_orig.cpu().numpy(), orig), what + ": d_original was written"
    assert np.array_equal(d_rec.cpu().numpy(), rec), what + ": d_recovery was written"
    return got


def profiled(torch, rs, fn):
    rs.profile_enable(True)
    try:
        rs.profile_collect()
        fn()
        torch.cuda.synchronize()
        return rs.profile_collect()
    finally:
        rs.profile_enable(False)


def run(torch, rs, rate, N, M, S, kind, pad=0, mask=None, fused=None):
    """One verify of the corrupted stripe on fresh device copies; (flags, launch records)."""
    orig, rec, want = corrupt(kind, rate, N, M, S)
    d_orig, d_rec = view(torch, orig, pad), view(torch, rec, pad)
    flags, buf = guarded_flags(torch, (M,))
    if fused is not None:
        rs.verify_set_fused(fused)
    recs = profiled(torch, rs, lambda: rs.verify_device(N, M, S, d_orig, d_rec, recovery_rows=mask,
                                                        d_mismatch=flags, rate_=RATE[rate]))
    what = f"{rate} {N}:{M} x {S} pad {pad} {kind} fused {fused}"
    got = check_untouched(buf, flags, d_orig, orig, d_rec, rec, what)
    if mask is not None:
        want = want * (np.asarray(mask) != 0)
    assert np.array_equal(got, want), f"{what}: flagged rows {np.flatnonzero(got).tolist()[:8]}, " \
                                      f"want {np.flatnonzero(want).tolist()[:8]}"
    return got, recs


@pytest.mark.parametrize("S,pad", LAYOUTS, ids=lambda v: str(v))
@pytest.mark.parametrize("rate,N,M", FUSED, ids=lambda v: str(v))
def test_fused_shapes(torch, rs, rate, N, M, S, pad):
    """Every corruption, with 2-element packs (the default at this size) and 4-element packs
    (mono_enable + 8), on the fused route and with verify_set_fused(0): the same flags, the
    constructed ones.  The fused call is one launch of k_mono_verify in the pack format asked for."""
    for enable, elems in ((1, 2), (1 + 8, 4)):
        rs.mono_enable(enable)
        for kind in CORRUPTIONS:
            a, recs = run(torch, rs, rate, N, M, S, kind, pad, fused=1)
            names = [r[0] for r in recs]
            assert len(names) == 1 and names[0].startswith("k_mono_verify<") and names[0].endswith(f", {elems}>"), names
            b, recs = run(torch, rs, rate, N, M, S, kind, pad, fused=0)
            assert recs[-1][0] == "k_verify_rows" and not any(r[0].startswith("k_mono_verify") for r in recs), recs
            assert np.array_equal(a, b)
    rs.mono_enable(True)


@pytest.mark.parametrize("rate,N,M,S", UNFUSED, ids=lambda v: str(v))
def test_unfused_shapes(torch, rs, rate, N, M, S):
    """Shapes with no fused form (k_pass, k_chunks with unaligned rows, multi-chunk LowRate, the
    pass kernels of 2^12 rows): whatever verify_set_fused says, the call ends with k_verify_rows."""
    for fused in (1, 0):
        for kind in CORRUPTIONS:
            _, recs = run(torch, rs, rate, N, M, S, kind, fused=fused)
            assert recs[-1][0] == "k_verify_rows" and not any(r[0].startswith("k_mono_verify") for r in recs), recs


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("rate,N,M,S,pad", [("high", 70, 100, 64, 64), ("default", 1024, 1024, 72, 8),
                                            ("high", 1000, 100, 66, 2)], ids=lambda v: str(v))
def test_padding_is_not_compared(torch, rs, rate, N, M, S, pad, fused):
    """The bytes between shard_bytes and the row stride differ from anything an encode would
    leave there (0xC3 in the originals' padding, 0x5A in the recovery's): no row is flagged."""
    orig, rec = stripe(rate, N, M, S)
    d_orig, d_rec = view(torch, orig, pad), view(torch, rec, pad, fill=0x5A)
    flags, buf = guarded_flags(torch, (M,))
    rs.verify_set_fused(fused)
    rs.verify_device(N, M, S, d_orig, d_rec, d_mismatch=flags, rate_=RATE[rate])
    torch.cuda.synchronize()
    got = check_untouched(buf, flags, d_orig, orig, d_rec, rec, "padding")
    assert not got.any(), np.flatnonzero(got)
    # ... and a real difference in the last byte of a padded row still is
    bad = rec.copy()
    bad[M - 2, S - 1] ^= 0x40
    d_bad = view(torch, bad, pad, fill=0x5A)
    got = rs.verify_device(N, M, S, d_orig, d_bad, rate_=RATE[rate]).cpu().numpy()
    assert np.flatnonzero(got).tolist() == [M - 2]


def span_masks(rate, N, M):
    """The spans of tests/span_cases.py (the ends of the matrix, odd rows, the rows around n / 2, a
    pass level and, for LowRate's output chunks, the chunk boundaries, whole and partial chunks and
    rows inside them) as masks, every third row inside a span unselected."""
    forced = rate if rate != "default" else "high" if O.lib().orc_use_high_rate(N, M) == 1 else "low"
    return [SC.span_mask(M, lo, hi) for _, lo, hi in SC.spans(forced, N, M)]


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("rate,N,M,S", [("high", 70, 100, 64), ("default", 300, 500, 72), ("high", 1000, 100, 66),
                                        ("default", 4096, 4096, 64)] + SC.MASK_SHAPES, ids=lambda v: str(v))
def test_masks(torch, rs, rate, N, M, S, fused):
    """Unselected rows hold junk that differs and stay 0; the selected rows are right, those of a
    narrowed span with unselected rows inside it included; a mask that selects nothing gives
    all-zero flags and launches no kernel."""
    check_masks(torch, rs, rate, N, M, S, fused)


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("rate,N,M,S,mode", SC.MASK_SHAPES_MODE0, ids=lambda v: str(v))
def test_masks_on_the_pass_kernels(torch, rs, rate, N, M, S, mode, fused):
    """test_masks with the column kernels off: two pass levels over several chunks."""
    try:
        rs.mono_enable(mode)
        check_masks(torch, rs, rate, N, M, S, fused)
    finally:
        rs.mono_enable(True)


def check_masks(torch, rs, rate, N, M, S, fused):
    orig, rec = stripe(rate, N, M, S)
    rng = np.random.default_rng(M)
    rs.verify_set_fused(fused)
    d_orig = view(torch, orig, 0)
    span = np.zeros(M, np.uint8)  # a span in the middle with holes in it
    span[[M // 4, M // 4 + 1, M // 2, M - M // 4]] = 1
    one = np.zeros(M, np.uint8)
    one[M - 1] = 1
    most = np.ones(M, np.uint8)
    most[1::3] = 0
    # (the second `span`: the mask changes back)
    for mask in [span, one, most, np.ones(M, np.uint8), span] + span_masks(rate, N, M):
        sel = np.flatnonzero(mask)
        clean = rec.copy()  # the selected rows right, junk in the others
        clean[mask == 0] = rng.integers(0, 256, (int((mask == 0).sum()), S), dtype=np.uint8)
        hit = sorted({int(sel[0]), int(sel[len(sel) // 2]), int(sel[-1])})  # the span's two ends and a middle row
        bad = clean.copy()
        for k, j in enumerate(hit):
            bad[j, (11 * k) % S] ^= 0x20
        for held, want in ((clean, []), (bad, hit)):
            d_rec = view(torch, held, 0)
            flags, buf = guarded_flags(torch, (M,))
            rs.verify_device(N, M, S, d_orig, d_rec, recovery_rows=mask, d_mismatch=flags, rate_=RATE[rate])
            torch.cuda.synchronize()
            got = check_untouched(buf, flags, d_orig, orig, d_rec, held, "mask")
            assert np.flatnonzero(got).tolist() == want, (np.flatnonzero(got)[:8], want)
    # nothing selected
    d_rec = view(torch, rng.integers(0, 256, (M, S), dtype=np.uint8), 0)
    flags, buf = guarded_flags(torch, (M,))
    recs = profiled(torch, rs, lambda: rs.verify_device(N, M, S, d_orig, d_rec, recovery_rows=np.zeros(M, np.uint8),
                                                        d_mismatch=flags, rate_=RATE[rate]))
    assert recs == []
    h = buf.cpu().numpy()
    assert (h[:GUARD] == 0xFF).all() and (h[-GUARD:] == 0xFF).all() and not h[GUARD:-GUARD].any()


def batch_case(rate, N, M, S, B=3):
    """B stripes (3 by default), a different corruption in each of three neighbours, one of them clean."""
    kinds = (["middle", "none", "last"] * ((B + 2) // 3))[:B]
    parts = [corrupt(k, rate, N, M, S, seed=b) for b, k in enumerate(kinds)]
    return tuple(np.stack([p[i] for p in parts]) for i in range(3))


def padded_batch(torch, a, extra, pad=0):
    """[B, rows, S] on the device with `extra` junk rows after every stripe (stripe padding)."""
    B, rows, S = a.shape
    t = torch.full((B, rows + extra, S + pad), 0xC3, dtype=torch.uint8, device="cuda")
    v = t[:, :rows, :S]
    v.copy_(torch.from_numpy(a).cuda())
    return v


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("rate,N,M,S", [("high", 70, 100, 64), ("default", 1024, 1024, 72), ("high", 1000, 100, 66)],
                         ids=lambda v: str(v))
def test_batch(torch, rs, rate, N, M, S, fused):
    check_batch(torch, rs, rate, N, M, S, fused)


def check_batch(torch, rs, rate, N, M, S, fused, B=3, pad=0, singles=False):
    """test_batch's body; the launch names of the batch call.  (B, pad, singles:
    tests/test_gpu_wide_shards.py's -- more stripes, row padding, and every stripe's flags against a
    verify_device of that stripe alone.)"""
    origs, recs, wants = batch_case(rate, N, M, S, B)
    d_orig, d_rec = padded_batch(torch, origs, 2, pad), padded_batch(torch, recs, 3, pad)
    flags, buf = guarded_flags(torch, (B, M))
    rs.verify_set_fused(fused)
    names = [r[0] for r in profiled(torch, rs, lambda: rs.verify_device_batch(N, M, S, d_orig, d_rec, d_mismatch=flags,
                                                                              rate_=RATE[rate]))]
    got = check_untouched(buf, flags, d_orig, origs, d_rec, recs, "batch")
    for b in range(B):
        assert np.array_equal(got[b], wants[b]), (b, np.flatnonzero(got[b])[:8], np.flatnonzero(wants[b])[:8])
        if singles:
            alone = rs.verify_device(N, M, S, d_orig[b], d_rec[b], rate_=RATE[rate]).cpu().numpy()
            assert np.array_equal(alone, got[b]), f"stripe {b} alone: {np.flatnonzero(alone)[:8]}"
    # one mask for every stripe, and a tensor the call allocates itself
    mask = np.ones(M, np.uint8)
    mask[M // 2] = 0
    got = rs.verify_device_batch(N, M, S, d_orig, d_rec, recovery_rows=mask, rate_=RATE[rate])
    assert got.shape == (B, M) and str(got.dtype) == "torch.uint8" and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), wants * mask)
    return names


def test_launches(torch, rs):
    """A fused call, single and batch, is exactly one record named k_mono_verify<...> that counts
    (N + rows compared) x packs x 8 x stripes bytes; an unfused call ends with k_verify_rows."""
    rate, N, M, S = "default", 1024, 1024, 64
    orig, rec = stripe(rate, N, M, S)
    d_orig, d_rec = view(torch, orig, 0), view(torch, rec, 0)
    origs, recs, _ = batch_case(rate, N, M, S)
    b_orig, b_rec = view(torch, origs, 0), view(torch, recs, 0)
    mask = np.zeros(M, np.uint8)
    mask[100:400:2] = 1
    packs = S // 8
    rs.verify_set_fused(1)
    for fn, rows, stripes in ((lambda: rs.verify_device(N, M, S, d_orig, d_rec), M, 1),
                              (lambda: rs.verify_device(N, M, S, d_orig, d_rec, recovery_rows=mask), 150, 1),
                              (lambda: rs.verify_device_batch(N, M, S, b_orig, b_rec), M, 3)):
        got = profiled(torch, rs, fn)
        assert len(got) == 1 and got[0][0].startswith("k_mono_verify<10, "), got
        assert got[0][2] == (N + rows) * packs * 8 * stripes, got
    rs.verify_set_fused(0)
    got = profiled(torch, rs, lambda: rs.verify_device_batch(N, M, S, b_orig, b_rec))
    assert [r[0] for r in got][-1] == "k_verify_rows" and len(got) == 2, got  # the batch encode is one launch
    got = profiled(torch, rs, lambda: rs.verify_device(4096, 4096, 64, *(view(torch, x, 0) for x in
                                                                        stripe("default", 4096, 4096, 64))))
    assert got[-1][0] == "k_verify_rows" and len(got) >= 2, got


@pytest.mark.parametrize("fused", [1, 0])
def test_verifies_in_flight(torch, rs, fused):
    """Two verifies of different stripes back to back on one stream with two flag arrays, two on
    two streams, and an encode_device between two verifies."""
    rate, N, M, S = "default", 200, 200, 72
    rs.verify_set_fused(fused)
    oa, ra, wa = corrupt("middle", rate, N, M, S)
    ob, rb, wb = corrupt("last", rate, N, M, S)
    d = [view(torch, x, 0) for x in (oa, ra, ob, rb)]
    fa, fb = torch.full((M,), 0xFF, dtype=torch.uint8, device="cuda"), torch.full((M,), 0xFF, dtype=torch.uint8, device="cuda")
    mask = np.ones(M, np.uint8)
    mask[0] = 0  # (a mask on the second call only: the selection travels between the two)
    torch.cuda.synchronize()
    rs.verify_device(N, M, S, d[0], d[1], d_mismatch=fa)
    rs.verify_device(N, M, S, d[2], d[3], recovery_rows=mask, d_mismatch=fb)
    torch.cuda.synchronize()
    assert np.array_equal(fa.cpu().numpy(), wa) and np.array_equal(fb.cpu().numpy(), wb * mask)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    fa.fill_(0xFF), fb.fill_(0xFF)
    torch.cuda.synchronize()
    rs.verify_device(N, M, S, d[0], d[1], d_mismatch=fa, stream=s1)
    rs.verify_device(N, M, S, d[2], d[3], d_mismatch=fb, stream=s2)
    torch.cuda.synchronize()
    assert np.array_equal(fa.cpu().numpy(), wa) and np.array_equal(fb.cpu().numpy(), wb)
    rs.release_stream_scratch(s1)
    rs.release_stream_scratch(s2)
    # an encode of the same shape between two verifies: undisturbed, and its output verifies clean
    _, rec = stripe(rate, N, M, S)
    d_enc = torch.zeros((M, S), dtype=torch.uint8, device="cuda")
    f1 = rs.verify_device(N, M, S, d[0], d[1])
    rs.encode_device(N, M, S, d[0], d_enc)
    f2 = rs.verify_device(N, M, S, d[0], d_enc)
    torch.cuda.synchronize()
    assert np.array_equal(d_enc.cpu().numpy(), rec)
    assert np.array_equal(f1.cpu().numpy(), wa) and not f2.cpu().numpy().any()


@pytest.mark.parametrize("fused", [1, 0])
def test_scrub(torch, rs, fused):
    """Verify a batch, feed the flags to repair_device_batch_masks as absent rows, verify again."""
    rate, N, M, S, B = "high", 70, 100, 64, 3
    rs.verify_set_fused(fused)
    pairs = [stripe(rate, N, M, S, seed=b) for b in range(B)]
    origs, recs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    bad = recs.copy()
    bad[1, 17, 40] ^= 0x08
    bad[1, 93, 3] ^= 0x80
    d_orig, d_rec = view(torch, origs, 0), view(torch, bad, 0)
    flags = rs.verify_device_batch(N, M, S, d_orig, d_rec, rate_=RATE[rate]).cpu().numpy()
    assert [np.flatnonzero(f).tolist() for f in flags] == [[], [17, 93], []]
    rs.repair_device_batch_masks(N, M, S, d_orig, np.ones((B, N), np.uint8), d_rec, 1 - flags, d_orig, d_rec,
                                 rate_=RATE[rate])
    again = rs.verify_device_batch(N, M, S, d_orig, d_rec, rate_=RATE[rate]).cpu().numpy()
    assert not again.any()
    assert np.array_equal(d_rec.cpu().numpy(), recs) and np.array_equal(d_orig.cpu().numpy(), origs)
