"""GPU: rs_update_device_batch_lists -- a batch of partial-stripe writes, one index list and one
recovery-row mask per stripe.

The reference of every test is the CPU oracle's encode of each stripe with its originals replaced
(tests/update_lists_cases.py), compared byte for byte over the whole recovery buffer: selected rows
must equal the oracle, and unselected rows, left-alone stripes, row and stripe padding and the
inputs must hold what they held before the call.
"""
import numpy as np
import pytest

import oracle_lib as O
import update_lists_cases as C

pytestmark = pytest.mark.gpu

RATE = C.RATE

# (rate, N, M, S, positional)
SHAPES = [
    ("default", 3, 2, 2, False),
    ("default", 100, 30, 64, False),
    ("default", 30, 100, 72, False),       # tail
    ("high", 1000, 100, 66, False),        # rows not 4-byte aligned: the byte-wise path
    ("default", 101, 30, 64, False),       # odd table pitch: the halfword select
    ("low", 128, 1024, 64, False),
    ("default", 1024, 1024, 1024, False),
    ("default", 70, 100, 2056, True),      # 257 packs: a second pack tile (tests/wide_cases.py)
    ("default", 4096, 4096, 64, False),    # the table at its bound, built by pass encodes
    ("default", 4100, 30, 64, False),      # beyond RS_LOCATE_MAX_ORIGINALS: stripe by stripe
]


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


def dev(torch, a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def check(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        at = tuple(int(x) for x in np.argwhere(got != want)[0])
        raise AssertionError(f"{what}: first difference at {at}: got {int(got[at]):#04x}, want {int(want[at]):#04x}")


def abi_call(rs, bt, max_count, junk_seed, d_old, d_new, d_rec, masks, packed):
    """rs_update_device_batch_lists itself, with max_count as given (the wrapper always passes the
    longest list): the index array is [stripes, max_count] with junk -- mostly out of range, and
    other junk for another seed -- in every entry past a stripe's count.  packed: d_old / d_new
    are dense [stripes, max_count, S] and go with stripe strides of 0, the max_count-row default."""
    import ctypes
    rng = np.random.default_rng([junk_seed, 99])
    index = rng.integers(0, 1 << 40, (bt.B, max_count), dtype=np.uint64)
    for b, idx in enumerate(bt.lists):
        index[b, :len(idx)] = idx
    counts = np.array([len(idx) for idx in bt.lists], np.uint32)
    m = None if masks is None else np.ascontiguousarray(np.asarray(masks) != 0, dtype=np.uint8)

    def strides(t):  # (row stride, stripe stride) in bytes
        if packed and t is not d_rec:
            assert t.is_contiguous() and t.shape[1] == max_count
            return 0, 0
        return t.stride(1), t.stride(0)

    (o_row, o_b) = (0, 0) if d_old is None else strides(d_old)
    (n_row, n_b), (r_row, r_b) = strides(d_new), strides(d_rec)
    err = rs._RsError()
    code = rs._lib.rs_update_device_batch_lists(
        rs.default_context().handle, RATE[bt.rate], bt.N, bt.M, bt.S, bt.B,
        index.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
        max_count, None if d_old is None else d_old.data_ptr(), o_row, o_b, d_new.data_ptr(), n_row, n_b,
        d_rec.data_ptr(), r_row, r_b, None if m is None else m.ctypes.data, None, ctypes.byref(err))
    assert code == 0, (code, err.index, err.got)


def run(torch, rs, bt, form="delta", masks=None, junk_seed=1, slack=2, direct_max=256, pads=(0, 0), held=None,
        packed=True):
    """One call on fresh device copies of batch `bt` (stripe and row padding `pads` round the recovery
    matrix); returns the recovery matrix after it.  The inputs and the padding must be untouched.
    slack > 0: through the C ABI with max_count = the longest list + slack (abi_call), d_old / d_new
    holding junk in their slack rows; slack == 0: through the Python wrapper."""
    h_old, h_new = bt.inputs(form, junk_seed, slack)
    d_old = None if h_old is None else dev(torch, h_old)
    d_new = dev(torch, h_new)
    d_rec, buf, covered = C.place(torch, bt.recs if held is None else held, 0, pads[0], pads[1])
    rs.update_set_direct_max(direct_max)
    if slack:
        abi_call(rs, bt, bt.K + slack, junk_seed, d_old, d_new, d_rec, masks, packed)
    else:
        rs.update_device_batch_lists(bt.N, bt.M, bt.S, bt.lists, d_old, d_new, d_rec, recovery_rows=masks,
                                     rate_=RATE[bt.rate])
    torch.cuda.synchronize()
    what = f"{bt.rate} {bt.N}:{bt.M} x {bt.S} {form} direct_max {direct_max}"
    assert C.untouched(buf, covered), what + ": recovery padding written"
    check(d_new.cpu().numpy(), h_new, what + ": d_new was written")
    if d_old is not None:
        check(d_old.cpu().numpy(), h_old, what + ": d_old was written")
    return d_rec.cpu().numpy()


@pytest.mark.parametrize("rate,N,M,S,positional", SHAPES, ids=lambda v: str(v))
def test_mixed_batch(torch, rs, rate, N, M, S, positional):
    bt = C.batch(rate, N, M, S, positional=positional)
    assert [len(x) for x in bt.lists][:2] == [1, 1] and bt.lists[5] == [] and bt.lists[6] == bt.lists[0]
    # max_count = the longest list + 2: larger than every count.  The delta form goes with stripe
    # strides of 0 (max_count rows per stripe by default), old/new with explicit ones
    for form, packed in (("delta", True), ("oldnew", False)):
        a = run(torch, rs, bt, form, junk_seed=1, pads=(4, 3 * (S + 4)), packed=packed)
        check(a, bt.wants, f"{rate} {N}:{M} x {S} {form}")
        check(a[5], bt.recs[5], "the empty stripe was written")
        # other junk in the slack rows and in the slack index entries
        b = run(torch, rs, bt, form, junk_seed=2, pads=(4, 3 * (S + 4)), packed=packed)
        check(b, a, f"{rate} {N}:{M} x {S} {form}: the slack rows changed the result")


@pytest.mark.parametrize("rate,N,M,S", [("default", 100, 30, 64), ("default", 30, 100, 72),
                                         ("default", 101, 30, 64), ("default", 1024, 1024, 1024)],
                         ids=lambda v: str(v))
def test_per_stripe_row_masks(torch, rs, rate, N, M, S):
    rng = np.random.default_rng(N)
    lists = [C.some_indices(N, k, rng) for k in (1, 3, 17, 2, 5, 16, 4)]  # stripe 4: the mask selects nothing
    bt = C.batch(rate, N, M, S, lists)
    masks = C.stripe_masks(bt.B, M)
    assert not masks[4].any() and masks[0].all()
    held, want = bt.masked(masks)
    for form in ("delta", "oldnew"):
        got = run(torch, rs, bt, form, masks=masks, held=held)
        check(got, want, f"{rate} {N}:{M} x {S} {form} masks")
    # no mask at all = every row of every stripe
    a = run(torch, rs, bt, masks=None)
    b = run(torch, rs, bt, masks=np.ones((bt.B, M), np.uint8))
    check(a, bt.wants, "no mask")
    check(b, a, "all-ones masks differ from no mask")


@pytest.mark.parametrize("rate,N,M,S", [("default", 30, 100, 72), ("default", 100, 30, 64)], ids=lambda v: str(v))
def test_routes_agree_with_a_loop_of_single_calls(torch, rs, rate, N, M, S):
    """direct_max 256: every stripe in the launch; 16: the count-17 stripe takes the loop; 0: every
    stripe re-encodes."""
    bt = C.batch(rate, N, M, S)
    masks = C.stripe_masks(bt.B, M)
    masks[4] = 1
    masks[4, ::2] = 0  # the count-17 stripe with a mask of its own
    held, want = bt.masked(masks)
    h_old, h_new = bt.inputs("oldnew", 1, 0)
    results = {}
    for direct_max in (256, rs.UPDATE_DIRECT_MAX_DEFAULT, 0):
        names = profiled(torch, rs, lambda: results.__setitem__(
            direct_max, run(torch, rs, bt, "oldnew", masks=masks, held=held, direct_max=direct_max)))
        check(results[direct_max], want, f"direct_max {direct_max}")
        lists_launches = sum(n.startswith("k_update_lists") for n in names)
        singles = sum(n.startswith("k_update<") for n in names)
        xors = names.count("k_rows_xor")
        # stripes with work: all but stripe 5, the empty list (every mask here selects something)
        work = [b for b in range(bt.B) if bt.lists[b] and masks[b].any()]
        if direct_max == 256:
            assert (lists_launches, singles, xors) == (1, 0, 0), names
        elif direct_max == 0:
            assert (lists_launches, singles, xors) == (0, 0, 2 * len(work)), names
        else:
            assert (lists_launches, singles) == (1, 0) and xors == 2, names  # count 17 > 16: re-encoded
    rs.update_set_direct_max(256)
    loop = held.copy()
    for b, idx in enumerate(bt.lists):
        if not idx:
            continue
        d_rec = dev(torch, held[b])
        rs.update_device(N, M, S, idx, dev(torch, h_old[b, :len(idx)]), dev(torch, h_new[b, :len(idx)]), d_rec,
                         recovery_rows=masks[b], rate_=RATE[rate])
        torch.cuda.synchronize()
        loop[b] = d_rec.cpu().numpy()
    for direct_max, got in results.items():
        check(got, loop, f"direct_max {direct_max} differs from the loop of update_device calls")


def test_one_list_for_all_stripes_equals_update_device_batch(torch, rs):
    rate, N, M, S = "default", 30, 100, 72
    idx = C.some_indices(N, 4, np.random.default_rng(3))
    bt = C.batch(rate, N, M, S, [idx] * 3)
    mask = np.ones(M, np.uint8)
    mask[::5] = 0
    for form in ("delta", "oldnew"):
        got = run(torch, rs, bt, form, masks=np.stack([mask] * 3), slack=0)
        h_old, h_new = bt.inputs(form, 1, 0)
        d_rec = dev(torch, bt.recs)
        rs.update_set_direct_max(256)
        rs.update_device_batch(N, M, S, idx, None if h_old is None else dev(torch, h_old), dev(torch, h_new), d_rec,
                               recovery_rows=mask)
        torch.cuda.synchronize()
        check(got, d_rec.cpu().numpy(), f"{form}: differs from update_device_batch")
        check(got[:, mask == 1], bt.wants[:, mask == 1], form)


def profiled(torch, rs, fn):
    rs.profile_enable(True)
    try:
        rs.profile_collect()
        fn()
        torch.cuda.synchronize()
        return [name for name, _, _ in rs.profile_collect()]
    finally:
        rs.profile_enable(False)


def test_launches(torch, rs):
    rate, N, M, S = "default", 100, 30, 64
    bt = C.batch(rate, N, M, S)
    h_old, h_new = bt.inputs("delta", 1, 0)
    d_new = dev(torch, h_new)
    rs.update_set_direct_max(256)

    def lists_call():
        d_rec = dev(torch, bt.recs)
        names = profiled(torch, rs, lambda: rs.update_device_batch_lists(N, M, S, bt.lists, None, d_new, d_rec))
        check(d_rec.cpu().numpy(), bt.wants, "lists call")
        return names

    def table_build(names):
        return sum(n == "k_coef_unit_slab" for n in names), sum(n == "k_coef_log_slab" for n in names)

    def only_the_launch(names):
        return len(names) == 1 and names[0].startswith("k_update_lists")

    rs.release_stream_scratch()
    cold = lists_call()
    assert table_build(cold) == (1, 1), cold  # one slab of originals: the locate table, once
    assert sum(n.startswith("k_update_lists") for n in cold) == 1 and cold[-1].startswith("k_update_lists"), cold
    assert not any(n in ("k_coef_unit", "k_coef_log") or n.startswith("k_update<") for n in cold), cold
    warm = lists_call()
    assert only_the_launch(warm), warm
    # the locate of the shape finds the table there ...
    orig, rec = C.stripe(rate, N, M, S)
    d_orig, d_rec1 = dev(torch, orig), dev(torch, rec)
    names = profiled(torch, rs, lambda: rs.locate_device(N, M, S, d_orig, d_rec1))
    assert table_build(names) == (0, 0), names
    # ... and the reverse: a locate builds it, the update after it builds nothing
    rs.release_stream_scratch()
    names = profiled(torch, rs, lambda: rs.locate_device(N, M, S, d_orig, d_rec1))
    assert table_build(names) == (1, 1), names
    assert only_the_launch(lists_call())
    # an update_device before and after keeps its own table
    idx = bt.lists[3]
    one = dev(torch, h_new[3, :len(idx)])

    def single():
        d = dev(torch, bt.recs[3])
        names = profiled(torch, rs, lambda: rs.update_device(N, M, S, idx, None, one, d))
        check(d.cpu().numpy(), bt.wants[3], "update_device")
        return names

    first = single()
    assert "k_coef_unit" in first and "k_coef_log" in first, first
    assert only_the_launch(lists_call())
    again = single()
    assert len(again) == 1 and again[0].startswith("k_update<"), again
    # after a release the table is rebuilt
    rs.release_stream_scratch()
    assert table_build(lists_call()) == (1, 1)
    # an all-empty batch launches nothing
    d_rec = dev(torch, bt.recs)
    names = profiled(torch, rs, lambda: rs.update_device_batch_lists(N, M, S, [[]] * 3 , None, d_new[:3], d_rec[:3]))
    assert names == [], names
    names = profiled(torch, rs, lambda: rs.update_device_batch_lists(
        N, M, S, bt.lists, None, d_new, d_rec, recovery_rows=np.zeros((bt.B, M), np.uint8)))
    assert names == [], names
    check(d_rec.cpu().numpy(), bt.recs, "a batch with nothing to change was written")


def test_more_than_one_launch_group(torch, rs):
    """65537 stripes of 3:2 x 2: two launch groups (65535 stripes each at the most), tiled from six
    (index list, delta) cases."""
    rate, N, M, S, B = "default", 3, 2, 2, 65537
    orig, rec = C.stripe(rate, N, M, S)
    cases = [[0], [1], [2], [2, 0], [1, 2], [0, 1]]
    deltas = np.zeros((6, 2, S), np.uint8)
    wants = np.zeros((6, M, S), np.uint8)
    for k, idx in enumerate(cases):
        new = O.generate_original(len(idx), S, 60 + k)
        mod = orig.copy()
        mod[idx] = new
        deltas[k, :len(idx)] = orig[idx] ^ new
        deltas[k, len(idx):] = 0xEE  # slack
        wants[k] = O.encode(rate, mod, M)
    assert len({w.tobytes() for w in wants}) == 6
    which = np.arange(B) % 6
    lists = [cases[k] for k in which]
    d_new = dev(torch, deltas[which])
    d_rec = dev(torch, np.repeat(rec[None], B, axis=0))
    rs.update_set_direct_max(rs.UPDATE_DIRECT_MAX_DEFAULT)
    names = profiled(torch, rs, lambda: rs.update_device_batch_lists(N, M, S, lists, None, d_new, d_rec))
    assert sum(n.startswith("k_update_lists") for n in names) == 2, names
    got = d_rec.cpu().numpy()
    for b in (65534, 65535, 65536):
        check(got[b], wants[b % 6], f"stripe {b}")
    check(got, wants[which], "65537 stripes")


@pytest.mark.parametrize("which", ["old", "new", "rec"])
@pytest.mark.parametrize("layout", ["unaligned", "padded", "stripe stride"])
def test_layouts(torch, rs, which, layout):
    """Each matrix in turn at base 1 mod 4 with rows of S + 2, with padded aligned rows, and with a
    stripe stride that is no multiple of 4 (the byte-wise path)."""
    base, row_pad, stripe_pad = {"unaligned": (1, 2, 0), "padded": (0, 64, 128), "stripe stride": (0, 0, 2)}[layout]
    for rate, N, M, S in (("default", 30, 100, 72), ("default", 100, 30, 64)):
        bt = C.batch(rate, N, M, S)
        masks = C.stripe_masks(bt.B, M)
        masks[4] = 1
        held, want = bt.masked(masks)
        h_old, h_new = bt.inputs("oldnew", 1, 1)
        lay = {w: ((base, row_pad, stripe_pad) if w == which else (0, 0, 0)) for w in ("old", "new", "rec")}
        d_old, b_old, c_old = C.place(torch, h_old, *lay["old"])
        d_new, b_new, c_new = C.place(torch, h_new, *lay["new"])
        d_rec, b_rec, c_rec = C.place(torch, held, *lay["rec"])
        rs.update_set_direct_max(256)
        rs.update_device_batch_lists(N, M, S, bt.lists, d_old, d_new, d_rec, recovery_rows=masks)
        torch.cuda.synchronize()
        what = f"{N}:{M} x {S} {which} {layout}"
        check(d_rec.cpu().numpy(), want, what)
        check(d_old.cpu().numpy(), h_old, what + ": d_old written")
        check(d_new.cpu().numpy(), h_new, what + ": d_new written")
        assert C.untouched(b_rec, c_rec) and C.untouched(b_old, c_old) and C.untouched(b_new, c_new), what


def test_calls_in_flight_and_other_calls(torch, rs):
    """Two calls with different lists and masks back to back on one stream, the second on top of the
    first, with an encode between them; the same two on two streams; then a decode from the updated
    recovery shards restores the new originals."""
    rate, N, M, S = "default", 100, 30, 64
    B = 3
    origs = np.stack([C.stripe(rate, N, M, S, b)[0] for b in range(B)])
    recs = np.stack([C.stripe(rate, N, M, S, b)[1] for b in range(B)])
    listsA, listsB = [[99, 7], [], [5]], [[0, 50, 3], [98], [6, 99]]
    maskA, maskB = np.ones((B, M), np.uint8), np.ones((B, M), np.uint8)
    maskA[2, 1::2] = 0
    maskB[0, ::3] = 0

    def deltas(lists, seed):
        K = max(len(x) for x in lists)
        d = np.zeros((B, K, S), np.uint8)
        mods = origs.copy()
        for b, idx in enumerate(lists):
            if idx:
                new = O.generate_original(len(idx), S, seed + b)
                d[b, :len(idx)] = origs[b][idx] ^ new
                mods[b][idx] = new
        return d, mods

    dA, modA = deltas(listsA, 40)
    dB, modB = deltas(listsB, 50)
    encA = np.stack([O.encode(rate, modA[b], M) for b in range(B)])
    encB = np.stack([O.encode(rate, modB[b], M) for b in range(B)])
    # the update is linear: after A (masked) then B (masked) row j of stripe b holds rec ^ (A's change) ^ (B's)
    wantA = np.where(maskA[:, :, None] != 0, encA, recs)
    wantB = np.where(maskB[:, :, None] != 0, encB, recs)
    both = wantA ^ wantB ^ recs
    rs.update_set_direct_max(rs.UPDATE_DIRECT_MAX_DEFAULT)
    d_dA, d_dB = dev(torch, dA), dev(torch, dB)
    d_orig0 = dev(torch, origs[0])
    d_enc = torch.zeros((M, S), dtype=torch.uint8, device="cuda")
    d_rec = dev(torch, recs)
    torch.cuda.synchronize()
    rs.update_device_batch_lists(N, M, S, listsA, None, d_dA, d_rec, recovery_rows=maskA)
    rs.encode_device(N, M, S, d_orig0, d_enc)
    rs.update_device_batch_lists(N, M, S, listsB, None, d_dB, d_rec, recovery_rows=maskB)
    torch.cuda.synchronize()
    check(d_rec.cpu().numpy(), both, "one stream")
    check(d_enc.cpu().numpy(), recs[0], "the encode between the two calls")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    r1, r2 = dev(torch, recs), dev(torch, recs)
    torch.cuda.synchronize()
    rs.update_device_batch_lists(N, M, S, listsA, None, d_dA, r1, recovery_rows=maskA, stream=s1)
    rs.encode_device(N, M, S, d_orig0, d_enc, stream=s1)
    rs.update_device_batch_lists(N, M, S, listsB, None, d_dB, r2, recovery_rows=maskB, stream=s2)
    torch.cuda.synchronize()
    check(r1.cpu().numpy(), wantA, "stream 1")
    check(r2.cpu().numpy(), wantB, "stream 2")
    rs.release_stream_scratch(s1)
    rs.release_stream_scratch(s2)
    # decode from stripe 0's updated recovery shards (no mask: every row follows)
    d_rec = dev(torch, recs)
    rs.update_device_batch_lists(N, M, S, listsB, None, d_dB, d_rec)
    idx = listsB[0]
    op = np.ones(N, np.uint8)
    op[idx] = 0
    lost = origs[0].copy()
    lost[idx] = 0xA5
    d_out = torch.zeros((N, S), dtype=torch.uint8, device="cuda")
    rs.decode_device(N, M, S, dev(torch, lost), op, d_rec[0], np.ones(M, np.uint8), d_out)
    torch.cuda.synchronize()
    check(d_out.cpu().numpy()[idx], modB[0][idx], "decode after the update")
