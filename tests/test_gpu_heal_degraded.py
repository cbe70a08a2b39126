"""GPU: rs_heal_device_degraded* -- the degraded locate that also writes the correction.

Expected values are constructed, not computed by the code under test: a clean stripe comes from the
CPU oracle, originals are declared missing (their rows then hold junk), bytes are flipped.  Every
result -- d_located, the WHOLE flag array, d_action and all three matrices -- must equal
tests/heal_degraded_model.py, the numpy statement of the contract on the oracle's decode and
encode, and the status each case is meant to show is asserted on the model first.  Every run also
checks that nothing else was written: the row padding, the guard rows around the three matrices and
the guards around d_located, the flags and d_action are as before, present rows of a separate
d_restored keep their poison, and the three outputs, pre-filled with 0xFF, come back fully defined.
"""
import numpy as np
import pytest

import heal_degraded_model as HDM
import heal_model as HM
import locate_degraded_model as DM
import test_gpu_locate_degraded as LD
import test_gpu_verify as V

pytestmark = pytest.mark.gpu

RATE = V.RATE
GUARD = V.GUARD
CLEAN, ROWS, UNKNOWN = DM.CLEAN, DM.ROWS, DM.UNKNOWN
ORIGINAL, RECOVERY = HDM.ORIGINAL, HDM.RECOVERY

# the degraded locate's shapes: a batch decodes as one launch everywhere but at 4096:4096 (the pass
# kernels, stripe by stripe) and 3:5 (the single fused pass)
SHAPES = [("default", 3, 5), ("high", 70, 100), ("low", 100, 70), ("default", 200, 200), ("default", 1024, 1024),
          ("high", 1000, 100), ("low", 128, 1024), ("default", 4096, 4096)]
LAYOUTS = LD.LAYOUTS  # (64, 0), (72, 0), (66, 4): whole blocks; a tail; a tail on the byte-wise path
MISSING = ["first", "last", "scattered", "most", "third"]
FORMS = ["separate", "alias"]  # d_restored: a buffer of its own, d_original itself
MODES = [ORIGINAL, RECOVERY, ORIGINAL | RECOVERY]


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


def pattern(kind, N, M):
    """(original_present [N], recovery mask or None).  "most": as many originals missing as a
    heal can take, m = c - 3, under a mask of exactly m + 3 rows -- more restored rows than check
    rows wherever m > 3.  "third": the scattered set under a mask with every third row out."""
    if kind == "third":
        return LD.pattern("scattered", N, M)[0], LD.third_mask(M)
    if kind != "most":
        return LD.pattern(kind, N, M)
    present = np.ones(N, np.uint8)
    present[np.linspace(0, N - 1, min(N, M - 3)).round().astype(int)] = 0
    m = int((present == 0).sum())
    mask = None
    if m + 3 < M:
        mask = np.zeros(M, np.uint8)
        mask[np.linspace(0, M - 1, m + 3).round().astype(int)] = 1
        assert int(mask.sum()) == m + 3
    return present, mask


def cases(rate, N, M, S, present, mask, wide=False):
    """[(name, originals, recovery, intended status, max_rows values)] of one stripe under the two
    masks.  Absent originals hold junk in every case, and so do unselected recovery rows.  wide: the
    positional cases of tests/test_gpu_locate_degraded.py's cases, max_rows 0."""
    if wide:
        return [c + ([0],) for c in LD.cases(rate, N, M, S, present, mask, wide=True)]
    orig, rec = (x.copy() for x in V.stripe(rate, N, M, S))
    pb, R, K = DM.split(present, mask, M)
    rng = np.random.default_rng(N * 7 + M + S + len(R))
    orig[~pb] = rng.integers(0, 256, (len(R), S), dtype=np.uint8)
    if mask is not None:
        unsel = np.asarray(mask) == 0
        rec[unsel] ^= rng.integers(1, 256, (int(unsel.sum()), S), dtype=np.uint8)
    have = np.flatnonzero(pb)
    out = [("clean", orig, rec, CLEAN, [0])]
    if len(have):
        bad = orig.copy()
        bad[have[0], 0] ^= 0x01  # one bit in byte 0
        out.append((f"original {have[0]} bit0", bad, rec, int(have[0]), [0]))
        bad = orig.copy()
        bad[have[-1], S - 1] ^= 0x80  # one bit in the tail's last high byte
        out.append((f"original {have[-1]} lastbit", bad, rec, int(have[-1]), [0]))
        bad = orig.copy()
        bad[have[len(have) // 2]] ^= rng.integers(1, 256, S, dtype=np.uint8)  # the whole shard
        out.append((f"original {have[len(have) // 2]} shard", bad, rec, int(have[len(have) // 2]), [0]))
    bad = rec.copy()
    bad[R[0], S // 2] ^= 0x10
    out.append((f"reference row {R[0]}", orig, bad, N + int(R[0]), [0]))
    bad = rec.copy()
    bad[R[-1]] ^= rng.integers(1, 256, S, dtype=np.uint8)  # the whole shard
    out.append((f"reference row {R[-1]} shard", orig, bad, N + int(R[-1]), [0]))
    # two check rows: the threshold below the count of differing rows, at it and above it
    bad = rec.copy()
    bad[K[-1], 5 % S] ^= 0x20
    bad[K[0], S - 1] ^= 0x80
    out.append((f"check rows {K[0]}, {K[-1]}", orig, bad, ROWS, [1, 2, 7]))
    # an information shard plus a check row; two information shards in different columns (each
    # column names another position, so no single one explains the stripe)
    bo, br = orig.copy(), rec.copy()
    if len(have):
        bo[have[len(have) // 2], 0] ^= 0x04
    else:
        br[R[len(R) // 2], 0] ^= 0x04
    br[K[0], S // 2] ^= 0x40
    out.append(("information shard and check row", bo, br, UNKNOWN, [M]))
    bo, br = orig.copy(), rec.copy()
    if len(have) >= 2:
        bo[have[0], 0] ^= 0x10
        bo[have[-1], S - 1] ^= 0x20
    elif len(have) == 1:
        bo[have[0], 0] ^= 0x10
        br[R[0], S - 1] ^= 0x20
    else:
        br[R[0], 0] ^= 0x10
        br[R[-1], S - 1] ^= 0x20
    out.append(("two information shards", bo, br, UNKNOWN, [M]))
    return out


def data_of(buf, rows, S):
    """(the data region [.., rows, S] of a padded(.., guard_rows=1) buffer on the host, the rest of
    the buffer with that region zeroed)."""
    image = buf.cpu().numpy()
    data = image[..., 1:rows + 1, :S].copy()
    image[..., 1:rows + 1, :S] = 0
    return data, image


def rest_of(a, pad, fill):
    image = LD.host_image(a, pad, fill=fill, guard_rows=1)
    image[..., 1:a.shape[-2] + 1, :a.shape[-1]] = 0
    return image


def heal(torch, rs, rate, N, M, S, orig, present, rec, pad=0, mask=None, form="separate", mode=3, max_rows=0,
         what="", stream=None):
    """One call (a batch when orig is 3-D) on fresh device copies; (located, flags, action, the
    originals, the recovery rows, the restored matrix or None when aliased, the device tensors) on
    the host, after every "nothing outside the matrices was written" check."""
    batch = orig.ndim == 3
    d_orig, orig_buf = LD.padded(torch, orig, pad, guard_rows=1)
    d_rec, rec_buf = LD.padded(torch, rec, pad, guard_rows=1)
    lead = orig.shape[:-2]
    loc, loc_buf = LD.guarded(torch, lead if batch else (1,), torch.int32)
    flags, flag_buf = LD.guarded(torch, lead + (M,), torch.uint8)
    action, action_buf = LD.guarded(torch, lead if batch else (1,), torch.uint8)
    if form == "separate":  # poison everywhere: present rows, padding and the guard rows keep it
        d_restored, res_buf = LD.padded(torch, np.full(orig.shape, 0xEE, np.uint8), pad, fill=0xEE, guard_rows=1)
    else:
        d_restored, res_buf = d_orig, None
    call = rs.heal_device_degraded_batch if batch else rs.heal_device_degraded
    call(N, M, S, d_orig, present, d_rec, d_restored, recovery_rows=mask, mode=mode, max_rows=max_rows, d_located=loc,
         d_mismatch=flags, d_action=action, rate_=RATE[rate], stream=stream)
    torch.cuda.synchronize()
    got, got_flags = LD.check_outputs(loc_buf, flag_buf, what)
    a = action_buf.cpu().numpy()
    assert (a[:GUARD] == 0xFF).all() and (a[-GUARD:] == 0xFF).all(), what + ": a byte outside d_action was written"
    assert (a[GUARD:-GUARD] <= 2).all(), what + ": an action is not defined"
    o_after, o_rest = data_of(orig_buf, N, S)
    r_after, r_rest = data_of(rec_buf, M, S)
    assert np.array_equal(o_rest, rest_of(orig, pad, 0xC3)), what + ": d_original's padding or guard rows were written"
    assert np.array_equal(r_rest, rest_of(rec, pad, 0xC3)), what + ": d_recovery's padding or guard rows were written"
    x_after = None
    if res_buf is not None:
        x_after, x_rest = data_of(res_buf, N, S)
        assert np.array_equal(x_rest, rest_of(np.full(orig.shape, 0xEE, np.uint8), pad, 0xEE)), \
            what + ": d_restored's padding or guard rows were written"
    return (got, got_flags.reshape(lead + (M,)), a[GUARD:-GUARD], o_after, r_after, x_after,
            (d_orig, d_rec, d_restored))


def expected(rate, orig, present, rec, mask, form, mode, max_rows, base):
    """The model's (located, flags, action, originals, recovery, restored or None) of one stripe
    for a form of d_restored."""
    pb = np.asarray(present) != 0
    if form == "separate":
        return HDM.heal(rate, orig, present, rec, np.full(orig.shape, 0xEE, np.uint8), mask, mode, max_rows, base)
    loc, flags, action, o, r, x = HDM.heal(rate, orig, present, rec, orig, mask, mode, max_rows, base)
    return loc, flags, action, np.where(pb[:, None], o, x), r, None


def compare(what, got, want):
    loc, flags, action, o, r, x = got[:6]
    wloc, wflags, waction, wo, wr, wx = want
    assert np.array_equal(flags, wflags), \
        f"{what}: flagged rows {np.flatnonzero(flags).tolist()[:8]}, want {np.flatnonzero(wflags).tolist()[:8]}"
    assert int(loc[0]) == wloc, f"{what}: located {int(loc[0])}, want {wloc}"
    assert int(action[0]) == waction, f"{what}: action {int(action[0])}, want {waction}"
    for name, a, b in (("d_original", o, wo), ("d_recovery", r, wr), ("d_restored", x, wx)):
        if b is not None:
            rows = np.flatnonzero((a != b).any(axis=1)).tolist()
            assert not rows, f"{what}: {name} differs from the model in rows {rows[:8]}"


def check_case(torch, rs, rate, N, M, S, pad, present, mask, name, orig, rec, intended, max_rows_list, modes=None):
    """(modes: the mode values to run, MODES by default.)"""
    pb = np.asarray(present) != 0
    clean_orig, clean_rec = V.stripe(rate, N, M, S)
    base = HDM.found(rate, orig, present, rec, mask)
    assert base[0] == intended, f"{name}: the model says {base[0]}, the case was built for {intended}"
    sel = np.ones(M, bool) if mask is None else np.asarray(mask) != 0
    for form in FORMS:
        for mode in modes or MODES:
            for max_rows in max_rows_list:
                what = (f"{rate} {N}:{M} x {S} pad {pad} m {int((~pb).sum())} {name} d_restored {form} mode {mode} "
                        f"max_rows {max_rows}")
                want = expected(rate, orig, present, rec, mask, form, mode, max_rows, base)
                got = heal(torch, rs, rate, N, M, S, orig, present, rec, pad, mask, form, mode, max_rows, what)
                compare(what, got, want)
                if intended == ROWS:  # (the case states what the threshold is meant to do)
                    assert want[2] == (RECOVERY if mode & RECOVERY and max_rows >= 2 else 0), what
                if intended < 0 or not want[2]:
                    continue
                # a healed located stripe: the constructed damage was the only damage, so the stripe
                # is the clean one; a verify under the call's mask flags nothing; a second heal is CLEAN
                d_orig, d_rec, d_restored = got[6]
                whole = got[3].copy()
                if form == "separate":
                    whole[~pb] = got[5][~pb]
                assert np.array_equal(whole, clean_orig), what + ": the healed originals are not the clean ones"
                assert np.array_equal(got[4][sel], clean_rec[sel]), what + ": the healed recovery rows are not the clean ones"
                if form == "separate":
                    miss = torch.from_numpy(np.flatnonzero(~pb)).cuda()
                    d_orig[miss] = d_restored[miss]
                bad = rs.verify_device(N, M, S, d_orig, d_rec, recovery_rows=mask, rate_=RATE[rate])
                assert not bad.cpu().numpy().any(), what + ": a selected row disagrees after the heal"
                again = rs.heal_device_degraded(N, M, S, d_orig, present, d_rec, d_restored, recovery_rows=mask,
                                                mode=mode, max_rows=max_rows, rate_=RATE[rate])
                torch.cuda.synchronize()
                assert [int(t.cpu()[0]) for t in (again[0], again[2])] == [CLEAN, 0] and not again[1].cpu().numpy().any(), what
                assert np.array_equal(d_restored.cpu().numpy()[~pb], clean_orig[~pb]), what + ": the second heal's rows"


def _shape_params():
    out = []
    for rate, N, M in SHAPES:
        for S, pad in (LAYOUTS if N != 4096 else LAYOUTS[:1]):
            for kind in MISSING:
                out.append(pytest.param(rate, N, M, S, pad, kind, id=f"{rate}-{N}-{M}-{S}-{pad}-{kind}"))
    return out


@pytest.mark.parametrize("rate,N,M,S,pad,kind", _shape_params())
def test_shapes(torch, rs, rate, N, M, S, pad, kind):
    present, mask = pattern(kind, N, M)
    if kind == "most" and N > 3:  # more restored rows than check rows: m drives the kernel's row groups
        _, R, K = DM.split(present, mask, M)
        assert len(K) == 3 and len(R) > len(K), (N, M)
    for name, orig, rec, intended, max_rows_list in cases(rate, N, M, S, present, mask):
        check_case(torch, rs, rate, N, M, S, pad, present, mask, name, orig, rec, intended, max_rows_list)


@pytest.mark.parametrize("rate,N,M,S,B,pad,form", [("high", 70, 100, 66, 8, 4, "alias"),
                                                   ("high", 70, 100, 72, 6, 0, "separate"),
                                                   ("default", 4096, 4096, 64, 5, 0, "alias")], ids=lambda v: str(v))
def test_batch(torch, rs, rate, N, M, S, B, pad, form):
    """A one-launch shape and the stripe-by-stripe shape, a different outcome in each stripe: the
    model's results, which are also those of a loop of single calls."""
    present, _ = LD.pattern("scattered", N, M)
    mask = LD.third_mask(M)
    origs, recs, want_loc, _, _ = LD.batch_case(rate, N, M, S, B, present, mask)
    mode, max_rows = ORIGINAL | RECOVERY, 1
    got = heal(torch, rs, rate, N, M, S, origs, present, recs, pad, mask, form, mode, max_rows, "batch")
    assert got[0].tolist() == want_loc.tolist(), (got[0], want_loc)
    actions = []
    for b in range(B):
        base = HDM.found(rate, origs[b], present, recs[b], mask)
        want = expected(rate, origs[b], present, recs[b], mask, form, mode, max_rows, base)
        one = [got[0][b:b + 1], got[1][b], got[2][b:b + 1], got[3][b], got[4][b], None if got[5] is None else got[5][b]]
        compare(f"batch stripe {b}", one, want)
        single = heal(torch, rs, rate, N, M, S, origs[b], present, recs[b], pad, mask, form, mode, max_rows, f"stripe {b}")
        compare(f"single stripe {b}", single, want)
        actions.append(want[2])
    assert actions[:5] == [ORIGINAL, 0, RECOVERY, RECOVERY, 0]  # orig, clean, check, ref, two
    # stripe padding, tensors the call allocates itself, and the launches: one of each kernel where
    # the batch repair is one launch, else stripe by stripe
    d_orig, d_rec = V.padded_batch(torch, origs, 2, pad), V.padded_batch(torch, recs, 3, pad)
    d_res = V.padded_batch(torch, np.full(origs.shape, 0xEE, np.uint8), 1, pad)
    out = []
    names = [r[0] for r in V.profiled(torch, rs, lambda: out.extend(rs.heal_device_degraded_batch(
        N, M, S, d_orig, present, d_rec, d_res, recovery_rows=mask, mode=mode, max_rows=max_rows, rate_=RATE[rate])))]
    l2, f2, a2 = out
    assert l2.shape == (B,) and str(l2.dtype) == "torch.int32" and f2.shape == (B, M) and l2.is_cuda
    assert a2.shape == (B,) and str(a2.dtype) == "torch.uint8" and a2.is_cuda
    assert l2.cpu().numpy().tolist() == want_loc.tolist() and a2.cpu().numpy().tolist() == actions
    assert np.array_equal(f2.cpu().numpy(), got[1])
    pb = present != 0
    assert (d_res.cpu().numpy()[:, pb] == 0xEE).all()
    if form == "separate":
        assert np.array_equal(d_res.cpu().numpy()[:, ~pb], got[5][:, ~pb])
        assert np.array_equal(d_orig.cpu().numpy(), got[3])
    assert np.array_equal(d_rec.cpu().numpy(), got[4])
    count = names.count("k_heal_degraded")
    assert count == names.count("k_locate_find") == names.count("k_locate_confirm") == names.count("k_verify_rows") \
        == names.count("k_locate_rename")
    assert count == {70: 1, 4096: B}[N], names


@pytest.mark.parametrize("rate,N,M,S,pad", [("high", 70, 100, 66, 4), ("default", 1024, 1024, 64, 0),
                                            ("default", 3, 5, 72, 0)], ids=lambda v: str(v))
def test_nothing_missing_is_the_heal(torch, rs, rate, N, M, S, pad):
    """m = 0: every output is heal_device_batch's, d_restored is untouched."""
    B = 4
    pairs = [V.stripe(rate, N, M, S, seed=b) for b in range(B)]
    origs, recs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    origs[1, N - 1, S - 1] ^= 0x80
    recs[2, M // 2, 0] ^= 1
    origs[3, 0, 0] ^= 1
    recs[3, 1, 1] ^= 1
    present = np.ones(N, np.uint8)
    for mask in (None, LD.third_mask(M)):
        got = heal(torch, rs, rate, N, M, S, origs, present, recs, pad, mask, "separate", 3, 1, "m = 0")
        d_orig, d_rec = V.padded_batch(torch, origs, 0, pad), V.padded_batch(torch, recs, 0, pad)
        l, f, a = rs.heal_device_batch(N, M, S, d_orig, d_rec, recovery_rows=mask, mode=3, max_rows=1, rate_=RATE[rate])
        torch.cuda.synchronize()
        assert np.array_equal(got[0], l.cpu().numpy()) and np.array_equal(got[1], f.cpu().numpy())
        assert np.array_equal(got[2], a.cpu().numpy())
        assert np.array_equal(got[3], d_orig.cpu().numpy()) and np.array_equal(got[4], d_rec.cpu().numpy())
        model = [HM.heal(rate, origs[b], recs[b], mask=mask, mode=3, max_rows=1) for b in range(B)]
        assert got[0].tolist() == [m[0] for m in model] and got[2].tolist() == [m[2] for m in model]
        if mask is None:
            assert got[0].tolist()[:3] == [CLEAN, N - 1, ROWS] and got[2].tolist()[:3] == [0, ORIGINAL, RECOVERY]
        assert (got[5] == 0xEE).all()


def test_errors_through_the_wrapper(torch, rs):
    """With a real context: c < m is NotEnoughShards with the decode's counts, c = m .. m + 2 are
    rejected, and nothing is written."""
    N, M, S = 8, 7, 64
    orig, rec = V.stripe("default", N, M, S)
    d_orig, d_rec = V.view(torch, orig, 0), V.view(torch, rec, 0)
    loc, loc_buf = LD.guarded(torch, (1,), torch.int32)
    flags, flag_buf = LD.guarded(torch, (M,), torch.uint8)
    action, action_buf = LD.guarded(torch, (1,), torch.uint8)
    present = [1, 0, 1, 1, 0, 1, 0, 1]  # m = 3
    kw = dict(d_located=loc, d_mismatch=flags, d_action=action)
    with pytest.raises(rs.NotEnoughShards) as e:
        rs.heal_device_degraded(N, M, S, d_orig, present, d_rec, d_orig, recovery_rows=[1, 0, 0, 1, 0, 0, 0], **kw)
    assert (e.value.original_count, e.value.original_received_count, e.value.recovery_received_count) == (N, 5, 2)
    for few in ([1, 1, 1, 0, 0, 0, 0], [1, 1, 0, 1, 0, 1, 0], [1, 1, 0, 1, 0, 1, 1]):
        with pytest.raises(ValueError, match="recovery_rows: 3 missing"):
            rs.heal_device_degraded(N, M, S, d_orig, present, d_rec, d_orig, recovery_rows=few, **kw)
    torch.cuda.synchronize()
    assert (loc_buf.cpu().numpy() == -1).all() and (flag_buf.cpu().numpy() == 0xFF).all()
    assert (action_buf.cpu().numpy() == 0xFF).all()
    assert np.array_equal(d_orig.cpu().numpy(), orig) and np.array_equal(d_rec.cpu().numpy(), rec)
    got = rs.heal_device_degraded(N, M, S, d_orig, present, d_rec, d_orig, recovery_rows=[1, 1, 1, 0, 1, 1, 1], **kw)
    assert int(got[0].cpu()[0]) == CLEAN and int(got[2].cpu()[0]) == 0
    assert np.array_equal(d_orig.cpu().numpy(), orig)


def test_tables_and_launches(torch, rs):
    """A cold heal adds exactly one k_coef_log_rows per slab to the cold degraded locate's
    launches; a warm one launches the repair's kernels, k_verify_rows, k_locate_find,
    k_locate_confirm, k_heal_degraded and k_locate_rename, and nothing else; a degraded locate
    after a heal builds no table; a cold degraded locate launches what it did; a heal after a
    degraded locate builds both tables again."""
    rate, N, M, S = "default", 300, 500, 72
    orig, rec = V.stripe(rate, N, M, S)
    present, _ = LD.pattern("scattered", N, M)
    pb = present != 0
    bad = orig.copy()
    bad[~pb] = 0x77
    bad[N - 1, 1] ^= 0x40
    d_rec = V.view(torch, rec, 0)
    fresh = lambda: V.view(torch, bad, 0)
    d_bad = fresh()
    heal_ = lambda d: rs.heal_device_degraded(N, M, S, d, present, d_rec, d, mode=3, max_rows=4)
    locate = lambda d: rs.locate_device_degraded(N, M, S, d, present, d_rec)
    rs.release_stream_scratch()
    first = V.profiled(torch, rs, lambda: heal_(d_bad))
    # two slabs of positions (256 + 44)
    assert LD.coef_launches(first) == ["k_coef_unit_degraded", "k_coef_log_slab", "k_coef_log_rows"] * 2, first
    whole = d_bad.cpu().numpy()
    assert np.array_equal(whole, orig)  # healed: original N - 1 and the three restored rows
    ref = np.zeros(M, np.uint8)
    ref[:3] = 1
    d_x, d_y = torch.zeros((N, S), dtype=torch.uint8, device="cuda"), torch.zeros((M, S), dtype=torch.uint8, device="cuda")
    repair = [r[0] for r in V.profiled(torch, rs, lambda: rs.repair_device(N, M, S, d_bad, present, d_rec, ref, d_x, d_y))]
    assert repair and not LD.coef_launches([(n,) for n in repair])
    tail = ["k_verify_rows", "k_locate_find", "k_locate_confirm", "k_heal_degraded", "k_locate_rename"]
    assert [r[0] for r in first][-len(repair) - 5:] == repair + tail
    d_bad = fresh()
    out = []
    second = V.profiled(torch, rs, lambda: out.extend(heal_(d_bad)))
    assert [r[0] for r in second] == repair + tail, second
    assert [int(out[0].cpu()[0]), int(out[2].cpu()[0])] == [N - 1, ORIGINAL] and np.array_equal(d_bad.cpu().numpy(), orig)
    # a degraded locate after a heal finds T, and launches what it always did
    d_bad = fresh()
    third = V.profiled(torch, rs, lambda: out.extend(locate(d_bad)))
    assert [r[0] for r in third] == repair + [t for t in tail if t != "k_heal_degraded"], third
    assert int(out[3].cpu()[0]) == N - 1
    # a cold degraded locate: its two launches per slab, as before this call existed
    rs.release_stream_scratch()
    cold = V.profiled(torch, rs, lambda: locate(d_bad))
    assert LD.coef_launches(cold) == ["k_coef_unit_degraded", "k_coef_log_slab"] * 2, cold
    assert LD.coef_launches(V.profiled(torch, rs, lambda: locate(d_bad))) == []
    # a heal after it builds both tables again, once
    again = V.profiled(torch, rs, lambda: heal_(d_bad))
    assert LD.coef_launches(again) == ["k_coef_unit_degraded", "k_coef_log_slab", "k_coef_log_rows"] * 2, again
    assert np.array_equal(d_bad.cpu().numpy(), orig)
    d_bad = fresh()
    assert LD.coef_launches(V.profiled(torch, rs, lambda: heal_(d_bad))) == []
    assert LD.coef_launches(V.profiled(torch, rs, lambda: locate(d_bad))) == []
    # another pattern rebuilds
    other, _ = LD.pattern("first", N, M)
    bad2 = orig.copy()
    bad2[0] = 0x11
    d_bad2 = V.view(torch, bad2, 0)
    assert len(LD.coef_launches(V.profiled(torch, rs, lambda: rs.heal_device_degraded(
        N, M, S, d_bad2, other, d_rec, d_bad2)))) == 6
    assert np.array_equal(d_bad2.cpu().numpy(), orig)
    rs.release_stream_scratch()


def test_calls_in_flight(torch, rs):
    """Two heals of different stripes and patterns on one stream with an encode between them, and
    two on two streams."""
    rate, N, M, S = "default", 200, 200, 72
    orig, rec = V.stripe(rate, N, M, S)
    pa, _ = LD.pattern("first", N, M)
    pbm, _ = LD.pattern("run", N, M)
    a, b = orig.copy(), orig.copy()
    a[0] = 0x33
    a[7, 0] ^= 1
    b[pbm == 0] = 0x44
    b[N - 2, S - 1] ^= 0x80
    mask = np.ones(M, np.uint8)
    mask[0] = 0  # (a mask on the second call only)
    d_rec = V.view(torch, rec, 0)
    d_enc = torch.zeros((M, S), dtype=torch.uint8, device="cuda")
    for streams in (None, "two"):
        d_a, d_b = V.view(torch, a, 0), V.view(torch, b, 0)
        s1, s2 = (torch.cuda.Stream(), torch.cuda.Stream()) if streams else (None, None)
        torch.cuda.synchronize()
        ra = rs.heal_device_degraded(N, M, S, d_a, pa, d_rec, d_a, stream=s1)
        if not streams:
            rs.encode_device(N, M, S, d_a, d_enc)  # (after the heal on the stream: the healed originals)
        rb = rs.heal_device_degraded(N, M, S, d_b, pbm, d_rec, d_b, recovery_rows=mask, stream=s2)
        torch.cuda.synchronize()
        assert (int(ra[0].cpu()[0]), int(rb[0].cpu()[0])) == (7, N - 2)
        assert (int(ra[2].cpu()[0]), int(rb[2].cpu()[0])) == (ORIGINAL, ORIGINAL)
        assert np.array_equal(d_a.cpu().numpy(), orig) and np.array_equal(d_b.cpu().numpy(), orig)
        if not streams:
            assert np.array_equal(d_enc.cpu().numpy(), rec)
        else:
            rs.release_stream_scratch(s1)
            rs.release_stream_scratch(s2)
