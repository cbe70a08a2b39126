"""GPU: rs_locate_device_degraded* -- the locate of a stripe with missing originals.

Expected values are constructed, not computed by the code under test: a clean stripe comes from the
CPU oracle, originals are declared missing (their rows then hold junk), bytes are flipped.  Every
result -- d_located, the WHOLE flag array and the restored originals -- must equal
tests/locate_degraded_model.py, the numpy statement of the contract on the oracle's decode and
encode, and the status each case is meant to show is asserted on the model first.  Every run also
checks that nothing else was written: the inputs equal their host copies (row padding included),
the guards around d_located, the flags and d_restored are as before, present rows of d_restored keep
their poison, and both outputs, pre-filled with 0xFF, come back fully defined.
"""
import numpy as np
import pytest

import locate_degraded_model as DM
import locate_model as LM
import oracle_lib as O
import test_gpu_verify as V
import wide_cases as W

pytestmark = pytest.mark.gpu

RATE = V.RATE
GUARD = V.GUARD
CLEAN, ROWS, UNKNOWN = DM.CLEAN, DM.ROWS, DM.UNKNOWN

# (rate, N, M): the decode is the fused column kernel (70:100, 100:70, 200:200, 1024:1024, 1000:100,
# 128:1024: a batch is one launch), the pass kernels (4096:4096) or the single fused pass (3:5)
SHAPES = [("high", 70, 100), ("low", 100, 70), ("default", 200, 200), ("default", 1024, 1024),
          ("default", 4096, 4096), ("high", 1000, 100), ("low", 128, 1024), ("default", 3, 5)]
# (S, row padding): whole blocks; a tail; a tail with rows that are not 4-byte aligned (byte-wise)
LAYOUTS = [(64, 0), (72, 0), (66, 4)]
MISSING = ["first", "middle", "last", "run", "scattered", "most"]
FORMS = ["none", "separate", "alias"]  # d_restored: NULL, a buffer of its own, d_original itself


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
    """(original_present [N], recovery mask or None) of a named missing set.  "most": as many
    originals missing as a call can take, m = c - 2, under a mask of exactly m + 2 rows."""
    present = np.ones(N, np.uint8)
    mask = None
    if kind == "first":
        present[0] = 0
    elif kind == "middle":
        present[N // 2] = 0
    elif kind == "last":
        present[N - 1] = 0
    elif kind == "run":
        present[N // 3:N // 3 + 3] = 0
    elif kind == "scattered":
        present[sorted({1 % N, N // 2, N - 2 if N > 2 else 0})] = 0
    else:
        assert kind == "most"
        m = min(N, M - 2)
        present[np.linspace(0, N - 1, m).round().astype(int)] = 0
        m = int((present == 0).sum())
        if m + 2 < M:
            mask = np.zeros(M, np.uint8)
            mask[np.linspace(0, M - 1, m + 2).round().astype(int)] = 1
            assert int(mask.sum()) == m + 2
    return present, mask


def exact_mask(present, M):
    """Exactly m + 2 rows, away from row 0."""
    m = int((np.asarray(present) == 0).sum())
    mask = np.zeros(M, np.uint8)
    mask[M - (m + 2):] = 1
    return mask


def third_mask(M):
    mask = np.ones(M, np.uint8)
    mask[2::3] = 0
    return mask


def cases(rate, N, M, S, present, mask, wide=False):
    """[(name, originals, recovery, intended status)] of one stripe under the two masks.  Absent
    originals hold junk in every case, and so do unselected recovery rows.  wide: the positional
    cases of a wide shard instead (tests/wide_cases.py) -- clean; a present original damaged in the
    last pack, and as a whole shard; a reference row damaged in pack 256 (the last pack where the
    shard has no second tile) and another in the last pack."""
    orig, rec = (x.copy() for x in V.stripe(rate, N, M, S))
    pb, R, K = DM.split(present, mask, M)
    rng = np.random.default_rng(N * 7 + M + S + len(R))
    orig[~pb] = rng.integers(0, 256, (len(R), S), dtype=np.uint8)
    if mask is not None:
        unsel = np.asarray(mask) == 0
        rec[unsel] ^= rng.integers(1, 256, (int(unsel.sum()), S), dtype=np.uint8)
    have = np.flatnonzero(pb)
    out = [("clean", orig, rec, CLEAN)]
    if wide:
        packs = W.packs_of(S)
        bad = orig.copy()
        W.damage_pack(bad, have[-1], packs - 1, rng)
        out.append((f"original {have[-1]} pack {packs - 1}", bad, rec, int(have[-1])))
        bad = orig.copy()
        bad[have[len(have) // 2]] ^= rng.integers(1, 256, S, dtype=np.uint8)
        out.append((f"original {have[len(have) // 2]} shard", bad, rec, int(have[len(have) // 2])))
        p = W.TILE if W.TILE < packs else packs - 1
        bad = rec.copy()
        W.damage_pack(bad, R[0], p, rng)
        out.append((f"reference row {R[0]} pack {p}", orig, bad, N + int(R[0])))
        bad = rec.copy()
        W.damage_pack(bad, R[-1], packs - 1, rng)
        out.append((f"reference row {R[-1]} pack {packs - 1}", orig, bad, N + int(R[-1])))
        return out
    if len(have):
        bad = orig.copy()
        bad[have[0], 0] ^= 0x01  # one bit in byte 0
        out.append((f"original {have[0]} bit0", bad, rec, int(have[0])))
        bad = orig.copy()
        bad[have[-1], S - 1] ^= 0x80  # one bit in the tail's last high byte
        out.append((f"original {have[-1]} lastbit", bad, rec, int(have[-1])))
    bad = rec.copy()
    bad[R[0], S // 2] ^= 0x10
    out.append((f"reference row {R[0]}", orig, bad, N + int(R[0])))
    bad = rec.copy()
    bad[R[-1]] ^= rng.integers(1, 256, S, dtype=np.uint8)  # the whole shard
    out.append((f"reference row {R[-1]} shard", orig, bad, N + int(R[-1])))
    bad = rec.copy()
    bad[K[-1], 5 % S] ^= 0x20
    out.append((f"check row {K[-1]}", orig, bad, ROWS))
    # an information shard plus a check row; two information shards in different columns (each
    # column names another position, so no single one explains the stripe)
    bo, br = orig.copy(), rec.copy()
    if len(have):
        bo[have[len(have) // 2], 0] ^= 0x04
    else:
        br[R[len(R) // 2], 0] ^= 0x04
    br[K[0], S // 2] ^= 0x40
    out.append(("information shard and check row", bo, br, UNKNOWN if len(K) >= 3 else None))
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
    out.append(("two information shards", bo, br, UNKNOWN))
    return out


def padded(torch, a, pad, fill=0xC3, guard_rows=0):
    """(view [.., rows, S], whole buffer) on the device: `pad` junk bytes after every row and
    `guard_rows` junk rows before and after the matrix."""
    rows, S = a.shape[-2:]
    buf = torch.full(a.shape[:-2] + (rows + 2 * guard_rows, S + pad), fill, dtype=torch.uint8, device="cuda")
    v = buf[..., guard_rows:guard_rows + rows, :S]
    v.copy_(torch.from_numpy(np.array(a, copy=True)).cuda())
    return v, buf


def host_image(a, pad, fill=0xC3, guard_rows=0):
    """What padded()'s whole buffer holds."""
    rows, S = a.shape[-2:]
    out = np.full(a.shape[:-2] + (rows + 2 * guard_rows, S + pad), fill, np.uint8)
    out[..., guard_rows:guard_rows + rows, :S] = a
    return out


def guarded(torch, shape, dtype):
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


def locate(torch, rs, rate, N, M, S, orig, present, rec, pad=0, mask=None, form="none", what="", stream=None):
    """One call (a batch when orig is 3-D) on fresh device copies; (located, flags, restored rows
    [.., N, S] or None) on the host, after every "nothing else was written" check."""
    batch = orig.ndim == 3
    pb = np.asarray(present) != 0
    d_orig, orig_buf = padded(torch, orig, pad)
    d_rec, rec_buf = padded(torch, rec, pad)
    lead = orig.shape[:-2]
    loc, loc_buf = guarded(torch, lead if batch else (1,), torch.int32)
    flags, flag_buf = guarded(torch, lead + (M,), torch.uint8)
    d_restored = res_buf = None
    if form == "separate":  # poison everywhere: present rows, padding and the guard rows keep it
        d_restored, res_buf = padded(torch, np.full(orig.shape, 0xEE, np.uint8), pad, fill=0xEE, guard_rows=1)
    elif form == "alias":
        d_restored = d_orig
    call = rs.locate_device_degraded_batch if batch else rs.locate_device_degraded
    call(N, M, S, d_orig, present, d_rec, recovery_rows=mask, d_restored=d_restored, d_located=loc, d_mismatch=flags,
         rate_=RATE[rate], stream=stream)
    torch.cuda.synchronize()
    got, got_flags = check_outputs(loc_buf, flag_buf, what)
    assert np.array_equal(rec_buf.cpu().numpy(), host_image(rec, pad)), what + ": d_recovery was written"
    after = orig_buf.cpu().numpy()
    restored = None
    if form == "alias":
        restored = after[..., :S].copy()
        after[..., ~pb, :S] = orig[..., ~pb, :]  # (only the missing rows may have changed)
    elif form == "separate":
        image = res_buf.cpu().numpy()
        restored = image[..., 1:N + 1, :S].copy()
        image[..., 1 + np.flatnonzero(~pb), :S] = 0xEE
        assert (image == 0xEE).all(), what + ": d_restored was written outside the missing originals' rows"
    assert np.array_equal(after, host_image(orig, pad)), what + ": d_original was written"
    return got, got_flags.reshape(lead + (M,)), restored


def check_case(torch, rs, rate, N, M, S, pad, present, mask, name, orig, rec, intended, form):
    what = f"{rate} {N}:{M} x {S} pad {pad} m {int((np.asarray(present) == 0).sum())} {name} d_restored {form}"
    pb = np.asarray(present) != 0
    want, want_flags, F = DM.locate(rate, orig, present, rec, mask)
    if intended is not None:
        assert want == intended, f"{what}: the model says {want}, the case was built for {intended}"
    got, got_flags, restored = locate(torch, rs, rate, N, M, S, orig, present, rec, pad, mask, form, what)
    assert np.array_equal(got_flags, want_flags), \
        f"{what}: flagged rows {np.flatnonzero(got_flags).tolist()[:8]}, want {np.flatnonzero(want_flags).tolist()[:8]}"
    assert int(got[0]) == want, f"{what}: located {int(got[0])}, want {want}"
    if restored is not None:
        assert np.array_equal(restored[~pb], F[~pb]), what + ": the restored originals differ from the oracle's decode"


def run_cases(torch, rs, rate, N, M, S, pad, present, mask):
    for k, (name, orig, rec, intended) in enumerate(cases(rate, N, M, S, present, mask)):
        # the clean stripe under every form of d_restored, the others in turn
        for form in (FORMS if k == 0 else [FORMS[k % 3]]):
            check_case(torch, rs, rate, N, M, S, pad, present, mask, name, orig, rec, intended, form)


def _shape_params():
    out = []
    for rate, N, M in SHAPES:
        for S, pad in (LAYOUTS if N != 4096 else LAYOUTS[:1]):
            for kind in MISSING:
                if N == 3 and kind in ("middle", "run"):
                    continue  # (3:5: "middle" is "scattered"'s neighbour, a run of 3 is "most")
                out.append(pytest.param(rate, N, M, S, pad, kind, id=f"{rate}-{N}-{M}-{S}-{pad}-{kind}"))
    return out


@pytest.mark.parametrize("rate,N,M,S,pad,kind", _shape_params())
def test_shapes(torch, rs, rate, N, M, S, pad, kind):
    present, mask = pattern(kind, N, M)
    run_cases(torch, rs, rate, N, M, S, pad, present, mask)


@pytest.mark.parametrize("which", ["exact", "third"])
@pytest.mark.parametrize("rate,N,M,S,pad,kind", [("high", 70, 100, 72, 0, "run"), ("low", 100, 70, 66, 4, "scattered"),
                                                 ("default", 1024, 1024, 64, 0, "scattered"),
                                                 ("high", 1000, 100, 66, 0, "first"), ("low", 128, 1024, 72, 8, "run"),
                                                 ("default", 4096, 4096, 64, 0, "last"), ("default", 3, 5, 190, 0, "last")],
                         ids=lambda v: str(v))
def test_masks(torch, rs, rate, N, M, S, pad, kind, which):
    """Masks of exactly m + 2 rows and masks with every third row out: the reference rows are the
    first m SELECTED rows; junk in the unselected rows and the padding is never read or flagged."""
    present, _ = pattern(kind, N, M)
    mask = exact_mask(present, M) if which == "exact" else third_mask(M)
    run_cases(torch, rs, rate, N, M, S, pad, present, mask)


def batch_case(rate, N, M, S, B, present, mask):
    """B stripes (5..8) with a different outcome in each."""
    pb, R, K = DM.split(present, mask, M)
    have = np.flatnonzero(pb)
    origs, recs, wants = [], [], []
    for b in range(B):
        o, r = (x.copy() for x in V.stripe(rate, N, M, S, seed=b))
        o[~pb] = 0x5A + b
        kind = ["orig", "clean", "check", "ref", "two", "orig2", "ref2", "both"][b]
        if kind == "orig":
            o[have[0], S - 1] ^= 0x80
            want = int(have[0])
        elif kind == "orig2":
            o[have[-1]] ^= np.random.default_rng(b).integers(1, 256, S, dtype=np.uint8)
            want = int(have[-1])
        elif kind == "check":
            r[K[len(K) // 2], 3 % S] ^= 0x02
            want = ROWS
        elif kind == "ref":
            r[R[0], 0] ^= 0x01
            want = N + int(R[0])
        elif kind == "ref2":
            r[R[-1], S - 1] ^= 0x80
            want = N + int(R[-1])
        elif kind == "two":
            o[have[0], 0] ^= 0x10
            o[have[-1], S - 1] ^= 0x20
            want = UNKNOWN
        elif kind == "both":
            o[have[1], 0] ^= 0x10
            r[K[0], 0] ^= 0x08
            want = UNKNOWN
        else:
            want = CLEAN
        model, flags, F = DM.locate(rate, o, present, r, mask)
        assert model == want, (b, kind, model)
        origs.append(o), recs.append(r), wants.append((want, flags, F))
    return (np.stack(origs), np.stack(recs), np.array([w[0] for w in wants]), np.stack([w[1] for w in wants]),
            np.stack([w[2] for w in wants]))


@pytest.mark.parametrize("rate,N,M,S,B,pad,form", [("default", 1024, 1024, 72, 6, 0, "separate"),
                                                   ("high", 70, 100, 66, 8, 4, "alias"),
                                                   ("high", 1000, 100, 66, 5, 0, "none"),
                                                   ("default", 4096, 4096, 64, 5, 0, "alias")], ids=lambda v: str(v))
def test_batch(torch, rs, rate, N, M, S, B, pad, form):
    """One-launch shapes and a stripe-by-stripe shape, with stripe padding: the constructed
    results, which are also those of a loop of single calls."""
    present, _ = pattern("scattered", N, M)
    pb = present != 0
    mask = third_mask(M)
    origs, recs, want, want_flags, F = batch_case(rate, N, M, S, B, present, mask)
    got, got_flags, restored = locate(torch, rs, rate, N, M, S, origs, present, recs, pad, mask, form, "batch")
    assert got.tolist() == want.tolist(), (got, want)
    assert np.array_equal(got_flags, want_flags)
    if restored is not None:
        assert np.array_equal(restored[:, ~pb], F[:, ~pb])
    for b in range(B):
        single, single_flags, single_restored = locate(torch, rs, rate, N, M, S, origs[b], present, recs[b], pad, mask,
                                                       form, f"stripe {b}")
        assert int(single[0]) == got[b] and np.array_equal(single_flags, got_flags[b])
        if restored is not None:
            assert np.array_equal(single_restored[~pb], restored[b][~pb])
    # stripe padding, tensors the call allocates itself, and the launches: one of each kernel where
    # the batch repair is one launch, else stripe by stripe
    d_orig, d_rec = V.padded_batch(torch, origs, 2, pad), V.padded_batch(torch, recs, 3, pad)
    d_res = V.padded_batch(torch, np.full(origs.shape, 0xEE, np.uint8), 1, pad)
    out = []
    names = [r[0] for r in V.profiled(torch, rs, lambda: out.extend(rs.locate_device_degraded_batch(
        N, M, S, d_orig, present, d_rec, recovery_rows=mask, d_restored=d_res, rate_=RATE[rate])))]
    l2, f2 = out
    assert l2.shape == (B,) and str(l2.dtype) == "torch.int32" and f2.shape == (B, M) and l2.is_cuda
    assert l2.cpu().numpy().tolist() == want.tolist() and np.array_equal(f2.cpu().numpy(), want_flags)
    assert np.array_equal(d_res.cpu().numpy()[:, ~pb], F[:, ~pb]) and (d_res.cpu().numpy()[:, pb] == 0xEE).all()
    assert np.array_equal(d_orig.cpu().numpy(), origs) and np.array_equal(d_rec.cpu().numpy(), recs)
    count = names.count("k_locate_find")
    assert count == names.count("k_locate_confirm") == names.count("k_verify_rows") == names.count("k_locate_rename")
    assert count == {1024: 1, 70: 1, 1000: 1, 4096: B}[N], names


@pytest.mark.parametrize("rate,N,M,S,pad", [("high", 70, 100, 66, 4), ("default", 1024, 1024, 64, 0),
                                            ("default", 4096, 4096, 64, 0), ("default", 3, 5, 72, 0)],
                         ids=lambda v: str(v))
def test_nothing_missing_is_the_locate(torch, rs, rate, N, M, S, pad):
    """m = 0: d_located and d_mismatch are locate_device_batch's, d_restored is untouched."""
    B = 4
    pairs = [V.stripe(rate, N, M, S, seed=b) for b in range(B)]
    origs, recs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    origs[1, N - 1, S - 1] ^= 0x80
    recs[2, M // 2, 0] ^= 1
    origs[3, 0, 0] ^= 1
    recs[3, 1, 1] ^= 1
    present = np.ones(N, np.uint8)
    for mask in (None, third_mask(M)):
        got, got_flags, restored = locate(torch, rs, rate, N, M, S, origs, present, recs, pad, mask, "separate", "m = 0")
        d_orig, d_rec = V.padded_batch(torch, origs, 0, pad), V.padded_batch(torch, recs, 0, pad)
        l, f = rs.locate_device_batch(N, M, S, d_orig, d_rec, recovery_rows=mask, rate_=RATE[rate])
        assert np.array_equal(got, l.cpu().numpy()) and np.array_equal(got_flags, f.cpu().numpy())
        model = [LM.locate(rate, origs[b], recs[b], mask=mask) for b in range(B)]
        assert got.tolist() == [m[0] for m in model]
        if mask is None:
            assert got.tolist()[:3] == [CLEAN, N - 1, ROWS]
        assert (restored == 0xEE).all()


def test_errors_through_the_wrapper(torch, rs):
    """With a real context: c < m is NotEnoughShards with the decode's counts, c = m and c = m + 1
    are rejected, and nothing is written."""
    N, M, S = 8, 6, 64
    orig, rec = V.stripe("default", N, M, S)
    d_orig, d_rec = V.view(torch, orig, 0), V.view(torch, rec, 0)
    loc, loc_buf = guarded(torch, (1,), torch.int32)
    flags, flag_buf = guarded(torch, (M,), torch.uint8)
    present = [1, 0, 1, 1, 0, 1, 0, 1]  # m = 3
    kw = dict(d_located=loc, d_mismatch=flags)
    with pytest.raises(rs.NotEnoughShards) as e:
        rs.locate_device_degraded(N, M, S, d_orig, present, d_rec, recovery_rows=[1, 0, 0, 1, 0, 0], **kw)
    assert (e.value.original_count, e.value.original_received_count, e.value.recovery_received_count) == (N, 5, 2)
    for few in ([1, 1, 1, 0, 0, 0], [1, 1, 0, 1, 0, 1]):
        with pytest.raises(ValueError, match="recovery_rows: 3 missing"):
            rs.locate_device_degraded(N, M, S, d_orig, present, d_rec, recovery_rows=few, **kw)
    torch.cuda.synchronize()
    assert (loc_buf.cpu().numpy() == -1).all() and (flag_buf.cpu().numpy() == 0xFF).all()
    got, _ = rs.locate_device_degraded(N, M, S, d_orig, present, d_rec, recovery_rows=[1, 1, 1, 0, 1, 1], **kw)
    assert int(got.cpu()[0]) == CLEAN


def coef_launches(recs):
    return [r[0] for r in recs if r[0].startswith("k_coef_")]


def test_table_is_built_once_per_pattern(torch, rs):
    """The table of a (shape, pattern) is built by the first call on a stream and reused; another
    pattern or release_stream_scratch rebuilds it; a plain locate and an update next to it keep
    their tables; a warm call launches the repair's kernels, k_verify_rows, k_locate_find,
    k_locate_confirm and k_locate_rename, and nothing else."""
    rate, N, M, S = "default", 300, 500, 72
    orig, rec = V.stripe(rate, N, M, S)
    present, _ = pattern("scattered", N, M)
    pb = present != 0
    bad = orig.copy()
    bad[~pb] = 0x77
    bad[N - 1, 1] ^= 0x40
    d_bad, d_rec = V.view(torch, bad, 0), V.view(torch, rec, 0)
    call = lambda **kw: rs.locate_device_degraded(N, M, S, d_bad, present, d_rec, **kw)
    rs.release_stream_scratch()
    first = V.profiled(torch, rs, call)
    # two slabs of positions (256 + 44): a unit stripe and a log launch each, around the repairs
    assert coef_launches(first) == ["k_coef_unit_degraded", "k_coef_log_slab"] * 2, first
    # what the repair of this pattern from the reference rows alone launches
    ref = np.zeros(M, np.uint8)
    ref[:3] = 1
    d_x, d_y = torch.zeros((N, S), dtype=torch.uint8, device="cuda"), torch.zeros((M, S), dtype=torch.uint8, device="cuda")
    repair = [r[0] for r in V.profiled(torch, rs, lambda: rs.repair_device(N, M, S, d_bad, present, d_rec, ref, d_x, d_y))]
    assert repair and not coef_launches([(n,) for n in repair])
    tail = ["k_verify_rows", "k_locate_find", "k_locate_confirm", "k_locate_rename"]
    assert [r[0] for r in first][-len(repair) - 4:] == repair + tail
    second = V.profiled(torch, rs, call)
    assert [r[0] for r in second] == repair + tail, second
    assert int(call()[0].cpu()[0]) == N - 1
    # a masked call (same reference rows), a call with d_restored and a batch use the same table
    mask = np.ones(M, np.uint8)
    mask[[5, 7, 400]] = 0
    d_res = torch.zeros((N, S), dtype=torch.uint8, device="cuda")
    assert [r[0] for r in V.profiled(torch, rs, lambda: call(recovery_rows=mask, d_restored=d_res))] == repair + tail
    d_bad3, d_rec3 = d_bad[None].expand(2, N, S).contiguous(), d_rec[None].expand(2, M, S).contiguous()
    assert coef_launches(V.profiled(torch, rs, lambda: rs.locate_device_degraded_batch(
        N, M, S, d_bad3, present, d_rec3))) == []
    # a plain locate and an update of the same shape in between: their own tables, built once; ours stays
    full = orig.copy()
    full[N - 1, 1] ^= 0x40
    d_full = V.view(torch, full, 0)
    plain = lambda: rs.locate_device(N, M, S, d_full, d_rec)
    assert coef_launches(V.profiled(torch, rs, plain)) == ["k_coef_unit_slab", "k_coef_log_slab"] * 2
    d_new = torch.zeros((1, S), dtype=torch.uint8, device="cuda")
    d_upd = d_rec.clone()
    upd = lambda: rs.update_device(N, M, S, [N - 1], None, d_new, d_upd)
    assert coef_launches(V.profiled(torch, rs, upd)) == ["k_coef_unit", "k_coef_log"]
    assert coef_launches(V.profiled(torch, rs, call)) == []
    assert coef_launches(V.profiled(torch, rs, plain)) == [] and coef_launches(V.profiled(torch, rs, upd)) == []
    assert int(plain()[0].cpu()[0]) == N - 1 and int(call()[0].cpu()[0]) == N - 1
    # another pattern rebuilds, other reference rows rebuild, and so does coming back
    other, _ = pattern("first", N, M)
    bad2 = orig.copy()
    bad2[0] = 0x11
    d_bad2 = V.view(torch, bad2, 0)
    got = []
    recs = V.profiled(torch, rs, lambda: got.extend(rs.locate_device_degraded(N, M, S, d_bad2, other, d_rec)))
    assert len(coef_launches(recs)) == 4 and int(got[0].cpu()[0]) == CLEAN
    assert len(coef_launches(V.profiled(torch, rs, call))) == 4
    shifted = np.ones(M, np.uint8)
    shifted[0] = 0  # R = {1, 2, 3} instead of {0, 1, 2}
    assert len(coef_launches(V.profiled(torch, rs, lambda: call(recovery_rows=shifted)))) == 4
    assert len(coef_launches(V.profiled(torch, rs, call))) == 4
    rs.release_stream_scratch()
    assert len(coef_launches(V.profiled(torch, rs, call))) == 4
    assert int(call()[0].cpu()[0]) == N - 1


def test_calls_in_flight(torch, rs):
    """Two calls of different stripes and patterns on one stream with an encode between them, and
    two on two streams."""
    rate, N, M, S = "default", 200, 200, 72
    orig, rec = V.stripe(rate, N, M, S)
    pa, _ = pattern("first", N, M)
    pbm, _ = pattern("run", N, M)
    a, b = orig.copy(), orig.copy()
    a[0] = 0x33
    a[7, 0] ^= 1
    b[pbm == 0] = 0x44
    b[N - 2, S - 1] ^= 0x80
    d_a, d_b, d_rec = V.view(torch, a, 0), V.view(torch, b, 0), V.view(torch, rec, 0)
    d_enc = torch.zeros((M, S), dtype=torch.uint8, device="cuda")
    d_ra, d_rb = torch.zeros((N, S), dtype=torch.uint8, device="cuda"), torch.zeros((N, S), dtype=torch.uint8, device="cuda")
    mask = np.ones(M, np.uint8)
    mask[0] = 0  # (a mask on the second call only)
    wa, fa_want, Fa = DM.locate(rate, a, pa, rec)
    wb, fb_want, Fb = DM.locate(rate, b, pbm, rec, mask)
    assert (wa, wb) == (7, N - 2)
    torch.cuda.synchronize()
    la, fa = rs.locate_device_degraded(N, M, S, d_a, pa, d_rec, d_restored=d_ra)
    rs.encode_device(N, M, S, d_a, d_enc)
    lb, fb = rs.locate_device_degraded(N, M, S, d_b, pbm, d_rec, recovery_rows=mask, d_restored=d_rb)
    torch.cuda.synchronize()
    assert (int(la.cpu()[0]), int(lb.cpu()[0])) == (7, N - 2)
    assert np.array_equal(fa.cpu().numpy(), fa_want) and np.array_equal(fb.cpu().numpy(), fb_want)
    assert np.array_equal(d_ra.cpu().numpy()[0], Fa[0]) and np.array_equal(d_rb.cpu().numpy()[pbm == 0], Fb[pbm == 0])
    assert np.array_equal(d_enc.cpu().numpy(), O.encode(rate, a, M))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    la, _ = rs.locate_device_degraded(N, M, S, d_a, pa, d_rec, stream=s1)
    lb, _ = rs.locate_device_degraded(N, M, S, d_b, pbm, d_rec, recovery_rows=mask, stream=s2)
    torch.cuda.synchronize()
    assert (int(la.cpu()[0]), int(lb.cpu()[0])) == (7, N - 2)
    rs.release_stream_scratch(s1)
    rs.release_stream_scratch(s2)


def test_scrub(torch, rs):
    """Locate a degraded batch in place, read the results, one repair_device_batch_masks with the
    named shard (or the flagged rows) absent: every stripe ends byte-identical to the clean one."""
    rate, N, M, S, B = "high", 70, 100, 66, 5
    pairs = [V.stripe(rate, N, M, S, seed=b) for b in range(B)]
    origs, recs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    present = np.ones(N, np.uint8)
    present[[3, 40]] = 0  # R = {0, 1}
    bad_o, bad_r = origs.copy(), recs.copy()
    bad_o[:, [3, 40]] = 0x99
    rng = np.random.default_rng(5)
    bad_o[0, 33] = rng.integers(0, 256, S, dtype=np.uint8)  # a whole present original
    bad_r[1, 17, 40] ^= 0x08  # two check rows
    bad_r[1, 93, 3] ^= 0x80
    bad_r[3, 1, S - 1] ^= 0x80  # a reference row: the tail's last high byte
    bad_o[4, 0, 0] ^= 0x01
    d_orig, d_rec = V.view(torch, bad_o, 0), V.view(torch, bad_r, 0)
    located, flags = (t.cpu().numpy() for t in rs.locate_device_degraded_batch(
        N, M, S, d_orig, present, d_rec, d_restored=d_orig, rate_=RATE[rate]))
    assert located.tolist() == [33, ROWS, CLEAN, N + 1, 0]
    now = d_orig.cpu().numpy()
    assert np.array_equal(now[[1, 2]], origs[[1, 2]])  # CLEAN and ROWS: the restored rows stand
    assert not np.array_equal(now[3][[3, 40]], origs[3][[3, 40]])  # decoded from a corrupt reference row
    orig_ok, rec_ok = np.ones((B, N), np.uint8), np.ones((B, M), np.uint8)
    for b, i in enumerate(located):
        if i >= N:
            orig_ok[b], rec_ok[b, i - N] = present, 0
        elif i >= 0:
            orig_ok[b] = present
            orig_ok[b, i] = 0
        elif i == ROWS:
            rec_ok[b] = 1 - flags[b]
    assert np.flatnonzero(1 - rec_ok[1]).tolist() == [17, 93]
    rs.repair_device_batch_masks(N, M, S, d_orig, orig_ok, d_rec, rec_ok, d_orig, d_rec, rate_=RATE[rate])
    torch.cuda.synchronize()
    assert np.array_equal(d_rec.cpu().numpy(), recs) and np.array_equal(d_orig.cpu().numpy(), origs)
    again, _ = rs.locate_device_batch(N, M, S, d_orig, d_rec, rate_=RATE[rate])
    assert (again.cpu().numpy() == CLEAN).all()
