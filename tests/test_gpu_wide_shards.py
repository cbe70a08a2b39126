"""GPU: the scrub calls -- verify, locate, heal, their robust, degraded and per-stripe-mask forms, and
update -- on shards wider than one wave, one pack tile and one scan step.

The families' own files stop at 190-byte shards (24 packs: one wave, blockIdx.x == 0, the find's first
unroll slot); the update's stops at 1024.  Here every family runs through its own runner -- whole
buffers against the numpy model over poisoned outputs, guards and junk padding -- at the sizes of
tests/wide_cases.py's table: 520, 1032, 2048, 2056, 2050 with byte-wise rows, 8200 and 65536 bytes, each
sitting on a threshold the kernels have in S, and with damage placed by pack number either side of
each threshold (packs 63 | 64, 255 | 256, 1023 | 1024 and the last).  tests/test_wide_shards_cpu.py
has checked that every case means what it was built for on the model alone.

The routing edges are read off the profile's kernel names, not assumed: a column-kernel shape launches
k_mono* up to 256 packs and nothing of that name past them; with the defaults its packs hold 2 elements
up to 128 packs and 4 beyond.
"""
import numpy as np
import pytest

import heal_masks_cases as HMC
import heal_model as HM
import oracle_lib as O
import test_gpu_heal as H
import test_gpu_heal_degraded as HD
import test_gpu_heal_masks as HK
import test_gpu_heal_robust as HR
import test_gpu_locate as L
import test_gpu_locate_degraded as LD
import test_gpu_locate_masks as LK
import test_gpu_locate_robust as LR
import test_gpu_update as U
import test_gpu_verify as V
import test_gpu_verify_masks as VK
import verify_masks_cases as C
import wide_cases as W

pytestmark = pytest.mark.gpu

RATE = V.RATE
CLEAN, ROWS, UNKNOWN = L.CLEAN, L.ROWS, L.UNKNOWN
ORIGINAL, RECOVERY = HM.ORIGINAL, HM.RECOVERY
SHAPES = W.shapes()
IDS = [f"{r}-{n}-{m}-{s}" for r, n, m, s, _ in SHAPES]


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
    reed_solomon_simd.update_set_direct_max(reed_solomon_simd.UPDATE_DIRECT_MAX_DEFAULT)
    reed_solomon_simd.mono_enable(True)


def on_column(N, M, S):
    return (N, M) in W.ON_COLUMN and W.packs_of(S) <= W.MONO_MAX_PACKS


def check_route(names, rate, N, M, S, stripes=1):
    """The edge at mono_max_packs, and for the two L = 7 shapes the one at e2_max_packs, from the
    launch names of one call with the library's defaults."""
    what = f"{rate} {N}:{M} x {S}: {names}"
    mono = [n for n in names if n.startswith("k_mono")]
    if not on_column(N, M, S):
        assert not mono, what + ": a column kernel past mono_max_packs"
        return
    assert mono, what + ": no column kernel at or below mono_max_packs"
    if (rate, N, M) in W.COLUMN:
        elems = 2 if W.packs_of(S) * stripes <= W.E2_MAX_PACKS else 4
        assert all(n.endswith(f", {elems}>") for n in mono), what + f": not {elems}-element packs"


def warm_names(torch, rs, fn):
    """The launches of the second of two identical calls: the first builds the coefficient table,
    whose unit stripes have a geometry of their own."""
    fn()
    return [r[0] for r in V.profiled(torch, rs, fn)]


# ---- verify ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("rate,N,M,S,pad", SHAPES, ids=IDS)
def test_verify(torch, rs, rate, N, M, S, pad):
    """Clean; one row at each pack position; every row at a pack of its own; an original in the last
    pack.  Asked to run fused and unfused: the constructed flags both times (V.run checks inputs and
    guards), and the fused route exists exactly up to 256 packs."""
    rs.mono_enable(True)
    for kind in W.verify_kinds(N, M, S):
        a, recs = V.run(torch, rs, rate, N, M, S, kind, pad, fused=1)
        names = [r[0] for r in recs]
        if on_column(N, M, S):
            assert len(names) == 1 and names[0].startswith("k_mono_verify<"), (kind, names)
        else:
            assert names[-1] == "k_verify_rows", (kind, names)
        check_route(names, rate, N, M, S)
        b, recs = V.run(torch, rs, rate, N, M, S, kind, pad, fused=0)
        names = [r[0] for r in recs]
        assert names[-1] == "k_verify_rows" and not any(n.startswith("k_mono_verify") for n in names), (kind, names)
        check_route(names, rate, N, M, S)
        assert np.array_equal(a, b), kind


# ---- locate and heal ------------------------------------------------------------------------------

@pytest.mark.parametrize("rate,N,M,S,pad", SHAPES, ids=IDS)
def test_locate(torch, rs, rate, N, M, S, pad):
    """Original i damaged at every pack position in turn, and as a whole shard, comes back as exactly
    i; two originals in different tiles, and an original with a recovery row damaged in the last pack
    alone, are UNKNOWN; recovery rows alone are ROWS.  Flags and located against the model."""
    rs.mono_enable(True)
    d_orig, d_rec = (V.view(torch, x, pad) for x in V.stripe(rate, N, M, S))
    names = warm_names(torch, rs, lambda: rs.locate_device(N, M, S, d_orig, d_rec, rate_=RATE[rate]))
    assert names[-3:] == ["k_verify_rows", "k_locate_find", "k_locate_confirm"], names
    check_route(names, rate, N, M, S)
    L.run_cases(torch, rs, rate, N, M, S, pad, wide=True)


def heal_subset(N):
    """The cases a single mode bit runs: clean, original 0 at its pack positions (every third: 63,
    256, the last), a whole shard, the UNKNOWN stripe and the ROWS stripe."""
    return ("none", "original 0 pack", f"original {N - 1} shard", "two originals", "recovery rows")


@pytest.mark.parametrize("mode", [ORIGINAL | RECOVERY, ORIGINAL, RECOVERY], ids=["both", "original", "recovery"])
@pytest.mark.parametrize("rate,N,M,S,pad", SHAPES, ids=IDS)
def test_heal(torch, rs, rate, N, M, S, pad, mode):
    """Every positional case healed: both matrices whole equal the model's and, where the stripe had
    one cause, the clean stripe (H.run_cases); the ROWS stripe with rows damaged in different tiles is
    rewritten to the oracle's encode; a second heal of what the first left is CLEAN with action 0."""
    rs.mono_enable(True)
    only = None if mode == ORIGINAL | RECOVERY else heal_subset(N)
    H.run_cases(torch, rs, rate, N, M, S, pad, mode=mode, only=only, wide=True, again=True)
    d_orig, d_rec = (V.view(torch, x, pad) for x in V.stripe(rate, N, M, S))
    names = warm_names(torch, rs, lambda: rs.heal_device(N, M, S, d_orig, d_rec, mode=mode, max_rows=2,
                                                         rate_=RATE[rate]))
    assert names[-4:] == ["k_verify_rows", "k_locate_find", "k_locate_confirm", "k_heal"], names
    check_route(names, rate, N, M, S)


# ---- robust ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("rate,N,M,S,pad", SHAPES, ids=IDS)
def test_locate_robust(torch, rs, rate, N, M, S, pad):
    """max_outliers 1 and 2: a corrupt original (a whole shard) with its outlier rows damaged in the
    last pack alone; an original damaged in pack 0 alone with outliers in the last pack, where e = 0;
    max_outliers + 1 outliers: UNKNOWN."""
    rs.mono_enable(True)
    assert LR.run_cases(torch, rs, rate, N, M, S, pad, wide=True) == {"i", CLEAN, UNKNOWN}


@pytest.mark.parametrize("rate,N,M,S,pad", SHAPES, ids=IDS)
def test_heal_robust(torch, rs, rate, N, M, S, pad):
    """The same cases healed: the original and its outlier rows, whole buffers against the model and
    the clean stripe."""
    rs.mono_enable(True)
    assert HR.run_cases(torch, rs, rate, N, M, S, pad, wide=True) == {("i", True), CLEAN, UNKNOWN}


# ---- degraded -------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["first", "scattered"])  # m = 1, and a scattered 3
@pytest.mark.parametrize("rate,N,M,S,pad", SHAPES, ids=IDS)
def test_locate_degraded(torch, rs, rate, N, M, S, pad, kind):
    """Clean; a present original corrupt in the last pack, and as a whole shard; reference rows corrupt
    in pack 256 (where there is one) and in the last pack; d_restored separate and aliased.  Past 256
    packs the repair under the call is the unfused one."""
    rs.mono_enable(True)
    present, mask = LD.pattern(kind, N, M)
    cases = LD.cases(rate, N, M, S, present, mask, wide=True)
    _, orig, rec, _ = cases[0]
    d_orig, d_rec = V.view(torch, orig, pad), V.view(torch, rec, pad)
    names = warm_names(torch, rs, lambda: rs.locate_device_degraded(N, M, S, d_orig, present, d_rec, rate_=RATE[rate]))
    assert names[-1] == "k_locate_rename", names
    if not on_column(N, M, S) and (N, M) in W.ON_COLUMN:
        assert not any(n.startswith("k_mono") for n in names), names
    for name, orig, rec, intended in cases:
        for form in ("separate", "alias"):
            LD.check_case(torch, rs, rate, N, M, S, pad, present, mask, name, orig, rec, intended, form)


@pytest.mark.parametrize("kind", ["first", "scattered"])
@pytest.mark.parametrize("rate,N,M,S,pad", SHAPES, ids=IDS)
def test_heal_degraded(torch, rs, rate, N, M, S, pad, kind):
    """The same cases healed with both mode bits, d_restored separate and aliased: the located shard
    and the restored rows against the model, the healed stripe the clean one, a verify clean and a
    second heal CLEAN (HD.check_case)."""
    rs.mono_enable(True)
    present, mask = LD.pattern(kind, N, M)
    for name, orig, rec, intended, max_rows_list in HD.cases(rate, N, M, S, present, mask, wide=True):
        HD.check_case(torch, rs, rate, N, M, S, pad, present, mask, name, orig, rec, intended, max_rows_list,
                      modes=[ORIGINAL | RECOVERY])


# ---- a mask per stripe ----------------------------------------------------------------------------

_MASKS = {}


def masks_batch(rate, N, M, S):
    key = (rate, N, M, S)
    if key not in _MASKS:
        origs, recs = C._clean(rate, N, M, S, 4)
        _MASKS[key] = W.masks_batch(origs, recs, lambda b, o: O.encode(rate, o, M))
        for a in _MASKS[key]:
            a.setflags(write=False)
    return _MASKS[key]


@pytest.mark.parametrize("rate,N,M,S,pad", SHAPES, ids=IDS)
def test_verify_masks(torch, rs, rate, N, M, S, pad):
    """4 stripes -- every row, two rows far apart, all but every third, rows 2.. -- whose unselected
    rows differ from the right ones in the last pack alone: never flagged, fused or unfused; the
    flags are the constructed ones and those of a loop of verify_device calls."""
    rs.mono_enable(True)
    store, held, masks, _, want = masks_batch(rate, N, M, S)
    a, recs, (d_orig, d_rec) = VK.run(torch, rs, rate, N, M, S, pad, 1, batch=(store, held, masks, want))
    names = [r[0] for r in recs]
    if on_column(N, M, S):
        assert len(names) == 1 and names[0].startswith("k_mono_verify_masks<"), names
    else:
        assert names[-1] == "k_verify_rows_masks" and not any(n.startswith("k_mono") for n in names), names
    assert np.array_equal(a, VK.loop_of_singles(torch, rs, rate, N, M, S, d_orig, d_rec, masks))
    b, recs, _ = VK.run(torch, rs, rate, N, M, S, pad, 0, batch=(store, held, masks, want))
    names = [r[0] for r in recs]
    assert names[-1] == "k_verify_rows_masks" and not any(n.startswith("k_mono_verify") for n in names), names
    assert np.array_equal(a, b)


@pytest.mark.parametrize("rate,N,M,S,pad", SHAPES, ids=IDS)
def test_locate_masks(torch, rs, rate, N, M, S, pad):
    """The same batch located: original 0 (corrupt in the last pack), ROWS, original N - 1, CLEAN;
    equal to the per-stripe model (LK.run) and to a loop of locate_device calls."""
    rs.mono_enable(True)
    store, held, masks, intent, want = masks_batch(rate, N, M, S)
    loc, got, _, recs, (d_orig, d_rec) = LK.run(torch, rs, rate, N, M, S, pad, batch=(store, held, masks, intent, want))
    LK.check_against_singles(torch, rs, rate, N, M, S, d_orig, d_rec, masks, loc, got)
    names = [r[0] for r in recs]
    assert names.count("k_locate_find_masks") == (1 if on_column(N, M, S) else len(masks)), names


@pytest.mark.parametrize("rate,N,M,S,pad", SHAPES, ids=IDS)
def test_heal_masks(torch, rs, rate, N, M, S, pad):
    """The same batch healed, with both bits (the two-row stripe is skipped) and with the recovery bit
    alone (its row is rewritten): results and both matrices whole -- the unselected rows' junk where it
    was -- against the per-stripe model, and every stripe against a heal_device of its own."""
    rs.mono_enable(True)
    store, held, masks, intent, _ = masks_batch(rate, N, M, S)
    for mode in (ORIGINAL | RECOVERY, RECOVERY):
        what = f"{rate} {N}:{M} x {S} pad {pad} mode {mode}"
        model = HMC.model(rate, N, M, S, mode=mode, max_rows=2, masks=masks, store=store, held=held)
        got = HK.heal(torch, rs, rate, N, M, S, store, held, masks, mode=mode, max_rows=2, pad=pad, extra=(2, 3))
        HK.check(got, model, what)
        names = [r[0] for r in got[6]]
        assert names.count("k_heal_masks") == (1 if on_column(N, M, S) else int((model[5] == 0).sum())), names
        for b in range(len(masks)):
            if model[5][b]:
                assert got[0][b] == rs.LOCATE_SKIPPED and got[2][b] == 0
                continue
            single = (int(model[0][b]), model[1][b], int(model[2][b]), model[3][b], model[4][b])
            H.heal_one(torch, rs, rate, N, M, S, store[b], held[b], pad, mask=masks[b], mode=mode, max_rows=2,
                       what=f"{what} stripe {b} alone", model=single)


# ---- batches with one mask ------------------------------------------------------------------------

# (rate, N, M, S, stripes, row padding, groups the batch runs in)
BATCHES = [("high", 70, 100, 2048, 3, 8, 1), ("high", 70, 100, 2056, 3, 8, 3), ("low", 100, 70, 2048, 3, 0, 1),
           ("low", 100, 70, 2056, 3, 0, 3), ("default", 1024, 1024, 1024, 8, 0, 1)]
BATCH_IDS = [f"{r}-{n}-{m}-{s}-{b}" for r, n, m, s, b, _, _ in BATCHES]


@pytest.mark.parametrize("rate,N,M,S,B,pad,groups", BATCHES, ids=BATCH_IDS)
def test_verify_batch(torch, rs, rate, N, M, S, B, pad, groups):
    """Stripe padding, a different corruption in each stripe: the constructed flags, which are those of
    the stripe-by-stripe loop; one fused launch up to 256 packs, 4-element packs (3 x 256 and 8 x 128
    packs are past the 2-element bound)."""
    rs.mono_enable(True)
    for fused in (1, 0):
        names = V.check_batch(torch, rs, rate, N, M, S, fused, B=B, pad=pad, singles=True)
        if fused and on_column(N, M, S):
            assert len(names) == 1 and names[0].startswith("k_mono_verify<"), names
        else:
            assert names.count("k_verify_rows") == groups, names
        check_route(names, rate, N, M, S, stripes=B)


@pytest.mark.parametrize("rate,N,M,S,B,pad,groups", BATCHES, ids=BATCH_IDS)
def test_locate_batch(torch, rs, rate, N, M, S, B, pad, groups):
    """One group on the column kernel at 2048 bytes, one stripe per group at 2056; 8 stripes at
    1024:1024 x 1024.  The constructed results, equal to a loop of single calls (L.test_batch)."""
    rs.mono_enable(True)
    L.test_batch(torch, rs, rate, N, M, S, B, pad, wide=True, groups=groups)


@pytest.mark.parametrize("rate,N,M,S,B,pad,groups", BATCHES, ids=BATCH_IDS)
def test_heal_batch(torch, rs, rate, N, M, S, B, pad, groups):
    """The same for the heal: the model, the loop of single calls, and a second heal (H.test_batch)."""
    rs.mono_enable(True)
    H.test_batch(torch, rs, rate, N, M, S, B, pad, wide=True, groups=groups)


# ---- update ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [1, 33])
@pytest.mark.parametrize("rate,N,M,S", W.UPDATE, ids=lambda v: str(v))
def test_update(torch, rs, rate, N, M, S, count):
    """1 and 33 indices (30:100 has 30 originals: all of them), the first new shard differing from the
    old one in the last pack alone and the second in pack 0 alone; every third recovery row
    unselected, 8 junk bytes after every row.  Both routes against the oracle's encode of the modified
    stripe (U.run), and against each other."""
    rng = np.random.default_rng(N * 7 + M + count)
    idx = U.indices(N, min(count, N), rng)
    mask = np.ones(M, np.uint8)
    mask[1::3] = 0
    got = {}

    def run(route, form):
        got[route] = U.run(torch, rs, rate, N, M, S, idx, route, form, mask, positional=True, pad=8)

    for form in ("delta", "oldnew"):
        direct = [r[0] for r in V.profiled(torch, rs, lambda: run(U.DIRECT, form))]
        assert sum(n.startswith("k_update") for n in direct) == 1, direct
        again = [r[0] for r in V.profiled(torch, rs, lambda: run(U.REENCODE, form))]
        assert not any(n.startswith("k_update") for n in again) and "k_rows_xor" in again, again
        U.check(got[U.DIRECT], got[U.REENCODE], f"{rate} {N}:{M} x {S} count {len(idx)} {form}: the routes differ")
