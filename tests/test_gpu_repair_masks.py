"""GPU: the batch repair with one pattern per stripe (rs_repair_device_batch_masks).

Every stripe is compared byte for byte with the CPU oracle: restored originals with the
originals themselves, rebuilt recovery rows with the oracle's encode.  Both outputs start
filled with a poison byte, so rows (and padding) that must not be written are checked too;
absent input rows hold junk, so a kernel that read them would restore wrong bytes.  The route
is asserted from the launch record: shapes on the fused column-kernel route run as ONE launch
of k_mono_repair_masks for the whole batch.
"""
import numpy as np
import pytest

import test_gpu_batch_masks as G

pytestmark = pytest.mark.gpu

RATE = G.RATE
POISON = G.POISON
_stripe, _dev, launches, work_rows = G._stripe, G._dev, G.launches, G.work_rows


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def rs(torch):
    import reed_solomon_simd
    return reed_solomon_simd


def _miss(N, M, lost_o, lost_r):
    op, rp = np.ones(N, np.uint8), np.ones(M, np.uint8)
    op[np.asarray(lost_o, dtype=np.int64)] = 0
    rp[np.asarray(lost_r, dtype=np.int64)] = 0
    return op, rp


def pattern(kind, N, M, rng):
    """One stripe's (original_present, recovery_present); decodable by construction (at most M of
    the N + M shards missing) unless the kind is "undecodable"."""
    if kind == "none":  # nothing missing
        p = _miss(N, M, [], [])
    elif kind == "rec_one":  # one recovery shard only
        p = _miss(N, M, [], [int(rng.integers(M))])
    elif kind == "rec_two":  # two separate runs of recovery shards only
        w = max(1, M // 16)
        p = _miss(N, M, [], list(range(1, 1 + w)) + list(range(M // 2 + 1, M // 2 + 1 + w)))
    elif kind == "orig":  # originals only
        p = _miss(N, M, rng.choice(N, max(1, min(N, M) // 10), replace=False), [])
    elif kind == "random":  # both kinds, ~10 %
        p = _miss(N, M, rng.choice(N, max(1, min(N, M) // 10), replace=False),
                  rng.choice(M, max(1, M // 10), replace=False))
    elif kind == "max":  # exactly M shards missing in total, split over both kinds
        ko = min(N, M // 2)
        p = _miss(N, M, rng.choice(N, ko, replace=False), rng.choice(M, M - ko, replace=False))
        assert int((p[0] == 0).sum() + (p[1] == 0).sum()) == M
    elif kind in ("lower", "upper"):  # every loss of either kind in one half of the indices
        k = max(1, min(N, M) // 20)
        o0, r0 = (0, 0) if kind == "lower" else (N - N // 2, M - M // 2)
        p = _miss(N, M, o0 + rng.choice(N // 2, k, replace=False), r0 + rng.choice(M // 2, k, replace=False))
    elif kind in ("comp_a", "comp_b"):
        # the complementary-wave pair of test_gpu_batch_masks.py: the received recovery sets of the
        # two stripes are complements, cut at a wave's 128 work rows where the shape has them; the
        # recovery rows NOT received are missing here, and rebuilt
        h = 128 if M >= 256 else M // 2
        k = max(1, min(5, N, h, M - h))
        p = _miss(N, M, rng.choice(N, k, replace=False), np.arange(0, h) if kind == "comp_a" else np.arange(h, M))
    else:  # undecodable: M + 1 shards missing
        assert kind == "undecodable"
        ko = min(N, M // 2 + 1)
        p = _miss(N, M, rng.choice(N, ko, replace=False), rng.choice(M, M + 1 - ko, replace=False))
        assert int(p[0].sum()) + int(p[1].sum()) == N - 1
        return p
    assert int(p[0].sum()) + int(p[1].sum()) >= N, kind
    return p


KINDS = ["none", "rec_one", "rec_two", "orig", "random", "max", "lower", "upper", "comp_a", "comp_b", "undecodable"]


def _decodable(op, rp):
    return int(op.sum()) + int(rp.sum()) >= op.size


def inputs(torch, rate, N, M, S, ops, rps, seeds=None):
    """Device inputs (absent rows hold junk) and poisoned outputs of the batch."""
    B = len(ops)
    seeds = range(B) if seeds is None else seeds
    data = [_stripe(rate, N, M, S, s) for s in seeds]
    d_o = _dev(torch, np.stack([np.where(ops[b][:, None] == 1, data[b][0], 0xA5).astype(np.uint8) for b in range(B)]))
    d_r = _dev(torch, np.stack([np.where(rps[b][:, None] == 1, data[b][1], 0x5A).astype(np.uint8) for b in range(B)]))
    d_x = torch.full((B, N, S), POISON, dtype=torch.uint8, device="cuda")
    d_y = torch.full((B, M, S), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return d_o, d_r, d_x, d_y


def run(torch, rs, rate, N, M, S, ops, rps, seeds=None, status=False, stream=None):
    d_o, d_r, d_x, d_y = inputs(torch, rate, N, M, S, ops, rps, seeds)
    ret = rs.repair_device_batch_masks(N, M, S, d_o, np.stack(ops), d_r, np.stack(rps), d_x, d_y, status=status,
                                       stream=stream, rate_=RATE[rate])
    return d_x, d_y, ret


def check(x, y, rate, N, M, S, ops, rps, seeds=None, what=""):
    """Stripe b: missing originals == the originals, missing recovery rows == the oracle's encode,
    every other byte of both outputs still poison (undecodable stripes: all of it)."""
    B = len(ops)
    seeds = range(B) if seeds is None else seeds
    for b in range(B):
        orig, rec = _stripe(rate, N, M, S, seeds[b])
        if not _decodable(ops[b], rps[b]):
            assert np.all(x[b] == POISON) and np.all(y[b] == POISON), f"{what} stripe {b}: must not be touched"
            continue
        for got, full, present, name in ((x[b], orig, ops[b], "original"), (y[b], rec, rps[b], "recovery")):
            miss = present == 0
            bad = np.flatnonzero((got[miss] != full[miss]).any(axis=1))
            assert bad.size == 0, (f"{what} stripe {b}: {bad.size} of {int(miss.sum())} missing {name} rows differ; "
                                   f"first missing-row ordinals {bad[:8].tolist()}")
            assert np.all(got[~miss] == POISON), f"{what} stripe {b}: a present {name} row was written"


def profiled(torch, rs, f):
    rs.profile_enable(True)
    try:
        rs.profile_collect()
        out = f()
        torch.cuda.synchronize()
        return out, launches(rs)
    finally:
        rs.profile_enable(False)


# ---------------------------------------------------------------------------
# mixed batches at the smallest shape of each kernel form

MIXED = [
    # (rate, N, M, S, B, first kind, kernel: k_mono_repair_masks<L, elements per pack> or None = stripe by stripe)
    ("default", 32, 32, 64, 3, 0, "k_mono_repair_masks<7, 2>"),        # 64 work rows, padded to 2^7
    ("default", 64, 64, 64, 4, 3, "k_mono_repair_masks<7, 2>"),
    ("default", 256, 256, 64, 3, 7, "k_mono_repair_masks<9, 2>"),
    ("default", 1024, 1024, 64, 6, 10, "k_mono_repair_masks<11, 2>"),  # 8 packs x 6 <= 128: 2-element packs
    ("default", 1024, 1024, 256, 6, 5, "k_mono_repair_masks<11, 4>"),  # 32 packs x 6 > 128: 4-element packs
    ("low", 100, 1000, 64, 3, 4, "k_mono_repair_masks<11, 2>"),
    ("default", 200, 56, 70, 3, 2, "k_mono_repair_masks<9, 2>"),       # tail block: byte-wise I/O
    ("high", 100, 300, 64, 4, 4, "k_mono_repair_masks<10, 2>"),        # padding rows [300, 512): erased, in no map
    ("default", 5000, 300, 64, 2, 3, None),                             # 2^13 work rows: off the fused route
]
# (tests/test_repair_masks_cpu.py checks, without a GPU, that each shape's work rows and packs
# give the kernel named here, and that the kinds above cover every kind)


def mixed_kinds(B, k0):
    return [KINDS[(k0 + b) % len(KINDS)] for b in range(B)]


def _mixed_patterns(N, M, S, B, k0):
    rng = np.random.default_rng(1000 * N + M + S)
    kinds = mixed_kinds(B, k0)
    pats = [pattern(k, N, M, rng) for k in kinds]
    return kinds, [p[0] for p in pats], [p[1] for p in pats]


@pytest.mark.parametrize("rate,N,M,S,B,k0,kernel", MIXED)
def test_mixed_batch_matches_oracle_per_stripe(torch, rs, rate, N, M, S, B, k0, kernel):
    kinds, ops, rps = _mixed_patterns(N, M, S, B, k0)
    (d_x, d_y, codes), names = profiled(torch, rs, lambda: run(torch, rs, rate, N, M, S, ops, rps, status=True))
    assert list(codes) == [7 if k == "undecodable" else 0 for k in kinds]
    check(d_x.cpu().numpy(), d_y.cpu().numpy(), rate, N, M, S, ops, rps, what=f"{rate} {N}:{M} x {S} {kinds}")
    if kernel is None:
        assert names and not any("k_mono_repair_masks" in n for n in names), names
    else:
        assert names == [kernel], names


def _loop_of_single_repairs(torch, rs, rate, N, M, S, ops, rps):
    d_o, d_r, d_x, d_y = inputs(torch, rate, N, M, S, ops, rps)
    for b in range(len(ops)):
        if _decodable(ops[b], rps[b]):
            rs.repair_device(N, M, S, d_o[b], ops[b], d_r[b], rps[b], d_x[b], d_y[b], rate_=RATE[rate])
    return d_o, d_r, d_x, d_y


@pytest.mark.parametrize("rate,N,M,S,kinds", [
    ("default", 256, 256, 64, ["random", "rec_one", "none", "max", "rec_two", "orig", "undecodable", "upper"]),
    # off the fused route: the narrowed encode (one run of recovery rows) and the decode's kernels
    ("default", 5000, 300, 64, ["rec_one", "random"]),
])
def test_equals_a_loop_of_single_repairs(torch, rs, rate, N, M, S, kinds):
    rng = np.random.default_rng(N + 31 * M)
    pats = [pattern(k, N, M, rng) for k in kinds]
    ops, rps = [p[0] for p in pats], [p[1] for p in pats]
    want = _loop_of_single_repairs(torch, rs, rate, N, M, S, ops, rps)
    got = inputs(torch, rate, N, M, S, ops, rps)
    rs.repair_device_batch_masks(N, M, S, got[0], np.stack(ops), got[1], np.stack(rps), got[2], got[3],
                                 status=True, rate_=RATE[rate])
    torch.cuda.synchronize()
    for a, b, name in zip(got, want, ("d_original", "d_recovery", "d_restored", "d_recovery_out")):
        assert torch.equal(a, b), name
    check(got[2].cpu().numpy(), got[3].cpu().numpy(), rate, N, M, S, ops, rps)


@pytest.mark.parametrize("B,elems", [(16, 2), (17, 4)])
def test_pack_threshold_straddle(torch, rs, B, elems):
    """64:64 x 64 bytes is 8 packs a stripe: 16 stripes are 128 packs (2-element packs), 17 are 136
    (4-element packs)."""
    N, M, S = 64, 64, 64
    rng = np.random.default_rng(B)
    pats = [pattern(KINDS[1 + b % 9], N, M, rng) for b in range(B)]
    ops, rps = [p[0] for p in pats], [p[1] for p in pats]
    seeds = [b % 4 for b in range(B)]
    (d_x, d_y, _), names = profiled(torch, rs, lambda: run(torch, rs, "default", N, M, S, ops, rps, seeds=seeds))
    check(d_x.cpu().numpy(), d_y.cpu().numpy(), "default", N, M, S, ops, rps, seeds=seeds)
    assert names == ["k_mono_repair_masks<7, %d>" % elems], names


# ---------------------------------------------------------------------------
# padded and unaligned layouts, in place

@pytest.mark.parametrize("rate,N,M,kernel", [("default", 64, 64, "k_mono_repair_masks<7, 2>"),
                                             ("high", 100, 300, "k_mono_repair_masks<10, 2>")])
def test_padded_unaligned_layout_keeps_poison(torch, rs, rate, N, M, kernel):
    """Stripes padded to rows + 3, rows 8 bytes wider than the shards, every base address 2 bytes
    off, d_recovery_out included: gap bytes, padding rows and present rows of both outputs keep the
    poison.  HighRate 100:300: the work rows [300, 512) are erased and belong to no map -- were they
    stored, rows 300.. of a stripe of d_recovery_out (its padding, the next stripe) would change."""
    S, B = 64, 3
    pitch = S + 8
    rng = np.random.default_rng(77)
    pats = [pattern(k, N, M, rng) for k in ("random", "rec_two", "max")]
    ops, rps = [p[0] for p in pats], [p[1] for p in pats]
    data = [_stripe(rate, N, M, S, b) for b in range(B)]

    def layout(rows, fill):
        flat = np.full(2 + B * (rows + 3) * pitch, fill, np.uint8)
        view = np.lib.stride_tricks.as_strided(flat[2:], (B, rows, S), ((rows + 3) * pitch, pitch, 1))
        return flat, view

    def on_device(flat, rows):
        d = _dev(torch, flat)
        return d, torch.as_strided(d, (B, rows, S), ((rows + 3) * pitch, pitch, 1), storage_offset=2)

    h_o, v_o = layout(N, 0xA5)
    h_r, v_r = layout(M, 0x5A)
    want_x, v_x = layout(N, POISON)
    want_y, v_y = layout(M, POISON)
    for b in range(B):
        v_o[b][ops[b] == 1] = data[b][0][ops[b] == 1]
        v_r[b][rps[b] == 1] = data[b][1][rps[b] == 1]
        v_x[b][ops[b] == 0] = data[b][0][ops[b] == 0]
        v_y[b][rps[b] == 0] = data[b][1][rps[b] == 0]
    d_o, t_o = on_device(h_o, N)
    d_r, t_r = on_device(h_r, M)
    d_x, t_x = on_device(np.full_like(want_x, POISON), N)
    d_y, t_y = on_device(np.full_like(want_y, POISON), M)
    assert t_x.data_ptr() % 4 == 2 and t_y.data_ptr() % 4 == 2
    _, names = profiled(torch, rs, lambda: rs.repair_device_batch_masks(
        N, M, S, t_o, np.stack(ops), t_r, np.stack(rps), t_x, t_y, rate_=RATE[rate]))
    assert names == [kernel], names
    for got, want, name in ((d_x, want_x, "d_restored"), (d_y, want_y, "d_recovery_out")):
        bad = np.flatnonzero(got.cpu().numpy() != want)
        assert bad.size == 0, f"{name}: {bad.size} bytes differ, first at flat offset {bad[:8].tolist()}"
    assert np.array_equal(d_o.cpu().numpy(), h_o) and np.array_equal(d_r.cpu().numpy(), h_r), "inputs were written"


def test_in_place_heals_both_matrices(torch, rs):
    rate, N, M, S = "default", 256, 256, 64
    kinds = ["random", "rec_two", "none", "max", "orig", "comp_a", "comp_b"]
    rng = np.random.default_rng(12)
    pats = [pattern(k, N, M, rng) for k in kinds]
    ops, rps = [p[0] for p in pats], [p[1] for p in pats]
    d_o, d_r, _, _ = inputs(torch, rate, N, M, S, ops, rps)
    _, names = profiled(torch, rs, lambda: rs.repair_device_batch_masks(N, M, S, d_o, np.stack(ops), d_r,
                                                                        np.stack(rps), d_o, d_r))
    assert names == ["k_mono_repair_masks<9, 2>"], names
    data = [_stripe(rate, N, M, S, b) for b in range(len(kinds))]
    assert np.array_equal(d_o.cpu().numpy(), np.stack([d[0] for d in data]))
    assert np.array_equal(d_r.cpu().numpy(), np.stack([d[1] for d in data]))


# ---------------------------------------------------------------------------
# batches the decode would not run at all

def test_recovery_only_batch_runs_where_the_decode_launches_nothing(torch, rs):
    rate, N, M, S = "default", 256, 256, 64
    kinds = ["rec_one", "rec_two", "none", "rec_one"]
    rng = np.random.default_rng(4)
    pats = [pattern(k, N, M, rng) for k in kinds]
    ops, rps = [p[0] for p in pats], [p[1] for p in pats]
    assert all(op.all() for op in ops)
    (d_x, d_y, _), names = profiled(torch, rs, lambda: run(torch, rs, rate, N, M, S, ops, rps))
    assert names == ["k_mono_repair_masks<9, 2>"], names
    check(d_x.cpu().numpy(), d_y.cpu().numpy(), rate, N, M, S, ops, rps)
    assert bool((d_x == POISON).all())
    (d_out, _), names = profiled(torch, rs, lambda: G.run(torch, rs, rate, N, M, S, ops, rps))
    assert names == [], names
    assert bool((d_out == POISON).all())


# ---------------------------------------------------------------------------
# status mode

def _one_short(N, M, rng):
    kinds = ["random", "rec_one", "undecodable", "orig", "max"]
    pats = [pattern(k, N, M, rng) for k in kinds]
    return [p[0] for p in pats], [p[1] for p in pats]


def test_undecodable_stripe_all_or_nothing(torch, rs):
    rate, N, M, S = "default", 64, 64, 64
    ops, rps = _one_short(N, M, np.random.default_rng(9))
    d_o, d_r, d_x, d_y = inputs(torch, rate, N, M, S, ops, rps)
    with pytest.raises(rs.NotEnoughShards) as e:
        rs.repair_device_batch_masks(N, M, S, d_o, np.stack(ops), d_r, np.stack(rps), d_x, d_y)
    assert e.value.stripe == 2
    assert e.value == rs.NotEnoughShards(original_count=N, original_received_count=int(ops[2].sum()),
                                         recovery_received_count=int(rps[2].sum()))
    torch.cuda.synchronize()
    assert bool((d_x == POISON).all()) and bool((d_y == POISON).all()), "nothing may be written when the call fails"


def test_undecodable_stripe_status_mode(torch, rs):
    rate, N, M, S = "default", 64, 64, 64
    ops, rps = _one_short(N, M, np.random.default_rng(9))
    d_x, d_y, codes = run(torch, rs, rate, N, M, S, ops, rps, status=True)
    torch.cuda.synchronize()
    assert list(codes) == [0, 0, 7, 0, 0]
    check(d_x.cpu().numpy(), d_y.cpu().numpy(), rate, N, M, S, ops, rps)  # (stripe 2: untouched)


# ---------------------------------------------------------------------------
# two calls in flight on one stream; the decode's masks call next to a repair

def test_two_calls_back_to_back_on_one_stream(torch, rs):
    """The second call's descriptors must not overwrite staging the first call's copy still reads."""
    rate, N, M, S = "default", 256, 256, 64
    rng = np.random.default_rng(21)
    sets = [[pattern(k, N, M, rng) for k in kinds]
            for kinds in (("random", "max", "rec_one"), ("upper", "rec_two", "orig"))]
    bufs = [inputs(torch, rate, N, M, S, [p[0] for p in pats], [p[1] for p in pats]) for pats in sets]
    s = torch.cuda.Stream()
    for pats, (d_o, d_r, d_x, d_y) in zip(sets, bufs):
        rs.repair_device_batch_masks(N, M, S, d_o, np.stack([p[0] for p in pats]), d_r,
                                     np.stack([p[1] for p in pats]), d_x, d_y, stream=s)
    s.synchronize()
    for k, (pats, (_, _, d_x, d_y)) in enumerate(zip(sets, bufs)):
        check(d_x.cpu().numpy(), d_y.cpu().numpy(), rate, N, M, S, [p[0] for p in pats], [p[1] for p in pats],
              what=f"call {k}")
    rs.release_stream_scratch(s)


def test_decode_masks_call_is_unaffected_next_to_a_repair(torch, rs):
    rate, N, M, S, B = "default", 256, 256, 64, 3
    rng = np.random.default_rng(8)
    pats = [pattern(k, N, M, rng) for k in ("random", "max", "rec_two")]
    ops, rps = [p[0] for p in pats], [p[1] for p in pats]
    dpats = [G.pattern(k, N, M, rng) for k in ("random", "all", "one")]
    dops, drps = [p[0] for p in dpats], [p[1] for p in dpats]

    def both():
        r = run(torch, rs, rate, N, M, S, ops, rps)
        d = G.run(torch, rs, rate, N, M, S, dops, drps)
        return r, d

    ((d_x, d_y, _), (d_out, _)), names = profiled(torch, rs, both)
    assert names == ["k_mono_repair_masks<9, 2>", "k_mono_masks<9, 2>"], names
    check(d_x.cpu().numpy(), d_y.cpu().numpy(), rate, N, M, S, ops, rps)
    G.check(d_out.cpu().numpy(), rate, N, M, S, dops, drps)
