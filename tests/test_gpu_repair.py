"""GPU: rs_repair_device* -- the decode that also restores the missing recovery shards.

Restored recovery rows are compared byte for byte with the CPU oracle's encode, restored
originals with the originals themselves (and, where only originals are missing, with
decode_device's output).  Both outputs start filled with a poison byte and absent input rows
hold junk (0xA5 / 0x5A), so a kernel that reads an absent row, or writes a present row or
padding, fails.  The route is taken from the launch records and asserted where a case exists to
reach it: every decode route of the library carries the second destination.
"""
import numpy as np
import pytest

import oracle_lib as O
import test_gpu_batch_masks as G

pytestmark = pytest.mark.gpu

RATE = G.RATE
POISON = 0x33


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


def packs_of(S):
    return S // 64 * 8 + ((S % 64) // 2 + 3) // 4


def pattern(kind, rate, N, M, rng=None):
    """(original_present, recovery_present); at most M shards missing in all."""
    rng = rng or np.random.default_rng(N * 131 + M)
    op, rp = np.ones(N, np.uint8), np.ones(M, np.uint8)
    high = G._high(rate, N, M)
    if kind == "none":
        pass
    elif kind == "rec_only_one":  # the last recovery row, every original present
        rp[M - 1] = 0
    elif kind == "rec_only_many":
        rp[rng.choice(M, max(2, M // 3), replace=False)] = 0
    elif kind == "orig_only":
        op[rng.choice(N, max(1, min(N, M) // 4), replace=False)] = 0
    elif kind == "both_random":
        op[rng.choice(N, max(1, min(N, M // 8)), replace=False)] = 0
        rp[rng.choice(M, max(1, M // 8), replace=False)] = 0
    elif kind == "both_max":  # missing originals + missing recoveries = M
        ko = max(1, min(N, M // 2))
        op[rng.choice(N, ko, replace=False)] = 0
        rp[rng.choice(M, M - ko, replace=False)] = 0
    elif kind == "halves":
        # HighRate (recovery rows first, originals from `chunk` on): originals lost only at the top
        # indices, recoveries only at the bottom; LowRate the mirror -- outputs in both halves
        ko, kr = max(1, min(N, M) // 8), max(1, M // 8)
        if high:
            op[N - ko:] = 0
            rp[:kr] = 0
        else:
            op[:ko] = 0
            rp[M - kr:] = 0
    elif kind == "spread":  # many separate runs of missing rows of both kinds
        op[np.arange(3, N, max(2, -(-N // max(1, M // 4))))] = 0
        rp[np.arange(1, M, 4)] = 0
        rp[M // 2:M // 2 + 3] = 0
    else:
        raise ValueError(kind)
    assert int((op == 0).sum()) + int((rp == 0).sum()) <= M, (kind, N, M)
    return op, rp


KINDS = ["rec_only_one", "rec_only_many", "orig_only", "both_random", "both_max", "halves", "none"]


def first_diff(got, want):
    r, b = np.argwhere(got != want)[0]
    return f"first difference at (row {int(r)}, byte {int(b)}): got {int(got[r, b]):#04x}, want {int(want[r, b]):#04x}"


def assert_rows_equal(got, want, present, what, untouched=POISON):
    """Missing rows of `got` equal `want`; present rows still hold `untouched` (a byte, or the
    matrix they must still equal)."""
    miss = present == 0
    if miss.any() and not np.array_equal(got[miss], want[miss]):
        idx = np.flatnonzero(miss)
        bad = idx[(got[miss] != want[miss]).any(axis=1)]
        full = np.where(miss[:, None], want, got)
        raise AssertionError(f"{what}: {bad.size} of {idx.size} restored rows differ, rows {bad[:8].tolist()}; "
                             + first_diff(got, full))
    keep = np.broadcast_to(np.uint8(untouched), got.shape) if np.isscalar(untouched) else untouched
    if not np.array_equal(got[~miss], keep[~miss]):
        full = np.where(miss[:, None], got, keep)
        raise AssertionError(f"{what}: a present row was written; " + first_diff(got, full))


def inputs(torch, rate, N, M, S, op, rp, seed=0):
    orig, rec = G._stripe(rate, N, M, S, seed)
    d_o = G._dev(torch, np.where(op[:, None] == 1, orig, 0xA5).astype(np.uint8))
    d_r = G._dev(torch, np.where(rp[:, None] == 1, rec, 0x5A).astype(np.uint8))
    return orig, rec, d_o, d_r


def profiled(torch, rs, fn):
    rs.profile_enable(True)
    try:
        rs.profile_collect()
        out = fn()
        torch.cuda.synchronize()
        return out, [name for name, _, _ in rs.profile_collect()]
    finally:
        rs.profile_enable(False)


def repair(torch, rs, rate, N, M, S, op, rp, seed=0):
    """One repair into poisoned outputs, checked; returns (launch names, restored, recovery_out)."""
    orig, rec, d_o, d_r = inputs(torch, rate, N, M, S, op, rp, seed)
    d_x = torch.full((N, S), POISON, dtype=torch.uint8, device="cuda")
    d_y = torch.full((M, S), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _, names = profiled(torch, rs, lambda: rs.repair_device(N, M, S, d_o, op, d_r, rp, d_x, d_y, rate_=RATE[rate]))
    x, y = d_x.cpu().numpy(), d_y.cpu().numpy()
    what = f"{rate} {N}:{M} x {S}"
    assert_rows_equal(x, orig, op, what + " restored originals")
    assert_rows_equal(y, rec, rp, what + " recovery_out")
    return names, x, y


def decode_ref(torch, rs, rate, N, M, S, op, rp, seed=0):
    _, _, d_o, d_r = inputs(torch, rate, N, M, S, op, rp, seed)
    d_x = torch.full((N, S), POISON, dtype=torch.uint8, device="cuda")
    _, names = profiled(torch, rs, lambda: rs.decode_device(N, M, S, d_o, op, d_r, rp, d_x, rate_=RATE[rate]))
    return names, d_x.cpu().numpy()


def outputs_split(rate, N, M, op, rp):
    """(all outputs in one half of the work rows, that half) -- what the split plan needs."""
    chunk, _, nd = G.work_rows(rate, N, M)
    high = G._high(rate, N, M)
    rows = np.concatenate([np.flatnonzero(op == 0) + (chunk if high else 0),
                           np.flatnonzero(rp == 0) + (0 if high else chunk)])
    halves = set((rows >= nd // 2).tolist())
    return len(halves) == 1, int(True in halves)


def rec_runs(rp):
    """Runs of consecutive missing recovery rows."""
    miss = np.concatenate([[0], (rp == 0).astype(np.int8)])
    return int((np.diff(miss) == 1).sum())


def check_route(route, names, rate, N, M, S, op, rp, mode=1):
    miss_o, miss_r = int((op == 0).sum()), int((rp == 0).sum())
    if miss_o + miss_r == 0:
        assert names == [], names  # nothing launched
        return
    if miss_r == 0:
        assert names and not any("repair" in n for n in names), names  # the decode, launch for launch
        return
    if miss_o == 0 and rec_runs(rp) == 1:
        # every original present, one run of recovery rows missing: the encode, its destination
        # narrowed to the run (no eval_poly, no decode kernel)
        assert names and not any("repair" in n or n == "k_eval_poly" for n in names), names
        return
    nd = G.work_rows(rate, N, M)[2]
    L = nd.bit_length() - 1
    if route == "pass1":  # the single fused pass (eval_poly inside)
        assert len(names) == 1 and names[0].startswith("k_pass<"), names
    elif route == "fused":
        E = 4 if (mode & 8) or packs_of(S) > 128 else 2
        one_half, _ = outputs_split(rate, N, M, op, rp)
        split = one_half and not (mode & 4) and L >= 10
        assert names == ["k_mono_repair<%d, 1, 2, true, true, %s, %d>" % (L, "true" if split else "false", E)], names
    elif route == "unfused":
        assert len(names) == 2 and names[0] == "k_eval_poly" and names[1].startswith("k_mono_repair<12, "), names
        assert ", false, false, false, 4>" in names[1], names
    elif route == "half":
        assert names[0] == "k_eval_poly" and len(names) == 3, names
        assert names[1].startswith("k_mono<11, 1, 4, ") and names[2].startswith("k_mono_repair<11, 1, 6, "), names
    elif route == "passes":
        assert names[0] == "k_eval_poly" and len(names) >= 4, names
        assert all(n.startswith("k_pass<") for n in names[1:]), names
    else:
        raise ValueError(route)


# (rate, N, M, S, rs_mono_enable mode, route, kinds)
SHAPES = [
    # 3:5 and 5:3 have 16 work rows (chunk 4 or 8, end 9 or 11): padded to the 2^7 column kernel by
    # default, the single fused pass (eval_poly inside) with the column kernels off
    ("default", 3, 5, 64, 1, "fused", KINDS),
    ("high", 5, 3, 128, 1, "fused", KINDS),
    ("low", 3, 5, 128, 1, "fused", KINDS),
    ("default", 3, 5, 64, 0, "pass1", KINDS),
    ("high", 5, 3, 128, 0, "pass1", KINDS),
    ("low", 3, 5, 128, 0, "pass1", KINDS),
    # single fused pass at the default, < 16 work rows (chunk 4, end 8 / chunk 2, end 4)
    ("high", 4, 3, 64, 1, "pass1", KINDS),
    ("low", 2, 2, 66, 1, "pass1", ["rec_only_one", "orig_only", "both_max", "halves", "none"]),
    # padded to the 2^7 column kernel
    ("default", 32, 32, 64, 1, "fused", KINDS),
    # fused column kernel
    ("high", 64, 64, 64, 1, "fused", KINDS),
    ("high", 256, 256, 128, 1, "fused", KINDS),
    ("low", 256, 200, 64, 1, "fused", KINDS),
    # tails on the column kernel
    ("high", 128, 128, 2, 1, "fused", KINDS),
    ("high", 128, 128, 8, 1, "fused", KINDS),
    ("high", 128, 128, 66, 1, "fused", KINDS),
    ("high", 128, 128, 130, 1, "fused", KINDS),
    # unfused column kernel, half-split
    ("high", 2048, 2048, 64, 2, "unfused", KINDS),
    ("high", 2048, 2048, 64, 1 | 128, "half", KINDS),
    # pass kernels: two levels, more levels, per-row store masks (rows >= 8 KiB)
    ("high", 4096, 4096, 128, 1, "passes", KINDS + ["spread"]),
    ("high", 4096, 4096, 128, 0, "passes", KINDS + ["spread"]),
    ("low", 3000, 5000, 64, 1, "passes", KINDS + ["spread"]),
    ("low", 3000, 5000, 64, 0, "passes", KINDS + ["spread"]),
    ("high", 16384, 16384, 64, 1, "passes", ["rec_only_one", "both_random", "halves", "spread"]),
    ("high", 4096, 4096, 8192, 1, "passes", ["rec_only_one", "both_random", "spread"]),
]
# fused column kernel of 2^11 rows: split plan on / off, 2- / 4-element packs -- the same bytes
for _mode in (1, 1 | 4, 1 | 8, 1 | 4 | 8):
    SHAPES.append(("high", 1024, 1024, 64, _mode, "fused", KINDS))
    SHAPES.append(("low", 1024, 1000, 512, _mode, "fused", KINDS))

CASES = [(r, N, M, S, mode, route, k) for r, N, M, S, mode, route, kinds in SHAPES for k in kinds]


@pytest.mark.parametrize("rate,N,M,S,mode,route,kind", CASES,
                         ids=["%s-%d-%d-%d-m%d-%s" % (c[0], c[1], c[2], c[3], c[4], c[6]) for c in CASES])
def test_repair_matches_oracle(torch, rs, rate, N, M, S, mode, route, kind):
    op, rp = pattern(kind, rate, N, M)
    try:
        rs.mono_enable(mode)
        names, x, _ = repair(torch, rs, rate, N, M, S, op, rp)
        check_route(route, names, rate, N, M, S, op, rp, mode)
        if kind == "orig_only":  # the decode call's bytes and launches; recovery_out all poison (checked above)
            dnames, dx = decode_ref(torch, rs, rate, N, M, S, op, rp)
            assert np.array_equal(x, dx), first_diff(x, dx)
            assert names == dnames, (names, dnames)
        rs.check_device()
    finally:
        rs.mono_enable(1)


def test_split_plan_follows_the_outputs_of_both_kinds(torch, rs):
    """The split plan of the 2^11-row kernel runs the FFT on one half of the work rows: a
    recovery-only HighRate repair has its outputs in the lower half (out_half 0), a HighRate repair
    with losses of both kinds in both halves (no split)."""
    N = M = 1024
    assert outputs_split("high", N, M, *pattern("rec_only_many", "high", N, M)) == (True, 0)
    assert rec_runs(pattern("rec_only_many", "high", N, M)[1]) > 1  # (one run would go to the encode)
    assert outputs_split("high", N, M, *pattern("both_random", "high", N, M))[0] is False
    assert outputs_split("low", 1024, 1000, *pattern("rec_only_many", "low", 1024, 1000)) == (True, 1)
    names, _, _ = repair(torch, rs, "high", N, M, 64, *pattern("rec_only_many", "high", N, M))
    assert names == ["k_mono_repair<11, 1, 2, true, true, true, 2>"], names
    names, _, _ = repair(torch, rs, "low", 1024, 1000, 64, *pattern("rec_only_many", "low", 1024, 1000))
    assert names == ["k_mono_repair<11, 1, 2, true, true, true, 2>"], names
    names, _, _ = repair(torch, rs, "high", N, M, 64, *pattern("both_random", "high", N, M))
    assert names == ["k_mono_repair<11, 1, 2, true, true, false, 2>"], names
    rs.check_device()


# ---------------------------------------------------------------------------
# strided, unaligned, in place

def _wide(torch, rows, S, margin, fill, off=0):
    """A [rows, S] view of a wider poisoned buffer (margins left and right), its base `off` bytes
    into the buffer; returns (buffer, view)."""
    W = S + 2 * margin
    buf = torch.full((rows * W + 8,), fill, dtype=torch.uint8, device="cuda")
    view = buf[off:off + rows * W].view(rows, W)[:, margin:margin + S]
    return buf, view


@pytest.mark.parametrize("N,M,S", [(256, 256, 128), (1024, 1024, 64)])
@pytest.mark.parametrize("off", [0, 1])
def test_column_slices_with_poisoned_margins(torch, rs, N, M, S, off):
    """Every matrix a column slice of a wider one (off = 1: a base address of 1 mod 4, the
    byte-wise path); the margins and the present rows are still poison afterwards."""
    rate = "high"
    op, rp = pattern("both_random", rate, N, M)
    orig, rec = G._stripe(rate, N, M, S, 0)
    margin = 64 if off == 0 else 6
    bo, vo = _wide(torch, N, S, margin, 0xA5, off)
    br, vr = _wide(torch, M, S, margin, 0x5A, off)
    vo.copy_(G._dev(torch, np.where(op[:, None] == 1, orig, 0xA5).astype(np.uint8)))
    vr.copy_(G._dev(torch, np.where(rp[:, None] == 1, rec, 0x5A).astype(np.uint8)))
    bx, vx = _wide(torch, N, S, margin, POISON, off)
    by, vy = _wide(torch, M, S, margin, POISON, off)
    torch.cuda.synchronize()
    rs.repair_device(N, M, S, vo, op, vr, rp, vx, vy, rate_=RATE[rate])
    torch.cuda.synchronize()
    assert_rows_equal(vx.cpu().numpy(), orig, op, "restored originals")
    assert_rows_equal(vy.cpu().numpy(), rec, rp, "recovery_out")
    for buf, view, rows in ((bx, vx, N), (by, vy, M)):
        after = buf.clone()
        after[off:off + rows * (S + 2 * margin)].view(rows, -1)[:, margin:margin + S] = POISON
        assert bool((after == POISON).all()), "a margin was written"
    rs.check_device()


@pytest.mark.parametrize("N,M,S", [(256, 256, 128), (1024, 1024, 64)])
@pytest.mark.parametrize("kind", ["both_random", "both_max", "rec_only_many", "rec_only_one"])
def test_in_place_heals_the_stripe(torch, rs, N, M, S, kind):
    """d_recovery_out aliasing d_recovery and d_restored aliasing d_original: afterwards the two
    matrices are the full stripe."""
    rate = "high"
    op, rp = pattern(kind, rate, N, M)
    orig, rec, d_o, d_r = inputs(torch, rate, N, M, S, op, rp)
    torch.cuda.synchronize()
    rs.repair_device(N, M, S, d_o, op, d_r, rp, d_o, d_r, rate_=RATE[rate])
    torch.cuda.synchronize()
    assert_rows_equal(d_o.cpu().numpy(), orig, op, "healed originals", untouched=orig)
    assert_rows_equal(d_r.cpu().numpy(), rec, rp, "healed recovery", untouched=rec)
    assert np.array_equal(d_o.cpu().numpy(), orig) and np.array_equal(d_r.cpu().numpy(), rec)
    rs.check_device()


# ---------------------------------------------------------------------------
# batches

@pytest.mark.parametrize("N,M,S,one_launch", [(256, 256, 128, True), (4096, 4096, 128, False)])
def test_batch_equals_single_calls(torch, rs, N, M, S, one_launch):
    """5 stripes, one pattern, padded stripe strides: the result equals 5 single calls (which
    test_repair_matches_oracle checks against the oracle), the padding is not written."""
    rate, B = "high", 5
    op, rp = pattern("both_random", rate, N, M)
    data = [G._stripe(rate, N, M, S, s) for s in range(B)]
    pad = 3  # rows of padding after each stripe

    def padded(rows, fill):
        return torch.full((B, rows + pad, S), fill, dtype=torch.uint8, device="cuda")

    d_o, d_r, d_x, d_y = padded(N, 0xA5), padded(M, 0x5A), padded(N, POISON), padded(M, POISON)
    for b in range(B):
        d_o[b, :N] = G._dev(torch, np.where(op[:, None] == 1, data[b][0], 0xA5).astype(np.uint8))
        d_r[b, :M] = G._dev(torch, np.where(rp[:, None] == 1, data[b][1], 0x5A).astype(np.uint8))
    torch.cuda.synchronize()
    _, names = profiled(torch, rs, lambda: rs.repair_device_batch(
        N, M, S, d_o[:, :N], op, d_r[:, :M], rp, d_x[:, :N], d_y[:, :M], rate_=RATE[rate]))
    if one_launch:
        assert len(names) == 1 and names[0].startswith("k_mono_repair<9, 1, 2, true, true, "), names
    else:
        assert len(names) > B and names.count("k_eval_poly") == B, names
    x, y = d_x.cpu().numpy(), d_y.cpu().numpy()
    for b in range(B):
        s_x = torch.full((N, S), POISON, dtype=torch.uint8, device="cuda")
        s_y = torch.full((M, S), POISON, dtype=torch.uint8, device="cuda")
        rs.repair_device(N, M, S, d_o[b, :N], op, d_r[b, :M], rp, s_x, s_y, rate_=RATE[rate])
        torch.cuda.synchronize()
        assert np.array_equal(x[b, :N], s_x.cpu().numpy()), f"stripe {b} restored: " + first_diff(x[b, :N], s_x.cpu().numpy())
        assert np.array_equal(y[b, :M], s_y.cpu().numpy()), f"stripe {b} recovery: " + first_diff(y[b, :M], s_y.cpu().numpy())
        assert_rows_equal(x[b, :N], data[b][0], op, f"stripe {b} restored originals")
        assert_rows_equal(y[b, :M], data[b][1], rp, f"stripe {b} recovery_out")
    assert np.all(x[:, N:] == POISON) and np.all(y[:, M:] == POISON), "stripe padding was written"
    rs.check_device()


# ---------------------------------------------------------------------------
# streams, and the decode next to it

@pytest.mark.parametrize("two_streams", [False, True])
def test_repairs_in_flight(torch, rs, two_streams):
    """Two repairs of different shapes enqueued back to back (one stream), and one on each of
    two streams (scratch per context and stream): both results are right."""
    jobs = [("high", 4096, 4096, 128, "both_random"), ("low", 3000, 5000, 64, "spread")]  # pass kernels: scratch rows
    streams = [torch.cuda.Stream(), torch.cuda.Stream()] if two_streams else [torch.cuda.Stream()] * 2
    state = []
    for (rate, N, M, S, kind) in jobs:
        op, rp = pattern(kind, rate, N, M)
        orig, rec, d_o, d_r = inputs(torch, rate, N, M, S, op, rp)
        d_x = torch.full((N, S), POISON, dtype=torch.uint8, device="cuda")
        d_y = torch.full((M, S), POISON, dtype=torch.uint8, device="cuda")
        state.append((rate, N, M, S, op, rp, orig, rec, d_o, d_r, d_x, d_y))
    torch.cuda.synchronize()
    for st, (rate, N, M, S, op, rp, _, _, d_o, d_r, d_x, d_y) in zip(streams, state):
        rs.repair_device(N, M, S, d_o, op, d_r, rp, d_x, d_y, stream=st, rate_=RATE[rate])
    torch.cuda.synchronize()
    for rate, N, M, S, op, rp, orig, rec, _, _, d_x, d_y in state:
        assert_rows_equal(d_x.cpu().numpy(), orig, op, f"{rate} {N}:{M} restored originals")
        assert_rows_equal(d_y.cpu().numpy(), rec, rp, f"{rate} {N}:{M} recovery_out")
    rs.check_device()


@pytest.mark.parametrize("N,M,S", [(1024, 1024, 64), (4096, 4096, 128)])
def test_decode_is_not_disturbed_by_a_repair(torch, rs, N, M, S):
    """A decode, a repair and the same decode again on one context: the decode's bytes and its
    launches are the same both times."""
    rate = "high"
    op, rp = pattern("both_random", rate, N, M)
    n1, x1 = decode_ref(torch, rs, rate, N, M, S, op, rp)
    repair(torch, rs, rate, N, M, S, *pattern("both_max", rate, N, M), seed=1)
    n2, x2 = decode_ref(torch, rs, rate, N, M, S, op, rp)
    assert n1 == n2 and not any("repair" in n for n in n1), (n1, n2)
    assert np.array_equal(x1, x2)
    assert_rows_equal(x1, G._stripe(rate, N, M, S, 0)[0], op, "decode")
    rs.check_device()
