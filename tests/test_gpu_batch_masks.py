"""GPU: the batch decode with one erasure pattern per stripe (rs_decode_device_batch_masks).

Every stripe is compared byte for byte with the CPU oracle's decode of that stripe with
its own pattern.  Outputs start filled with a poison byte, so rows (and padding) that must
not be written are checked too; absent input rows hold junk, so a kernel that read them
would restore wrong bytes.  The route is asserted from the launch record: shapes on the
fused column-kernel route run as ONE launch of k_mono_masks for the whole batch.
"""
import functools

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

RATE = {"default": 0, "high": 1, "low": 2}
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


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _stripe(rate, N, M, S, seed):
    """(original, recovery) of one stripe from the oracle; computed once, never modified."""
    orig = O.generate_original(N, S, seed)
    rec = O.encode(rate, orig, M)
    orig.setflags(write=False)
    rec.setflags(write=False)
    return orig, rec


def _high(rate, N, M):
    return rate == "high" or (rate == "default" and O.lib().orc_use_high_rate(N, M) == 1)


def work_rows(rate, N, M):
    """(chunk, end, 2^L work rows) as the decoder lays the shards out (rate_high.rs / rate_low.rs:
    the first kind at rows 0.., the second from the next power of two on); 16..64 work rows run
    the 2^7-row kernel."""
    pow2 = lambda x: 1 << max(0, int(x - 1).bit_length())
    chunk = pow2(M) if _high(rate, N, M) else pow2(N)
    end = chunk + (N if _high(rate, N, M) else M)
    nd = pow2(end)
    return chunk, end, 128 if 16 <= nd < 128 else nd


def _lose(N, M, lost, received):
    op = np.ones(N, np.uint8)
    op[np.asarray(lost, dtype=np.int64)] = 0
    rp = np.zeros(M, np.uint8)
    rp[np.asarray(received, dtype=np.int64)] = 1
    return op, rp


def pattern(kind, N, M, rng):
    """One stripe's (original_present, recovery_present)."""
    if kind == "none":  # nothing missing
        return _lose(N, M, [], rng.choice(M, M // 2, replace=False))
    if kind == "one":  # one original, recovered from the last recovery shard
        return _lose(N, M, [int(rng.integers(N))], [M - 1])
    if kind == "all":  # every original (as many as the recovery shards can restore)
        k = min(N, M)
        return _lose(N, M, rng.choice(N, k, replace=False), rng.choice(M, k, replace=False))
    if kind == "random":  # ~10 %
        k = max(1, min(N, M) // 10)
        return _lose(N, M, rng.choice(N, k, replace=False), rng.choice(M, k, replace=False))
    if kind in ("lower", "upper"):  # every loss, and every recovery shard used, in one half of the indices
        k = max(1, min(N, M) // 20)
        o0, r0 = (0, 0) if kind == "lower" else (N - N // 2, M - M // 2)
        return _lose(N, M, o0 + rng.choice(N // 2, k, replace=False), r0 + rng.choice(M // 2, k, replace=False))
    # comp_a / comp_b: complementary received recovery sets, cut at a wave's 128 work rows where the
    # shape has them (a recovery index is a work row, or 128-aligned chunk + index): the waves that
    # hold received recovery rows in one stripe hold none in the other
    h = 128 if M >= 256 else M // 2
    k = max(1, min(5, N, h, M - h))
    lost = rng.choice(N, k, replace=False)
    return _lose(N, M, lost, np.arange(h, M) if kind == "comp_a" else np.arange(0, h))


KINDS = ["none", "one", "all", "random", "lower", "upper", "comp_a", "comp_b"]


def run(torch, rs, rate, N, M, S, ops, rps, seeds=None, status=False, stream=None):
    """Decode the batch; returns (restored bytes [B, N, S], what the call returned)."""
    B = len(ops)
    seeds = range(B) if seeds is None else seeds
    data = [_stripe(rate, N, M, S, s) for s in seeds]
    d_o = _dev(torch, np.stack([np.where(ops[b][:, None] == 1, data[b][0], 0xA5).astype(np.uint8) for b in range(B)]))
    d_r = _dev(torch, np.stack([np.where(rps[b][:, None] == 1, data[b][1], 0x5A).astype(np.uint8) for b in range(B)]))
    d_out = torch.full((B, N, S), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ret = rs.decode_device_batch_masks(N, M, S, d_o, np.stack(ops), d_r, np.stack(rps), d_out, status=status,
                                       stream=stream, rate_=RATE[rate])
    return d_out, ret


def check(out, rate, N, M, S, ops, rps, seeds=None, what=""):
    """Stripe b of `out` == the oracle's decode with pattern b; every other byte is still poison."""
    B = len(ops)
    seeds = range(B) if seeds is None else seeds
    for b in range(B):
        orig, rec = _stripe(rate, N, M, S, seeds[b])
        miss = ops[b] == 0
        decodable = int(ops[b].sum()) + int(rps[b].sum()) >= N
        if decodable and miss.any():
            want = O.decode(rate, np.where(ops[b][:, None] == 1, orig, 0), ops[b],
                            np.where(rps[b][:, None] == 1, rec, 0), rps[b])
            assert np.array_equal(want[miss], orig[miss]), "oracle decode does not restore the originals"
            bad = np.flatnonzero((out[b][miss] != want[miss]).any(axis=1))
            assert bad.size == 0, (f"{what} stripe {b}: {bad.size} of {int(miss.sum())} restored rows differ; "
                                   f"first lost-row ordinals {bad[:8].tolist()}")
            assert np.all(out[b][~miss] == POISON), f"{what} stripe {b}: a present row was written"
        else:
            assert np.all(out[b] == POISON), f"{what} stripe {b}: must not be touched"


def launches(rs):
    return [name for name, _, _ in rs.profile_collect()]


# ---------------------------------------------------------------------------
# mixed batches at the smallest shape of each kernel form

MIXED = [
    # (rate, N, M, S, B, first kind, kernel: k_mono_masks<L, elements per pack> or None = stripe by stripe)
    ("default", 32, 32, 64, 3, 0, "k_mono_masks<7, 2>"),       # 64 work rows, padded to 2^7
    ("default", 64, 64, 64, 4, 4, "k_mono_masks<7, 2>"),
    ("default", 256, 256, 64, 3, 5, "k_mono_masks<9, 2>"),
    ("default", 1024, 1024, 64, 6, 0, "k_mono_masks<11, 2>"),  # 8 packs x 6 <= 128: 2-element packs
    ("default", 1024, 1024, 256, 6, 2, "k_mono_masks<11, 4>"),  # 32 packs x 6 > 128: 4-element packs
    ("low", 100, 1000, 64, 3, 6, "k_mono_masks<11, 2>"),
    ("default", 200, 56, 70, 3, 1, "k_mono_masks<9, 2>"),      # tail block: byte-wise I/O
    ("default", 5000, 300, 64, 2, 3, None),                     # 2^13 work rows: off the fused route
]


# (tests/test_batch_masks_cpu.py checks, without a GPU, that each shape's work rows and packs
# give the kernel named here)


@pytest.mark.parametrize("rate,N,M,S,B,k0,kernel", MIXED)
def test_mixed_batch_matches_oracle_per_stripe(torch, rs, rate, N, M, S, B, k0, kernel):
    rng = np.random.default_rng(1000 * N + M + S)
    kinds = [KINDS[(k0 + b) % len(KINDS)] for b in range(B)]
    pats = [pattern(k, N, M, rng) for k in kinds]
    ops, rps = [p[0] for p in pats], [p[1] for p in pats]
    rs.profile_enable(True)
    try:
        rs.profile_collect()
        d_out, _ = run(torch, rs, rate, N, M, S, ops, rps)
        torch.cuda.synchronize()
        names = launches(rs)
    finally:
        rs.profile_enable(False)
    check(d_out.cpu().numpy(), rate, N, M, S, ops, rps, what=f"{rate} {N}:{M} x {S} {kinds}")
    if kernel is None:
        assert names and not any("k_mono_masks" in n for n in names), names
    else:
        assert names == [kernel], names


@pytest.mark.parametrize("B,elems", [(16, 2), (17, 4)])
def test_pack_threshold_straddle(torch, rs, B, elems):
    """64:64 x 64 bytes is 8 packs a stripe: 16 stripes are 128 packs (2-element packs), 17 are 136
    (4-element packs)."""
    N, M, S = 64, 64, 64
    rng = np.random.default_rng(B)
    pats = [pattern(KINDS[1 + b % 7], N, M, rng) for b in range(B)]
    ops, rps = [p[0] for p in pats], [p[1] for p in pats]
    seeds = [b % 4 for b in range(B)]
    rs.profile_enable(True)
    try:
        rs.profile_collect()
        d_out, _ = run(torch, rs, "default", N, M, S, ops, rps, seeds=seeds)
        torch.cuda.synchronize()
        names = launches(rs)
    finally:
        rs.profile_enable(False)
    check(d_out.cpu().numpy(), "default", N, M, S, ops, rps, seeds=seeds)
    assert names == ["k_mono_masks<7, %d>" % elems], names


def test_complementary_waves_literal(torch, rs):
    """HighRate 100:300 (2^10 work rows: recovery at rows 0..299, originals at 512..611).  Stripe 0
    receives nothing in work rows 0..127, stripe 1 receives ONLY those rows (128 recovery shards,
    no original): the same wave is live in one stripe and not in the other, for every wave."""
    rate, N, M, S = "high", 100, 300, 64
    assert work_rows(rate, N, M) == (512, 612, 1024)
    rng = np.random.default_rng(5)
    a = _lose(N, M, rng.choice(N, 40, replace=False), np.arange(128, M))
    b = _lose(N, M, np.arange(N), np.arange(0, 128))
    ops, rps = [a[0], b[0], a[0]], [a[1], b[1], a[1]]
    d_out, _ = run(torch, rs, rate, N, M, S, ops, rps)
    torch.cuda.synchronize()
    check(d_out.cpu().numpy(), rate, N, M, S, ops, rps)


# ---------------------------------------------------------------------------
# padded and unaligned layouts

def test_padded_unaligned_layout_keeps_poison(torch, rs):
    """Recovery stripes padded to M + 3 rows, rows 8 bytes wider than the shards, every base
    address 2 bytes off: gap bytes, padding rows and present rows of d_restored keep the poison."""
    rate, N, M, S, B = "default", 64, 64, 64, 3
    pitch = S + 8
    rng = np.random.default_rng(77)
    pats = [pattern(k, N, M, rng) for k in ("random", "one", "all")]
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
    want, v_w = layout(N, POISON)
    for b in range(B):
        v_o[b][ops[b] == 1] = data[b][0][ops[b] == 1]
        v_r[b][rps[b] == 1] = data[b][1][rps[b] == 1]
        v_w[b][ops[b] == 0] = data[b][0][ops[b] == 0]
    d_o, t_o = on_device(h_o, N)
    d_r, t_r = on_device(h_r, M)
    d_x, t_x = on_device(np.full_like(want, POISON), N)
    assert t_x.data_ptr() % 4 == 2
    rs.profile_enable(True)
    try:
        rs.profile_collect()
        rs.decode_device_batch_masks(N, M, S, t_o, np.stack(ops), t_r, np.stack(rps), t_x)
        torch.cuda.synchronize()
        names = launches(rs)
    finally:
        rs.profile_enable(False)
    assert names == ["k_mono_masks<7, 2>"], names
    got = d_x.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at flat offset {bad[:8].tolist()}"
    assert np.array_equal(d_o.cpu().numpy(), h_o) and np.array_equal(d_r.cpu().numpy(), h_r), "inputs were written"


# ---------------------------------------------------------------------------
# status mode

def _one_short(N, M, rng):
    pats = [pattern("random", N, M, rng) for _ in range(5)]
    op, rp = pats[2]
    rp = rp.copy()
    rp[np.flatnonzero(rp)[0]] = 0  # one shard short
    pats[2] = (op, rp)
    return [p[0] for p in pats], [p[1] for p in pats]


def test_undecodable_stripe_all_or_nothing(torch, rs):
    rate, N, M, S = "default", 64, 64, 64
    ops, rps = _one_short(N, M, np.random.default_rng(9))
    B = len(ops)
    data = [_stripe(rate, N, M, S, b) for b in range(B)]
    d_o = _dev(torch, np.stack([d[0] for d in data]))
    d_r = _dev(torch, np.stack([d[1] for d in data]))
    d_out = torch.full((B, N, S), POISON, dtype=torch.uint8, device="cuda")
    with pytest.raises(rs.NotEnoughShards) as e:
        rs.decode_device_batch_masks(N, M, S, d_o, np.stack(ops), d_r, np.stack(rps), d_out)
    assert e.value.stripe == 2
    assert e.value == rs.NotEnoughShards(original_count=N, original_received_count=int(ops[2].sum()),
                                         recovery_received_count=int(rps[2].sum()))
    torch.cuda.synchronize()
    assert bool((d_out == POISON).all()), "nothing may be written when the call fails"


def test_undecodable_stripe_status_mode(torch, rs):
    rate, N, M, S = "default", 64, 64, 64
    ops, rps = _one_short(N, M, np.random.default_rng(9))
    d_out, codes = run(torch, rs, rate, N, M, S, ops, rps, status=True)
    torch.cuda.synchronize()
    assert list(codes) == [0, 0, 7, 0, 0]
    check(d_out.cpu().numpy(), rate, N, M, S, ops, rps)  # (stripe 2: untouched)


# ---------------------------------------------------------------------------
# against the shared-pattern entry, and two calls in flight on one stream

def test_equal_patterns_match_shared_pattern_batch(torch, rs):
    rate, N, M, S, B = "default", 1024, 1024, 64, 4
    op, rp = pattern("random", N, M, np.random.default_rng(3))
    data = [_stripe(rate, N, M, S, b) for b in range(B)]
    d_o = _dev(torch, np.stack([np.where(op[:, None] == 1, d[0], 0xA5).astype(np.uint8) for d in data]))
    d_r = _dev(torch, np.stack([np.where(rp[:, None] == 1, d[1], 0x5A).astype(np.uint8) for d in data]))
    d_a = torch.full((B, N, S), POISON, dtype=torch.uint8, device="cuda")
    d_b = torch.full((B, N, S), POISON, dtype=torch.uint8, device="cuda")
    rs.decode_device_batch(N, M, S, d_o, op, d_r, rp, d_a)
    rs.decode_device_batch_masks(N, M, S, d_o, np.stack([op] * B), d_r, np.stack([rp] * B), d_b)
    torch.cuda.synchronize()
    assert torch.equal(d_a, d_b)
    check(d_b.cpu().numpy(), rate, N, M, S, [op] * B, [rp] * B)


def test_two_calls_back_to_back_on_one_stream(torch, rs):
    """The second call's descriptors must not overwrite staging the first call's copy still reads."""
    rate, N, M, S, B = "default", 256, 256, 64, 3
    rng = np.random.default_rng(21)
    sets = [[pattern(k, N, M, rng) for k in kinds] for kinds in (("random", "all", "one"), ("upper", "one", "random"))]
    data = [_stripe(rate, N, M, S, b) for b in range(B)]
    ins, outs = [], []
    for pats in sets:
        ins.append((_dev(torch, np.stack([np.where(pats[b][0][:, None] == 1, data[b][0], 0xA5).astype(np.uint8) for b in range(B)])),
                    _dev(torch, np.stack([np.where(pats[b][1][:, None] == 1, data[b][1], 0x5A).astype(np.uint8) for b in range(B)]))))
        outs.append(torch.full((B, N, S), POISON, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    for pats, (d_o, d_r), d_x in zip(sets, ins, outs):
        rs.decode_device_batch_masks(N, M, S, d_o, np.stack([p[0] for p in pats]), d_r, np.stack([p[1] for p in pats]),
                                     d_x, stream=s)
    s.synchronize()
    for k, (pats, d_x) in enumerate(zip(sets, outs)):
        check(d_x.cpu().numpy(), rate, N, M, S, [p[0] for p in pats], [p[1] for p in pats], what=f"call {k}")
    rs.release_stream_scratch(s)


# ---------------------------------------------------------------------------
# seeded sweep

SWEEP_SHAPES = {  # (L, rate) -> (N, M) with 2^L work rows
    (7, "high"): (40, 60), (7, "low"): (50, 60), (8, "high"): (100, 100), (8, "low"): (100, 120),
    (9, "high"): (200, 250), (9, "low"): (250, 200), (10, "high"): (300, 500), (10, "low"): (500, 300),
    (11, "high"): (1000, 1000), (11, "low"): (1000, 1000),
}


def _sweep_cases():
    rng = np.random.default_rng(20240607)
    cases = []
    for i in range(24):
        L = 7 + i % 5  # every size several times; the rest drawn
        rate = ("high", "low")[int(rng.integers(2))]
        S = int(rng.choice([64, 70, 128, 576, 1024]))
        B = int(rng.integers(1, 7))
        cases.append((L, rate, S, B, int(rng.integers(1 << 30))))
    return cases


@pytest.mark.parametrize("L,rate,S,B,seed", _sweep_cases())
def test_seeded_sweep(torch, rs, L, rate, S, B, seed):
    N, M = SWEEP_SHAPES[(L, rate)]
    rng = np.random.default_rng(seed)
    ops, rps, losses = [], [], []
    for b in range(B):
        k = int(rng.integers(0, min(N, M) + 1))  # lost originals = received recovery shards
        losses.append(k)
        op, rp = _lose(N, M, rng.choice(N, k, replace=False), rng.choice(M, k, replace=False))
        ops.append(op), rps.append(rp)
    what = f"L={L} {rate} {N}:{M} x {S} B={B} seed={seed} losses={losses}"
    print(what)
    d_out, _ = run(torch, rs, rate, N, M, S, ops, rps)
    torch.cuda.synchronize()
    check(d_out.cpu().numpy(), rate, N, M, S, ops, rps, what=what)
