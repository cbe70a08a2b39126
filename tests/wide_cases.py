"""Shard sizes and positional damage for the scrub calls (verify, locate, heal, update and their robust,
degraded and per-stripe-mask forms) past one wave, one pack tile and one scan step.  No tests here:
tests/test_wide_shards_cpu.py and tests/test_gpu_wide_shards.py import it, and the case builders of the
families' own GPU files take its positional cases through an optional argument.

The per-pack kernels of these families (k_verify_rows, k_locate_confirm, k_heal, k_update, ...) run one
thread per pack.  A shard of S bytes has packs_of(S) packs -- 8 per whole 64-byte block, one per 4
elements of the tail (rs_codec.cpp packs_of) -- and the launch shape is

    threads = packs >= TILE ? TILE : ceil(packs / WAVE) * WAVE        tiles = ceil(packs / threads)

The thresholds in S, each with the constant it comes from (tests/test_wide_shards_cpu.py reads the
constants back out of the sources, so that a default that moves fails there and not silently here):

    packs > WAVE (64)            S > 512    a second wave in the workgroup
    packs > E2_MAX_PACKS (128)   S > 1024   packs x stripes past rs_context::e2_max_packs (half the CU
                                            count, 256 / 2 on this chip): 4-element packs, not 2
    packs > TILE (256)           S > 2048   a second pack tile: blockIdx.x != 0, dead lanes beside live
                                            ones in the last tile, rows_per_group sees tiles > 1
    packs > MONO_MAX_PACKS (256) S > 2048   rs_context::mono_max_packs: use_mono is false -- no column
                                            kernel, no fused verify, no fused repair under the degraded
                                            calls, batches run one stripe per group
    packs > FIND_STEP (1024)     S > 8192   k_locate_find* scan kFindThreads * kFindUnroll packs per
                                            step: a second step (unroll slots 1..3 hold packs 256..1023)

SIZES is the table of the sizes that sit on these edges; damage goes by pack number (damage_pack), at
the positions either side of each edge (positions).
"""
import numpy as np

WAVE = 64            # lanes of a wave
TILE = 256           # threads of a full per-pack workgroup (the launch shape above)
E2_MAX_PACKS = 128   # rs_context::e2_max_packs on a 256-CU chip
MONO_MAX_PACKS = 256  # rs_context::mono_max_packs
FIND_THREADS, FIND_UNROLL = 256, 4  # rs_locate.hip / rs_locate_robust.hip kFindThreads, kFindUnroll
FIND_STEP = FIND_THREADS * FIND_UNROLL

# (S, row padding, packs, what it reaches)
SIZES = [
    (520, 0, 65, "a second wave with one live lane (threads = 128)"),
    (1032, 0, 129, "one stripe past the 2-element pack bound: 4-element packs by default"),
    (2048, 0, 256, "a full 256-thread workgroup, one tile; the last size on the column kernel"),
    (2056, 0, 257, "two tiles, one live thread in the second; column kernel off, group = 1"),
    (2050, 4, 257, "the same with a one-element tail pack and byte-wise rows"),
    (8200, 0, 1025, "the find's second scan step holding a single pack; 5 tiles"),
    (65536, 0, 8192, "64 KiB: 32 tiles, 8 scan steps"),
]


# (rate, N, M): on the column kernel up to 2048 bytes, off it from 2056; run at every size of the table
COLUMN = [("high", 70, 100), ("low", 100, 70)]
# (rate, N, M, S, row padding): the lane shape either side of the edge, a shape that is never on the
# column kernel, and the scrub shape at 1 KiB
OTHER = [("default", 200, 200, 2048, 0), ("default", 200, 200, 2056, 0), ("high", 1000, 100, 2056, 0),
         ("default", 1024, 1024, 1024, 0)]
# the column-kernel shapes: their encode is k_mono* / k_lane up to MONO_MAX_PACKS packs
ON_COLUMN = {(70, 100), (100, 70), (200, 200), (1024, 1024)}
# (rate, N, M, S) of the update
UPDATE = [(r, n, m, s) for r, n, m in (("default", 100, 30), ("default", 30, 100)) for s in (2056, 8200, 65536)]


def shapes():
    """[(rate, N, M, S, row padding)] every family runs at."""
    return [(r, n, m, s, pad) for r, n, m in COLUMN for s, pad, _, _ in SIZES] + OTHER


def packs_of(S):
    """rs_codec.cpp packs_of: 8 packs per whole block, one per 4 elements of the tail."""
    return S // 64 * 8 + ((S % 64) // 2 + 3) // 4


def launch_shape(packs):
    """(threads, tiles) of a per-pack launch."""
    threads = TILE if packs >= TILE else (packs + WAVE - 1) // WAVE * WAVE
    return threads, (packs + threads - 1) // threads


def find_steps(packs):
    return (packs + FIND_STEP - 1) // FIND_STEP


def pack_columns(S, p):
    """(low-half columns, high-half columns) of pack p in the caller's layout (rs_device.hpp pack_io):
    a whole block's pack p % 8 has 4 low bytes at 4 (p % 8) and 4 high bytes 32 further; tail pack q of
    a tail of th elements has its low bytes at 4q .. and its high bytes th further, min(4, th - 4q) of
    each (the layout test_gpu_locate.damage_original's `lastpack` encodes)."""
    full, th = S // 64, (S % 64) // 2
    assert 0 <= p < packs_of(S)
    if p < full * 8:
        lo = (p // 8) * 64 + (p % 8) * 4
        return np.arange(lo, lo + 4), np.arange(lo + 32, lo + 36)
    e = 4 * (p - full * 8)
    cnt = min(4, th - e)
    lo = full * 64 + e
    return np.arange(lo, lo + cnt), np.arange(lo + th, lo + th + cnt)


def positions(S):
    """The pack positions damage is placed at: either side of the wave, tile and scan-step edges, and
    the last pack -- those that exist at S."""
    packs = packs_of(S)
    edges = (WAVE - 1, WAVE, TILE - 1, TILE, FIND_STEP - 1, FIND_STEP, packs - 1)
    return sorted({p for p in edges if p < packs})


def damage_pack(a, row, p, rng):
    """Flip one random non-zero byte value into one random byte of pack p of row `row`, in place (an
    original or a recovery row); the column."""
    lo, hi = pack_columns(a.shape[1], p)
    col = int(rng.choice(np.concatenate([lo, hi])))
    a[row, col] ^= np.uint8(rng.integers(1, 256))
    return col


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


# ---- verify ---------------------------------------------------------------------------------------

def verify_kinds(N, M, S):
    """The corruptions of a wide verify, as kinds for test_gpu_verify.corrupt: clean; one recovery row
    at each pack position, spread over rows 0, M // 2, M - 1; every row, each at its own pack; one
    original in the last pack."""
    rows = [0, M // 2, M - 1]
    kinds = ["none"]
    kinds += [("row", rows[k % 3], p) for k, p in enumerate(positions(S))]
    kinds += [("every row",), ("original", N // 2, packs_of(S) - 1)]
    return kinds


def every_row_packs(M, S):
    """Row j's pack when every row is damaged: spread over the whole shard, row 0 in pack 0 and the
    last row in the last pack; different for every row where there are packs enough."""
    packs = packs_of(S)
    if M == 1:
        return [packs - 1]
    return [j * (packs - 1) // (M - 1) for j in range(M)]


def verify_corrupt(kind, orig, rec, encode):
    """(originals, recovery, expected flags) after corruption `kind` (a tuple of verify_kinds) of the
    clean stripe; encode(originals) is the oracle's."""
    N, S = orig.shape
    M = rec.shape[0]
    orig, rec = orig.copy(), rec.copy()
    want = np.zeros(M, np.uint8)
    if kind[0] == "row":
        _, j, p = kind
        damage_pack(rec, j, p, _rng(S, j, p))
        want[j] = 1
    elif kind[0] == "every row":
        rng = _rng(S, M)
        for j, p in enumerate(every_row_packs(M, S)):
            damage_pack(rec, j, p, rng)
        want[:] = 1
    else:
        assert kind[0] == "original"
        _, i, p = kind
        damage_pack(orig, i, p, _rng(S, i, p, 1))
        want = (encode(orig) != rec).any(axis=1).astype(np.uint8)
        assert want.any()
    return orig, rec, want


# ---- locate and heal ------------------------------------------------------------------------------

def locate_cases(orig, rec, CLEAN=-1, ROWS=-2, UNKNOWN=-3):
    """[(name, originals, recovery, intended status)] of one wide stripe, in the form of
    test_gpu_locate.cases: one original damaged at every pack position in turn (originals 0, N // 2 and
    N - 1 in rotation) and each of the three as a whole shard; two originals in different tiles; an original in pack 0 with a recovery row whose only
    damage is in the last pack (the confirm must refute from there); recovery rows alone, in three
    different tiles where there are three."""
    N, S = orig.shape
    M = rec.shape[0]
    packs = packs_of(S)
    rng = _rng(N, M, S)
    out = [("none", orig, rec, CLEAN)]
    three = sorted({0, N // 2, N - 1})
    for k, p in enumerate(positions(S)):  # every position in turn, the three originals in rotation
        i = three[k % len(three)]
        bad = orig.copy()
        damage_pack(bad, i, p, rng)
        out.append((f"original {i} pack {p}", bad, rec, i))
    for i in three:
        bad = orig.copy()
        bad[i] ^= rng.integers(1, 256, S, dtype=np.uint8)
        out.append((f"original {i} shard", bad, rec, i))
    bad = orig.copy()
    damage_pack(bad, 0, 0, rng)
    damage_pack(bad, N - 1, packs - 1, rng)
    out.append((f"two originals, packs 0 and {packs - 1}", bad, rec, UNKNOWN))
    bad, badr = orig.copy(), rec.copy()
    damage_pack(bad, N - 1, 0, rng)
    damage_pack(badr, M // 2, packs - 1, rng)
    out.append((f"original pack 0 and recovery row {M // 2} pack {packs - 1}", bad, badr, UNKNOWN))
    badr = rec.copy()
    spread = sorted({0, packs // 2, packs - 1})
    for j, p in zip([0, M // 2, M - 1], spread):
        damage_pack(badr, j, p, rng)
    out.append((f"recovery rows, packs {spread}", orig, badr, ROWS))
    return out


# ---- a mask per stripe ----------------------------------------------------------------------------

def stripe_masks(M):
    """4 stripes: every row; two rows far apart; all but every third; rows 2.. ."""
    m = np.ones((4, M), np.uint8)
    m[1] = 0
    m[1, [0, M - 1]] = 1
    m[2, 1::3] = 0
    m[3, :2] = 0
    return m


def masks_intent(N, ROWS=-2, CLEAN=-1):
    """The outcome each stripe of masks_batch is built for."""
    return np.array([0, ROWS, N - 1, CLEAN], np.int32)


def masks_batch(origs, recs, encode):
    """(stored originals, stored recovery, masks, intended located, expected flags) of a batch of 4
    clean stripes origs [4, N, S], recs [4, M, S] with a mask each.  Every unselected row holds junk of
    its own that differs from the right row in the last pack alone -- a compare that looked at it there
    would flag it, a heal that took it for selected would rewrite it.  Stripe 0: original 0 corrupt in
    the last pack; stripe 1 (rows 0 and M - 1): row M - 1 corrupt in the last pack, ROWS; stripe 2:
    original N - 1 corrupt in pack 0; stripe 3: clean.  encode(b, originals): the oracle's."""
    B, N, S = origs.shape
    M = recs.shape[1]
    assert B == 4
    packs = packs_of(S)
    masks = stripe_masks(M)
    rng = _rng(N, M, S, 4)
    store, held = origs.copy(), recs.copy()
    for b in range(B):
        for j in np.flatnonzero(masks[b] == 0):
            damage_pack(held[b], int(j), packs - 1, rng)
    damage_pack(store[0], 0, packs - 1, rng)
    damage_pack(held[1], M - 1, packs - 1, rng)
    damage_pack(store[2], N - 1, 0, rng)
    want = np.stack([(encode(b, store[b]) != held[b]).any(axis=1) & (masks[b] != 0) for b in range(B)]).astype(np.uint8)
    return store, held, masks, masks_intent(N), want


# ---- update ---------------------------------------------------------------------------------------

def update_new_rows(old, new):
    """`new` with its first row differing from `old` in the last pack only and, where there are two
    rows or more, its second in pack 0 only; the other rows are left as generated."""
    S = old.shape[1]
    out = new.copy()
    rng = _rng(S, len(old))
    out[0] = old[0]
    damage_pack(out, 0, packs_of(S) - 1, rng)
    if len(old) > 1:
        out[1] = old[1]
        damage_pack(out, 1, 0, rng)
    return out
