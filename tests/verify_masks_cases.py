"""The constructed batches of tests/test_verify_masks_cpu.py, tests/test_gpu_verify_masks.py and
tests/test_gpu_locate_masks.py: stripes with a recovery-row mask of their own.  No tests here.

Ground truth is constructed, never computed by the code under test.  Recovery shards come from the
CPU oracle; the rows a stripe's mask leaves out are overwritten with junk that differs from stripe
to stripe (they stand for rows that no longer exist); chosen bytes of selected rows and of
originals are then flipped, and the expected flags are the selected rows touched (for a corrupt
original: the selected rows where the oracle's encode of the stored originals differs).
"""
import numpy as np

import oracle_lib as O

RATE = {"default": 0, "high": 1, "low": 2}

# (S, row padding): whole blocks; a tail; a tail with rows that are not 4-byte aligned (byte-wise)
LAYOUTS = [(64, 0), (72, 0), (66, 4)]
# the encode is the staged single-chunk column kernel: L = 7 at both rates, the lane shape, the headline
FUSED = [(r, n, m, s, p) for r, n, m in (("high", 70, 100), ("low", 100, 70), ("default", 200, 200))
         for s, p in LAYOUTS] + [("default", 1024, 1024, 72, 0)]
# k_pass, k_chunks with unaligned rows, multi-chunk LowRate, the pass kernels of 2^12 rows
UNFUSED = [("default", 3, 5, 2, 0), ("high", 1000, 100, 66, 0), ("low", 128, 1024, 64, 0),
           ("default", 4096, 4096, 64, 0)]

CLEAN, ROWS, UNKNOWN, SKIPPED = -1, -2, -3, -4

_CACHE = {}


def _rows(M, *idx):
    m = np.zeros(M, np.uint8)
    m[list(idx)] = 1
    return m


def verify_masks(M):
    """7 stripes: every row; row 0 only; the last row only; two rows far apart (the union span is
    the whole matrix, the stripe's own two rows); every third row out; nothing; rows 2.. (its
    first selected row is not the union's first)."""
    third = np.ones(M, np.uint8)
    third[1::3] = 0
    late = np.ones(M, np.uint8)
    late[:2] = 0
    return np.stack([np.ones(M, np.uint8), _rows(M, 0), _rows(M, M - 1), _rows(M, 0, M - 1), third,
                     np.zeros(M, np.uint8), late])


def locate_masks(M):
    """8 stripes: verify_masks' with the empty stripe replaced (a locate skips the two one-row
    stripes, 1 and 2) and two more that select most rows."""
    m = verify_masks(M)
    most = np.ones(M, np.uint8)
    most[1] = 0
    some = np.ones(M, np.uint8)
    some[[0, 2]] = 0
    if M > 8:
        some[M // 2::5] = 0
    return np.stack([m[0], m[1], m[2], m[3], m[4], m[6], most, some])


def _clean(rate, N, M, S, B):
    key = ("clean", rate, N, M, S, B)
    if key not in _CACHE:
        pairs = []
        for b in range(B):
            orig = O.generate_original(N, S, b)
            pairs.append((orig, O.encode(rate, orig, M)))
        origs, recs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        origs.setflags(write=False)
        recs.setflags(write=False)
        _CACHE[key] = (origs, recs)
    return _CACHE[key]


def _junk(recs, masks, seed):
    """The rows a stripe's mask leaves out hold junk, different in every stripe."""
    rng = np.random.default_rng(seed)
    held = recs.copy()
    for b in range(len(masks)):
        out = masks[b] == 0
        held[b][out] = rng.integers(0, 256, (int(out.sum()), recs.shape[2]), dtype=np.uint8)
        # junk must differ from the right row (a 2-byte shard could repeat it by chance)
        held[b][out] ^= (held[b][out] == recs[b][out]).all(axis=1, keepdims=True).astype(np.uint8)
    return held


def verify_batch(rate, N, M, S):
    """(clean originals, clean recovery, stored originals, stored recovery, masks, expected flags)
    of the verify's batch; computed once, read-only."""
    key = ("verify", rate, N, M, S)
    if key in _CACHE:
        return _CACHE[key]
    masks = verify_masks(M)
    B = len(masks)
    origs, recs = _clean(rate, N, M, S, B)
    held, store = _junk(recs, masks, 1000 + M), origs.copy()
    want = np.zeros((B, M), np.uint8)

    def flip(b, j, col, bit):
        held[b, j, col % S] ^= bit
        want[b, j] = masks[b, j]

    flip(0, 0, 0, 0x01)          # row 0: selected and corrupt in stripe 0, unselected junk in stripe 6
    flip(0, M - 1, S - 1, 0x80)  # the last byte of the last row
    flip(0, M // 2, 5, 0x10)
    flip(1, 0, 3, 0x02)          # the one row of stripe 1; stripe 2's one row stays right
    flip(3, M - 1, 1, 0x40)      # the far one of stripe 3's two rows
    flip(6, 2, 7, 0x08)          # stripe 6's own first row, and its last
    flip(6, M - 1, 0, 0x04)
    # stripe 4: a corrupt original -- the stored recovery no longer belongs to the stored originals
    store[4, N // 2, (S // 3) % S] ^= 0x04
    want[4] = (O.encode(rate, store[4], M) != recs[4]).any(axis=1) & (masks[4] != 0)
    assert want[4].any() and want[5].sum() == 0 and want[2].sum() == 0
    assert held[6, 0].tobytes() != recs[6, 0].tobytes() and want[0, 0] == 1 and want[6, 0] == 0
    out = (origs, recs, store, held, masks, want)
    for a in out:
        a.setflags(write=False)
    _CACHE[key] = out
    return out


# the outcome each stripe of the locate's batch is built for (N: original_count)
def locate_intent(N):
    return [0, SKIPPED, SKIPPED, N // 2, UNKNOWN, N - 1, ROWS, CLEAN]


def locate_batch(rate, N, M, S):
    """(clean originals, clean recovery, stored originals, stored recovery, masks, intended located,
    expected flags) of the locate's batch; computed once, read-only.  Stripes 1 and 2 select one
    row: all or nothing refuses the batch at stripe 1, status mode skips both."""
    key = ("locate", rate, N, M, S)
    if key in _CACHE:
        return _CACHE[key]
    masks = locate_masks(M)
    B = len(masks)
    origs, recs = _clean(rate, N, M, S, B)
    held, store = _junk(recs, masks, 2000 + M), origs.copy()
    store[0, 0, 0] ^= 0x01                      # one corrupt original: 0, N / 2, N - 1
    store[3, N // 2, (S // 3) % S] ^= 0x20
    store[5, N - 1, S - 1] ^= 0x80
    # two corrupt originals, in two columns of one pack where the shard has two (in one column their
    # contributions can cancel in some row, which would be ROWS: include/rs_mi355x.h RS_LOCATE_ROWS)
    store[4, 0, 0] ^= 0x01
    store[4, N - 1, 1 if S >= 4 else 0] ^= 0x02
    sel6 = np.flatnonzero(masks[6])
    held[6, sel6[len(sel6) // 2], 5 % S] ^= 0x10  # one selected recovery row; the others agree
    intent = np.array(locate_intent(N), np.int32)
    want = np.zeros((B, M), np.uint8)
    for b in range(B):
        if intent[b] == SKIPPED:
            continue
        want[b] = (O.encode(rate, store[b], M) != held[b]).any(axis=1) & (masks[b] != 0)
    out = (origs, recs, store, held, masks, intent, want)
    for a in out:
        a.setflags(write=False)
    _CACHE[key] = out
    return out
