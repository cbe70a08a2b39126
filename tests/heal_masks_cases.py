"""The constructed batch of tests/test_heal_masks_cpu.py and tests/test_gpu_heal_masks.py: 8 stripes,
each with a recovery-row mask of its own and built for a different outcome of a heal.  No tests here.

Ground truth is constructed as in tests/verify_masks_cases.py (whose clean stripes, junk and shapes
these are): recovery shards from the CPU oracle, per-stripe junk in the rows a mask leaves out, then
chosen bytes flipped.  What a heal must leave behind is tests/heal_model.py's answer stripe by
stripe, each with its own mask; it is computed once per (shape, mode, max_rows) and read-only.
"""
import numpy as np

import heal_model as HM
import verify_masks_cases as C

CLEAN, ROWS, UNKNOWN, SKIPPED = C.CLEAN, C.ROWS, C.UNKNOWN, C.SKIPPED
ORIGINAL, RECOVERY = HM.ORIGINAL, HM.RECOVERY

_CACHE = {}


def heal_masks(M):
    """8 stripes: every row; row 0 only; rows {0, M - 1}; rows {0, M // 2, M - 1} (exactly three);
    every third row out; rows 2.. (its first selected row is not the union's first); every row but
    row 1; every row but rows 0 and 2 (and M // 2 :: 5 where M > 8)."""
    m = np.ones((8, M), np.uint8)
    m[1] = 0
    m[1, 0] = 1
    m[2] = 0
    m[2, [0, M - 1]] = 1
    m[3] = 0
    m[3, [0, M // 2, M - 1]] = 1
    m[4, 1::3] = 0
    m[5, :2] = 0
    m[6, 1] = 0
    m[7, [0, 2]] = 0
    if M > 8:
        m[7, M // 2::5] = 0
    return m


def need(mode):
    """The selected rows a stripe needs (include/rs_mi355x.h: three to write an original)."""
    return 3 if mode & ORIGINAL else 2


# the outcome each stripe is built for with both mode bits and max_rows = 2 (N: original_count)
def heal_intent(N):
    located = [0, SKIPPED, SKIPPED, N // 2, UNKNOWN, N - 1, ROWS, CLEAN]
    action = [ORIGINAL, 0, 0, ORIGINAL, 0, ORIGINAL, RECOVERY, 0]
    return np.array(located, np.int32), np.array(action, np.uint8)


def heal_batch(rate, N, M, S):
    """(clean originals, clean recovery, stored originals, stored recovery, masks) of the heal's
    batch; computed once, read-only."""
    key = ("heal", rate, N, M, S)
    if key in _CACHE:
        return _CACHE[key]
    masks = heal_masks(M)
    B = len(masks)
    origs, recs = C._clean(rate, N, M, S, B)
    held, store = C._junk(recs, masks, 3000 + M), origs.copy()
    store[0, 0, 0] ^= 0x01
    for b in (2, 3):  # stripe 2 has two rows: located with the recovery bit alone, never healed
        store[b, N // 2, (S // 3) % S] ^= 0x20
    # two corrupt originals, in two columns of one pack where the shard has two: UNKNOWN
    store[4, 0, 0] ^= 0x01
    store[4, N - 1, 1 if S >= 4 else 0] ^= 0x02
    store[5, N - 1, S - 1] ^= 0x80  # the tail's last high byte; its e comes from row 2
    sel6 = np.flatnonzero(masks[6])
    held[6, sel6[0], 5 % S] ^= 0x10  # its first and its last selected row: two rows differ
    held[6, sel6[-1], S - 1] ^= 0x80
    out = (origs, recs, store, held, masks)
    for a in out:
        a.setflags(write=False)
    _CACHE[key] = out
    return out


def model(rate, N, M, S, mode=ORIGINAL | RECOVERY, max_rows=2, masks=None, store=None, held=None):
    """heal_model.heal stripe by stripe, each with its own mask: (located [B], flags [B, M],
    action [B], originals after, recovery after, status codes [B]).  A stripe that selects fewer
    than need(mode) rows is skipped: SKIPPED, flags 0, action 0, untouched, code 101.  The default
    batch's answer is computed once per (shape, mode, max_rows) and read-only."""
    key = ("model", rate, N, M, S, mode, max_rows)
    default = masks is None and store is None and held is None
    if default and key in _CACHE:
        return _CACHE[key]
    _, _, store0, held0, masks0 = heal_batch(rate, N, M, S)
    masks = masks0 if masks is None else masks
    store = store0 if store is None else store
    held = held0 if held is None else held
    B = len(masks)
    located, action = np.zeros(B, np.int32), np.zeros(B, np.uint8)
    flags, codes = np.zeros((B, M), np.uint8), np.zeros(B, np.uint8)
    o2, r2 = np.array(store), np.array(held)
    for b in range(B):
        if masks[b].sum() < need(mode):
            located[b], codes[b] = SKIPPED, 101
            continue
        located[b], flags[b], action[b], o2[b], r2[b] = HM.heal(rate, store[b], held[b], mask=masks[b], mode=mode,
                                                                max_rows=max_rows)
    out = (located, flags, action, o2, r2, codes)
    if default:
        for a in out:
            a.setflags(write=False)
        _CACHE[key] = out
    return out
