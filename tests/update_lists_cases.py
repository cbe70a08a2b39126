"""Case builders of tests/test_gpu_update_lists.py (rs_update_device_batch_lists).  No tests here.

A batch is B stripes of one shape, each with its own index list; the expected recovery matrix of
every stripe is the CPU oracle's encode of the stripe with its originals replaced.  Everything the
oracle computes is computed once per key, shared, and read-only.
"""
import numpy as np

import oracle_lib as O
import wide_cases as W

RATE = {"default": 0, "high": 1, "low": 2}
FILL = 0xC3

_STRIPES, _BATCHES = {}, {}


def stripe(rate, N, M, S, seed=0):
    """(originals, their recovery shards) from the oracle, read-only."""
    key = (rate, N, M, S, seed)
    if key not in _STRIPES:
        orig = O.generate_original(N, S, seed)
        rec = O.encode(rate, orig, M)
        orig.setflags(write=False)
        rec.setflags(write=False)
        _STRIPES[key] = (orig, rec)
    return _STRIPES[key]


def some_indices(N, count, rng):
    """`count` (at most N) distinct originals: the last and the first and random ones between,
    handed over out of order."""
    count = min(count, N)
    if count == 1:
        return [N - 1]
    rest = rng.choice(np.arange(1, N - 1), count - 2, replace=False).tolist() if count > 2 else []
    return [N - 1] + rest + [0]


def mixed_lists(N, seed=0):
    """7 stripes whose lists differ: the last original; the first; counts 2 and 16 (first and last
    plus random ones, out of order); 17, a second delta tile; nothing; stripe 0's original again."""
    rng = np.random.default_rng([N, seed])
    return [[N - 1], [0], some_indices(N, 2, rng), some_indices(N, 16, rng), some_indices(N, 17, rng), [],
            [N - 1]]


class Batch:
    """olds / news [B, K, S] (rows past a stripe's count zero), recs / wants [B, M, S], read-only."""

    def __init__(self, rate, N, M, S, lists, positional=False):
        self.rate, self.N, self.M, self.S, self.lists = rate, N, M, S, [list(x) for x in lists]
        B, K = len(lists), max(len(x) for x in lists)
        self.B, self.K = B, K
        self.olds, self.news = np.zeros((B, K, S), np.uint8), np.zeros((B, K, S), np.uint8)
        self.recs, self.wants = np.zeros((B, M, S), np.uint8), np.zeros((B, M, S), np.uint8)
        for b, idx in enumerate(self.lists):
            orig, rec = stripe(rate, N, M, S, b % 3)
            self.recs[b] = self.wants[b] = rec
            if not idx:
                continue
            new = O.generate_original(len(idx), S, 100 + b)
            if positional and len(idx) > 1:  # the changed bytes in the last pack / in pack 0 alone
                new = W.update_new_rows(orig[idx], new)
            mod = orig.copy()
            mod[idx] = new
            self.olds[b, :len(idx)], self.news[b, :len(idx)] = orig[idx], new
            self.wants[b] = O.encode(rate, mod, M)
        for a in (self.olds, self.news, self.recs, self.wants):
            a.setflags(write=False)

    def inputs(self, form, junk_seed, slack=0):
        """(d_old or None, d_new) as host arrays [B, K + slack, S]: every row past a stripe's count
        holds junk drawn from junk_seed."""
        rng = np.random.default_rng(junk_seed)
        K = self.K + slack
        old = rng.integers(0, 256, (self.B, K, self.S), dtype=np.uint8)
        new = rng.integers(0, 256, (self.B, K, self.S), dtype=np.uint8)
        for b, idx in enumerate(self.lists):
            old[b, :len(idx)], new[b, :len(idx)] = self.olds[b, :len(idx)], self.news[b, :len(idx)]
            if form == "delta":
                new[b, :len(idx)] ^= old[b, :len(idx)]
        return (None if form == "delta" else old), new

    def masked(self, masks, junk_seed=7):
        """(recovery matrix to hand in, expected result) under per-stripe masks [B, M]: unselected
        rows hold junk of their own and keep it."""
        held = self.recs.copy()
        junk = np.random.default_rng(junk_seed).integers(0, 256, held.shape, dtype=np.uint8)
        off = np.asarray(masks) == 0
        held[off] = junk[off]
        want = np.where(off[:, :, None], held, self.wants)
        for b, idx in enumerate(self.lists):
            if not idx:
                want[b] = held[b]
        return held, want


def batch(rate, N, M, S, lists=None, positional=False):
    lists = mixed_lists(N) if lists is None else lists
    key = (rate, N, M, S, tuple(tuple(x) for x in lists), positional)
    if key not in _BATCHES:
        _BATCHES[key] = Batch(rate, N, M, S, lists, positional)
    return _BATCHES[key]


def stripe_masks(B, M):
    """Masks in rotation over the stripes: every row; row 0 only; the last row only; every third
    row out; nothing."""
    kinds = np.ones((5, M), np.uint8)
    kinds[1] = 0
    kinds[1, 0] = 1
    kinds[2] = 0
    kinds[2, M - 1] = 1
    kinds[3, 1::3] = 0
    kinds[4] = 0
    return np.stack([kinds[b % 5] for b in range(B)])


def place(torch, a, base=0, row_pad=0, stripe_pad=0):
    """A device copy of a [B, rows, S] inside a FILLed buffer: `base` bytes in front, row_pad bytes
    after every row, stripe_pad bytes after every stripe.  Returns (view, buffer, covered) with
    covered the boolean host map of the buffer's bytes that belong to rows."""
    B, rows, S = a.shape
    rs_, ss = S + row_pad, rows * (S + row_pad) + stripe_pad
    n = base + B * ss
    buf = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    v = torch.as_strided(buf, (B, rows, S), (ss, rs_, 1), base)
    v.copy_(torch.from_numpy(np.array(a, copy=True)).cuda())
    covered = np.zeros(n, bool)
    at = base + (np.arange(B)[:, None, None] * ss + np.arange(rows)[None, :, None] * rs_ + np.arange(S)[None, None, :])
    covered[at.reshape(-1)] = True
    return v, buf, covered


def untouched(buf, covered):
    return bool((buf.cpu().numpy()[~covered] == FILL).all())
