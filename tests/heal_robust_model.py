"""A numpy model of rs_heal_device_robust's contract (include/rs_mi355x.h "robust heal"), on the CPU
oracle, tests/locate_robust_model.py and tests/heal_model.py's division alone.  No tests here:
tests/test_heal_robust_cpu.py and tests/test_gpu_heal_robust.py import it.

The report (located, flags, outlier) is the robust locate's, for the stripe as found.  Then, with
want = the oracle's encode of the STORED originals and D = want ^ recovery,

    located = i >= 0, outlier set B        e = D_r / G[r][i] per column, r the first selected row
                                           outside B
      mode & ORIGINAL                      original_i ^= e;                          action |= ORIGINAL
      mode & RECOVERY, B not empty         row j of B = want_j ^ G[j][i] * e;        action |= RECOVERY
    located = ROWS, mode & RECOVERY,       every flagged row = want of that row;
    flags.sum() <= max_rows                                                         action = RECOVERY
    anything else                          nothing;                                  action = 0
"""
import numpy as np

import locate_model as LM
import locate_robust_model as RM
import oracle_lib as O
from heal_model import ORIGINAL, RECOVERY, gf_div
from test_update_cpu import elements, shard_bytes_of


def error(rate, N, M, D, located, r):
    """e = D_r / G[r][located] per column."""
    return gf_div(D[r], LM.coefficients(rate, N, M)[r, located])


def heal(rate, orig, rec, t, mask=None, mode=ORIGINAL | RECOVERY, max_rows=0, want=None):
    """(located, flags [M] uint8, outlier [M] uint8, action, orig_after, rec_after) of one stripe
    under the contract.  The two matrices are copies; the inputs are left as they were.  want: the
    oracle's encode of `orig`, where the caller has it."""
    N, M = orig.shape[0], rec.shape[0]
    S = orig.shape[1]
    sel = np.flatnonzero(np.ones(M, bool) if mask is None else np.asarray(mask) != 0)
    if want is None:
        want = O.encode(rate, orig, M)
    D = elements(want ^ rec).astype(np.int64)
    located, flags, outlier = RM.locate(rate, orig, rec, t, mask=mask, D=D)
    orig_after, rec_after = orig.copy(), rec.copy()
    action = 0
    if located >= 0:
        r = int(next(j for j in sel if not outlier[j]))
        e = error(rate, N, M, D, located, r)
        if mode & ORIGINAL:
            orig_after[located] ^= shard_bytes_of(e[None, :].astype(np.uint16), S)[0]
            action |= ORIGINAL
        B = np.flatnonzero(outlier)
        if mode & RECOVERY and len(B):
            G = LM.coefficients(rate, N, M)
            fix = np.stack([LM.gf_mul(e, G[j, located]) for j in B])  # (a zero coefficient: nothing)
            rec_after[B] = want[B] ^ shard_bytes_of(fix.astype(np.uint16), S)
            action |= RECOVERY
    elif located == RM.ROWS and mode & RECOVERY and int(flags.sum()) <= max_rows:
        rows = np.flatnonzero(flags)
        rec_after[rows] = want[rows]
        action = RECOVERY
    return located, flags, outlier, action, orig_after, rec_after
