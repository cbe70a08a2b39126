"""A numpy model of rs_heal_device's contract (include/rs_mi355x.h "heal"), on the CPU oracle and
tests/locate_model.py alone.  No tests here: tests/test_heal_cpu.py and tests/test_gpu_heal.py
import it.

The report (located, flags) is the locate's, for the stripe as found.  Then

    located = i >= 0, mode & ORIGINAL      original_i ^= e,  e = D_j0 / G[j0][i] per column
                                           (j0: the first selected row);        action = ORIGINAL
    located = ROWS, mode & RECOVERY,       every flagged row = the oracle's encode of the
    flags.sum() <= max_rows                stored originals;                   action = RECOVERY
    anything else                          nothing;                             action = 0
"""
import numpy as np

import locate_model as LM
import oracle_lib as O
from test_update_cpu import elements, shard_bytes_of

ORIGINAL, RECOVERY = 1, 2


def gf_div(a, g):
    """a / g element-wise for one nonzero g: a * exp(65535 - log g)."""
    exp, log = LM.tables()
    assert g != 0
    return LM.gf_mul(a, exp[(65535 - log[int(g)]) % 65535])


def heal(rate, orig, rec, mask=None, mode=ORIGINAL | RECOVERY, max_rows=0):
    """(located, flags [M] uint8, action, orig_after, rec_after) of one stripe under the contract.
    The two matrices are copies; the inputs are left as they were."""
    N, M = orig.shape[0], rec.shape[0]
    S = orig.shape[1]
    sel = np.flatnonzero(np.ones(M, bool) if mask is None else np.asarray(mask) != 0)
    want = O.encode(rate, orig, M)
    D = elements(want ^ rec).astype(np.int64)
    located, flags = LM.locate(rate, orig, rec, mask=mask, D=D)
    orig_after, rec_after = orig.copy(), rec.copy()
    action = 0
    if located >= 0 and mode & ORIGINAL:
        j0 = int(sel[0])
        e = gf_div(D[j0], LM.coefficients(rate, N, M)[j0, located])
        orig_after[located] ^= shard_bytes_of(e[None, :].astype(np.uint16), S)[0]
        action = ORIGINAL
    elif located == LM.ROWS and mode & RECOVERY and int(flags.sum()) <= max_rows:
        rows = np.flatnonzero(flags)
        rec_after[rows] = want[rows]
        action = RECOVERY
    return located, flags, action, orig_after, rec_after
