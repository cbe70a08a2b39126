"""A numpy model of rs_heal_device_degraded's contract (include/rs_mi355x.h "degraded heal"), on
the CPU oracle, tests/locate_degraded_model.py and tests/heal_model.py alone.  No tests here:
tests/test_heal_degraded_cpu.py and tests/test_gpu_heal_degraded.py import it.

Notation is the degraded locate's (m missing originals, R the reference rows, K the check rows, F
the originals completed from R, D = encode(F) ^ recovery, T the table over information positions).

    U    [m, N]: U[r][q] = the element that the decode from R puts into the r-th missing original
         when information position q holds the element 1 and every other one holds zero -- the
         restored rows of the unit stripe that T's second oracle call starts from

The report (located, flags) is the degraded locate's, for the stripe as found.  With q the located
information position, j0 = K[0] and e = D_j0 / T[j0][q] per column:

    located = i < N, mode & ORIGINAL       original_i ^= e; restored row of the r-th missing
                                           original = F ^ U[r][i] * e;          action = ORIGINAL
    located = N + j, mode & RECOVERY       recovery_j ^= e; the restored rows the same way with
                                           that row's position;                 action = RECOVERY
    located = ROWS, mode & RECOVERY,       every flagged row of K = the oracle's encode of F; the
    flags.sum() <= max_rows                restored rows are F's;               action = RECOVERY
    anything else                          the restored rows are F's;           action = 0

Only the missing originals' rows of the restored matrix are written.

The algebra was checked with this model on the oracle (tests/test_heal_degraded_cpu.py runs it): 96
constructed stripes over 3:5, 12:5 high, 5:12 low, 70:100 high, 100:70 low and 200:200, each at
shard sizes 64, 72 and 66, with m = 1 and m = min(N, M - 3), each carrying one corrupt present
original (a whole shard, or the last high bit of the tail) or one flipped bit in the last
reference row.  In all of them the two corrections give back the clean stripe byte for byte, and no
U[r][q] is zero: the codeword with 1 at q and 0 at the other N - 1 information positions would
otherwise have N zeros, and an [N + M, N] MDS code allows N - 1 at most.
"""
import numpy as np

import heal_model as HM
import locate_degraded_model as DM
import locate_model as LM
import oracle_lib as O
from test_update_cpu import elements, shard_bytes_of

ORIGINAL, RECOVERY = HM.ORIGINAL, HM.RECOVERY
CLEAN, ROWS, UNKNOWN = DM.CLEAN, DM.ROWS, DM.UNKNOWN

_U = {}


def restored_coefficients(rate, N, M, present, R):
    """U [m, N] uint16, from the unit stripe of DM.coefficients.  Once per key."""
    present = np.asarray(present) != 0
    key = (rate, N, M, present.tobytes(), tuple(int(j) for j in R))
    if key not in _U:
        W = 64 * ((N + 31) // 32)
        p = np.arange(N)
        col = (p // 32) * 64 + p % 32
        uo, ur = np.zeros((N, W), np.uint8), np.zeros((M, W), np.uint8)
        uo[p[present], col[present]] = 1
        ur[np.asarray(R, np.int64), col[~present]] = 1
        F = DM.complete(rate, uo, present, ur, R)[~present]
        U = F[:, col].astype(np.uint16) | F[:, col + 32].astype(np.uint16) << 8  # (16 bits: m x N can be large)
        U.setflags(write=False)
        _U[key] = U
    return _U[key]


def found(rate, orig, present, rec, mask=None):
    """What the degraded locate finds, once per stripe: (located, flags, F, encode(F))."""
    located, flags, F = DM.locate(rate, orig, present, rec, mask=mask)
    return located, flags, F, O.encode(rate, F, rec.shape[0])


def heal(rate, orig, present, rec, restored, mask=None, mode=ORIGINAL | RECOVERY, max_rows=0, base=None):
    """(located, flags [M] uint8, action, orig_after, rec_after, restored_after) of one stripe
    under the contract.  The three matrices are copies; the inputs are left as they were.  With
    `restored` = `orig` (the aliased call) the device matrix is orig_after in the present rows and
    restored_after in the missing ones.  base: found() of the same stripe and masks, to share it
    among the calls of a test."""
    N, M, S = orig.shape[0], rec.shape[0], orig.shape[1]
    pb, R, K = DM.split(present, mask, M)
    assert len(K) >= 3, "the call needs three check rows at least"
    located, flags, F, want = base if base is not None else found(rate, orig, present, rec, mask)
    orig_after, rec_after, restored_after = orig.copy(), rec.copy(), restored.copy()
    restored_after[~pb] = F[~pb]
    action = 0
    if located >= 0:
        q = int(np.flatnonzero(DM.names(pb, R, N) == located)[0])
        bit = ORIGINAL if located < N else RECOVERY
        if mode & bit:
            j0 = int(K[0])
            D = elements(want[j0:j0 + 1] ^ rec[j0:j0 + 1]).astype(np.int64)[0]
            e = HM.gf_div(D, DM.coefficients(rate, N, M, pb, R)[j0, q])
            eb = shard_bytes_of(e[None, :].astype(np.uint16), S)[0]
            if located < N:
                orig_after[located] ^= eb
            else:
                rec_after[located - N] ^= eb
            U = restored_coefficients(rate, N, M, pb, R)
            fix = LM.gf_mul(U[:, q][:, None], e[None, :]).astype(np.uint16)
            restored_after[~pb] ^= shard_bytes_of(fix, S)
            action = bit
    elif located == ROWS and mode & RECOVERY and int(flags.sum()) <= max_rows:
        rows = np.flatnonzero(flags)
        rec_after[rows] = want[rows]
        action = RECOVERY
    return located, flags, action, orig_after, rec_after, restored_after
