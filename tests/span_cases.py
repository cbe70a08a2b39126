"""The case table of the row-filtered encode: every route of encode_high / encode_low with a
narrowed span [lo, hi) of recovery rows to store.  A helper module: no tests here, nothing that
touches the GPU.  tests/test_encode_span_cpu.py checks the table against itself and the oracle,
tests/test_gpu_encode_span.py runs it through repair_device, and the masks of
tests/test_gpu_verify.py / tests/test_gpu_locate.py are drawn from spans().

Rates are the forced ones ("high" / "low"), so nothing here depends on the default-rate rule.
With n = pow2(M) (HighRate) or pow2(N) (LowRate) rows per transform, L = log2 n and
C = ceil(N / n) (HighRate: INPUT chunks, M <= n) or ceil(M / n) (LowRate: OUTPUT chunks, each with
its own FFT), the host picks the route (rs_codec.cpp use_mono, use_chunks, use_half, try_lane,
try_quad, chunk_parallel, levels); each Case names the kernel family it is built to reach and
launches() the exact launch names, so a case that silently ran elsewhere fails.
"""
import collections
import functools

import numpy as np

import oracle_lib as O

POISON = 0x33   # outputs before the call
JUNK_O = 0xA5   # (no original is absent here; the padding of d_original)
JUNK_R = 0x5A   # absent rows and the padding of d_recovery


def pow2(x):
    return 1 << max(0, int(x - 1).bit_length())


def geometry(rate, N, M):
    """(n, L, C) of the encode's transforms."""
    assert rate in ("high", "low"), rate
    n = pow2(M) if rate == "high" else pow2(N)
    return n, n.bit_length() - 1, -(-(N if rate == "high" else M) // n)


def pass_levels(L, max_k=8):
    """[(lo, K)] of the pass kernels' bit levels, low to high (rs_codec.cpp levels())."""
    m = 1 if L == 0 else -(-L // max_k)
    out, rest = [], L
    for k in range(m):
        K = -(-rest // (m - k))
        out.append((L - rest, K))
        rest -= K
    return out


def packs_of(S):
    """4-element packs of a shard: 8 per whole 64-byte block, one per 4 tail elements."""
    return S // 64 * 8 + ((S % 64) // 2 + 3) // 4


# ---------------------------------------------------------------------------
# spans

def spans(rate, N, M):
    """[(name, lo, hi)]: every span class that exists for the shape, 0 <= lo < hi <= M, no two
    alike (a class that coincides with an earlier one, or does not fit in M rows, is left out).

    first / last / all / inner: the ends of the matrix.  odd: three rows that start and end on odd
    rows (2 rows per lane, pair rows).  mid: the two rows around n / 2, the top butterfly layer of
    chunk 0 (the half-split boundary 2047 / 2048 at L = 12).  body: a long run from M / 3 to
    M - M / 4, neither end at an end of the matrix or on a boundary.  level / level3: two rows around
    2^lo and 3 * 2^lo, lo the low bit of the pass kernels' second level (only where they have one).

    LowRate with C >= 2 (output chunks): edge1 / edge_last, the two rows around the first and the
    last chunk boundary; chunk_mid / chunk_last, a whole middle chunk and the last one (partial
    where n does not divide M); inside1 / inside_last, two rows inside chunk 1 and the last chunk;
    two, [n / 2, n + n / 2).  HighRate's chunks are INPUT chunks and M <= n: every recovery row
    lies in the one FFT, so only the single-chunk spans apply and no chunk span is emitted."""
    n, L, C = geometry(rate, N, M)
    h = (M // 2) | 1
    want = [("first", 0, 1), ("last", M - 1, M), ("all", 0, M), ("inner", 1, M - 1), ("odd", h, h + 3),
            ("mid", n // 2 - 1, n // 2 + 1), ("body", M // 3, M - M // 4)]
    lv = pass_levels(L)
    if len(lv) >= 2:
        b = 1 << lv[1][0]
        want += [("level", b - 1, b + 1), ("level3", 3 * b - 1, 3 * b + 1)]
    if rate == "low" and C >= 2:
        last = (C - 1) * n
        want += [("edge1", n - 1, n + 1), ("edge_last", last - 1, last + 1)]
        if C >= 3:
            c = C // 2
            want.append(("chunk_mid", c * n, (c + 1) * n))
        want += [("chunk_last", last, M), ("inside1", n + 1, n + 3), ("inside_last", last + 1, last + 3),
                 ("two", n // 2, n + n // 2)]
    out, seen = [], set()
    for name, lo, hi in want:
        if 0 <= lo < hi <= M and (lo, hi) not in seen:
            seen.add((lo, hi))
            out.append((name, lo, hi))
    return out


def span_mask(M, lo, hi):
    """The span as a row mask with every third row inside it unselected (rows lo + 2, lo + 5, ...);
    its two ends stay selected, so the span the host derives is [lo, hi) itself."""
    mask = np.zeros(M, np.uint8)
    mask[lo:hi] = 1
    mask[lo + 2:hi - 1:3] = 0
    return mask


# ---------------------------------------------------------------------------
# routes

# mode: the rs_mono_enable value; env: settings for a fresh Context; family: pass / chunks /
# staged / lane / quad / unstaged / half; passes: how many k_pass launches a pass route takes;
# layouts: (S, row padding) pairs, None = LAYOUTS; probe: also run with the extra layouts
# (one route per kernel family)
Case = collections.namedtuple("Case", "route rate N M mode env family passes layouts probe")

LAYOUTS = [(64, 0), (66, 4)]   # whole blocks; a tail, rows of 70 bytes


def _case(route, rate, N, M, mode=1, env=None, family="pass", passes=0, layouts=None, probe=False):
    return Case(route, rate, N, M, mode, dict(env or {}), family, passes, layouts, probe)


SERIAL = {"RS_MI355X_CHUNK_PARALLEL": "0"}
GRID = {"RS_MI355X_CHUNK_PARALLEL": "1"}

CASES = [
    # one level (L <= 8), one chunk: L < 7 by default, the column kernels off at L = 8
    _case("pass1", "high", 20, 30, passes=1, probe=True),
    _case("pass1", "low", 30, 20, passes=1),
    _case("pass1", "high", 100, 200, mode=0, passes=1),
    # k_chunks: 2- and 4-element packs, two packs per wave (> 256 packs), a partial last chunk
    _case("chunks-e2", "high", 1000, 100, family="chunks"),
    _case("chunks-e2", "low", 128, 1024, family="chunks", probe=True),
    _case("chunks-e4", "high", 1000, 100, mode=1 | 8, family="chunks"),
    _case("chunks-e4", "low", 128, 1024, mode=1 | 8, family="chunks"),
    _case("chunks-pw2", "high", 1000, 100, family="chunks", layouts=[(4096, 0), (4034, 6)]),
    _case("chunks-partial", "high", 300, 100, family="chunks"),
    _case("chunks-partial", "low", 100, 300, family="chunks"),
    # one level, several chunks on the pass kernels: serial (in_chunks / out_chunks) ...
    _case("pass1-serial", "high", 1000, 100, env=SERIAL, passes=1),
    _case("pass1-serial", "low", 100, 1000, env=SERIAL, passes=1),
    # ... and over the grid (HighRate: IFFTs into work rows, then fold + FFT; LowRate: grid_chunks + in_chunk0)
    _case("pass1-grid", "high", 1000, 100, env=GRID, passes=2),
    _case("pass1-grid", "low", 100, 1000, env=GRID, passes=1),
    # staged column kernel, 2- and 4-element packs
    *[_case("staged", rate, N, M, mode=mode, family="staged", probe=(N == 70 and mode == 1))
      for rate, N, M in (("high", 70, 100), ("low", 100, 70), ("high", 600, 1000), ("high", 2048, 2048),
                         ("low", 2048, 1500))
      for mode in (1, 1 | 8)],
    # lane kernel: 2^8 and 2^9 rows by default, 2^10 with + 32
    _case("lane", "high", 150, 200, family="lane", probe=True),
    _case("lane", "low", 200, 150, family="lane"),
    _case("lane", "high", 300, 500, family="lane"),
    _case("lane", "low", 500, 300, family="lane"),
    _case("lane", "high", 600, 1000, mode=1 | 32, family="lane"),
    _case("lane", "low", 1000, 600, mode=1 | 32, family="lane"),
    # quad encode
    _case("quad", "high", 600, 1000, mode=1 | 2048, family="quad"),
    _case("quad", "low", 1000, 600, mode=1 | 2048, family="quad"),
    # unstaged column kernel: several chunks, 2^12 rows
    _case("unstaged", "high", 300, 128, mode=2, family="unstaged", probe=True),
    _case("unstaged", "low", 128, 300, mode=2, family="unstaged"),
    _case("unstaged", "high", 4096, 4096, mode=2, family="unstaged"),
    # half split
    _case("half", "high", 4096, 4096, mode=1 | 128, family="half"),
    _case("half", "low", 4096, 4096, mode=1 | 128, family="half"),
    # two levels, one chunk: IFFT level 0, the fused top level, FFT level 0
    _case("pass2", "high", 4096, 4096, passes=3),
    _case("pass2", "low", 4096, 4096, passes=3),
    _case("pass2", "high", 512, 512, mode=0, passes=3),
    _case("pass2", "low", 512, 512, mode=0, passes=3),
    # two levels, several chunks (grid_chunks; LowRate: dst on the last FFT level under grid_chunks)
    _case("pass2-chunks", "high", 1100, 512, mode=0, passes=3),
    _case("pass2-chunks", "low", 512, 1100, mode=0, passes=3),
    _case("pass2-chunks", "low", 3000, 5000, passes=3),
]

# the layouts a probe case adds: a tail on 4-byte aligned rows (72 bytes), and whole blocks at a
# base address of 1 mod 4 (the byte-wise path); (S, row padding, base offset)
PROBE_LAYOUTS = [(66, 6, 0), (64, 0, 1)]

# (rate, N, M, S, mode) of the batch repairs: a staged shape (one launch), k_chunks and the
# two-level passes (stripe by stripe)
BATCH = [("high", 70, 100, 64, 1), ("low", 128, 1024, 64, 1), ("low", 512, 1100, 64, 0)]

# (rate, N, M, S) added to test_masks of the verify and the locate, and (rate, N, M, S, mode)
# of their mode-0 runs
MASK_SHAPES = [("low", 100, 70, 66), ("low", 128, 1024, 64), ("low", 100, 300, 72), ("low", 3000, 5000, 64)]
MASK_SHAPES_MODE0 = [("high", 1100, 512, 64, 0), ("low", 512, 1100, 64, 0)]


def case_id(c):
    env = "".join("-cp" + v for v in c.env.values())
    return f"{c.route}-{c.rate}-{c.N}-{c.M}-m{c.mode}{env}"


def launches(c, S, stripes=1):
    """The launch names of one narrowed encode of the case at shard_bytes S: the exact list, or
    for the pass kernels (prefix, count)."""
    n, L, C = geometry(c.rate, c.N, c.M)
    packs = packs_of(S)
    high = "true" if c.rate == "high" else "false"
    batch = "true" if stripes > 1 else "false"
    enc = 0 if c.rate == "high" else 1  # kMonoEncodeHigh / kMonoEncodeLow
    e2 = lambda count: 2 if not (c.mode & 8) and count <= 128 else 4
    if c.family == "pass":
        return ("k_pass<", c.passes * stripes)
    if c.family == "chunks":  # one stripe per launch
        return ["k_chunks<%d, %d, %s, %d>" % (L, e2(packs), high, 2 if packs > 256 else 1)] * stripes
    if c.family == "staged":
        return ["k_mono<%d, 1, %d, true, %s, false, %d>" % (L, enc, batch, e2(packs * stripes))]
    if c.family == "lane":
        return ["k_lane<%d, %s>" % (L, batch)]
    if c.family == "quad":  # kMonoQuadEnc = 7, 2^9 pair rows
        return ["k_mono<9, 1, 7, true, %s, false, 4>" % batch]
    if c.family == "unstaged":
        return ["k_mono<%d, %d, %d, false, false, false, 4>" % (L, 1 if L <= 10 else L - 9, enc)] * stripes
    if c.family == "half":  # kMonoHalfIEnc = 3, kMonoHalfFEnc = 5; both halves' workgroups count
        return ["k_mono<11, 1, %d, true, false, false, %d>" % (m, e2(2 * packs)) for m in (3, 5)] * stripes
    raise ValueError(c.family)


def check_launches(c, S, names, stripes=1):
    """The launch record of a narrowed encode: no decode kernel, and the case's own family."""
    assert names, "nothing was launched"
    assert not any("repair" in x or x == "k_eval_poly" for x in names), f"not the encode route: {names}"
    want = launches(c, S, stripes)
    if isinstance(want, tuple):
        assert len(names) == want[1] and all(x.startswith(want[0]) for x in names), (case_id(c), names, want)
    else:
        assert names == want, (case_id(c), names, want)


# ---------------------------------------------------------------------------
# the oracle's stripe and what a narrowed encode must leave behind

@functools.lru_cache(maxsize=None)
def stripe(rate, N, M, S, seed=0):
    """(originals, recovery) from the oracle; computed once, never modified."""
    orig = O.generate_original(N, S, seed)
    rec = O.encode(rate, orig, M)
    orig.setflags(write=False)
    rec.setflags(write=False)
    return orig, rec


def held_recovery(rec, lo, hi):
    """d_recovery before the repair: the oracle's rows, junk in the absent ones."""
    held = rec.copy()
    held[lo:hi] = JUNK_R
    return held


def expected_out(rec, lo, hi):
    """d_recovery_out after the repair: rows [lo, hi) of the oracle's encode, poison elsewhere."""
    want = np.full_like(rec, POISON)
    want[lo:hi] = rec[lo:hi]
    return want
