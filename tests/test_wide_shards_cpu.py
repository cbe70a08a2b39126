"""The wide-shard cases of tests/wide_cases.py without a GPU: the size table against a restatement of
packs_of and against the constants in the sources, pack_columns as a partition of the shard, and --
for every (family, shape, size, case) that tests/test_gpu_wide_shards.py runs -- the family's numpy
model giving the outcome the case was built for, so that a failure on the GPU is the kernels'.

Every family keeps the table's largest size, 65536 bytes: the models are linear in S and the slowest
(the locate's, 15 cases of a 70:100 stripe) takes about 3 s there.  To stay inside a minute the heal is
modelled with both mode bits only; a single bit changes the action alone (tests/test_heal_cpu.py).
"""
import os
import re

import numpy as np
import pytest

import heal_degraded_model as HDM
import heal_masks_cases as HMC
import heal_model as HM
import locate_degraded_model as DM
import locate_model as LM
import locate_robust_cases as RC
import oracle_lib as O
import test_gpu_heal_degraded as HD
import test_gpu_locate as L
import test_gpu_locate_degraded as LD
import test_gpu_update as U
import test_gpu_verify as V
import verify_masks_cases as C
import wide_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reed-solomon-simd_amd", "csrc")
SHAPES = W.shapes()
IDS = [f"{r}-{n}-{m}-{s}" for r, n, m, s, _ in SHAPES]
CLEAN, ROWS, UNKNOWN = LM.CLEAN, LM.ROWS, LM.UNKNOWN


def source(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_table_against_packs_of():
    """Every size sits where the table says, by the restated packs_of and launch shape."""
    assert [W.packs_of(s) for s, _, _, _ in W.SIZES] == [p for _, _, p, _ in W.SIZES]
    by = {(s, pad): p for s, pad, p, _ in W.SIZES}
    assert W.launch_shape(by[520, 0]) == (2 * W.WAVE, 1) and by[520, 0] == W.WAVE + 1
    assert by[1032, 0] == W.E2_MAX_PACKS + 1 and W.packs_of(1024) == W.E2_MAX_PACKS
    assert by[2048, 0] == W.TILE == W.MONO_MAX_PACKS and W.launch_shape(by[2048, 0]) == (W.TILE, 1)
    for key in ((2056, 0), (2050, 4)):
        assert by[key] == W.TILE + 1 == W.MONO_MAX_PACKS + 1 and W.launch_shape(by[key]) == (W.TILE, 2)
    lo, hi = W.pack_columns(2050, 256)
    assert len(lo) == len(hi) == 1 and (2050 + 4) % 4 != 0  # a one-element tail pack; rows not 4-byte aligned
    assert by[8200, 0] == W.FIND_STEP + 1 and W.launch_shape(by[8200, 0])[1] == 5 and W.find_steps(by[8200, 0]) == 2
    assert W.launch_shape(by[65536, 0])[1] == 32 and W.find_steps(by[65536, 0]) == 8
    # S <= 190, the widest shard of the families' own files, stays inside one wave
    assert W.launch_shape(W.packs_of(190)) == (W.WAVE, 1)
    # the positions: either side of each edge, and the last pack
    assert W.positions(520) == [63, 64] and W.positions(2048) == [63, 64, 255]
    assert W.positions(2056) == [63, 64, 255, 256] and W.positions(8200) == [63, 64, 255, 256, 1023, 1024]
    assert W.positions(65536) == [63, 64, 255, 256, 1023, 1024, 8191]


def test_the_constants_are_the_sources():
    """The thresholds restated in tests/wide_cases.py are the ones the library is built with."""
    codec, locate, robust = source("rs_codec.cpp"), source("rs_locate.hip"), source("rs_locate_robust.hip")
    m = re.search(r"uint32_t packs_of\(uint64_t S\) \{ return uint32_t\((.*?)\); \}", codec)
    assert m and m.group(1) == "S / 64 * 8 + ((S % 64) / 2 + 3) / 4", m
    assert int(re.search(r"uint32_t mono_max_packs = (\d+);", codec).group(1)) == W.MONO_MAX_PACKS
    # e2_max_packs is half the CU count (256 CUs on this chip; the GPU file reads it off the kernel names)
    assert re.search(r"e2_max_packs = ctx->e2_default = cus > 1 \? uint32_t\(cus\) / 2 : 1u;", codec)
    for text in (locate, robust):
        assert int(re.search(r"constexpr uint32_t kFindThreads = (\d+);", text).group(1)) == W.FIND_THREADS
        assert int(re.search(r"constexpr uint32_t kFindUnroll = (\d+);", text).group(1)) == W.FIND_UNROLL
        assert "base += kFindThreads * kFindUnroll" in text
    # the launch shape of the per-pack kernels
    shape = re.compile(r"packs >= (\d+) \? (\d+)u? : \((?:\w+\.)?packs \+ (\d+)u?\) / (\d+)u? \* (\d+)u?")
    seen = 0
    for name in ("rs_locate.hip", "rs_locate_robust.hip", "rs_update.hip", "rs_verify.hip"):
        for m in shape.finditer(source(name)):
            assert [int(x) for x in m.groups()] == [W.TILE, W.TILE, W.WAVE - 1, W.WAVE, W.WAVE], (name, m.group(0))
            seen += 1
    assert seen >= 9, seen  # the verify's two, the locate's and the heal's five, the robust one, the update's


@pytest.mark.parametrize("S", [s for s, _, _, _ in W.SIZES] + [1024, 190, 66, 2])
def test_pack_columns_partition_the_shard(S):
    packs = W.packs_of(S)
    seen = np.zeros(S, np.int32)
    for p in range(packs):
        lo, hi = W.pack_columns(S, p)
        assert len(lo) == len(hi) >= 1, p  # both halves occur in every pack
        assert lo.max() < hi.min()
        seen[lo] += 1
        seen[hi] += 1
    assert (seen == 1).all()
    # damage_pack stays inside its pack, and reaches both halves
    a = np.zeros((1, S), np.uint8)
    rng = np.random.default_rng(S)
    halves = set()
    for _ in range(32):
        a[:] = 0
        col = W.damage_pack(a, 0, packs - 1, rng)
        lo, hi = W.pack_columns(S, packs - 1)
        assert np.flatnonzero(a[0]).tolist() == [col] and (col in lo or col in hi)
        halves.add(col in lo)
    assert halves == {True, False}


@pytest.mark.parametrize("rate,N,M,S,pad", SHAPES, ids=IDS)
def test_verify_kinds_flag_what_they_touch(rate, N, M, S, pad):
    orig, rec = V.stripe(rate, N, M, S)
    kinds = W.verify_kinds(N, M, S)
    assert [k[2] for k in kinds if k[0] == "row"] == W.positions(S)
    for kind in kinds:
        o, r, want = V.corrupt(kind, rate, N, M, S)
        truth = (O.encode(rate, o, M) != r).any(axis=1)
        assert np.array_equal(want, truth), kind
        if kind[0] == "row":
            assert np.flatnonzero(want).tolist() == [kind[1]]
            cols = np.flatnonzero(r[kind[1]] != rec[kind[1]])
            assert len(cols) == 1 and cols[0] in np.concatenate(W.pack_columns(S, kind[2])), kind
    packs = W.every_row_packs(M, S)
    assert packs[0] == 0 and packs[-1] == W.packs_of(S) - 1
    assert len(set(packs)) == (M if W.packs_of(S) >= M else len(set(packs)))
    o, r, want = V.corrupt(("every row",), rate, N, M, S)
    assert want.all() and np.array_equal(o, orig)


@pytest.mark.parametrize("rate,N,M,S,pad", SHAPES, ids=IDS)
def test_locate_and_heal_models_give_the_intended_outcome(rate, N, M, S, pad):
    clean_orig, clean_rec = V.stripe(rate, N, M, S)
    cases = L.cases(rate, N, M, S, wide=True)
    names = [c[0] for c in cases]
    for p in W.positions(S):
        assert any(n.startswith("original ") and n.endswith(f" pack {p}") for n in names), (p, names)
    assert {c[3] for c in cases} >= {CLEAN, ROWS, UNKNOWN, 0, N // 2, N - 1}
    for name, orig, rec, intended in cases:
        loc, flags, act, o2, r2 = HM.heal(rate, orig, rec, mode=3, max_rows=M - 1)
        assert loc == intended, f"{name}: the model says {loc}, the case was built for {intended}"
        if intended >= 0 or intended == ROWS:
            assert act and np.array_equal(o2, clean_orig) and np.array_equal(r2, clean_rec), name
        else:
            assert act == 0 and np.array_equal(o2, orig) and np.array_equal(r2, rec), name


@pytest.mark.parametrize("rate,N,M,S,pad", SHAPES, ids=IDS)
def test_robust_models_give_the_intended_outcome(rate, N, M, S, pad):
    cases = RC.cases(rate, N, M, S, wide=True)
    seen = set()
    for case in cases:
        located, flags, outlier = RC.model(rate, case)  # (asserts the intended status and outliers)
        seen.add((case[1], "i" if located >= 0 else located))
    assert seen >= {(1, "i"), (2, "i"), (1, UNKNOWN), (2, UNKNOWN), (1, CLEAN)}, seen
    # the outliers' damage is in the last pack alone
    last = np.concatenate(W.pack_columns(S, W.packs_of(S) - 1))
    _, rec = V.stripe(rate, N, M, S)
    for name, t, orig, r, enc, intended in cases:
        assert np.isin(np.flatnonzero((r != rec).any(axis=0)), last).all(), name


@pytest.mark.parametrize("kind", ["first", "scattered"])
@pytest.mark.parametrize("rate,N,M,S,pad", SHAPES, ids=IDS)
def test_degraded_models_give_the_intended_outcome(rate, N, M, S, pad, kind):
    present, mask = LD.pattern(kind, N, M)
    assert int((present == 0).sum()) == {"first": 1, "scattered": 3}[kind]
    cases = HD.cases(rate, N, M, S, present, mask, wide=True)
    assert len(cases) == 5
    for name, orig, rec, intended, _ in cases:
        want, _, _ = DM.locate(rate, orig, present, rec, mask)
        assert want == intended, f"{name}: the model says {want}, the case was built for {intended}"
        assert HDM.found(rate, orig, present, rec, mask)[0] == intended, name


def masks_batch(rate, N, M, S):
    origs, recs = C._clean(rate, N, M, S, 4)
    return W.masks_batch(origs, recs, lambda b, o: O.encode(rate, o, M))


@pytest.mark.parametrize("rate,N,M,S,pad", SHAPES, ids=IDS)
def test_mask_models_give_the_intended_outcome(rate, N, M, S, pad):
    store, held, masks, intent, want = masks_batch(rate, N, M, S)
    _, recs = C._clean(rate, N, M, S, 4)
    last = np.concatenate(W.pack_columns(S, W.packs_of(S) - 1))
    assert [int(m.sum()) for m in masks] == [M, 2, M - len(range(1, M, 3)), M - 2]
    for b in range(4):
        loc, flags = LM.locate(rate, store[b], held[b], masks[b])
        assert loc == intent[b], (b, loc, int(intent[b]))
        assert np.array_equal(flags, want[b]), b
        out = np.flatnonzero(masks[b] == 0)  # the junk differs, in the last pack alone
        assert (held[b][out] != recs[b][out]).any(axis=1).all()
        assert np.isin(np.flatnonzero((held[b][out] != recs[b][out]).any(axis=0)), last).all()
    # the heal's model stripe by stripe: with both bits the two-row stripe is skipped, with the
    # recovery bit alone it is rewritten
    for mode, act, codes in ((3, [HM.ORIGINAL, 0, HM.ORIGINAL, 0], [0, 101, 0, 0]),
                             (HM.RECOVERY, [0, HM.RECOVERY, 0, 0], [0, 0, 0, 0])):
        m = HMC.model(rate, N, M, S, mode=mode, max_rows=2, masks=masks, store=store, held=held)
        assert m[2].tolist() == act and m[5].tolist() == codes, (mode, m[2], m[5])
        assert m[0].tolist() == [HMC.SKIPPED if c else int(i) for i, c in zip(intent, codes)]


@pytest.mark.parametrize("rate,N,M,S", W.UPDATE, ids=lambda v: str(v))
def test_update_rows_differ_where_they_are_built_to(rate, N, M, S):
    rng = np.random.default_rng(N * 7 + M)
    packs = W.packs_of(S)
    for count in (1, min(33, N)):  # (30:100 has 30 originals in all)
        idx = U.indices(N, count, rng)
        old, new, want = U.change(rate, N, M, S, idx, positional=True)
        where = lambda k: np.flatnonzero(old[k] != new[k])
        assert len(where(0)) == 1 and where(0)[0] in np.concatenate(W.pack_columns(S, packs - 1))
        if len(idx) > 1:
            assert len(where(1)) == 1 and where(1)[0] in np.concatenate(W.pack_columns(S, 0))
        mod = U.stripe(rate, N, M, S)[0].copy()
        mod[idx] = new
        assert np.array_equal(want, O.encode(rate, mod, M))
