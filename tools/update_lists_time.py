"""Time rs_update_device_batch_lists against what a caller has without it (development aid; the
figures in DESIGN.md "Update", per-stripe lists, come from it).  Every GPU step under a time limit
of its own, the steps chained:

    timeout -k 10 300 python tools/update_lists_time.py && \
    timeout -k 10 300 python tools/update_lists_time.py --pkg <package dir of the parent commit's build> \
        --label "the parent commit's build"

The second step loads another build of the library (one without the call) and runs leg 2 alone: its
kernels are the same in both builds, so the pair gives the baseline and its run-to-run spread.
--label names the build in the header line (default: the package directory, relative to the
repository); profiles/update_lists/ keeps the standard output of the two steps as they came,
update_lists_time.txt and update_lists_time_parent.txt.

1024:1024, delta form, every recovery row; 64 stripes x 1 KiB and one stripe x 64 KiB; k = 1 and
k = 8 random indices per stripe, different in every stripe.  Method of tools/update_time.py: warm-up,
median of 5 rounds of 50 back-to-back pre-bound calls (DeviceCall), one synchronize per round, host
clock, the legs alternating in rounds.
  (1) lists_warm:  the new call, the locate table on the stream
  (2) shared:      rs_update_device_batch with stripe 0's list for every stripe (computes something
                   else unless every stripe changed the same originals)
  (3) loop:        one rs_update_device per stripe with the stripe's own list: every call a new list,
                   so every call pays the coefficient step
  (4) lists_cold:  the new call with rs_release_stream_scratch before it: the table rebuilt
The script has a time limit of its own (an alarm), checks the new call's bytes once per case against
the batch encode of the modified stripes, and tries nothing twice.
"""
import ctypes
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "reed-solomon-simd_amd")
if "--pkg" in sys.argv:
    PKG = os.path.abspath(sys.argv[sys.argv.index("--pkg") + 1])
LABEL = sys.argv[sys.argv.index("--label") + 1] if "--label" in sys.argv else os.path.relpath(PKG, ROOT)
sys.path.insert(0, PKG)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import reed_solomon_simd as rs  # noqa: E402

signal.alarm(280)  # the whole run; a hang ends the process

N, M = 1024, 1024
rounds, iters = 5, 50
HAVE = hasattr(rs._lib, "rs_update_device_batch_lists")
ctx = rs.default_context()
u, vp = ctypes.c_uint64, ctypes.c_void_p
g = torch.Generator(device="cuda")
g.manual_seed(1)
rng = np.random.default_rng(1)
p = lambda t: vp(t.data_ptr())


def head(S):
    return (vp(ctx.handle.value), ctypes.c_int(0), u(N), u(M), u(S))


def lists_call(S, lists, d_new, d_rec):
    B, K = lists.shape
    idx = (u * (B * K))(*[int(i) for i in lists.reshape(-1)])
    cnt = (ctypes.c_uint32 * B)(*([K] * B))
    a = head(S) + (u(B), idx, cnt, u(K), vp(None), u(0), u(0), p(d_new), u(0), u(0), p(d_rec), u(0), u(0), vp(None),
                   vp(None))
    return rs.DeviceCall(rs._lib.rs_update_device_batch_lists, a, (idx, cnt, d_new, d_rec))


def shared_call(S, lists, d_new, d_rec):
    B, K = lists.shape
    idx = (u * K)(*[int(i) for i in lists[0]])
    a = head(S) + (u(B), idx, u(K), vp(None), u(0), u(0), p(d_new), u(0), u(0), p(d_rec), u(0), u(0), None, vp(None))
    return rs.DeviceCall(rs._lib.rs_update_device_batch, a, (idx, d_new, d_rec))


def loop_call(S, lists, d_new, d_rec):
    B, K = lists.shape
    calls = []
    for b in range(B):
        idx = (u * K)(*[int(i) for i in lists[b]])
        a = head(S) + (idx, u(K), vp(None), u(0), p(d_new[b]), u(0), p(d_rec[b]), u(0), None, vp(None))
        calls.append(rs.DeviceCall(rs._lib.rs_update_device, a, (idx, d_new, d_rec)))

    def run():
        for c in calls:
            c()
    return run


def time_legs(legs):
    for f in legs.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    us = {name: [] for name in legs}
    for _ in range(rounds):
        for name, f in legs.items():
            t0 = time.perf_counter()
            for _ in range(iters):
                f()
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) / iters * 1e6)
    return {n: (statistics.median(v), min(v), max(v)) for n, v in us.items()}


print(f"{N}:{M} ({rs.version()}; {'with' if HAVE else 'WITHOUT'} rs_update_device_batch_lists: {LABEL}); "
      f"us per call, "
      f"median of {rounds} rounds of {iters} calls (min .. max of the rounds)")
rs.update_set_direct_max(rs.UPDATE_DIRECT_MAX_DEFAULT)
for B, S in ((64, 1024), (1, 65536)):
    orig = torch.randint(0, 256, (B, N, S), dtype=torch.uint8, device="cuda", generator=g)
    rec0 = torch.empty((B, M, S), dtype=torch.uint8, device="cuda")
    rs.encode_device_batch(N, M, S, orig, rec0)
    torch.cuda.synchronize()
    for K in (1, 8):
        lists = np.stack([rng.choice(N, K, replace=False) for _ in range(B)])
        new = torch.randint(0, 256, (B, K, S), dtype=torch.uint8, device="cuda", generator=g)
        rows = torch.from_numpy(lists).cuda()
        at = rows[:, :, None].expand(B, K, S)
        delta = (torch.gather(orig, 1, at) ^ new).contiguous()
        rec = rec0.clone()
        legs, ok = {}, "-"
        if HAVE:
            mod = orig.clone()
            mod.scatter_(1, at, new)
            want = torch.empty_like(rec0)
            rs.encode_device_batch(N, M, S, mod, want)
            r = rec0.clone()
            lists_call(S, lists, delta, r)()
            torch.cuda.synchronize()
            ok = torch.equal(r, want)
            del mod, want, r
            warm = lists_call(S, lists, delta, rec)

            def cold():
                rs.release_stream_scratch()
                warm()

            legs["lists_warm"] = warm
        legs["shared"] = shared_call(S, lists, delta, rec)
        if HAVE:
            legs["loop"] = loop_call(S, lists, delta, rec)
            legs["lists_cold"] = cold
        res = time_legs(legs)
        print(f"{B:3d} stripes x {S:5d} B, k = {K}: "
              + "   ".join(f"{n} {m:.1f} ({lo:.1f} .. {hi:.1f})" for n, (m, lo, hi) in res.items())
              + f"   bytes_ok={ok}")
        assert ok is not False
        if HAVE:
            rs.profile_enable(True)
            rs.profile_collect()
            warm()
            legs["shared"]()
            torch.cuda.synchronize()
            print("    kernel time (warm new call; shared-list call): "
                  + "; ".join(f"{n} {ms * 1e3:.1f} us" for n, ms, _ in rs.profile_collect()))
            rs.profile_enable(False)
    del orig, rec0, rec
rs.check_device()
