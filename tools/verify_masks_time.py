"""Time rs_verify_device_batch_masks and rs_locate_device_batch_masks against the shared-mask batch
calls and against a loop of single-stripe calls (development aid; the numbers in DESIGN.md §4.4k
come from it):

    timeout -k 10 300 python tools/verify_masks_time.py [--package DIR] [--shared-only]

One process, one build.  Cases: 1024:1024 x 1 KiB as a 64-stripe batch and 1024:1024 x 64 KiB as a
batch of one stripe (past the column kernel's pack bound: the unfused route only).  Every stripe
gets a random 10 % of its recovery rows unselected.  Method of tools/verify_time.py: warm-up, 50
back-to-back calls, one synchronize, host clock, median of 5 rounds; the legs alternate within a
round, every call pre-bound (DeviceCall).
  verify  masks fused / masks unfused: rs_verify_device_batch_masks under rs_verify_set_fused(1 / 0)
          singles: one rs_verify_device per stripe with that stripe's mask (a leg = all of them)
          shared:  rs_verify_device_batch, every row -- the yardstick
  locate  masks:   rs_locate_device_batch_masks
          shared:  rs_locate_device_batch, every row -- the yardstick
--package DIR imports reed_solomon_simd from DIR (another build of the library); --shared-only runs
the two yardstick legs alone (a build without the masks calls: the parent commit's).  The script has
a time limit of its own (an alarm), checks the results once per case and tries nothing twice.
"""
import ctypes
import os
import signal
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
package = args[args.index("--package") + 1] if "--package" in args else os.path.join(ROOT, "reed-solomon-simd_amd")
shared_only = "--shared-only" in args
sys.path.insert(0, package)
import torch  # noqa: E402
import reed_solomon_simd as rs  # noqa: E402

signal.alarm(280)  # the whole run; a hang ends the process

N = M = 1024
rounds, iters = 5, 50
ctx = rs.default_context()
u, vp = ctypes.c_uint64, ctypes.c_void_p
g = torch.Generator(device="cuda")
g.manual_seed(1)
p = lambda t: vp(t.data_ptr())


def head(S):
    return (vp(ctx.handle.value), ctypes.c_int(0), u(N), u(M), u(S))


def batch_tail(B, orig, rec):
    return (u(B), p(orig), u(0), u(0), p(rec), u(0), u(0))


def time_legs(legs):
    """legs: name -> (fused mode or None, callable); us per call of every round."""
    for mode, f in legs.values():
        if mode is not None:
            rs.verify_set_fused(mode)
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    us = {name: [] for name in legs}
    for _ in range(rounds):
        for name, (mode, f) in legs.items():
            if mode is not None:
                rs.verify_set_fused(mode)
            t0 = time.perf_counter()
            for _ in range(iters):
                f()
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) / iters * 1e6)
    return us


def show(us, yard):
    med = {k: statistics.median(v) for k, v in us.items()}
    for k, v in us.items():
        print(f"  {k:22s} median {med[k]:8.2f}   rounds " + " ".join(f"{x:8.2f}" for x in v)
              + f"   spread (max - min) {max(v) - min(v):6.2f}")
    spread = max(us[yard]) - min(us[yard])
    for k in med:
        if k != yard:
            d = med[k] - med[yard]
            print(f"  {k} / {yard} = {med[k] / med[yard]:.3f}  ({d:+.2f} us; the yardstick's spread is {spread:.2f} us)")
    return med


print(f"{N}:{M} ({rs.version()}); us per call, median of {rounds} rounds of {iters} back-to-back calls")
rng = np.random.default_rng(7)
for S, B in ((1024, 64), (65536, 1)):
    orig = torch.randint(0, 256, (B, N, S), dtype=torch.uint8, device="cuda", generator=g)
    rec = torch.empty((B, M, S), dtype=torch.uint8, device="cuda")
    rs.encode_device_batch(N, M, S, orig, rec)
    torch.cuda.synchronize()
    flags = torch.empty((B, M), dtype=torch.uint8, device="cuda")
    located = torch.empty((B,), dtype=torch.int32, device="cuda")
    masks = np.ones((B, M), np.uint8)
    for b in range(B):
        masks[b, rng.choice(M, M // 10, replace=False)] = 0
    has_fused = S <= 2048  # the column kernel's bound: 256 packs of 8 bytes
    print(f"shards of {S} B, batch of {B} stripe(s), {M // 10} of {M} rows unselected per stripe")

    shared_v = rs.DeviceCall(rs._lib.rs_verify_device_batch,
                             head(S) + batch_tail(B, orig, rec) + (None, p(flags), vp(None)), (orig, rec, flags))
    shared_l = rs.DeviceCall(rs._lib.rs_locate_device_batch,
                             head(S) + batch_tail(B, orig, rec) + (None, p(located), p(flags), vp(None)),
                             (orig, rec, flags, located))
    shared_mode = 1 if has_fused else 0
    vlegs = {"shared": (shared_mode, shared_v)}
    llegs = {"shared": (None, shared_l)}
    if not shared_only:
        mptr = vp(masks.ctypes.data)
        masks_v = rs.DeviceCall(rs._lib.rs_verify_device_batch_masks,
                                head(S) + batch_tail(B, orig, rec) + (mptr, p(flags), vp(None)),
                                (orig, rec, flags, masks))
        masks_l = rs.DeviceCall(rs._lib.rs_locate_device_batch_masks,
                                head(S) + batch_tail(B, orig, rec) + (mptr, p(located), p(flags), None, vp(None)),
                                (orig, rec, flags, located, masks))
        rows = [masks[b].tobytes() for b in range(B)]
        singles = [rs.DeviceCall(rs._lib.rs_verify_device,
                                 head(S) + (p(orig[b]), u(0), p(rec[b]), u(0), rows[b], p(flags[b]), vp(None)),
                                 (orig, rec, flags, rows)) for b in range(B)]

        def loop():
            for c in singles:
                c()

        # once per case: a clean batch gives no flag, a corrupt selected row and a corrupt unselected one
        # give exactly the selected one, by either route; the locate finds a corrupt original
        bad = rec.clone()
        sel0, out0 = int(np.flatnonzero(masks[0])[3]), int(np.flatnonzero(masks[0] == 0)[0])
        bad[0, sel0, 5] ^= 1
        bad[0, out0, 7] ^= 1
        ok = True
        for mode in ((1, 0) if has_fused else (0,)):
            rs.verify_set_fused(mode)
            for held, want in ((rec, []), (bad, [sel0])):
                got = rs.verify_device_batch_masks(N, M, S, orig, held, masks).cpu().numpy()
                ok = ok and np.flatnonzero(got.reshape(-1)).tolist() == want
        worse = orig.clone()
        worse[B - 1, 77, 9] ^= 4
        loc, _ = rs.locate_device_batch_masks(N, M, S, worse, rec, masks)
        ok = ok and loc.cpu().numpy().tolist() == [-1] * (B - 1) + [77]
        print(f"  results_ok={ok}")
        assert ok
        vlegs = dict(([("masks fused", (1, masks_v))] if has_fused else []) +
                     [("masks unfused", (0, masks_v)), (f"{B} singles", (shared_mode, loop))], **vlegs)
        llegs = dict([("masks", (None, masks_l))], **llegs)
    print(" verify")
    show(time_legs(vlegs), "shared")
    print(" locate (clean stripes)")
    show(time_legs(llegs), "shared")
    if not shared_only:
        rs.profile_enable(True)
        rs.profile_collect()
        for mode in ((1, 0) if has_fused else (0,)):
            rs.verify_set_fused(mode)
            masks_v()
        masks_l()
        torch.cuda.synchronize()
        recs = rs.profile_collect()
        rs.profile_enable(False)
        print("  launches (masks verify" + (" fused," if has_fused else "") + " unfused, masks locate): "
              + "; ".join(f"{n} {ms * 1e3:.1f} us" for n, ms, _ in recs))
    del orig, rec, flags
rs.verify_set_fused(rs.VERIFY_FUSED_DEFAULT)
rs.check_device()
