"""Time rs_heal_device_batch_masks against rs_locate_device_batch_masks on the same batch, against a
loop of rs_heal_device single calls and against the shared-mask batch heal (development aid; the
numbers in DESIGN.md §4.4l come from it):

    timeout -k 10 300 python tools/heal_masks_time.py [--package DIR] [--parent]

One process, one build.  Cases: 1024:1024 x 1 KiB as a 64-stripe batch and 1024:1024 x 64 KiB as a
batch of one stripe.  Every stripe gets a random 10 % of its recovery rows unselected; both mode
bits, max_rows 16.  Method of tools/heal_time.py and tools/verify_masks_time.py: warm-up, 50
back-to-back calls, one synchronize, host clock, median of 5 rounds; the legs alternate within a
round, every library call pre-bound (DeviceCall).
  locate masks / + orig / + rows:  rs_locate_device_batch_masks on the clean batch -- the yardstick
               (its kernels are the parent commit's but for one optional store); on the batch with
               one corrupt original in every stripe; with one corrupt selected row in every stripe
  heal masks / + orig / + rows:    rs_heal_device_batch_masks on the same three batches
  singles:     one rs_heal_device per stripe with that stripe's mask, clean (a leg = all of them)
  locate shared, heal shared / + orig / + rows:  rs_locate_device_batch and rs_heal_device_batch,
               every row selected, on the same batches
  damage:      what every damaged leg begins each call with, alone: one index_copy_ that writes
               the corrupt bytes back (a heal leaves the stripe healed)
The damaged legs are printed as measured and net of the damage leg.  --package DIR imports
reed_solomon_simd from DIR (another build of the library); --parent runs only the legs a build
without rs_heal_device_batch_masks has (the parent commit's).  The script has a time limit of its
own (an alarm), checks the results once per case and tries nothing twice.
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
parent = "--parent" in args
sys.path.insert(0, package)
import torch  # noqa: E402
import reed_solomon_simd as rs  # noqa: E402

signal.alarm(280)  # the whole run; a hang ends the process

N = M = 1024
MAX_ROWS = 16
MODE = rs.HEAL_ORIGINAL | rs.HEAL_RECOVERY
rounds, iters = 5, 50
ctx = rs.default_context()
u, u32, vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p
g = torch.Generator(device="cuda")
g.manual_seed(1)
p = lambda t: vp(t.data_ptr())


def head(S):
    return (vp(ctx.handle.value), ctypes.c_int(0), u(N), u(M), u(S))


def tail(B, orig, rec):
    return (u(B), p(orig), u(0), u(0), p(rec), u(0), u(0))


def time_legs(legs):
    """legs: name -> callable; us per call of every round."""
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
    return us


print(f"{N}:{M} ({rs.version()}); us per call, median of {rounds} rounds of {iters} back-to-back calls"
      + ("; the legs of a build without the masks heal" if parent else ""))
rng = np.random.default_rng(7)
for S, B in ((1024, 64), (65536, 1)):
    orig = torch.randint(0, 256, (B, N, S), dtype=torch.uint8, device="cuda", generator=g)
    rec = torch.empty((B, M, S), dtype=torch.uint8, device="cuda")
    rs.encode_device_batch(N, M, S, orig, rec)
    torch.cuda.synchronize()
    loc = torch.empty((B,), dtype=torch.int32, device="cuda")
    flags = torch.empty((B, M), dtype=torch.uint8, device="cuda")
    act = torch.empty((B,), dtype=torch.uint8, device="cuda")
    masks = np.ones((B, M), np.uint8)
    for b in range(B):
        masks[b, rng.choice(M, M // 10, replace=False)] = 0
    mptr = vp(masks.ctypes.data)
    # working copies that the damaged legs corrupt and heal: original 7 b + 3 and the (5 b + 1)-th
    # SELECTED recovery row of stripe b, one bit in a middle byte
    w_orig, w_rec = orig.clone(), rec.clone()
    where_o = [(7 * b + 3) % N for b in range(B)]
    where_r = [int(np.flatnonzero(masks[b])[(5 * b + 1) % int(masks[b].sum())]) for b in range(B)]
    at_o = torch.tensor([(b * N + i) * S + S // 2 + 1 for b, i in enumerate(where_o)], device="cuda")
    at_r = torch.tensor([(b * M + j) * S + S // 2 + 1 for b, j in enumerate(where_r)], device="cuda")
    bad_o, bad_r = orig.view(-1)[at_o] ^ 0x10, rec.view(-1)[at_r] ^ 0x10
    flat_o, flat_r = w_orig.view(-1), w_rec.view(-1)

    def locate_masks(o, r):
        return rs.DeviceCall(rs._lib.rs_locate_device_batch_masks,
                             head(S) + tail(B, o, r) + (mptr, p(loc), p(flags), None, vp(None)),
                             (o, r, loc, flags, masks))

    def heal_masks(o, r):
        return rs.DeviceCall(rs._lib.rs_heal_device_batch_masks,
                             head(S) + tail(B, o, r) + (mptr, u32(MODE), u32(MAX_ROWS), p(loc), p(flags), p(act), None,
                                                        vp(None)), (o, r, loc, flags, act, masks))

    def locate_shared(o, r):
        return rs.DeviceCall(rs._lib.rs_locate_device_batch,
                             head(S) + tail(B, o, r) + (None, p(loc), p(flags), vp(None)), (o, r, loc, flags))

    def heal_shared(o, r):
        return rs.DeviceCall(rs._lib.rs_heal_device_batch,
                             head(S) + tail(B, o, r) + (None, u32(MODE), u32(MAX_ROWS), p(loc), p(flags), p(act),
                                                        vp(None)), (o, r, loc, flags, act))

    def with_orig(call):
        def f():
            flat_o.index_copy_(0, at_o, bad_o)
            call()
        return f

    def with_rows(call):
        def f():
            flat_r.index_copy_(0, at_r, bad_r)
            call()
        return f

    def damage():
        flat_o.index_copy_(0, at_o, bad_o)

    def repair():  # (the locate legs leave the damage in place)
        w_orig.copy_(orig)
        w_rec.copy_(rec)

    legs = {"locate masks": locate_masks(orig, rec), "locate masks + orig": with_orig(locate_masks(w_orig, rec)),
            "locate masks + rows": with_rows(locate_masks(orig, w_rec)),
            "locate shared": locate_shared(orig, rec), "heal shared": heal_shared(orig, rec),
            "heal shared + orig": with_orig(heal_shared(w_orig, rec)),
            "heal shared + rows": with_rows(heal_shared(orig, w_rec)), "damage": damage}
    checks = [("locate masks", [rs.LOCATE_CLEAN] * B, None), ("locate masks + orig", where_o, None),
              ("locate masks + rows", [rs.LOCATE_ROWS] * B, None), ("heal shared", [rs.LOCATE_CLEAN] * B, 0),
              ("heal shared + orig", where_o, rs.HEAL_ORIGINAL), ("heal shared + rows", [rs.LOCATE_ROWS] * B, rs.HEAL_RECOVERY)]
    if not parent:
        rows = [masks[b].tobytes() for b in range(B)]
        singles = [rs.DeviceCall(rs._lib.rs_heal_device,
                                 head(S) + (p(orig[b]), u(0), p(rec[b]), u(0), rows[b], u32(MODE), u32(MAX_ROWS),
                                            p(loc[b:]), p(flags[b]), p(act[b:]), vp(None)),
                                 (orig, rec, loc, flags, act, rows)) for b in range(B)]

        def loop():
            for c in singles:
                c()

        legs = dict([("heal masks", heal_masks(orig, rec)), ("heal masks + orig", with_orig(heal_masks(w_orig, rec))),
                     ("heal masks + rows", with_rows(heal_masks(orig, w_rec))), (f"{B} singles", loop)], **legs)
        checks += [("heal masks", [rs.LOCATE_CLEAN] * B, 0), ("heal masks + orig", where_o, rs.HEAL_ORIGINAL),
                   ("heal masks + rows", [rs.LOCATE_ROWS] * B, rs.HEAL_RECOVERY), (f"{B} singles", [rs.LOCATE_CLEAN] * B, 0)]

    # the results, once: the report, the action, and a heal leaves the working copies clean
    ok = True
    for name, want_loc, want_act in checks:
        loc.fill_(-9), flags.fill_(0xFF), act.fill_(0xFF)
        legs[name]()
        torch.cuda.synchronize()
        ok = ok and loc.tolist() == want_loc and (want_act is None or act.tolist() == [want_act] * B)
        if want_act is None:
            repair()
        ok = ok and bool(torch.equal(w_orig, orig)) and bool(torch.equal(w_rec, rec))
        if not ok:
            print(f"  results differ at leg {name}")
            break
    print(f"shards of {S} B, batch of {B} stripe(s), {M // 10} of {M} rows unselected per stripe; results_ok={ok}")
    assert ok
    us = time_legs(legs)
    repair()
    med = {k: statistics.median(v) for k, v in us.items()}
    for k, v in us.items():
        print(f"  {k:20s} median {med[k]:8.2f}   rounds " + " ".join(f"{x:8.2f}" for x in v)
              + f"   spread (max - min) {max(v) - min(v):6.2f}")
    d = med["damage"]
    yard = med["locate masks"]
    print(f"  the yardstick's spread (locate masks): {max(us['locate masks']) - min(us['locate masks']):.2f} us")
    for kind in ("orig", "rows"):
        print(f"  locate masks + {kind} net of the damage leg = {med['locate masks + ' + kind] - d:.2f} us "
              f"({med['locate masks + ' + kind] - d - yard:+.2f} over locate masks)")
    print(f"  heal shared - locate shared = {med['heal shared'] - med['locate shared']:+.2f} us")
    for kind in ("orig", "rows"):
        print(f"  heal shared + {kind} net = {med['heal shared + ' + kind] - d:.2f} us "
              f"({med['heal shared + ' + kind] - d - med['locate shared']:+.2f} over locate shared)")
    if not parent:
        print(f"  heal masks - locate masks = {med['heal masks'] - yard:+.2f} us  ({med['heal masks'] / yard:.3f})")
        for kind in ("orig", "rows"):
            print(f"  heal masks + {kind} net = {med['heal masks + ' + kind] - d:.2f} us "
                  f"({med['heal masks + ' + kind] - d - yard:+.2f} over locate masks; the shared-mask heal adds "
                  f"{med['heal shared + ' + kind] - d - med['locate shared']:+.2f} over its locate)")
        print(f"  {B} singles / heal masks = {med[f'{B} singles'] / med['heal masks']:.2f}; heal masks / heal shared = "
              f"{med['heal masks'] / med['heal shared']:.3f}")
        rs.profile_enable(True)
        for name in ("heal masks", "heal masks + orig", "heal masks + rows", "heal shared"):
            rs.profile_collect()
            legs[name]()
            torch.cuda.synchronize()
            print(f"  launches ({name}): " + "; ".join(f"{n} {ms * 1e3:.1f} us" for n, ms, _ in rs.profile_collect()))
        rs.profile_enable(False)
    del orig, rec, w_orig, w_rec
rs.check_device()
