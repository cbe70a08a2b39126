"""Time rs_heal_device_batch against the locate alone and against today's three-call scrub
(development aid; the numbers in DESIGN.md "Heal" come from it):

    timeout -k 10 300 python tools/heal_time.py

One process, one build.  Cases: 1024:1024 x 1 KiB as one stripe and as a 64-stripe batch, and
1024:1024 x 64 KiB as one stripe, every recovery row.  Method of tools/locate_time.py: warm-up,
`iters` back-to-back calls, one synchronize, host clock; the legs alternate within a round; the
library's calls are pre-bound (DeviceCall: what a C caller of the ABI pays).
  locate:      rs_locate_device_batch on the clean batch -- the yardstick (its kernels are the
               parent commit's); its round-to-round spread (max - min) is printed
  heal clean:  rs_heal_device_batch (both mode bits, max_rows 16) on the clean batch
  heal orig:   ... with one corrupt original in every stripe
  heal rows:   ... with one corrupt recovery row in every stripe
  scrub orig / scrub rows:  the same damage by the three calls: rs_locate_device_batch, a
               synchronize and a read of d_located and the flags on the host, the masks built
               there, rs_repair_device_batch_masks in place
  damage:      what the four damaged legs begin every call with, alone: one index_copy_ that
               writes the corrupt bytes back (a heal leaves the stripe healed)
The damaged legs are printed as measured and net of the damage leg.  The script has a time limit
of its own (an alarm), checks the results once per case, and tries nothing twice.
"""
import ctypes
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reed-solomon-simd_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import reed_solomon_simd as rs  # noqa: E402

signal.alarm(280)  # the whole run; a hang ends the process

N = M = 1024
MAX_ROWS = 16
rounds, iters = 5, 50
ctx = rs.default_context()
u, u32, vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p
g = torch.Generator(device="cuda")
g.manual_seed(1)
p = lambda t: vp(t.data_ptr())


def head(S):
    return (vp(ctx.handle.value), ctypes.c_int(0), u(N), u(M), u(S))


def locate_call(S, B, orig, rec, loc, flags):
    return rs.DeviceCall(rs._lib.rs_locate_device_batch,
                         head(S) + (u(B), p(orig), u(0), u(0), p(rec), u(0), u(0), None, p(loc), p(flags), vp(None)),
                         (orig, rec, loc, flags))


def heal_call(S, B, orig, rec, loc, flags, act):
    return rs.DeviceCall(rs._lib.rs_heal_device_batch,
                         head(S) + (u(B), p(orig), u(0), u(0), p(rec), u(0), u(0), None,
                                    u32(rs.HEAL_ORIGINAL | rs.HEAL_RECOVERY), u32(MAX_ROWS), p(loc), p(flags), p(act),
                                    vp(None)), (orig, rec, loc, flags, act))


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


print(f"{N}:{M} ({rs.version()}); us per call, median of {rounds} rounds of {iters} back-to-back calls")
for S, B in ((1024, 1), (1024, 64), (65536, 1)):
    orig = torch.randint(0, 256, (B, N, S), dtype=torch.uint8, device="cuda", generator=g)
    rec = torch.empty((B, M, S), dtype=torch.uint8, device="cuda")
    rs.encode_device_batch(N, M, S, orig, rec)
    torch.cuda.synchronize()
    loc = torch.empty((B,), dtype=torch.int32, device="cuda")
    flags = torch.empty((B, M), dtype=torch.uint8, device="cuda")
    act = torch.empty((B,), dtype=torch.uint8, device="cuda")
    # working copies that the damaged legs corrupt and heal: original 7 b + 3 and recovery row
    # 5 b + 1 of stripe b, one bit in a middle byte
    w_orig, w_rec = orig.clone(), rec.clone()
    where_o = [(7 * b + 3) % N for b in range(B)]
    where_r = [(5 * b + 1) % M for b in range(B)]
    at_o = torch.tensor([(b * N + i) * S + S // 2 + 1 for b, i in enumerate(where_o)], device="cuda")
    at_r = torch.tensor([(b * M + j) * S + S // 2 + 1 for b, j in enumerate(where_r)], device="cuda")
    bad_o, bad_r = orig.view(-1)[at_o] ^ 0x10, rec.view(-1)[at_r] ^ 0x10
    flat_o, flat_r = w_orig.view(-1), w_rec.view(-1)
    all_orig, all_rec = np.ones((B, N), np.uint8), np.ones((B, M), np.uint8)

    locate = locate_call(S, B, orig, rec, loc, flags)
    heal_clean = heal_call(S, B, orig, rec, loc, flags, act)
    heal_o = heal_call(S, B, w_orig, rec, loc, flags, act)
    heal_r = heal_call(S, B, orig, w_rec, loc, flags, act)
    locate_o = locate_call(S, B, w_orig, rec, loc, flags)
    locate_r = locate_call(S, B, orig, w_rec, loc, flags)

    def damage():
        flat_o.index_copy_(0, at_o, bad_o)

    def heal_orig():
        flat_o.index_copy_(0, at_o, bad_o)
        heal_o()

    def heal_rows():
        flat_r.index_copy_(0, at_r, bad_r)
        heal_r()

    def scrub(call, d_o, d_r):
        call()
        torch.cuda.synchronize()
        located, fl = loc.cpu().numpy(), flags.cpu().numpy()
        orig_ok, rec_ok = all_orig.copy(), all_rec.copy()
        for b, i in enumerate(located):
            if i >= 0:
                orig_ok[b, i] = 0
            elif i == rs.LOCATE_ROWS:
                rec_ok[b] = 1 - fl[b]
        rs.repair_device_batch_masks(N, M, S, d_o, orig_ok, d_r, rec_ok, d_o, d_r)

    def scrub_orig():
        flat_o.index_copy_(0, at_o, bad_o)
        scrub(locate_o, w_orig, rec)

    def scrub_rows():
        flat_r.index_copy_(0, at_r, bad_r)
        scrub(locate_r, orig, w_rec)

    # the results, once
    ok = True
    for f, want_loc, want_act in ((heal_clean, [rs.LOCATE_CLEAN] * B, 0), (heal_orig, where_o, rs.HEAL_ORIGINAL),
                                  (heal_rows, [rs.LOCATE_ROWS] * B, rs.HEAL_RECOVERY), (scrub_orig, where_o, None),
                                  (scrub_rows, [rs.LOCATE_ROWS] * B, None)):
        loc.fill_(-9), flags.fill_(0xFF), act.fill_(0xFF)
        f()
        torch.cuda.synchronize()
        ok = ok and loc.tolist() == want_loc and (want_act is None or act.tolist() == [want_act] * B)
        ok = ok and bool(torch.equal(w_orig, orig)) and bool(torch.equal(w_rec, rec))
    legs = {"locate": locate, "heal clean": heal_clean, "heal orig": heal_orig, "heal rows": heal_rows,
            "scrub orig": scrub_orig, "scrub rows": scrub_rows, "damage": damage}
    us = time_legs(legs)
    med = {k: statistics.median(v) for k, v in us.items()}
    print(f"shards of {S} B, " + (f"batch of {B} stripes" if B > 1 else "one stripe"))
    for k, v in us.items():
        print(f"  {k:10s} median {med[k]:8.2f}   rounds " + " ".join(f"{x:8.2f}" for x in v)
              + f"   spread (max - min) {max(v) - min(v):6.2f} us = {(max(v) - min(v)) / med[k] * 100:4.1f} %")
    base, d = med["locate"], med["damage"]
    print(f"  heal clean - locate = {med['heal clean'] - base:+.2f} us  ({med['heal clean'] / base:.3f})")
    for k in ("heal orig", "heal rows", "scrub orig", "scrub rows"):
        print(f"  {k} net of the damage leg = {med[k] - d:.2f} us; - locate = {med[k] - d - base:+.2f} us "
              f"({(med[k] - d) / base:.3f})")
    print(f"  scrub orig - heal orig = {med['scrub orig'] - med['heal orig']:+.2f} us, scrub rows - heal rows = "
          f"{med['scrub rows'] - med['heal rows']:+.2f} us")
    rs.profile_enable(True)
    for name, call in (("heal clean", heal_clean), ("heal orig", heal_orig), ("heal rows", heal_rows),
                       ("scrub orig", scrub_orig), ("scrub rows", scrub_rows)):
        rs.profile_collect()
        call()
        torch.cuda.synchronize()
        print(f"  launches ({name}): " + "; ".join(f"{n} {ms * 1e3:.1f} us" for n, ms, _ in rs.profile_collect()))
    rs.profile_enable(False)
    print(f"  results_ok={ok}")
    assert ok
    del orig, rec, w_orig, w_rec
rs.check_device()
