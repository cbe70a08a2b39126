"""Time rs_heal_device_robust_batch against the robust locate alone and against the three-call scrub
(development aid; the numbers in DESIGN.md "Robust heal" come from it):

    timeout -k 10 300 python tools/heal_robust_time.py [--package DIR] [--locate-only]

One process, one build.  Cases: 1024:1024 x 1 KiB as one stripe and as a 64-stripe batch, and
1024:1024 x 64 KiB as one stripe, every recovery row, both mode bits, max_outliers 1 and 7.  Method
of tools/heal_time.py: warm-up, `iters` back-to-back calls, one synchronize, host clock; the legs
alternate within a round; the library's calls are pre-bound (DeviceCall: what a C caller of the ABI
pays).  Per max_outliers T:
  locate clean / outlier / row tT:  rs_locate_device_robust_batch on the clean batch, with one
               corrupt original plus a flipped bit in recovery row 0 of every stripe, and with one
               corrupt recovery row in every stripe -- the yardstick (its kernels are the parent
               commit's); each leg's round-to-round spread (max - min) is printed
  heal clean / outlier / row tT:    rs_heal_device_robust_batch (both mode bits, max_rows 16) on the
               same three inputs
  scrub outlier tT:  the first damage by the three calls: rs_locate_device_robust_batch, a
               synchronize and a read of d_located, the flags and d_outlier on the host, the masks
               built there, rs_repair_device_batch_masks in place
  damage outlier / damage row:  what the damaged heal and scrub legs begin every call with, alone:
               one index_copy_ that writes the corrupt bytes back (a heal leaves the stripe healed)
The damaged heal and scrub legs are printed as measured and net of their damage leg.  --package DIR
imports reed_solomon_simd from DIR instead of this tree (another build of the library);
--locate-only runs the locate legs alone (a build without the robust heal).  The script has a time
limit of its own (an alarm), checks the results once per case, and tries nothing twice.
"""
import ctypes
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
package = args[args.index("--package") + 1] if "--package" in args else os.path.join(ROOT, "reed-solomon-simd_amd")
locate_only = "--locate-only" in args
sys.path.insert(0, package)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import reed_solomon_simd as rs  # noqa: E402

signal.alarm(280)  # the whole run; a hang ends the process

N = M = 1024
MAX_ROWS = 16
MODE = 3  # RS_HEAL_ORIGINAL | RS_HEAL_RECOVERY
rounds, iters = 5, 50
ctx = rs.default_context()
u, u32, vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p
g = torch.Generator(device="cuda")
g.manual_seed(1)
p = lambda t: vp(t.data_ptr())


def head(S):
    return (vp(ctx.handle.value), ctypes.c_int(0), u(N), u(M), u(S))


def locate_call(S, B, orig, rec, t, loc, flags, out):
    return rs.DeviceCall(rs._lib.rs_locate_device_robust_batch,
                         head(S) + (u(B), p(orig), u(0), u(0), p(rec), u(0), u(0), None, u32(t), p(loc), p(flags),
                                    p(out), vp(None)), (orig, rec, loc, flags, out))


def heal_call(S, B, orig, rec, t, loc, flags, out, act):
    return rs.DeviceCall(rs._lib.rs_heal_device_robust_batch,
                         head(S) + (u(B), p(orig), u(0), u(0), p(rec), u(0), u(0), None, u32(t), u32(MODE),
                                    u32(MAX_ROWS), p(loc), p(flags), p(out), p(act), vp(None)),
                         (orig, rec, loc, flags, out, act))


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
    out = torch.empty((B, M), dtype=torch.uint8, device="cuda")
    act = torch.empty((B,), dtype=torch.uint8, device="cuda")
    # the outlier case: original 7 b + 3 of stripe b, one bit in a middle byte, and one bit of
    # recovery row 0 in another column -- both matrices in ONE buffer, so that one index_copy_ puts
    # the damage back.  The row case: recovery row 5 b + 1 of stripe b
    both = torch.cat([orig.view(-1), rec.view(-1)])
    w_orig, w_rec = both[:orig.numel()].view(B, N, S), both[orig.numel():].view(B, M, S)
    where_o = [(7 * b + 3) % N for b in range(B)]
    where_r = [(5 * b + 1) % M for b in range(B)]
    at_both = torch.tensor([(b * N + i) * S + S // 2 + 1 for b, i in enumerate(where_o)]
                           + [orig.numel() + b * M * S + 5 for b in range(B)], device="cuda")
    bad_both = both[at_both] ^ torch.tensor([0x10] * B + [0x04] * B, dtype=torch.uint8, device="cuda")
    r_rec = rec.clone()
    at_r = torch.tensor([(b * M + j) * S + S // 2 + 1 for b, j in enumerate(where_r)], device="cuda")
    bad_r = rec.view(-1)[at_r] ^ 0x10
    flat_r = r_rec.view(-1)
    # the locate legs read damaged copies that nothing heals
    l_both = both.clone()
    l_both.index_copy_(0, at_both, bad_both)
    l_orig, l_rec = l_both[:orig.numel()].view(B, N, S), l_both[orig.numel():].view(B, M, S)
    l_row = rec.clone()
    l_row.view(-1).index_copy_(0, at_r, bad_r)
    all_orig, all_rec = np.ones((B, N), np.uint8), np.ones((B, M), np.uint8)

    def damage_outlier():
        both.index_copy_(0, at_both, bad_both)

    def damage_row():
        flat_r.index_copy_(0, at_r, bad_r)

    def scrub(call):
        call()
        torch.cuda.synchronize()
        located, fl, ol = loc.cpu().numpy(), flags.cpu().numpy(), out.cpu().numpy()
        orig_ok, rec_ok = all_orig.copy(), all_rec.copy()
        for b, i in enumerate(located):
            if i >= 0:
                orig_ok[b, i] = 0
                rec_ok[b] = 1 - ol[b]
            elif i == rs.LOCATE_ROWS:
                rec_ok[b] = 1 - fl[b]
        rs.repair_device_batch_masks(N, M, S, w_orig, orig_ok, w_rec, rec_ok, w_orig, w_rec)

    legs, checks = {}, []
    outlier0 = np.zeros((B, M), np.uint8)
    outlier0[:, 0] = 1
    for t in (1, 7):
        legs[f"locate clean t{t}"] = locate_call(S, B, orig, rec, t, loc, flags, out)
        legs[f"locate outlier t{t}"] = locate_call(S, B, l_orig, l_rec, t, loc, flags, out)
        legs[f"locate row t{t}"] = locate_call(S, B, orig, l_row, t, loc, flags, out)
        checks += [(legs[f"locate clean t{t}"], [rs.LOCATE_CLEAN] * B, 0 * outlier0, None),
                   (legs[f"locate outlier t{t}"], where_o, outlier0, None),
                   (legs[f"locate row t{t}"], [rs.LOCATE_ROWS] * B, 0 * outlier0, None)]
        if locate_only:
            continue
        heal_o = heal_call(S, B, w_orig, w_rec, t, loc, flags, out, act)
        heal_r = heal_call(S, B, orig, r_rec, t, loc, flags, out, act)
        scrub_o = locate_call(S, B, w_orig, w_rec, t, loc, flags, out)
        legs[f"heal clean t{t}"] = heal_call(S, B, orig, rec, t, loc, flags, out, act)
        legs[f"heal outlier t{t}"] = lambda h=heal_o: (damage_outlier(), h())
        legs[f"heal row t{t}"] = lambda h=heal_r: (damage_row(), h())
        legs[f"scrub outlier t{t}"] = lambda c=scrub_o: (damage_outlier(), scrub(c))
        checks += [(legs[f"heal clean t{t}"], [rs.LOCATE_CLEAN] * B, 0 * outlier0, 0),
                   (legs[f"heal outlier t{t}"], where_o, outlier0, 3),
                   (legs[f"heal row t{t}"], [rs.LOCATE_ROWS] * B, 0 * outlier0, 2),
                   (legs[f"scrub outlier t{t}"], where_o, outlier0, None)]
    if not locate_only:
        legs["damage outlier"], legs["damage row"] = damage_outlier, damage_row

    ok = True  # the results, once
    for f, want_loc, want_out, want_act in checks:
        loc.fill_(-9), flags.fill_(0xFF), out.fill_(0xFF), act.fill_(0xFF)
        f()
        torch.cuda.synchronize()
        ok = ok and loc.tolist() == want_loc and np.array_equal(out.cpu().numpy(), want_out)
        ok = ok and (want_act is None or act.tolist() == [want_act] * B)
        ok = ok and bool(torch.equal(w_orig, orig)) and bool(torch.equal(w_rec, rec)) and bool(torch.equal(r_rec, rec))
    us = time_legs(legs)
    med = {k: statistics.median(v) for k, v in us.items()}
    print(f"shards of {S} B, " + (f"batch of {B} stripes" if B > 1 else "one stripe"))
    for k, v in us.items():
        print(f"  {k:18s} median {med[k]:8.2f}   rounds " + " ".join(f"{x:8.2f}" for x in v)
              + f"   spread (max - min) {max(v) - min(v):6.2f} us = {(max(v) - min(v)) / med[k] * 100:4.1f} %")
    if not locate_only:
        d_o, d_r = med["damage outlier"], med["damage row"]
        for t in (1, 7):
            base = med[f"locate clean t{t}"]
            print(f"  t={t}: heal clean - locate clean = {med[f'heal clean t{t}'] - base:+.2f} us "
                  f"({med[f'heal clean t{t}'] / base:.3f})")
            ho, hr, so = med[f"heal outlier t{t}"] - d_o, med[f"heal row t{t}"] - d_r, med[f"scrub outlier t{t}"] - d_o
            print(f"  t={t}: heal outlier net of its damage leg = {ho:.2f} us; - locate outlier = "
                  f"{ho - med[f'locate outlier t{t}']:+.2f} us ({ho / base:.3f} of the clean locate)")
            print(f"  t={t}: heal row net of its damage leg = {hr:.2f} us; - locate row = "
                  f"{hr - med[f'locate row t{t}']:+.2f} us ({hr / base:.3f} of the clean locate)")
            print(f"  t={t}: scrub outlier net of its damage leg = {so:.2f} us ({so / base:.3f} of the clean locate); "
                  f"scrub outlier - heal outlier = {so - ho:+.2f} us ({so / ho:.2f} x)")
    rs.profile_enable(True)
    for name, call in legs.items():
        if name.startswith("damage") or not name.endswith(("t1", "t7")):
            continue
        rs.profile_collect()
        call()
        torch.cuda.synchronize()
        print(f"  launches ({name}): " + "; ".join(f"{n} {ms * 1e3:.1f} us" for n, ms, _ in rs.profile_collect()))
    rs.profile_enable(False)
    print(f"  results_ok={ok}")
    assert ok
    del orig, rec, both, w_orig, w_rec, r_rec, l_both, l_orig, l_rec, l_row
rs.check_device()
