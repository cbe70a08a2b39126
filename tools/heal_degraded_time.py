"""Time rs_heal_device_degraded_batch against the degraded locate alone and against what a caller
had before (development aid; the numbers in DESIGN.md "Degraded heal" come from it):

    timeout -k 10 300 python tools/heal_degraded_time.py [--package DIR] [--locate-only]

One process, one build.  Cases: 1024:1024 x 1 KiB as one stripe and as a 64-stripe batch, and
1024:1024 x 64 KiB as one stripe, every recovery row selected, both mode bits, with m = 1 and m = 16
originals missing (the same ones in every stripe), d_restored = d_original.  Method of
tools/heal_time.py: warm-up, `iters` back-to-back calls, one synchronize, host clock; the legs
alternate within a round; the library's calls are pre-bound (DeviceCall: what a C caller of the ABI
pays).
  locate clean / corrupt:  rs_locate_device_degraded_batch on the clean batch and with one corrupt
               present original in every stripe -- the yardstick of the clean case (its kernels are
               the parent commit's); each leg's round-to-round spread (max - min) is printed
  heal clean / corrupt:    rs_heal_device_degraded_batch (max_rows 16) on the same two inputs
  scrub corrupt:  the yardstick of the damaged case: the degraded locate, a synchronize and a read
               of d_located on the host, the masks built there, rs_repair_device_batch_masks in
               place with the named shard absent
  damage:      what the corrupt heal and scrub legs begin every call with, alone: one index_copy_
               that writes the corrupt bytes back (a heal leaves the stripe healed)
The corrupt heal and scrub legs are printed as measured and net of the damage leg.  The launch
floor is the shortest launch of the clean heal by the library's own events.  The verdict per case:
does the clean heal land within the clean locate's spread plus one launch floor of it?  --package
DIR imports reed_solomon_simd from DIR instead of this tree (another build of the library);
--locate-only runs the locate legs alone (a build without the degraded heal).  The script has a
time limit of its own (an alarm), checks the results once per case, and tries nothing twice.
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


def locate_call(S, B, orig, present, rec, loc, flags):
    return rs.DeviceCall(rs._lib.rs_locate_device_degraded_batch,
                         head(S) + (u(B), p(orig), u(0), u(0), present, p(rec), u(0), u(0), None, p(orig), u(0), u(0),
                                    p(loc), p(flags), vp(None)), (orig, rec, loc, flags, present))


def heal_call(S, B, orig, present, rec, loc, flags, act):
    return rs.DeviceCall(rs._lib.rs_heal_device_degraded_batch,
                         head(S) + (u(B), p(orig), u(0), u(0), present, p(rec), u(0), u(0), None, p(orig), u(0), u(0),
                                    u32(MODE), u32(MAX_ROWS), p(loc), p(flags), p(act), vp(None)),
                         (orig, rec, loc, flags, act, present))


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
    clean_o = torch.randint(0, 256, (B, N, S), dtype=torch.uint8, device="cuda", generator=g)
    rec = torch.empty((B, M, S), dtype=torch.uint8, device="cuda")
    rs.encode_device_batch(N, M, S, clean_o, rec)
    torch.cuda.synchronize()
    loc = torch.empty((B,), dtype=torch.int32, device="cuda")
    flags = torch.empty((B, M), dtype=torch.uint8, device="cuda")
    act = torch.empty((B,), dtype=torch.uint8, device="cuda")
    for m in (1, 16):
        missing = [5 + 64 * k for k in range(m)]
        present_np = np.ones(N, np.uint8)
        present_np[missing] = 0
        present = bytes(present_np)
        # one corrupt present original per stripe: original 8 b + 2 of stripe b (even: never a
        # missing one), one bit in a middle byte
        where = [(8 * b + 2) % N for b in range(B)]
        assert not set(where) & set(missing)
        at = torch.tensor([(b * N + i) * S + S // 2 + 1 for b, i in enumerate(where)], device="cuda")
        bad_bytes = clean_o.view(-1)[at] ^ 0x10
        orig, l_bad, w_orig, w_rec = clean_o.clone(), clean_o.clone(), clean_o.clone(), rec.clone()
        l_bad.view(-1).index_copy_(0, at, bad_bytes)  # the locate leg reads a damaged copy that nothing heals
        for t in (orig, l_bad, w_orig):
            t[:, missing] = 0x5A  # absent rows hold junk until the first call fills them
        flat = w_orig.view(-1)

        def damage():
            flat.index_copy_(0, at, bad_bytes)

        scrub_locate = locate_call(S, B, w_orig, present, w_rec, loc, flags)
        all_rec = np.ones((B, M), np.uint8)

        def scrub():
            scrub_locate()
            torch.cuda.synchronize()
            located = loc.cpu().numpy()
            orig_ok, rec_ok = np.tile(present_np, (B, 1)), all_rec.copy()
            for b, i in enumerate(located):
                if i >= N:
                    rec_ok[b, i - N] = 0
                elif i >= 0:
                    orig_ok[b, i] = 0
            rs.repair_device_batch_masks(N, M, S, w_orig, orig_ok, w_rec, rec_ok, w_orig, w_rec)

        want_flags = np.zeros((B, M), np.uint8)
        want_flags[:, m:] = 1
        legs = {"locate clean": locate_call(S, B, orig, present, rec, loc, flags),
                "locate corrupt": locate_call(S, B, l_bad, present, rec, loc, flags)}
        checks = [(legs["locate clean"], [rs.LOCATE_CLEAN] * B, 0 * want_flags, None),
                  (legs["locate corrupt"], where, want_flags, None)]
        if not locate_only:
            heal_w = heal_call(S, B, w_orig, present, w_rec, loc, flags, act)
            legs["heal clean"] = heal_call(S, B, orig, present, rec, loc, flags, act)
            legs["heal corrupt"] = lambda h=heal_w: (damage(), h())
            legs["scrub corrupt"] = lambda: (damage(), scrub())
            legs["damage"] = damage
            checks += [(legs["heal clean"], [rs.LOCATE_CLEAN] * B, 0 * want_flags, 0),
                       (legs["heal corrupt"], where, want_flags, 1),
                       (legs["scrub corrupt"], where, want_flags, None)]
        ok = True  # the results, once
        for f, want_loc, wf, want_act in checks:
            loc.fill_(-9), flags.fill_(0xFF), act.fill_(0xFF)
            f()
            torch.cuda.synchronize()
            ok = ok and loc.tolist() == want_loc and np.array_equal(flags.cpu().numpy(), wf)
            ok = ok and (want_act is None or act.tolist() == [want_act] * B)
            ok = ok and bool(torch.equal(orig, clean_o)) and bool(torch.equal(w_rec, rec))
            if want_act == 1 or f is legs.get("scrub corrupt"):  # the two legs that leave w_orig healed
                ok = ok and bool(torch.equal(w_orig, clean_o))
        us = time_legs(legs)
        med = {k: statistics.median(v) for k, v in us.items()}
        spread = {k: max(v) - min(v) for k, v in us.items()}
        print(f"shards of {S} B, " + (f"batch of {B} stripes" if B > 1 else "one stripe") + f", m = {m}")
        for k, v in us.items():
            print(f"  {k:15s} median {med[k]:8.2f}   rounds " + " ".join(f"{x:8.2f}" for x in v)
                  + f"   spread (max - min) {spread[k]:6.2f} us = {spread[k] / med[k] * 100:4.1f} %")
        rs.profile_enable(True)
        recs = {}
        for name, call in legs.items():
            if name == "damage":
                continue
            rs.profile_collect()
            call()
            torch.cuda.synchronize()
            recs[name] = [(n, ms * 1e3) for n, ms, _ in rs.profile_collect()]
            print(f"  launches ({name}): " + "; ".join(f"{n} {t:.1f} us" for n, t in recs[name]))
        rs.profile_enable(False)
        if not locate_only:
            floor = min(t for _, t in recs["heal clean"])
            d, bound = med["heal clean"] - med["locate clean"], spread["locate clean"] + floor
            print(f"  launch floor (the shortest launch of the clean heal, by the events): {floor:.2f} us")
            print(f"  heal clean - locate clean = {d:+.2f} us; the locate's spread + one launch floor = {bound:.2f} us: "
                  + ("within" if d <= bound else "NOT within"))
            hc, sc = med["heal corrupt"] - med["damage"], med["scrub corrupt"] - med["damage"]
            print(f"  heal corrupt net of the damage leg = {hc:.2f} us; - locate corrupt = "
                  f"{hc - med['locate corrupt']:+.2f} us")
            print(f"  scrub corrupt net of the damage leg = {sc:.2f} us; scrub corrupt - heal corrupt = {sc - hc:+.2f} us "
                  f"({sc / hc:.2f} x)")
        print(f"  results_ok={ok}")
        assert ok
        del orig, l_bad, w_orig, w_rec
    del clean_o, rec
rs.check_device()
