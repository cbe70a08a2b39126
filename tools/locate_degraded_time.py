"""Time rs_locate_device_degraded* against the two calls it replaces (development aid; the numbers
in DESIGN.md "Degraded locate" come from it):

    timeout -k 10 300 python tools/locate_degraded_time.py

One process, one build.  Cases: 1024:1024 x 1 KiB as a single stripe and as a 64-stripe batch, and
1024:1024 x 64 KiB, every recovery row selected, with m = 1 and m = 16 originals missing (the same
ones in every stripe).  Method of tools/locate_time.py: warm-up, `iters` back-to-back calls, one
synchronize, host clock; the legs alternate within a round, every call pre-bound (DeviceCall: what
a C caller of the ABI pays).
  clean:      rs_locate_device_degraded_batch on clean stripes, d_restored = d_original
  corrupt:    the same with one corrupt present original in every stripe (every stripe is
              confirmed over every check row)
  yardstick:  what a caller had before -- rs_repair_device_batch with recovery_present = R, in
              place on the same matrix, then rs_locate_device_batch under the mask K on it; both
              are the parent commit's kernels.  On the clean and on the corrupt stripes (where
              it can only say UNKNOWN: its confirm has no candidate to run over).
  cold:       the clean call with the table rebuilt every time (two presence masks alternate);
              timed in rounds of its own after the others
Every leg's rounds are printed with its round-to-round spread (max - min).  The launch floor is the
shortest launch of the call by the library's own events.  The verdict per case: does the call land
within the yardstick's spread plus one launch floor of the yardstick?  The script has a time limit
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


def encode(S, orig, rec, B):
    rs.DeviceCall(rs._lib.rs_encode_device_batch,
                  head(S) + (u(B), p(orig), u(0), u(0), p(rec), u(0), u(0), vp(None)), (orig, rec))()


def degraded_call(S, orig, present, rec, loc, flags, B):
    return rs.DeviceCall(rs._lib.rs_locate_device_degraded_batch,
                         head(S) + (u(B), p(orig), u(0), u(0), present, p(rec), u(0), u(0), None, p(orig), u(0), u(0),
                                    p(loc), p(flags), vp(None)), (orig, rec, loc, flags, present))


def yardstick_call(S, orig, present, rec, ref, check, out, loc, flags, B):
    repair = rs.DeviceCall(rs._lib.rs_repair_device_batch,
                           head(S) + (u(B), p(orig), u(0), u(0), present, p(rec), u(0), u(0), ref, p(orig), u(0), u(0),
                                      p(out), u(0), u(0), vp(None)), (orig, rec, out, present, ref))
    locate = rs.DeviceCall(rs._lib.rs_locate_device_batch,
                           head(S) + (u(B), p(orig), u(0), u(0), p(rec), u(0), u(0), check, p(loc), p(flags), vp(None)),
                           (orig, rec, loc, flags, check))

    def both():
        repair()
        locate()
    return both


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


def launches(call):
    rs.profile_collect()
    call()
    torch.cuda.synchronize()
    return [(n, ms * 1e3) for n, ms, _ in rs.profile_collect()]


print(f"{N}:{M} ({rs.version()}); us per call, median of {rounds} rounds of {iters} back-to-back calls")
for S, stripes in ((1024, 1), (1024, 64), (65536, 1)):
    B = stripes
    clean_o = torch.randint(0, 256, (B, N, S), dtype=torch.uint8, device="cuda", generator=g)
    rec = torch.empty((B, M, S), dtype=torch.uint8, device="cuda")
    encode(S, clean_o, rec, B)
    torch.cuda.synchronize()
    out = torch.empty_like(rec)
    flags = torch.empty((B, M), dtype=torch.uint8, device="cuda")
    loc = torch.empty((B,), dtype=torch.int32, device="cuda")
    for m in (1, 16):
        missing = [5 + 64 * k for k in range(m)]
        other = [7 + 64 * k for k in range(m)]  # the cold leg's second pattern
        present, present2 = bytearray([1] * N), bytearray([1] * N)
        for i in missing:
            present[i] = 0
        for i in other:
            present2[i] = 0
        present, present2 = bytes(present), bytes(present2)
        ref = bytes([1] * m + [0] * (M - m))
        check = bytes([0] * m + [1] * (M - m))
        # one corrupt present original per stripe: original 8 b + 2 of stripe b (even: never a missing
        # one), one bit in a middle byte
        where = [(8 * b + 2) % N for b in range(B)]
        assert not set(where) & (set(missing) | set(other))
        orig, bad = clean_o.clone(), clean_o.clone()
        for b, i in enumerate(where):
            bad[b, i, S // 2 + 1] ^= 0x10
        for t in (orig, bad):
            t[:, missing] = 0x5A  # absent rows hold junk until the first call fills them
        cold_o = clean_o.clone()
        clean = degraded_call(S, orig, present, rec, loc, flags, B)
        corrupt = degraded_call(S, bad, present, rec, loc, flags, B)
        cold_a = degraded_call(S, cold_o, present, rec, loc, flags, B)
        cold_b = degraded_call(S, cold_o, present2, rec, loc, flags, B)
        y_clean = yardstick_call(S, orig, present, rec, ref, check, out, loc, flags, B)
        y_corrupt = yardstick_call(S, bad, present, rec, ref, check, out, loc, flags, B)
        state = [0]

        def cold():
            state[0] ^= 1
            (cold_a if state[0] else cold_b)()

        # the results, once: clean, the constructed originals, by the call and by the yardstick
        ok = True
        # (the yardstick cannot name the original: its table is over the N originals, and the
        # restored ones carry the damage too -- every check row differs and it says UNKNOWN)
        for call, want in ((clean, [rs.LOCATE_CLEAN] * B), (corrupt, where), (y_clean, [rs.LOCATE_CLEAN] * B),
                           (y_corrupt, [rs.LOCATE_UNKNOWN] * B), (cold_a, [rs.LOCATE_CLEAN] * B),
                           (cold_b, [rs.LOCATE_CLEAN] * B)):
            loc.fill_(-9), flags.fill_(0xFF)
            call()
            torch.cuda.synchronize()
            want_flags = torch.zeros((B, M), dtype=torch.uint8, device="cuda")
            if want[0] != rs.LOCATE_CLEAN:
                want_flags[:, m:] = 1
            ok = ok and loc.tolist() == want and bool((flags == want_flags).all())
        ok = ok and bool((orig == clean_o).all()) and bool((cold_o == clean_o).all())
        us = time_legs({"clean": clean, "y_clean": y_clean, "corrupt": corrupt, "y_corrupt": y_corrupt})
        us.update(time_legs({"cold": cold}))
        med = {k: statistics.median(v) for k, v in us.items()}
        spread = {k: max(v) - min(v) for k, v in us.items()}
        print(f"shards of {S} B, " + (f"batch of {B} stripes" if B > 1 else "one stripe") + f", m = {m}")
        for k, v in us.items():
            print(f"  {k:10s} median {med[k]:8.2f}   rounds " + " ".join(f"{x:8.2f}" for x in v)
                  + f"   spread (max - min) {spread[k]:6.2f} us = {spread[k] / med[k] * 100:4.1f} %")
        rs.profile_enable(True)
        recs = {name: launches(call) for name, call in (("clean", clean), ("corrupt", corrupt), ("cold", cold),
                                                        ("y_clean", y_clean))}
        rs.profile_enable(False)
        for name, r in recs.items():
            print(f"  launches ({name}): " + "; ".join(f"{n} {t:.1f} us" for n, t in r))
        floor = min(t for _, t in recs["clean"])
        print(f"  launch floor (the shortest launch of the clean call, by the events): {floor:.2f} us")
        for a, y in (("clean", "y_clean"), ("corrupt", "y_corrupt")):
            d, bound = med[a] - med[y], spread[y] + floor
            print(f"  {a} - yardstick = {d:+.2f} us; the yardstick's spread + one launch floor = {bound:.2f} us: "
                  + ("within" if d <= bound else "NOT within"))
        print(f"  cold - clean = {med['cold'] - med['clean']:+.2f} us")
        print(f"  results_ok={ok}")
        assert ok
        del orig, bad, cold_o
    del clean_o, rec, out
rs.check_device()
