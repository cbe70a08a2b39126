"""Time rs_locate_device_robust* against rs_locate_device* of the same shape (development aid; the
numbers in DESIGN.md "Robust locate" come from it):

    timeout -k 10 300 python tools/locate_robust_time.py [--package DIR] [--locate-only]

One process, one build.  Cases: 1024:1024 x 1 KiB as a single stripe and as a 64-stripe batch, and
1024:1024 x 64 KiB, every recovery row, max_outliers 1 and 7.  Method of tools/locate_time.py:
warm-up, `iters` back-to-back calls, one synchronize, host clock; the legs alternate within a round,
every call pre-bound (DeviceCall: what a C caller of the ABI pays).
  locate clean / locate original:  rs_locate_device[_batch] on clean stripes / with one corrupt
            original in every stripe -- the yardstick
  clean tT:     the robust call on the clean stripes (what a scrub mostly sees)
  original tT:  one corrupt original in every stripe (every pair names it: T + 1 equal candidates)
  outlier tT:   the same plus one corrupt recovery row per stripe, the first selected row (pair 0's
                reference: its candidate fails, the others pass)
Every leg's rounds are printed, with the yardstick's own round-to-round spread (max - min).
--package DIR imports reed_solomon_simd from DIR instead of this tree (another build of the
library); --locate-only runs the two locate legs alone (a build without the robust call).  The
script has a time limit of its own (an alarm), checks the results once per case, and tries nothing
twice.
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
import torch  # noqa: E402
import reed_solomon_simd as rs  # noqa: E402

signal.alarm(280)  # the whole run; a hang ends the process

N = M = 1024
rounds, iters = 5, 50
ctx = rs.default_context()
u, u32, vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p
g = torch.Generator(device="cuda")
g.manual_seed(1)
p = lambda t: vp(t.data_ptr())


def head(S):
    return (vp(ctx.handle.value), ctypes.c_int(0), u(N), u(M), u(S))


def encode_call(S, orig, rec, stripes):
    if stripes:
        return rs.DeviceCall(rs._lib.rs_encode_device_batch,
                             head(S) + (u(stripes), p(orig), u(0), u(0), p(rec), u(0), u(0), vp(None)), (orig, rec))
    return rs.DeviceCall(rs._lib.rs_encode_device, head(S) + (p(orig), p(rec), vp(None)), (orig, rec))


def locate_call(S, orig, rec, loc, flags, stripes):
    if stripes:
        return rs.DeviceCall(rs._lib.rs_locate_device_batch,
                             head(S) + (u(stripes), p(orig), u(0), u(0), p(rec), u(0), u(0), None, p(loc), p(flags),
                                        vp(None)), (orig, rec, loc, flags))
    return rs.DeviceCall(rs._lib.rs_locate_device,
                         head(S) + (p(orig), u(0), p(rec), u(0), None, p(loc), p(flags), vp(None)),
                         (orig, rec, loc, flags))


def robust_call(S, orig, rec, t, loc, flags, out, stripes):
    if stripes:
        return rs.DeviceCall(rs._lib.rs_locate_device_robust_batch,
                             head(S) + (u(stripes), p(orig), u(0), u(0), p(rec), u(0), u(0), None, u32(t), p(loc),
                                        p(flags), p(out), vp(None)), (orig, rec, loc, flags, out))
    return rs.DeviceCall(rs._lib.rs_locate_device_robust,
                         head(S) + (p(orig), u(0), p(rec), u(0), None, u32(t), p(loc), p(flags), p(out), vp(None)),
                         (orig, rec, loc, flags, out))


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
for S, stripes in ((1024, 0), (1024, 64), (65536, 0)):
    shape = (stripes,) if stripes else ()
    B = max(stripes, 1)
    orig = torch.randint(0, 256, shape + (N, S), dtype=torch.uint8, device="cuda", generator=g)
    rec = torch.empty(shape + (M, S), dtype=torch.uint8, device="cuda")
    encode_call(S, orig, rec, stripes)()
    torch.cuda.synchronize()
    flags = torch.empty(shape + (M,), dtype=torch.uint8, device="cuda")
    out = torch.empty(shape + (M,), dtype=torch.uint8, device="cuda")
    loc = torch.empty((B,), dtype=torch.int32, device="cuda")
    # one corrupt original per stripe: original 7 b + 3 of stripe b, one bit in a middle byte; the
    # outlier: one bit of recovery row 0, in another column
    bad = orig.clone()
    where = [(7 * b + 3) % N for b in range(B)]
    for b, i in enumerate(where):
        bad.view(B, N, S)[b, i, S // 2 + 1] ^= 0x10
    rec_out = rec.clone()
    rec_out.view(B, M, S)[:, 0, 5] ^= 0x04
    legs = {"locate clean": locate_call(S, orig, rec, loc, flags, stripes),
            "locate original": locate_call(S, bad, rec, loc, flags, stripes)}
    checks = [(legs["locate clean"], [rs.LOCATE_CLEAN] * B, None), (legs["locate original"], where, None)]
    if not locate_only:
        for t in (1, 7):
            legs[f"clean t{t}"] = robust_call(S, orig, rec, t, loc, flags, out, stripes)
            legs[f"original t{t}"] = robust_call(S, bad, rec, t, loc, flags, out, stripes)
            legs[f"outlier t{t}"] = robust_call(S, bad, rec_out, t, loc, flags, out, stripes)
            checks += [(legs[f"clean t{t}"], [rs.LOCATE_CLEAN] * B, 0), (legs[f"original t{t}"], where, 0),
                       (legs[f"outlier t{t}"], where, 1)]
    ok = True  # the results, once
    for call, want, outliers in checks:
        loc.fill_(-9), flags.fill_(0xFF), out.fill_(0xFF)
        call()
        torch.cuda.synchronize()
        ok = ok and loc.tolist() == want and bool((flags == (0 if want[0] < 0 else 1)).all())
        if outliers is not None:
            o = out.view(B, M)
            ok = ok and int(o.sum()) == outliers * B and bool((o[:, 0] == outliers).all())
    us = time_legs(legs)
    med = {k: statistics.median(v) for k, v in us.items()}
    print(f"shards of {S} B, " + (f"batch of {stripes} stripes" if stripes else "one stripe"))
    for k, v in us.items():
        print(f"  {k:16s} median {med[k]:8.2f}   rounds " + " ".join(f"{x:8.2f}" for x in v)
              + f"   spread (max - min) {max(v) - min(v):6.2f} us = {(max(v) - min(v)) / med[k] * 100:4.1f} %")
    if not locate_only:
        for t in (1, 7):
            print(f"  t={t}: clean - locate clean = {med[f'clean t{t}'] - med['locate clean']:+.2f} us, original - locate "
                  f"original = {med[f'original t{t}'] - med['locate original']:+.2f} us, outlier - locate original = "
                  f"{med[f'outlier t{t}'] - med['locate original']:+.2f} us")
    rs.profile_enable(True)
    for name, call in legs.items():
        rs.profile_collect()
        call()
        torch.cuda.synchronize()
        print(f"  launches ({name}): " + "; ".join(f"{n} {ms * 1e3:.1f} us" for n, ms, _ in rs.profile_collect()))
    rs.profile_enable(False)
    print(f"  results_ok={ok}")
    assert ok
    del orig, rec, bad, rec_out
rs.check_device()
