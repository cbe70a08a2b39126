"""Time rs_verify_device* by both of its routes against the encode of the same shape (development
aid; the numbers in DESIGN.md "Verify" and the default of rs_verify_set_fused come from it):

    timeout -k 10 300 python tools/verify_time.py [--package DIR] [--encode-only]

One process, one build.  Cases: 1024:1024 x 1 KiB as a single stripe and as a 64-stripe batch,
and 1024:1024 x 64 KiB (past the column kernel's pack bound: the unfused route only).  Method of
tools/update_time.py: warm-up, `iters` back-to-back calls, one synchronize, host clock; the legs
alternate within a round, every call pre-bound (DeviceCall: what a C caller of the ABI pays).
  fused:    rs_verify_device[_batch] with rs_verify_set_fused(1): one k_mono_verify launch
  unfused:  the same with rs_verify_set_fused(0): the encode into scratch, then k_verify_rows
  encode:   rs_encode_device[_batch] of the same shape -- the yardstick
Every leg's rounds are printed, with the encode leg's own round-to-round spread (max - min).
--package DIR imports reed_solomon_simd from DIR instead of this tree (another build of the
library); --encode-only runs the encode leg alone (a build without the verify).  The script has a
time limit of its own (an alarm), checks the flags once per case (a clean stripe, then one with
two rows corrupted), and tries nothing twice.
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
encode_only = "--encode-only" in args
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


def encode_call(S, orig, rec, stripes):
    head = (vp(ctx.handle.value), ctypes.c_int(0), u(N), u(M), u(S))
    if stripes:
        return rs.DeviceCall(rs._lib.rs_encode_device_batch,
                             head + (u(stripes), p(orig), u(0), u(0), p(rec), u(0), u(0), vp(None)), (orig, rec))
    return rs.DeviceCall(rs._lib.rs_encode_device, head + (p(orig), p(rec), vp(None)), (orig, rec))


def verify_call(S, orig, rec, flags, stripes):
    head = (vp(ctx.handle.value), ctypes.c_int(0), u(N), u(M), u(S))
    if stripes:
        return rs.DeviceCall(rs._lib.rs_verify_device_batch,
                             head + (u(stripes), p(orig), u(0), u(0), p(rec), u(0), u(0), None, p(flags), vp(None)),
                             (orig, rec, flags))
    return rs.DeviceCall(rs._lib.rs_verify_device, head + (p(orig), u(0), p(rec), u(0), None, p(flags), vp(None)),
                         (orig, rec, flags))


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


def flags_ok(S, orig, rec, flags, stripes, modes):
    """A clean stripe gives no flag; two corrupted rows give exactly those two (once per route)."""
    ok = True
    bad = rec.clone()
    rows = bad.view(-1, S)
    hit = [3, rows.shape[0] - 1]
    rows[hit[0], 5] ^= 1
    rows[hit[1], S - 1] ^= 0x80
    for mode in modes:
        rs.verify_set_fused(mode)
        for held, want in ((rec, []), (bad, hit)):
            flags.fill_(0xFF)
            verify_call(S, orig, held, flags, stripes)()
            torch.cuda.synchronize()
            ok = ok and torch.nonzero(flags.view(-1)).view(-1).tolist() == want
    return ok


print(f"{N}:{M} ({rs.version()}); us per call, median of {rounds} rounds of {iters} back-to-back calls")
for S, stripes in ((1024, 0), (1024, 64), (65536, 0)):
    shape = (stripes,) if stripes else ()
    orig = torch.randint(0, 256, shape + (N, S), dtype=torch.uint8, device="cuda", generator=g)
    rec = torch.empty(shape + (M, S), dtype=torch.uint8, device="cuda")
    (rs.encode_device_batch if stripes else rs.encode_device)(N, M, S, orig, rec)
    torch.cuda.synchronize()
    enc_out = torch.empty_like(rec)
    legs = {"encode": (None, encode_call(S, orig, enc_out, stripes))}
    what = f"shards of {S} B, " + (f"batch of {stripes} stripes" if stripes else "one stripe")
    if not encode_only:
        flags = torch.empty(shape + (M,), dtype=torch.uint8, device="cuda")
        has_fused = S <= 2048  # the column kernel's bound: 256 packs of 8 bytes
        ver = verify_call(S, orig, rec, flags, stripes)
        ok = flags_ok(S, orig, rec, flags, stripes, (1, 0) if has_fused else (0,))
        legs = dict(([("fused", (1, ver))] if has_fused else []) + [("unfused", (0, ver))], **legs)
    us = time_legs(legs)
    med = {k: statistics.median(v) for k, v in us.items()}
    print(what)
    for k, v in us.items():
        print(f"  {k:8s} median {med[k]:8.2f}   rounds " + " ".join(f"{x:8.2f}" for x in v)
              + f"   spread (max - min) {max(v) - min(v):6.2f} us = {(max(v) - min(v)) / med[k] * 100:4.1f} %")
    if not encode_only:
        e = med["encode"]
        spread = max(us["encode"]) - min(us["encode"])
        for k in [k for k in ("fused", "unfused") if k in med]:
            d = med[k] - e
            print(f"  {k} / encode = {med[k] / e:.3f}  ({d:+.2f} us; the encode leg's spread is {spread:.2f} us: "
                  + ("inside" if abs(d) <= spread else "outside") + ")")
        if "fused" in med:
            print(f"  fused / unfused = {med['fused'] / med['unfused']:.3f}")
        rs.profile_enable(True)
        rs.profile_collect()
        for mode in ((1, 0) if "fused" in med else (0,)):
            rs.verify_set_fused(mode)
            ver()
        legs["encode"][1]()
        torch.cuda.synchronize()
        recs = rs.profile_collect()
        rs.profile_enable(False)
        print("  launches (" + ("fused, " if "fused" in med else "") + "unfused, encode): "
              + "; ".join(f"{n} {ms * 1e3:.1f} us" for n, ms, _ in recs))
        print(f"  flags_ok={ok}")
        assert ok
    del orig, rec, enc_out
if not encode_only:
    rs.verify_set_fused(rs.VERIFY_FUSED_DEFAULT)
rs.check_device()
