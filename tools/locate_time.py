"""Time rs_locate_device* against the verify's two routes and the encode of the same shape
(development aid; the numbers in DESIGN.md "Locate" come from it):

    timeout -k 10 300 python tools/locate_time.py [--package DIR] [--encode-only]

One process, one build.  Cases: 1024:1024 x 1 KiB as a single stripe and as a 64-stripe batch, and
1024:1024 x 64 KiB, every recovery row.  Method of tools/verify_time.py: warm-up, `iters`
back-to-back calls, one synchronize, host clock; the legs alternate within a round, every call
pre-bound (DeviceCall: what a C caller of the ABI pays).
  clean:    rs_locate_device[_batch] on clean stripes (what a scrub mostly sees)
  corrupt:  the same with one corrupt original in every stripe (the worst case: every stripe is
            confirmed over every row)
  cold:     the clean call with the coefficient table rebuilt every time (the rate alternates
            between high and low, each on its own clean recovery matrix: another table key);
            timed in rounds of its own after the others
  unfused / fused:  rs_verify_device[_batch] by its two routes
  encode:   rs_encode_device[_batch] of the same shape -- the yardstick
Every leg's rounds are printed, with the encode leg's own round-to-round spread (max - min).
--package DIR imports reed_solomon_simd from DIR instead of this tree (another build of the
library); --encode-only runs the encode leg alone (a build without the locate).  The script has a
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


def head(S, rate=0):
    return (vp(ctx.handle.value), ctypes.c_int(rate), u(N), u(M), u(S))


def encode_call(S, orig, rec, stripes, rate=0):
    if stripes:
        return rs.DeviceCall(rs._lib.rs_encode_device_batch,
                             head(S, rate) + (u(stripes), p(orig), u(0), u(0), p(rec), u(0), u(0), vp(None)), (orig, rec))
    return rs.DeviceCall(rs._lib.rs_encode_device, head(S, rate) + (p(orig), p(rec), vp(None)), (orig, rec))


def verify_call(S, orig, rec, flags, stripes):
    if stripes:
        return rs.DeviceCall(rs._lib.rs_verify_device_batch,
                             head(S) + (u(stripes), p(orig), u(0), u(0), p(rec), u(0), u(0), None, p(flags), vp(None)),
                             (orig, rec, flags))
    return rs.DeviceCall(rs._lib.rs_verify_device, head(S) + (p(orig), u(0), p(rec), u(0), None, p(flags), vp(None)),
                         (orig, rec, flags))


def locate_call(S, orig, rec, loc, flags, stripes, rate=0):
    if stripes:
        return rs.DeviceCall(rs._lib.rs_locate_device_batch,
                             head(S, rate) + (u(stripes), p(orig), u(0), u(0), p(rec), u(0), u(0), None, p(loc),
                                              p(flags), vp(None)), (orig, rec, loc, flags))
    return rs.DeviceCall(rs._lib.rs_locate_device,
                         head(S, rate) + (p(orig), u(0), p(rec), u(0), None, p(loc), p(flags), vp(None)),
                         (orig, rec, loc, flags))


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


print(f"{N}:{M} ({rs.version()}); us per call, median of {rounds} rounds of {iters} back-to-back calls")
for S, stripes in ((1024, 0), (1024, 64), (65536, 0)):
    shape = (stripes,) if stripes else ()
    B = max(stripes, 1)
    orig = torch.randint(0, 256, shape + (N, S), dtype=torch.uint8, device="cuda", generator=g)
    rec = torch.empty(shape + (M, S), dtype=torch.uint8, device="cuda")
    encode_call(S, orig, rec, stripes)()
    torch.cuda.synchronize()
    enc_out = torch.empty_like(rec)
    legs = {"encode": (None, encode_call(S, orig, enc_out, stripes))}
    what = f"shards of {S} B, " + (f"batch of {stripes} stripes" if stripes else "one stripe")
    if not encode_only:
        flags = torch.empty(shape + (M,), dtype=torch.uint8, device="cuda")
        loc = torch.empty((B,), dtype=torch.int32, device="cuda")
        # one corrupt original per stripe: original 7 b + 3 of stripe b, one bit in a middle byte
        bad = orig.clone()
        where = [(7 * b + 3) % N for b in range(B)]
        for b, i in enumerate(where):
            bad.view(B, N, S)[b, i, S // 2 + 1] ^= 0x10
        rec_hi, rec_lo = torch.empty_like(rec), torch.empty_like(rec)
        encode_call(S, orig, rec_hi, stripes, rate=1)()
        encode_call(S, orig, rec_lo, stripes, rate=2)()
        clean = locate_call(S, orig, rec, loc, flags, stripes)
        corrupt = locate_call(S, bad, rec, loc, flags, stripes)
        cold_hi = locate_call(S, orig, rec_hi, loc, flags, stripes, rate=1)
        cold_lo = locate_call(S, orig, rec_lo, loc, flags, stripes, rate=2)
        state = [0]

        def cold():
            state[0] ^= 1
            (cold_hi if state[0] else cold_lo)()

        # the results, once: clean, the constructed originals, and both cold calls clean
        ok = True
        for call, want in ((clean, [rs.LOCATE_CLEAN] * B), (corrupt, where), (cold_hi, [rs.LOCATE_CLEAN] * B),
                           (cold_lo, [rs.LOCATE_CLEAN] * B)):
            loc.fill_(-9), flags.fill_(0xFF)
            call()
            torch.cuda.synchronize()
            ok = ok and loc.tolist() == want and bool((flags == (0 if want[0] < 0 else 1)).all())
        has_fused = S <= 2048  # the column kernel's bound: 256 packs of 8 bytes
        ver = verify_call(S, orig, rec, flags, stripes)
        legs = dict([("clean", (None, clean)), ("corrupt", (None, corrupt)), ("unfused", (0, ver))]
                    + ([("fused", (1, ver))] if has_fused else []), **legs)
    us = time_legs(legs)
    if not encode_only:
        # rounds of its own: with the cold leg inside a round, whichever leg followed it read
        # 6-19 us high at the single 1 KiB stripe (profiles/locate/locate_time_cold_interleaved.txt)
        us.update(time_legs({"cold": (None, cold)}))
    med = {k: statistics.median(v) for k, v in us.items()}
    print(what)
    for k, v in us.items():
        print(f"  {k:8s} median {med[k]:8.2f}   rounds " + " ".join(f"{x:8.2f}" for x in v)
              + f"   spread (max - min) {max(v) - min(v):6.2f} us = {(max(v) - min(v)) / med[k] * 100:4.1f} %")
    if not encode_only:
        e = med["encode"]
        for k in [k for k in med if k != "encode"]:
            print(f"  {k} / encode = {med[k] / e:.3f}  ({med[k] - e:+.2f} us)")
        print(f"  clean - unfused = {med['clean'] - med['unfused']:+.2f} us, corrupt - clean = "
              f"{med['corrupt'] - med['clean']:+.2f} us, cold - clean = {med['cold'] - med['clean']:+.2f} us")
        rs.profile_enable(True)
        for name, call in (("clean", clean), ("corrupt", corrupt), ("cold", cold)):
            rs.profile_collect()
            call()
            torch.cuda.synchronize()
            print(f"  launches ({name}): " + "; ".join(f"{n} {ms * 1e3:.1f} us" for n, ms, _ in rs.profile_collect()))
        rs.profile_enable(False)
        print(f"  results_ok={ok}")
        assert ok
        del bad, rec_hi, rec_lo
    del orig, rec, enc_out
if not encode_only:
    rs.verify_set_fused(rs.VERIFY_FUSED_DEFAULT)
rs.check_device()
