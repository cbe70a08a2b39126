"""Time a partial-stripe write (rs_update_device*) by both of its routes against the full encode
(development aid; the table in DESIGN.md "Update" and the default direct_max come from it):

    timeout -k 10 300 python tools/update_time.py [N M]        default 1024 1024

One process, one build; shards of 1 KiB and 64 KiB; count in {1, 2, 4, 8, 16, 32, 64}.  Method of
tools/repair_time.py: warm-up, `iters` back-to-back calls, one synchronize, host clock; the forms
alternate in rounds, every call pre-bound (DeviceCall: what a C caller of the ABI pays).
  (a) direct_cold:  the direct route with the index list rotated every call, so every call pays
                    the coefficient step (unit stripe, its encode, the logs)
  (b) direct_warm:  the direct route with one index list: the single k_update launch
  (c) reencode:     the re-encode route (delta stripe in zeroed scratch, encode, XOR)
  (e) encode:       rs_encode_device on the full stripe: what a caller without this call runs
All in the delta form (d_old = NULL) on every recovery row.  Then a 64-stripe batch at count 1
(1 KiB shards).  The script has a time limit of its own (an alarm), checks each route's bytes once
per case against the encode of the modified stripe, and tries nothing twice.
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

args = sys.argv[1:]
N, M = (int(a) for a in args[:2]) if len(args) >= 2 else (1024, 1024)
COUNTS = (1, 2, 4, 8, 16, 32, 64)
B = 64
rounds, iters = 5, 50
ROTATIONS = 4
ctx = rs.default_context()
u, vp = ctypes.c_uint64, ctypes.c_void_p
g = torch.Generator(device="cuda")
g.manual_seed(1)
rng = np.random.default_rng(1)


def update_call(S, idx, d_new, d_rec, stripes=0):
    arr = (u * len(idx))(*[int(i) for i in idx])
    head = (vp(ctx.handle.value), ctypes.c_int(0), u(N), u(M), u(S))
    p = lambda t: vp(t.data_ptr())
    if stripes:
        a = head + (u(stripes), arr, u(len(idx)), vp(None), u(0), u(0), p(d_new), u(0), u(0), p(d_rec), u(0), u(0),
                    None, vp(None))
        return rs.DeviceCall(rs._lib.rs_update_device_batch, a, (arr, d_new, d_rec))
    a = head + (arr, u(len(idx)), vp(None), u(0), p(d_new), u(0), p(d_rec), u(0), None, vp(None))
    return rs.DeviceCall(rs._lib.rs_update_device, a, (arr, d_new, d_rec))


def time_forms(forms):
    """forms: name -> (direct_max or None, callable)."""
    for dm, f in forms.values():
        if dm is not None:
            rs.update_set_direct_max(dm)
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    us = {name: [] for name in forms}
    for _ in range(rounds):
        for name, (dm, f) in forms.items():
            if dm is not None:
                rs.update_set_direct_max(dm)
            t0 = time.perf_counter()
            for _ in range(iters):
                f()
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) / iters * 1e6)
    return {name: statistics.median(v) for name, v in us.items()}, \
           {name: (max(v) - min(v)) / statistics.median(v) * 100 for name, v in us.items()}


def verified(S, idx, orig, rec0, stripes=0):
    """Both routes give the encode of the modified stripe (checked once, on copies)."""
    batch = stripes > 0
    new = torch.randint(0, 256, orig[..., idx, :].shape, dtype=torch.uint8, device="cuda", generator=g)
    mod = orig.clone()
    mod[..., idx, :] = new
    want = torch.empty_like(rec0)
    (rs.encode_device_batch if batch else rs.encode_device)(N, M, S, mod, want)
    delta = (orig[..., idx, :] ^ new).contiguous()
    ok = True
    for dm in (256, 0):
        rs.update_set_direct_max(dm)
        r = rec0.clone()
        update_call(S, idx, delta, r, stripes)()
        torch.cuda.synchronize()
        ok = ok and torch.equal(r, want)
    return ok, delta


print(f"{N}:{M} ({rs.version()}); us per call, median of {rounds} rounds of {iters} calls (spread % of the median)")
crossover = {}
for S in (1024, 65536):
    orig = torch.randint(0, 256, (N, S), dtype=torch.uint8, device="cuda", generator=g)
    rec0 = torch.empty((M, S), dtype=torch.uint8, device="cuda")
    rs.encode_device(N, M, S, orig, rec0)
    torch.cuda.synchronize()
    enc_out = torch.empty_like(rec0)
    enc = rs.encode_device_call(N, M, S, orig, enc_out)
    print(f"shards of {S} B")
    print("  count  direct_cold  direct_warm     reencode       encode   warm/reenc  warm/encode  bytes_ok")
    for count in COUNTS:
        idx = rng.choice(N, count, replace=False)
        ok, delta = verified(S, idx, orig, rec0)
        rec = rec0.clone()
        warm = update_call(S, idx, delta, rec)
        cold = [update_call(S, (idx + r + 1) % N, delta, rec) for r in range(ROTATIONS)]
        state = {"k": 0}

        def cold_call():
            state["k"] = (state["k"] + 1) % ROTATIONS
            cold[state["k"]]()

        med, spread = time_forms({"direct_cold": (256, cold_call), "direct_warm": (256, warm),
                                  "reencode": (0, warm), "encode": (None, enc)})
        print(f"  {count:5d}" + "".join(f"  {med[k]:7.1f} ({spread[k]:2.0f})" for k in med)
              + f"   {med['direct_warm'] / med['reencode']:9.2f}  {med['direct_warm'] / med['encode']:11.2f}  {ok}")
        if med["direct_warm"] < med["reencode"]:
            crossover.setdefault(S, []).append(count)
        assert ok
    rs.profile_enable(True)
    rs.profile_collect()
    rs.update_set_direct_max(256)
    cold[0]()
    warm()
    rs.update_set_direct_max(0)
    warm()
    torch.cuda.synchronize()
    recs = rs.profile_collect()
    rs.profile_enable(False)
    print(f"  launches at count {COUNTS[-1]} (cold, warm, reencode): "
          + "; ".join(f"{n} {ms * 1e3:.1f} us" for n, ms, _ in recs))
    del orig, rec0, enc_out, rec

S = 1024
orig = torch.randint(0, 256, (B, N, S), dtype=torch.uint8, device="cuda", generator=g)
rec0 = torch.empty((B, M, S), dtype=torch.uint8, device="cuda")
rs.encode_device_batch(N, M, S, orig, rec0)
torch.cuda.synchronize()
idx = rng.choice(N, 1, replace=False)
ok, delta = verified(S, idx, orig, rec0, B)
rec, enc_out = rec0.clone(), torch.empty_like(rec0)
warm = update_call(S, idx, delta, rec, B)
head = (vp(ctx.handle.value), ctypes.c_int(0), u(N), u(M), u(S), u(B))
enc = rs.DeviceCall(rs._lib.rs_encode_device_batch,
                    head + (vp(orig.data_ptr()), u(0), u(0), vp(enc_out.data_ptr()), u(0), u(0), vp(None)), ())
med, spread = time_forms({"direct_warm": (256, warm), "reencode": (0, warm), "encode": (None, enc)})
print(f"batch of {B} stripes, shards of {S} B, count 1: "
      + "  ".join(f"{k} {med[k]:.1f} us ({spread[k]:.0f} %)" for k in med) + f"  bytes_ok={ok}")
assert ok
both = [c for c in COUNTS if all(c in crossover.get(S, []) for S in (1024, 65536))]
print(f"largest count at which direct_warm beats reencode at both shard sizes: {max(both) if both else 0}")
rs.update_set_direct_max(rs.UPDATE_DIRECT_MAX_DEFAULT)
rs.check_device()
