"""Time a repair (rs_repair_device*) against the decode alone and against today's route to the
same bytes (development aid):

    timeout -k 10 300 python tools/repair_time.py [N M S [stripes [loss]]]     default 1024 1024 1024 64 0.01

One process, one build, two shapes -- the single stripe and its `stripes`-stripe batch -- and two
loss patterns: `loss` x (N + M) shards chosen at random over originals AND recovery shards, and
"one recovery shard only" (every original present).  Method of tools/dec_time.py: warm-up,
`iters` back-to-back calls, one synchronize, host clock; the forms alternate in rounds, every
call pre-bound (DeviceCall: what a C caller of the ABI pays).
  (a) repair:  one rs_repair_device[_batch] call
  (b) decode:  rs_decode_device[_batch] with the same original losses (the recovery shards stay
               missing): what the second destination costs on top of the decode
  (c) today:   rs_decode_device[_batch], then rs_encode_device[_batch] of the full matrix into a
               scratch recovery matrix.  The caller's gather of present + restored rows and the copy
               of the missing recovery rows out of the scratch are left out, which favours (c).
  (e) encode:  the encode of (c) alone: the other way to serve "one recovery shard only"
With one recovery shard only (b) has nothing to do (the call returns at once) and (c) is the encode.
The script has a time limit of its own (an alarm), checks every form's bytes once, and tries
nothing twice.  Prints one line per round and form (us per call), the medians and a / b, a / c.
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
N, M, S = (int(a) for a in args[:3]) if len(args) >= 3 else (1024, 1024, 1024)
B = int(args[3]) if len(args) > 3 else 64
loss = float(args[4]) if len(args) > 4 else 0.01
rounds, iters = 7, 100

rng = np.random.default_rng(1)
g = torch.Generator(device="cuda")
g.manual_seed(1)
full_o = torch.randint(0, 256, (B, N, S), dtype=torch.uint8, device="cuda", generator=g)
full_r = torch.empty((B, M, S), dtype=torch.uint8, device="cuda")
rs.encode_device_batch(N, M, S, full_o, full_r)
torch.cuda.synchronize()


def patterns():
    k = max(2, round((N + M) * loss))
    lost = rng.choice(N + M, k, replace=False)
    while not ((lost < N).any() and (lost >= N).any()):  # both kinds missing
        lost = rng.choice(N + M, k, replace=False)
    op, rp = np.ones(N, np.uint8), np.ones(M, np.uint8)
    op[lost[lost < N]] = 0
    rp[lost[lost >= N] - N] = 0
    one = (np.ones(N, np.uint8), np.ones(M, np.uint8))
    one[1][M - 1] = 0
    return {"random_%g" % loss: (op, rp), "one_recovery_shard": one}


def time_forms(forms):
    for f in forms.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    us = {name: [] for name in forms}
    for r in range(rounds):
        for name, f in forms.items():
            t0 = time.perf_counter()
            for _ in range(iters):
                f()
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) / iters * 1e6)
            print(f"  round {r} {name}: {us[name][-1]:.1f} us")
    return us


ctx = rs.default_context()
print(f"{N}:{M} x {S} B ({rs.version()})")
for stripes in (1, B):
    for pname, (op, rp) in patterns().items():
        batch = stripes > 1
        # the damaged stripe(s): absent rows hold junk
        d_o, d_r = full_o[:stripes].clone(), full_r[:stripes].clone()
        d_o[:, op == 0] = 0xA5
        d_r[:, rp == 0] = 0x5A
        out_a = (torch.zeros_like(d_o), torch.zeros_like(d_r))
        out_b = torch.zeros_like(d_o)
        out_c = (torch.zeros_like(d_o), torch.zeros_like(d_r))
        u, vp = ctypes.c_uint64, ctypes.c_void_p
        opb, rpb = op.tobytes(), rp.tobytes()
        head = (vp(ctx.handle.value), ctypes.c_int(0), u(N), u(M), u(S))
        p = lambda t: vp(t.data_ptr())
        if batch:
            z3 = (u(0), u(0))
            hb = head + (u(stripes),)
            a = rs.DeviceCall(rs._lib.rs_repair_device_batch,
                              hb + (p(d_o),) + z3 + (opb, p(d_r)) + z3 + (rpb, p(out_a[0])) + z3 + (p(out_a[1]),) + z3
                              + (vp(None),), ())
            dec = lambda out: rs.DeviceCall(rs._lib.rs_decode_device_batch,
                                            hb + (p(d_o),) + z3 + (opb, p(d_r)) + z3 + (rpb, p(out)) + z3
                                            + (vp(None),), ())
            b, dec_c = dec(out_b), dec(out_c[0])
            e = rs.DeviceCall(rs._lib.rs_encode_device_batch,
                              hb + (p(full_o),) + z3 + (p(out_c[1]),) + z3 + (vp(None),), ())
        else:
            a = rs.DeviceCall(rs._lib.rs_repair_device_strided,
                              head + (p(d_o), u(0), opb, p(d_r), u(0), rpb, p(out_a[0]), u(0), p(out_a[1]), u(0),
                                      vp(None)), ())
            b = rs.decode_device_call(N, M, S, d_o[0], op, d_r[0], rp, out_b[0])
            dec_c = rs.decode_device_call(N, M, S, d_o[0], op, d_r[0], rp, out_c[0][0])
            e = rs.encode_device_call(N, M, S, full_o[0], out_c[1][0])

        def c():
            dec_c()
            e()  # (on the full originals: the caller's gather is left out)

        print(f"{stripes} stripe(s), pattern {pname}: {int((op == 0).sum())} originals + "
              f"{int((rp == 0).sum())} recovery shards missing")
        forms = {"a_repair": a, "b_decode": b, "c_decode_encode": c, "e_encode": e}
        us = time_forms(forms)
        mo, mr = torch.from_numpy(op == 0).cuda(), torch.from_numpy(rp == 0).cuda()
        fo, fr = full_o[:stripes], full_r[:stripes]
        ok = {"a_repair": torch.equal(out_a[0][:, mo], fo[:, mo]) and torch.equal(out_a[1][:, mr], fr[:, mr])
              and not bool(out_a[0][:, ~mo].any()) and not bool(out_a[1][:, ~mr].any()),
              "b_decode": torch.equal(out_b[:, mo], fo[:, mo]),
              "c_decode_encode": torch.equal(out_c[0][:, mo], fo[:, mo]) and torch.equal(out_c[1], fr),
              "e_encode": torch.equal(out_c[1], fr)}
        med = {name: statistics.median(v) for name, v in us.items()}
        for name, v in us.items():
            print(f"{name}: median {med[name]:.1f} us  min {min(v):.1f} max {max(v):.1f} "
                  f"spread {(max(v) - min(v)) / med[name] * 100:.1f} %  bytes_ok={ok[name]}")
        print(f"a/b = {med['a_repair'] / med['b_decode']:.3f}   a/c = {med['a_repair'] / med['c_decode_encode']:.3f}   "
              f"a/e = {med['a_repair'] / med['e_encode']:.3f}   a < c: {med['a_repair'] < med['c_decode_encode']}")
        rs.profile_enable(True)
        rs.profile_collect()
        a()
        torch.cuda.synchronize()
        recs = rs.profile_collect()
        rs.profile_enable(False)
        print("a_repair launches: " + "; ".join(f"{n} {ms * 1e3:.1f} us" for n, ms, _ in recs))
        assert all(ok.values()), ok
rs.check_device()
