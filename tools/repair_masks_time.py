"""Time the batch repair with a pattern per stripe against the calls that existed before it
(development aid):

    timeout -k 10 300 python tools/repair_masks_time.py [stripes N M S [loss]]   default 64 1024 1024 1024 0.01

Method of tools/dec_time.py: warm-up, `iters` back-to-back calls, one synchronize, host clock;
four forms in one process, in alternating rounds, every call pre-bound (DeviceCall: what a C
caller of the ABI pays).  Every stripe loses its own random `loss` x (N + M) of its shards,
originals and recovery shards alike.
  (a) loop:    one rs_repair_device_strided call per stripe, each with its pattern (what a caller
               had to do before rs_repair_device_batch_masks existed)
  (b) masks:   one rs_repair_device_batch_masks call
  (c) shared:  one rs_repair_device_batch call, stripe 0's pattern for every stripe: the same work
               without the descriptor copy and the per-pattern host work, and with the split plan
               and the narrowed destination maps where they apply
  (d) decode:  one rs_decode_device_batch_masks call on the same masks: the originals only, the
               recovery shards stay missing -- what the second destination costs
Prints one line per round and form (us per batch), then the medians, the spread of each form's
rounds, b/a, b/c and b/d, and bytes_ok per form; last, the launches of one call of (b), (c) and
(d) with their device time by the library's events (rs_profile_collect).  The script has a time
limit of its own (an alarm), checks every form's bytes once, and tries nothing twice.
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
B, N, M, S = (int(a) for a in args[:4]) if len(args) >= 4 else (64, 1024, 1024, 1024)
loss = float(args[4]) if len(args) > 4 else 0.01
rounds, iters = 7, 100

rng = np.random.default_rng(1)
g = torch.Generator(device="cuda")
g.manual_seed(1)
full_o = torch.randint(0, 256, (B, N, S), dtype=torch.uint8, device="cuda", generator=g)
full_r = torch.empty((B, M, S), dtype=torch.uint8, device="cuda")
rs.encode_device_batch(N, M, S, full_o, full_r)
k = max(1, round((N + M) * loss))
assert k <= M
op = np.ones((B, N), np.uint8)
rp = np.ones((B, M), np.uint8)
for b in range(B):
    lost = rng.choice(N + M, k, replace=False)
    op[b, lost[lost < N]] = 0
    rp[b, lost[lost >= N] - N] = 0
mo, mr = torch.from_numpy(op == 0).cuda(), torch.from_numpy(rp == 0).cuda()
# the damaged stripes: absent rows hold junk
d_o, d_r = full_o.clone(), full_r.clone()
d_o[mo] = 0xA5
d_r[mr] = 0x5A
# (c)'s stripes, all damaged by stripe 0's pattern
d_o0, d_r0 = full_o.clone(), full_r.clone()
d_o0[:, op[0] == 0] = 0xA5
d_r0[:, rp[0] == 0] = 0x5A
outs = {f: (torch.zeros_like(d_o), torch.zeros_like(d_r)) for f in "abcd"}
torch.cuda.synchronize()

ctx = rs.default_context()
u, vp = ctypes.c_uint64, ctypes.c_void_p
p = lambda t: vp(t.data_ptr())
z = (u(0), u(0))
head = (vp(ctx.handle.value), ctypes.c_int(0), u(N), u(M), u(S))
hb = head + (u(B),)
loop = [rs.DeviceCall(rs._lib.rs_repair_device_strided,
                      head + (p(d_o[b]), u(0), op[b].tobytes(), p(d_r[b]), u(0), rp[b].tobytes(), p(outs["a"][0][b]),
                              u(0), p(outs["a"][1][b]), u(0), vp(None)), ()) for b in range(B)]
masks = rs.DeviceCall(rs._lib.rs_repair_device_batch_masks,
                      hb + (p(d_o),) + z + (vp(op.ctypes.data), p(d_r)) + z + (vp(rp.ctypes.data), p(outs["b"][0])) + z
                      + (p(outs["b"][1]),) + z + (None, vp(None)), (op, rp))
shared = rs.DeviceCall(rs._lib.rs_repair_device_batch,
                       hb + (p(d_o0),) + z + (op[0].tobytes(), p(d_r0)) + z + (rp[0].tobytes(), p(outs["c"][0])) + z
                       + (p(outs["c"][1]),) + z + (vp(None),), ())
decode = rs.DeviceCall(rs._lib.rs_decode_device_batch_masks,
                       hb + (p(d_o),) + z + (vp(op.ctypes.data), p(d_r)) + z + (vp(rp.ctypes.data), p(outs["d"][0])) + z
                       + (None, vp(None)), (op, rp))


def run_a():
    for c in loop:
        c()


forms = {"a_loop": run_a, "b_masks": masks, "c_shared": shared, "d_decode_masks": decode}
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
        print(f"round {r} {name}: {us[name][-1]:.1f} us")


def healed(out, o_rows, r_rows):
    """Missing rows restored, every other row of the (zeroed) outputs unwritten."""
    return (torch.equal(out[0][o_rows], full_o[o_rows]) and torch.equal(out[1][r_rows], full_r[r_rows])
            and not bool(out[0][~o_rows].any()) and not bool(out[1][~r_rows].any()))


mo0, mr0 = mo[:1].expand(B, N), mr[:1].expand(B, M)
ok = {"a_loop": healed(outs["a"], mo, mr), "b_masks": healed(outs["b"], mo, mr),
      "c_shared": healed(outs["c"], mo0, mr0),
      "d_decode_masks": torch.equal(outs["d"][0][mo], full_o[mo]) and not bool(outs["d"][0][~mo].any())}
med = {name: statistics.median(v) for name, v in us.items()}
print(f"{B} x {N}:{M} x {S} B, {k} of {N + M} shards lost per stripe: {int((op == 0).sum())} originals + "
      f"{int((rp == 0).sum())} recovery shards in all; {int(((op == 0).sum(1) == 0).sum())} stripe(s) miss no "
      f"original ({rs.version()})")
for name in forms:
    v = us[name]
    print(f"{name}: median {med[name]:.1f} us ({med[name] / B:.2f} us per stripe)  min {min(v):.1f} max {max(v):.1f} "
          f"spread {(max(v) - min(v)) / med[name] * 100:.1f} %  bytes_ok={ok[name]}")
print(f"b/a = {med['b_masks'] / med['a_loop']:.3f}   b/c = {med['b_masks'] / med['c_shared']:.3f}   "
      f"b/d = {med['b_masks'] / med['d_decode_masks']:.3f}   b < a: {med['b_masks'] < med['a_loop']}")
rs.profile_enable(True)
for name in ("b_masks", "c_shared", "d_decode_masks"):
    rs.profile_collect()
    for _ in range(5):
        forms[name]()
    torch.cuda.synchronize()
    recs = rs.profile_collect()
    print(f"{name}: {len(recs) // 5} launch(es) per call, device time "
          f"{statistics.median(ms for _, ms, _ in recs) * 1e3:.1f} us: {recs[-1][0]}")
rs.profile_enable(False)
assert all(ok.values()), ok
rs.check_device()
