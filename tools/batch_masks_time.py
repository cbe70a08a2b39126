"""Time the batch decode with a pattern per stripe against its alternatives (development aid):

    python tools/batch_masks_time.py [stripes N M S [loss]]      default 64 1024 1024 1024 0.01

Method of tools/dec_time.py: warm-up, `iters` back-to-back calls, one synchronize, host clock;
here for three forms in one process, in alternating rounds, every call pre-bound (DeviceCall:
what a C caller of the ABI pays).  Every stripe has its own random pattern of `loss` x N lost
originals and as many received recovery shards.
  (a) loop:   one rs_decode_device_strided call per stripe, each with its pattern (what a caller
              had to do before rs_decode_device_batch_masks existed)
  (b) masks:  one rs_decode_device_batch_masks call
  (c) shared: one rs_decode_device_batch call, stripe 0's pattern for every stripe: the ceiling
              (the same work without the descriptor copy and the per-pattern host work, and with
              the split plan and the narrowed destination map where they apply)
  (d) shared, split plan off (rs_mono_enable + 4): (c) on the plan (b) uses, to tell the plan's share
              of b - c from the descriptor copy's
Prints one line per round and form (us per batch), then the medians, the spread of each form's
rounds, b/a and b/c, and restored_ok per form; last, the device time of one launch of (b), (c) and
(d) by the library's events (rs_profile_collect): what is left of a form's time is launch, copy and
host work.  A shape off the fused route (more than 2^11 work
rows) shows what the fallback costs: (b) runs the loop inside the library.
"""
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reed-solomon-simd_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import reed_solomon_simd as rs  # noqa: E402

args = sys.argv[1:]
B, N, M, S = (int(a) for a in args[:4]) if len(args) >= 4 else (64, 1024, 1024, 1024)
loss = float(args[4]) if len(args) > 4 else 0.01
rounds, iters = 7, 100

rng = np.random.default_rng(1)
g = torch.Generator(device="cuda")
g.manual_seed(1)
d_orig = torch.randint(0, 256, (B, N, S), dtype=torch.uint8, device="cuda", generator=g)
d_rec = torch.empty((B, M, S), dtype=torch.uint8, device="cuda")
rs.encode_device_batch(N, M, S, d_orig, d_rec)
k = max(1, round(min(N, M) * loss))
op = np.ones((B, N), np.uint8)
rp = np.zeros((B, M), np.uint8)
for b in range(B):
    op[b, rng.choice(N, k, replace=False)] = 0
    rp[b, rng.choice(M, k, replace=False)] = 1
outs = {f: torch.zeros_like(d_orig) for f in "abc"}
ctx = rs.default_context()
u, vp = ctypes.c_uint64, ctypes.c_void_p
head = (vp(ctx.handle.value), ctypes.c_int(0), u(N), u(M), u(S), u(B))

loop = [rs.decode_device_call(N, M, S, d_orig[b], op[b], d_rec[b], rp[b], outs["a"][b]) for b in range(B)]
masks = rs.DeviceCall(rs._lib.rs_decode_device_batch_masks,
                      head + (vp(d_orig.data_ptr()), u(0), u(0), vp(op.ctypes.data), vp(d_rec.data_ptr()), u(0), u(0),
                              vp(rp.ctypes.data), vp(outs["b"].data_ptr()), u(0), u(0), None, vp(None)), (op, rp))
shared = rs.DeviceCall(rs._lib.rs_decode_device_batch,
                       head + (vp(d_orig.data_ptr()), u(0), u(0), op[0].tobytes(), vp(d_rec.data_ptr()), u(0), u(0),
                               rp[0].tobytes(), vp(outs["c"].data_ptr()), u(0), u(0), vp(None)), ())


def run_a():
    for c in loop:
        c()


def run_d():
    shared()


forms = {"a_loop": run_a, "b_masks": masks, "c_shared": shared, "d_shared_plain": run_d}
for f in forms.values():
    for _ in range(3):
        f()
torch.cuda.synchronize()
us = {name: [] for name in forms}
for r in range(rounds):
    for name, f in forms.items():
        rs.mono_enable(1 + 4 if f is run_d else 1)
        t0 = time.perf_counter()
        for _ in range(iters):
            f()
        torch.cuda.synchronize()
        us[name].append((time.perf_counter() - t0) / iters * 1e6)
        rs.mono_enable(1)
        print(f"round {r} {name}: {us[name][-1]:.1f} us")

miss = torch.from_numpy(op == 0).cuda()
ok = {"a_loop": torch.equal(outs["a"][miss], d_orig[miss]), "b_masks": torch.equal(outs["b"][miss], d_orig[miss]),
      "c_shared": torch.equal(outs["c"][:, op[0] == 0], d_orig[:, op[0] == 0])}
ok["d_shared_plain"] = ok["c_shared"]
med = {name: statistics.median(v) for name, v in us.items()}
gib = B * (N + M) * S / 2**30  # original + recovery, as bench.py counts
print(f"{B} x {N}:{M} x {S} B, {k} lost originals per stripe ({rs.version()})")
for name in forms:
    v = us[name]
    print(f"{name}: median {med[name]:.1f} us ({gib / (med[name] * 1e-6):.0f} GiB/s)  "
          f"min {min(v):.1f} max {max(v):.1f} spread {(max(v) - min(v)) / med[name] * 100:.1f} %  "
          f"restored_ok={ok[name]}")
print(f"b/a = {med['b_masks'] / med['a_loop']:.3f}   b/c = {med['b_masks'] / med['c_shared']:.3f}   "
      f"b/d = {med['b_masks'] / med['d_shared_plain']:.3f}")
rs.profile_enable(True)
for name in ("b_masks", "c_shared", "d_shared_plain"):
    rs.mono_enable(1 + 4 if name == "d_shared_plain" else 1)
    rs.profile_collect()
    for _ in range(5):
        forms[name]()
    torch.cuda.synchronize()
    recs = rs.profile_collect()
    print(f"{name}: {len(recs) // 5} launch(es) per call, device time "
          f"{statistics.median(ms for _, ms, _ in recs) * 1e3:.1f} us: {recs[-1][0]}")
rs.mono_enable(1)
rs.profile_enable(False)
