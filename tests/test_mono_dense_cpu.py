"""The host's condition for the column kernel's dense encode entry (csrc/rs_mono_dense.hpp
mono_dense_ok; rs_mono.hip launch_ls applies it): it holds at N = M = 2^L with shards of
whole 64-byte blocks and aligned matrices, and fails for a 66-byte shard, a base off by 2,
a narrowed recovery span, N < 2^L (there is no prefix form), two source maps, unaligned
strides and strides past the 32-bit lane offsets' bound.  tests/mono_dense_check.cpp is
compiled here with the build's compiler as a host-only unit and run.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_dense_condition(tmp_path):
    exe = str(tmp_path / "mono_dense_check")
    src = os.path.join(ROOT, "tests", "mono_dense_check.cpp")
    inc = os.path.join(ROOT, "reed-solomon-simd_amd", "csrc")
    c = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", inc, src, "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mono dense ok" in r.stdout, (r.returncode, r.stdout[-4000:], r.stderr[-2000:])


def test_dense_headline_listing(tmp_path_factory):
    """What the dense form is for, read from the built code object: in k_mono_dense<10, 1, 0, false, 2>
    no argument load after the preload prologue's, the four row loads as dword loads with a scalar
    base, four 16-bit stores, no byte-wise access, and fewer selects and branches than the general
    entry's kernel has."""
    import test_isa as ISA
    kernels = ISA._disassemble(tmp_path_factory)
    dense = next((k for k in kernels if "k_mono_denseILi10ELi1ELi0ELb0ELi2E" in k), None)
    general = next((k for k in kernels if "6k_monoILi10ELi1ELi0ELb1ELb0ELb0ELi2E" in k), None)
    assert dense and general, sorted(k for k in kernels if "k_mono" in k)[:8]
    d = [ins for _, ins, _ in kernels[dense]]
    g = [ins for _, ins, _ in kernels[general]]
    first_other = next(i for i, ins in enumerate(d) if not ins.startswith("s_load"))
    assert not any(ins.startswith("s_load") for ins in d[first_other + 1:]), "argument load after the prologue"
    assert first_other == 3, d[:6]  # the loading prologue for firmware that does not preload
    loads = [ins for ins in d if ins.startswith("global_load") and "lds" not in ins]
    assert len(loads) == 4 and all(re.match(r"global_load_dword v\d+, v\d+, s\[\d+:\d+\]", ins) for ins in loads), loads
    stores = [ins for ins in d if ins.startswith("global_store")]
    assert len(stores) == 4 and all(ins.startswith("global_store_short ") for ins in stores), stores
    assert not any(re.match(r"global_(load_ubyte|store_byte)", ins) for ins in d)

    def count(body, prefix):
        return sum(ins.startswith(prefix) for ins in body)

    assert count(d, "v_") <= count(g, "v_") - 100, (count(d, "v_"), count(g, "v_"))
    assert count(d, "v_cndmask") < count(g, "v_cndmask") and count(d, "s_cbranch") < count(g, "s_cbranch")


def test_switch_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "rs_mi355x.h")).read()
    assert re.search(r"uint64_t\s+rs_mono_dense_launches\s*\(\s*void\s*\)", header)
    assert "RS_MI355X_DENSE" in header and "8192" in header and "16384" in header
    import reed_solomon_simd as rs
    assert rs.mono_dense_launches() >= 0
