"""The split encode's arithmetic (csrc/rs_gf.hpp gf_half_mul, csrc/rs_mono.hip
split_layer0): a 4-element multiply as the two byte planes' half multiplies on a lane
pair.  tests/split_mul_check.cpp writes the device functions out in plain C++ with
v_perm_b32 emulated and checks them against csrc/gf_tables.cpp's tables and the field
product; it is compiled here with the build's compiler as a host-only program and run.
No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_half_multiplies_combine_to_the_whole(tmp_path):
    exe = str(tmp_path / "split_mul_check")
    inc = os.path.join(ROOT, "reed-solomon-simd_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "split_mul_check.cpp"), os.path.join(inc, "gf_tables.cpp")]
    # (gf_tables.cpp is built the way the library builds it: it includes the HIP runtime's
    # header for its declarations and calls nothing of it; --offload-host-only: no device pass)
    c = subprocess.run([HIPCC, "--offload-host-only", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", inc, "-x", "c++",
                        srcs[0], "-x", "hip", srcs[1], "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "split mul ok" in r.stdout, (r.returncode, r.stdout[-4000:], r.stderr[-2000:])
