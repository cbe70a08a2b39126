"""The split encode's plan, images, fills and table reads (csrc/rs_mono_plan.hpp Plan's
pair kind, csrc/rs_stage_map.hpp SplitImage).  tests/split_plan_check.cpp walks them and
runs the whole kernel for one column pack on the host, lane by lane, against the plain
transform; it is compiled here with the build's compiler as a host-only program and run.
No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_split_plan_maps_and_host_run(tmp_path):
    exe = str(tmp_path / "split_plan_check")
    inc = os.path.join(ROOT, "reed-solomon-simd_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "split_plan_check.cpp"), os.path.join(inc, "gf_tables.cpp")]
    # (gf_tables.cpp is built the way the library builds it: it includes the HIP runtime's
    # header for its declarations and calls nothing of it; --offload-host-only: no device pass)
    c = subprocess.run([HIPCC, "--offload-host-only", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", inc, "-x", "c++",
                        srcs[0], "-x", "hip", srcs[1], "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "split plan ok" in r.stdout, (r.returncode, r.stdout[-4000:], r.stderr[-2000:])
