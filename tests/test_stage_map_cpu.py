"""The slot maps of the column kernel's staged tables (csrc/rs_stage_map.hpp): the
forward maps (which LDS position an image piece goes to) and the inverse maps the
LDS-DMA fill puts on its source addresses.  tests/stage_map_check.cpp walks every
region of the staged encodes the way the kernel issues the fill; it is compiled here
with the build's compiler as a host-only unit and run.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_stage_maps_round_trip(tmp_path):
    exe = str(tmp_path / "stage_map_check")
    src = os.path.join(ROOT, "tests", "stage_map_check.cpp")
    inc = os.path.join(ROOT, "reed-solomon-simd_amd", "csrc")
    c = subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", inc, src, "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "stage map ok" in r.stdout, (r.returncode, r.stdout[-4000:], r.stderr[-2000:])
