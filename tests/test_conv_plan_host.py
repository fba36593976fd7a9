"""CPU test of the convection term's planning (csrc/conv_plan.cpp): builds tests/cpp/conv_plan_check.cpp
with the host-only planning source under ASan + UBSan (the library Makefile's conv_plan_check target) and
runs it as a child process.  The program checks every plan (active list, kernel-layout map, add-pass CSR:
coverage, order, signs, bounds, holder counts) for markers that select nothing, everything, a z slab and
stripes, and prints PASS; the sanitizers are linked into that program only."""
import os
import subprocess

from helpers import GOLDEN, ROOT

PKG = os.path.join(ROOT, "cardiac-ablation-ecm2_amd")


def test_convection_plans_check_on_the_host(tmp_path):
    exe = os.path.join(str(tmp_path), "conv_plan_check")
    subprocess.run(["make", "-s", "-C", PKG, f"OBJ={tmp_path}", exe], check=True, timeout=600)
    r = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "PASS"
