"""CPU test of the fused kernels' scatter planning (csrc/scatter_plan.cpp): builds
tests/cpp/plan_check.cpp with the host-only planning sources under ASan + UBSan (the library
Makefile's plan_check target) and runs it as a child process.  The program replays every plan on
the host in integers and prints PASS; the sanitizers are linked into that program only."""
import os
import subprocess

from helpers import GOLDEN, ROOT

PKG = os.path.join(ROOT, "cardiac-ablation-ecm2_amd")


def test_scatter_plans_replay_on_the_host(tmp_path):
    exe = os.path.join(str(tmp_path), "plan_check")
    subprocess.run(["make", "-s", "-C", PKG, f"OBJ={tmp_path}", exe], check=True, timeout=600)
    env = {k: v for k, v in os.environ.items() if k not in ("ECM2_RUN_ORDER", "ECM2_PLAN_DUMP")}
    r = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "PASS"
