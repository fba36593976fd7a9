"""CPU test of the merge-flag condition the snapshot kernel's lattice epilogue rests on
(csrc/scatter_plan.hpp tpe_lane_flags_in_row): builds tests/cpp/lane_flag_check.cpp with the host-only
planning sources under ASan + UBSan (the library Makefile's lane_flag_check target) and runs it as a
child process.  The program checks, on the plans of the meshes of test_gpu_ts_epilogue_bitwise.py in
both numberings and of a z-slab rank's local form, that every lattice block's in-wave x / y receive
bits stay inside the receiver's 16-lane DPP row, and that a block with such a bit outside it is not
classed a lattice block; it prints PASS.  The sanitizers are linked into that program only."""
import os
import subprocess

from helpers import ROOT

PKG = os.path.join(ROOT, "cardiac-ablation-ecm2_amd")


def test_lattice_blocks_keep_their_links_inside_a_dpp_row(tmp_path):
    exe = os.path.join(str(tmp_path), "lane_flag_check")
    subprocess.run(["make", "-s", "-C", PKG, f"OBJ={tmp_path}", exe], check=True, timeout=600)
    env = {k: v for k, v in os.environ.items() if k not in ("ECM2_RUN_ORDER", "ECM2_PLAN_DUMP")}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "PASS"
