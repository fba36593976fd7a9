"""CPU test of the transfer operator's host construction (csrc/transfer.cpp): builds
tests/cpp/transfer_plan_check.cpp with that source under ASan + UBSan (the library Makefile's transfer_plan_check
target, the one program that checks both kinds; the sanitizers are linked into that program only) and runs it as a
child process on three meshes: a
3 x 2 x 2 lattice, fichera.mesh's seven elements (shared faces with differing local orientations) and an
SFC-ordered 4 x 4 x 4.  The program checks the owner bits and the coarse transposed map, replays Mult and
MultTranspose from the plan, and this test compares what it prints with tests/mg_ref.py componentwise."""
import os
import subprocess

import numpy as np

import helpers  # noqa: F401
import ecm2_amd as E
import mg_cases as MC
import mg_ref as MR
from helpers import GOLDEN, ROOT

PKG = os.path.join(ROOT, "cardiac-ablation-ecm2_amd")


def _meshes():
    return [("3x2x2", MC.lattice((3, 2, 2), True), [(1, 2), (2, 3), (3, 4), (1, 4)]),
            ("fichera", E.Mesh(os.path.join(GOLDEN, "fichera.mesh")), [(1, 2), (2, 4)]),
            ("sfc 4x4x4", MC.lattice((4, 4, 4), False, sfc=True), [(1, 2), (2, 3)])]


def test_transfer_plans_replay_on_the_host(tmp_path):
    exe = os.path.join(str(tmp_path), "transfer_plan_check")
    subprocess.run(["make", "-s", "-C", PKG, f"OBJ={tmp_path}", exe], check=True, timeout=600)
    rng = np.random.default_rng(6)
    text, cases = [], []
    for name, mesh, pairs in _meshes():
        for pc, pf in pairs:
            lf, hf = E.H1Space(mesh, pc), E.H1Space(mesh, pf)
            gc, gf = lf.gather_map(), hf.gather_map()
            xc, xf = rng.uniform(-1, 1, lf.ndofs), rng.uniform(-1, 1, hf.ndofs)
            cases.append((name, pc, pf, MR.Transfer(gc, lf.ndofs, pc, gf, hf.ndofs, pf, MR.LD), xc, xf))
            text.append(f"pcase {lf.ne} {pc} {lf.ndofs} {pf} {hf.ndofs}\n" + " ".join(map(str, gc.reshape(-1))) + "\n"
                        + " ".join(map(str, gf.reshape(-1))) + "\n" + " ".join(float(v).hex() for v in xc) + "\n"
                        + " ".join(float(v).hex() for v in xf) + "\n")
    r = subprocess.run([exe], input="".join(text) + "end\n", capture_output=True, text=True, timeout=300)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "PASS" and lines[-2] == f"cases {len(cases)}"
    for k, (name, pc, pf, T, xc, xf) in enumerate(cases):
        up, down = lines[2 * k].split(), lines[2 * k + 1].split()
        assert up[0] == "mult" and down[0] == "multT"
        yf = np.array([float.fromhex(v) for v in up[1:]])
        yc = np.array([float.fromhex(v) for v in down[1:]])
        c1 = MR.HP.constant(yf, T.mult(xc), T.bound_mult(xc))
        c2 = MR.HP.constant(yc, T.mult_transpose(xf), T.bound_mult_transpose(xf))
        print(f"{name} p {pc} -> {pf}: constants {c1:.2f} (Mult), {c2:.2f} (MultTranspose)")
        assert c1 <= MR.C_XFER and c2 <= MR.C_XFER
