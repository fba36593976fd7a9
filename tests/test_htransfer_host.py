"""CPU test of the h-refinement transfer operator's host construction (csrc/transfer.cpp, build_htransfer_plan): builds
tests/cpp/transfer_plan_check.cpp with that source, fe.cpp and mesh.cpp under ASan + UBSan (the library Makefile's
transfer_plan_check target; the sanitizers are linked into that program only) and runs it as a child process on
the smaller transfer cases of tests/hmg_cases.py and on one embedding that is a permutation of the fine elements.
The program checks the owner bits, the children table, the tables and the coarse transposed map, replays Mult and
MultTranspose from the plan in the device's order and checks every refusal of the plan builder; this test compares
what it prints with the 80-bit evaluation of tests/hmg_ref.py componentwise under C_HXFER."""
import os
import subprocess

import numpy as np

import helpers  # noqa: F401
import hmg_cases as HC
import hmg_ref as HR
import hp_ref as HP
from helpers import ROOT

PKG = os.path.join(ROOT, "cardiac-ablation-ecm2_amd")
CASES = [("moved322", 1), ("moved322", 2), ("moved322", 3), ("moved322", 4), ("fichera", 1), ("fichera", 2),
         ("fichera1", 1), ("sfc4", 1), ("struct433", 2)]


def _ints(a):
    return " ".join(map(str, np.asarray(a).reshape(-1)))


def _hex(a):
    return " ".join(float(v).hex() for v in a)


def test_htransfer_plans_replay_on_the_host(tmp_path):
    exe = os.path.join(str(tmp_path), "transfer_plan_check")
    subprocess.run(["make", "-s", "-C", PKG, f"OBJ={tmp_path}", exe], check=True, timeout=600)
    text, cases = [], []
    for name, p in CASES:
        P = HC.pair(name, p)
        xc, xf = P.inputs["random"]
        cases.append((name, p, P.ref(HR.LD), xc, xf))
        text.append(f"hcase {p} {P.lf.ne} {P.lf.ndofs} {P.hf.ne} {P.hf.ndofs}\n" + _ints(P.lf.gather_map()) + "\n"
                    + _ints(P.hf.gather_map()) + "\n" + _ints(P.parent) + "\n" + _ints(P.octant) + "\n" + _hex(xc) + "\n"
                    + _hex(xf) + "\n")
    # the fine elements permuted: the embedding is no longer (e / 8, corner e % 8), the owners change with it
    P = HC.pair("moved322", 2)
    perm = np.random.default_rng(5).permutation(P.hf.ne)
    gf, parent, octant = P.hf.gather_map()[perm], P.parent[perm], P.octant[perm]
    xc, xf = P.inputs["random"]
    cases.append(("moved322 permuted", 2, P.ref(HR.LD, gf, parent, octant), xc, xf))
    text.append(f"hcase 2 {P.lf.ne} {P.lf.ndofs} {P.hf.ne} {P.hf.ndofs}\n" + _ints(P.lf.gather_map()) + "\n" + _ints(gf) + "\n"
                + _ints(parent) + "\n" + _ints(octant) + "\n" + _hex(xc) + "\n" + _hex(xf) + "\n")
    r = subprocess.run([exe], input="".join(text) + "end\n", capture_output=True, text=True, timeout=300)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "PASS" and lines[-2] == f"cases {len(cases)}"
    for k, (name, p, T, xc, xf) in enumerate(cases):
        up, down = lines[2 * k].split(), lines[2 * k + 1].split()
        assert up[0] == "mult" and down[0] == "multT"
        yf = np.array([float.fromhex(v) for v in up[1:]])
        yc = np.array([float.fromhex(v) for v in down[1:]])
        c1 = HP.constant(yf, T.mult(xc), T.bound_mult(xc))
        c2 = HP.constant(yc, T.mult_transpose(xf), T.bound_mult_transpose(xf))
        print(f"{name} p {p}: constants {c1:.2f} (Mult), {c2:.2f} (MultTranspose)")
        assert c1 <= HR.C_HXFER and c2 <= HR.C_HXFER
