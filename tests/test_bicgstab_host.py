"""CPU tests of the device BiCGSTAB's host side: the new symbols are declared in include/ecm2_pa.h, exported
by the library and bound with their signatures; the loop's stopping decision (csrc/bicgstab_stop.hpp, the
function the device's final-pass kernels call) against the table tests/bicgstab_ref.py's stop_decision
produces, in a program of its own under ASan + UBSan (the library Makefile's bicgstab_stop_check target; the
sanitizers are linked into that program only); and examples/implicit_convect_heat.cpp builds and fails
loudly without a GPU.  The GPU runs are tests/test_gpu_bicgstab.py's and tests/test_gpu_ode_bicgstab.py's."""
import inspect
import itertools
import os
import subprocess

import helpers  # noqa: F401
import ecm2_amd as E
import bicgstab_ref as BR
from helpers import ROOT

PKG = os.path.join(ROOT, "cardiac-ablation-ecm2_amd")
EXAMPLES = os.path.join(ROOT, "examples")
SYMBOLS = ["ecm2_operator_bicgstab", "ecm2_bicgstab_last_converged", "ecm2_ode_step_bicgstab"]


def test_symbols_declared_exported_and_bound():
    declared = E.declared_symbols()
    lib = E._par_lib()
    for name in SYMBOLS:
        assert name in declared
        fn = getattr(lib, name)          # exported
        assert name in E._PAR_SIGS and fn.argtypes == E._PAR_SIGS[name][1]
    assert len(E._PAR_SIGS["ecm2_operator_bicgstab"][1]) == 12
    assert len(E._PAR_SIGS["ecm2_ode_step_bicgstab"][1]) == 15
    assert E.bicgstab_last_converged() in (False, True)
    p = inspect.signature(E.Operator.BiCGSTAB).parameters
    assert [p[k].default for k in ("ess", "rel_tol", "abs_tol", "max_iter", "jacobi_of")] == [None, 1e-12, 0.0, 1000, None]
    p = inspect.signature(E.ode_step).parameters
    assert p["solver"].default == "pcg" and p["jacobi_of"].default is None
    # the header cites the reference's lines at each entry point
    txt = open(E.HEADER_PATH).read()
    assert txt.count("1579-1805") >= 3


def _stop_cases():
    inf, nan = float("inf"), float("nan")
    values = [0.0, -0.0, 5e-324, 0.5e-3, 1e-3, 1.0000000000000002e-3, 1.0, -1.0, 1e308, inf, -inf, nan]
    tols = [0.0, 1e-3, inf]
    its = [(1, 1), (1, 2), (4, 5), (5, 5), (6, 5), (1, 0)]
    return [(t, v, tol, it, mx) for t in range(5) for v, tol, (it, mx) in itertools.product(values, tols, its)]


def test_stop_decision_matches_the_reference_table(tmp_path):
    exe = os.path.join(str(tmp_path), "bicgstab_stop_check")
    subprocess.run(["make", "-s", "-C", PKG, f"OBJ={tmp_path}", exe], check=True, timeout=600)
    cases = _stop_cases()
    text = "".join(f"{t} {float(v).hex() if v == v and abs(v) != float('inf') else v} "
                   f"{float(tol).hex() if abs(tol) != float('inf') else tol} {it} {mx}\n" for t, v, tol, it, mx in cases)
    r = subprocess.run([exe], input=text + "end\n", capture_output=True, text=True, timeout=300)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")
    got = [int(s) for s in lines[:len(cases)]]
    want = [BR.stop_decision(*c) for c in cases]
    bad = [(c, g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not bad, bad[:5]
    # every status is reached by the table
    assert set(want) == {BR.RUNNING, BR.CONVERGED, BR.CONVERGED_S, BR.MAX_ITER, BR.RHO_ZERO, BR.OMEGA_ZERO, BR.NONFINITE}
    # the tests of one iteration in the kernels' order: (status, final_iter, converged)
    runs = [tuple(int(t) for t in s.split()[1:]) for s in lines if s.startswith("run ")]
    assert runs == [(BR.RUNNING, 1, 0), (BR.CONVERGED_S, 2, 1), (BR.CONVERGED, 3, 1), (BR.CONVERGED, 3, 1),
                    (BR.OMEGA_ZERO, 4, 0), (BR.MAX_ITER, 5, 0), (BR.RHO_ZERO, 6, 0), (BR.NONFINITE, 6, 0),
                    (BR.NONFINITE, 6, 0), (BR.NONFINITE, 6, 0), (BR.RUNNING, 7, 0)]
    assert lines[-2 if lines[-1] == "" else -1] == f"cases {len(cases)}"


def test_implicit_convect_example_builds_and_fails_loudly_without_gpu():
    """Compiles and links against the header + library; with no device the form's create returns
    ECM2_ERR_HIP and the program stops with status 2 (no CPU fallback), after the host setup."""
    subprocess.run(["make", "-s", "-C", EXAMPLES], check=True, timeout=300)
    binary = os.path.join(EXAMPLES, "implicit_convect_heat")
    assert os.access(binary, os.X_OK)
    if E.load_library().ecm2_device_count() > 0:
        return
    r = subprocess.run([binary], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, r.stdout + r.stderr
    assert "slab 8 x 2 x 2 elements" in r.stdout and "Pe = 10" in r.stdout  # host setup ran
    assert "ecm2_pa_form_create" in r.stderr and "no HIP device" in r.stderr
