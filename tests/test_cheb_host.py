"""CPU tests of the Chebyshev smoother's host side: the new symbols are declared in include/ecm2_pa.h, exported
by the library and bound with their signatures; the coefficients (csrc/cheb_coeffs.hpp, the function the
smoother's constructor calls) against tests/cheb_ref.py's, in a program of its own under ASan + UBSan (the
library Makefile's cheb_coeffs_check target; the sanitizers are linked into that program only); and
examples/rf_potential.cpp builds and fails loudly without a GPU.  The GPU runs are
tests/test_gpu_chebyshev.py's and tests/test_gpu_example_rf_potential.py's."""
import inspect
import os
import subprocess

import numpy as np

import helpers  # noqa: F401
import ecm2_amd as E
import cheb_ref as CR
from helpers import ROOT

PKG = os.path.join(ROOT, "cardiac-ablation-ecm2_amd")
EXAMPLES = os.path.join(ROOT, "examples")
ARGS = {"ecm2_chebyshev_create": 8, "ecm2_chebyshev_create_power": 10, "ecm2_chebyshev_info": 5,
        "ecm2_chebyshev_mult": 4, "ecm2_smoother_destroy": 1, "ecm2_power_method": 10, "ecm2_operator_pcg_prec": 12,
        "ecm2_ode_step_prec": 15}


def test_symbols_declared_exported_and_bound():
    declared = E.declared_symbols()
    lib = E._par_lib()
    for name, nargs in ARGS.items():
        assert name in declared
        fn = getattr(lib, name)          # exported
        assert name in E._PAR_SIGS and fn.argtypes == E._PAR_SIGS[name][1]
        assert len(E._PAR_SIGS[name][1]) == nargs
    # the trailing keywords; the existing defaults and positions are unchanged
    p = inspect.signature(E.Operator.PCG).parameters
    assert list(p)[-2:] == ["stream", "prec"] and p["prec"].default is None and p["jacobi"].default is True
    p = inspect.signature(E.ode_step).parameters
    assert list(p)[-3:] == ["solver", "jacobi_of", "prec"] and p["prec"].default is None and p["solver"].default == "pcg"
    p = inspect.signature(E.ChebyshevSmoother.__init__).parameters
    assert [p[k].default for k in ("ess", "order", "max_eig_estimate", "diag_of", "power_iterations", "power_tolerance",
                                   "v0")] == [None, 2, None, None, 10, 1e-8, None]
    p = inspect.signature(E.power_method).parameters
    assert [p[k].default for k in ("ess", "diag_of", "num_steps", "tol")] == [None, None, 10, 1e-8]
    # the header cites the reference's lines at the entry points
    txt = open(E.HEADER_PATH).read()
    assert txt.count("455-658") >= 1 and txt.count("871-928") >= 3 and txt.count("538-617") >= 2
    assert txt.count("619-658") >= 2


def test_coefficients_match_the_reference_table(tmp_path):
    exe = os.path.join(str(tmp_path), "cheb_coeffs_check")
    subprocess.run(["make", "-s", "-C", PKG, f"OBJ={tmp_path}", exe], check=True, timeout=600)
    lams = [10.0 ** e for e in range(-6, 7)] + [0.02, 1.3, 57.0, 1.6742056277]
    cases = [(o, lam) for o in CR.ORDERS_ALL for lam in lams] + [(0, 1.0), (6, 1.0), (-1, 1.0)]
    text = "".join(f"{o} {float(lam).hex()}\n" for o, lam in cases)
    r = subprocess.run([exe], input=text + "end\n", capture_output=True, text=True, timeout=300)
    print(r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")
    worst = 0.0
    for (o, lam), line in zip(cases, lines):
        f = line.split()
        rc, got = int(f[0]), np.array([float.fromhex(v) for v in f[1:]])
        if not 1 <= o <= 5:
            assert rc == 1          # ECM2_ERR_ARG
            continue
        want = CR.coefficients(o, lam)
        assert rc == 0 and not got[o:].any()
        # (pow against ** may differ in the last bit)
        worst = max(worst, float(np.abs(got[:o] / want - 1.0).max()))
    print(f"worst relative difference {worst:.2e}")
    assert worst <= 1e-15
    assert lines[len(cases)] == f"cases {len(cases)}"


def test_rf_potential_example_builds_and_fails_loudly_without_gpu():
    """Compiles and links against the header + library; with no device the form's create returns
    ECM2_ERR_HIP and the program stops with status 2 (no CPU fallback), after the host setup."""
    subprocess.run(["make", "-s", "-C", EXAMPLES], check=True, timeout=300)
    binary = os.path.join(EXAMPLES, "rf_potential")
    assert os.access(binary, os.X_OK)
    if E.load_library().ecm2_device_count() > 0:
        return
    r = subprocess.run([binary], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, r.stdout + r.stderr
    assert "unit cube 8^3 elements" in r.stdout and "1538 essential" in r.stdout  # host setup ran
    assert "ecm2_pa_form_create" in r.stderr and "no HIP device" in r.stderr
