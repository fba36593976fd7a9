"""examples/convect_heat.cpp: a native caller of the ConvectionIntegrator through include/ecm2_pa.h alone
-- a slab with u = x on its two x faces and a uniform flow v = (Pe, 0, 0); K = Diffusion + Convection is
the explicit operator of ecm2_ode_step_source, T = Mass + c dt Diffusion stays symmetric.  It checks
C (g . p) = (v . g) b_1 against the linear-form kernel (1e-12), that u = x is a fixed point of five
backward-Euler steps (1e-10) and that a perturbed start relaxes monotonically to <= 2% in thirty.  The GPU
run is tests/test_gpu_convection.py::test_example_convect_on_gpu's."""
import os
import subprocess

from helpers import ROOT

EXAMPLES = os.path.join(ROOT, "examples")
BINARY = os.path.join(EXAMPLES, "convect_heat")


def test_convect_example_builds_and_fails_loudly_without_gpu():
    """Compiles and links against the header + library; with no device the form's create returns
    ECM2_ERR_HIP and the program stops with status 2 (no CPU fallback), after the host setup."""
    subprocess.run(["make", "-s", "-C", EXAMPLES], check=True, timeout=300)
    assert os.access(BINARY, os.X_OK)
    import ecm2_amd as E
    if E.load_library().ecm2_device_count() > 0:
        return
    r = subprocess.run([BINARY], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, r.stdout + r.stderr
    assert "slab 8 x 4 x 4 elements" in r.stdout and "Pe = 1" in r.stdout  # host setup ran
    assert "ecm2_pa_form_create" in r.stderr and "no HIP device" in r.stderr
