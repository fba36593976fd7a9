"""CPU pins of tests/conv_ref.py, the numpy checker of the convection kernels, on the 5 x 4 x 3 mesh with
every vertex moved (non-affine hexes) and on fichera refined once: the sum-factorised PA path against the
independent dense element matrices (Mult and MultTranspose), C 1 = 0, the duality <w, C x> = <C^T w, x>,
the linear-field identity C (g . p) = alpha (v . g) M_1 1 against the oracle's unit mass, and the helper's
own float64 error against its np.longdouble restatement (it has to stay far below the GPU tests' 1e-12 bar).

Bounds: each quantity is a sum of at most (Q^3 + D^3 + 8) products per entry and per stage, rounded at
2^-53 = 1.1e-16; two different summation orders of the same sums differ by a few hundred units of that
against the largest entry, so 1e-13 relative (inf-norm) separates rounding from any wrong formula, whose
error is O(1)."""
import numpy as np
import pytest

import ecm2_amd as E
import oracle as O
import bdr_ref as BR
import conv_ref as R
from helpers import relerr

TOL = 1e-13
ALPHA = 1.7
VCONST = np.array([0.8, -0.3, 0.5])
G = np.array([0.4, -1.1, 0.7])

_CACHE = {}


def setup(name, p, q1d, dtype=np.float64):
    key = (name, p, q1d, dtype)
    if key not in _CACHE:
        mesh = BR.MESHES[name](E)
        fes = E.H1Space(mesh, p, E.NUMBERING_ENTITY)
        ref = R.ConvRef(p, q1d, fes.gather_map(), fes.ndofs, mesh.element_nodes(), dtype=dtype)
        rng = np.random.default_rng(5)
        _CACHE[key] = dict(mesh=mesh, fes=fes, ref=ref, x=rng.uniform(0.0, 1.0, fes.ndofs),
                           w=rng.uniform(0.0, 1.0, fes.ndofs), X=fes.dof_coords())
    return _CACHE[key]


def velocities(ref):
    return {"const": VCONST, "points": R.reference_velocity(ref.P.astype(np.float64))}


CASES = [(n, p, dq) for n in ("perturbed", "fichera") for p in (1, 2, 3, 4) for dq in (1, 2)]


@pytest.mark.parametrize("name,p,dq", CASES)
def test_pa_equals_full_assembly(name, p, dq):
    """The reference's own PA-vs-FA test (test_pa_kernels.cpp:498-578): Mult and MultTranspose."""
    s = setup(name, p, p + dq)
    ref = s["ref"]
    for vname, v in velocities(ref).items():
        for tr in (False, True):
            y_pa = ref.mult(v, s["x"], ALPHA, transpose=tr)
            y_fa = ref.fa_mult(v, s["x"], ALPHA, transpose=tr)
            err = relerr(y_pa, y_fa)
            print(f"{name} p={p} q1d={p + dq} {vname} transpose={tr}: PA vs FA {err:.2e}")
            assert np.abs(y_fa).max() > 1e-3 and err < TOL


@pytest.mark.parametrize("name,p,dq", CASES)
def test_constants_duality_and_linear_fields(name, p, dq):
    s = setup(name, p, p + dq)
    ref, x, w = s["ref"], s["x"], s["w"]
    one = np.ones(ref.ndofs)
    for vname, v in velocities(ref).items():
        y = ref.mult(v, x, ALPHA)
        scale = np.abs(y).max()
        # C 1 = 0: the gradient of a constant vanishes at every point
        assert np.abs(ref.mult(v, one, ALPHA)).max() < TOL * scale
        # <w, C x> = <C^T w, x>, against the sum of the magnitudes the first product adds up
        yt = ref.mult(v, w, ALPHA, transpose=True)
        assert abs(w @ y - yt @ x) < TOL * (np.abs(w) @ np.abs(y))
    # C (g . p) = alpha (v . g) M_1 1 for a constant v: the quadrature sums agree term by term
    # (adj(J) v . J^T g = det J (v . g)); M_1 1 from the oracle's unit mass
    op = O.OracleOperator(s["mesh"].element_nodes(), s["fes"].gather_map(), ref.ndofs, p, alpha=1.0, beta=None,
                          q1d=p + dq)
    m1 = op.mult(one)
    lhs = ref.mult(VCONST, s["X"] @ G, ALPHA)
    rhs = ALPHA * (VCONST @ G) * m1
    assert relerr(lhs, rhs) < TOL
    assert relerr(ref.unit_load(), m1) < TOL


def test_markers_zero_the_excluded_elements():
    s = setup("perturbed", 2, 4)
    ref = s["ref"]
    attr = 1 + (np.arange(ref.ne) % 3)
    keep = R.marker_keep(attr, [0, 1, 0])
    assert 0 < keep.sum() < ref.ne
    pa = ref.pa_data(VCONST, ALPHA, keep)
    assert np.all(pa[~keep] == 0.0) and np.all(np.abs(pa[keep]).max(axis=(1, 2)) > 0)
    y = ref.mult(VCONST, s["x"], ALPHA, keep)
    ye = ref.apply(ref.pa_data(VCONST, ALPHA), ref.gather(s["x"]))
    ye[~keep] = 0.0                                   # AddMultWithMarkers: the rows of excluded elements
    assert relerr(y, ref.scatter_add(ye)) < 1e-15
    assert R.marker_keep(attr, None).all()


@pytest.mark.parametrize("name,p,dq", [("perturbed", 1, 2), ("perturbed", 2, 2), ("fichera", 3, 1), ("perturbed", 4, 2)])
def test_float64_helper_against_longdouble(name, p, dq):
    """The float64 checker's own distance from the extended-precision restatement (80-bit on x86): the
    GPU tests' 1e-12 bar has to sit well above it.  Where longdouble is no wider than double the figure
    is 0 and says nothing; it is printed either way."""
    s = setup(name, p, p + dq)
    hi = setup(name, p, p + dq, np.longdouble)["ref"]
    worst = 0.0
    for vname, v in velocities(s["ref"]).items():
        for tr in (False, True):
            e = relerr(s["ref"].mult(v, s["x"], ALPHA, transpose=tr), hi.mult(v, s["x"], ALPHA, transpose=tr))
            worst = max(worst, e)
        worst = max(worst, relerr(s["ref"].pa_data(v, ALPHA), hi.pa_data(v, ALPHA)))
    print(f"{name} p={p} q1d={p + dq}: float64 checker vs longdouble {worst:.2e} "
          f"(longdouble eps {np.finfo(np.longdouble).eps:.1e}); the GPU bar is 1e-12")
    assert worst < 1e-14
