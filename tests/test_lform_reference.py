"""CPU pins of tests/lform_ref.py (the numpy restatement of DLFEvalAssemble3D + the source
coefficients that the GPU linear form is compared with), so that comparison means something:
identities against the oracle's mass operator, the exactness of a linear potential's gradient on a
non-affine mesh, the total source, and the helper's own float64 error against an extended-precision
restatement of the same formulas."""
import numpy as np
import pytest

import helpers  # noqa: F401
import ecm2_amd as E
import oracle as O
import lform_ref as R
from helpers import RTOL, relerr


def _space(name, p):
    m = R.MESHES[name](E)
    fes = E.H1Space(m, p, E.NUMBERING_ENTITY)
    return m, fes


def _ref(m, fes, p, q1d, dtype=np.float64):
    return R.LFRef(p, q1d, fes.gather_map(), fes.ndofs, enodes=m.element_nodes(), dtype=dtype)


def _mass(m, fes, p, q1d):
    return O.OracleOperator(m.element_nodes(), fes.gather_map(), fes.ndofs, p, alpha=1.0, beta=None, q1d=q1d)


@pytest.mark.parametrize("name", ["perturbed", "fichera"])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("dq", [1, 2])
def test_unit_source_is_mass_times_one(name, p, dq):
    """f = 1: b = M 1 of the oracle's mass operator at the same rule."""
    m, fes = _space(name, p)
    ref = _ref(m, fes, p, p + dq)
    b = ref.assemble([({"kind": "constant", "value": 1.0}, None)])
    assert relerr(b, _mass(m, fes, p, p + dq).mult(np.ones(fes.ndofs))) < RTOL


@pytest.mark.parametrize("name", ["perturbed", "fichera"])
@pytest.mark.parametrize("p", [1, 2, 3])
def test_field_source_is_mass_times_field(name, p):
    """f = g in V_h (GridFunctionCoefficient) at Q1D = p + 2: b = M g."""
    m, fes = _space(name, p)
    g = np.random.default_rng(2).uniform(0.5, 1.5, fes.ndofs)
    ref = _ref(m, fes, p, p + 2)
    b = ref.assemble([({"kind": "gridfunc", "field": g}, None)])
    assert relerr(b, _mass(m, fes, p, p + 2).mult(g)) < RTOL


@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("dq", [1, 2])
def test_linear_potential_on_nonaffine_mesh(p, dq):
    """phi = a . x on the perturbed mesh: the trilinear isoparametric map reproduces linear functions,
    so grad phi = a at every point and b = sigma |a|^2 (M 1): pins J^-T."""
    m, fes = _space("perturbed", p)
    a = np.array([1.5, -0.7, 0.4])
    phi = fes.dof_coords() @ a
    ref = _ref(m, fes, p, p + dq)
    b = ref.assemble([({"kind": "joule", "phi": phi, "sigma": 0.6, "slope": 0.0, "t_ref": 0.0, "T": None}, None)])
    want = 0.6 * (a @ a) * _mass(m, fes, p, p + dq).mult(np.ones(fes.ndofs))
    assert relerr(b, want) < RTOL


@pytest.mark.parametrize("kind", R.KINDS)
def test_total_source(kind):
    """1^T b = sum_q W det J f (partition of unity)."""
    p, q1d = 2, 3
    m, fes = _space("perturbed", p)
    ref = _ref(m, fes, p, q1d)
    src = R.make_source(kind, fes.dof_coords(), O.quad_points(m.element_nodes(), q1d))
    b = ref.assemble([(src, None)])
    total = float(np.sum(ref.W[None, :] * ref.detJ * ref.point_values(src)))
    assert abs(b.sum() - total) < RTOL * abs(total)


def test_markers_and_order():
    """An excluded element contributes nothing; integrators add in order."""
    p, q1d = 2, 3
    m, fes = _space("perturbed", p)
    ref = _ref(m, fes, p, q1d)
    X, P = fes.dof_coords(), O.quad_points(m.element_nodes(), q1d)
    keep = R.marker_keep(m.GetAttributes(), [0, 1])
    assert 0 < keep.sum() < fes.ne
    s1, s2 = R.make_source("joule_T", X, P), R.make_source("affine", X, P)
    b = ref.assemble([(s1, keep), (s2, None)])
    f1 = ref.point_values(s1) * keep[:, None]
    want = ref.reduce(ref.element_vectors(f1)) + ref.reduce(ref.element_vectors(ref.point_values(s2)))
    assert relerr(b, want) < 1e-15


@pytest.mark.parametrize("name,p,dq", R.CASES)
def test_float64_helper_against_extended_precision(name, p, dq):
    """The float64 helper agrees with the np.longdouble restatement of the same formulas to better
    than 1e-13 on the meshes and sources of the GPU tests (the GPU bar is 1e-12)."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is float64 on this platform")
    m, fes = _space(name, p)
    q1d = p + dq
    r64, rld = _ref(m, fes, p, q1d), _ref(m, fes, p, q1d, dtype=np.longdouble)
    X, P = fes.dof_coords(), O.quad_points(m.element_nodes(), q1d)
    for kind in R.KINDS:
        src = R.make_source(kind, X, P)
        be64 = r64.element_vectors(r64.point_values(src))
        beld = rld.element_vectors(rld.point_values(src))
        err = float(np.abs(be64 - beld).max() / np.abs(beld).max())
        b_err = relerr(r64.assemble([(src, None)]), rld.assemble([(src, None)]).astype(np.float64))
        print(f"{name} p={p} q1d={q1d} {kind}: element vectors {err:.2e}, b {b_err:.2e}")
        assert err < 1e-13 and b_err < 1e-13


def test_curved_jacobian_mode_helper(tmp_path):
    """The Jacobian-mode helper on the curved fichera mesh: f = 1 gives the oracle's M 1 from the same
    Jacobians, and float64 agrees with the extended-precision restatement."""
    p, q1d = 2, 3
    mesh, fes, J, X = helpers.curved_fichera(tmp_path, p, q1d)
    ref = R.LFRef(p, q1d, fes.gather_map(), fes.ndofs, J=J)
    b = ref.assemble([({"kind": "constant", "value": 1.0}, None)])
    op = O.OracleOperator.from_jacobians(J, fes.gather_map(), fes.ndofs, p, alpha=1.0, beta=None, q1d=q1d)
    assert relerr(b, op.mult(np.ones(fes.ndofs))) < RTOL
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:
        rld = R.LFRef(p, q1d, fes.gather_map(), fes.ndofs, J=J, dtype=np.longdouble)
        src = R.make_source("joule_T", X, None)
        assert relerr(ref.assemble([(src, None)]), rld.assemble([(src, None)]).astype(np.float64)) < 1e-13
