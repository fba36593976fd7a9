"""CPU pins of tests/bdr_ref.py, the numpy checker of the boundary-face kernels: exact integrals
(1^T H 1 = h area, sum b = g area over the marked faces), the sum-factorised face mass against the
face mass matrix assembled entry by entry, the marker rules, and the helper's own float64 error
against its np.longdouble restatement (it has to stay far below the GPU tests' 1e-12 bar)."""
import os

import numpy as np
import pytest

import ecm2_amd as E
import bdr_ref as R
from helpers import GOLDEN, relerr


def _ref(mesh, p, q1d, dtype=np.float64, numbering=None):
    fes = E.H1Space(mesh, p, E.NUMBERING_ENTITY if numbering is None else numbering)
    return fes, R.BdrRef(p, q1d, fes.boundary_map(), mesh.GetBdrAttributes(), fes.ndofs,
                         bnodes=mesh.boundary_nodes(), dtype=dtype)


def _quad_areas(mesh):
    """Areas of planar boundary quads from the vertices alone: |(v1 - v0) x (v3 - v0)| (rectangles)."""
    V, Q = mesh.vertices(), mesh.boundary()
    return np.linalg.norm(np.cross(V[Q[:, 1]] - V[Q[:, 0]], V[Q[:, 3]] - V[Q[:, 0]]), axis=1)


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_unit_cube_sides_have_area_one(p):
    """Attribute by attribute on the unit cube: 1^T H 1 = h and sum b = g (each side has area 1),
    with MassIntegrator's rule (p + 1) and BoundaryLFIntegrator's default."""
    mesh = E.Mesh.MakeCartesian3D(3, 2, 2)
    h, g = 7.5, 2.25
    fes, ref = _ref(mesh, p, p + 1)
    _, lref = _ref(mesh, p, R.lf_default_q1d(p))
    one = np.ones(fes.ndofs)
    for a in range(1, 7):
        mk = [1 if k + 1 == a else 0 for k in range(6)]
        assert abs(one @ ref.mult([(h, mk)], one) - h) < 1e-13 * h
        assert abs(lref.assemble([(g, mk)]).sum() - g) < 1e-13 * g
    assert abs(one @ ref.mult([(h, None)], one) - 6 * h) < 1e-12


@pytest.mark.parametrize("p", [1, 2, 3])
def test_fichera_file_attributes(p):
    """fichera.mesh (planar rectangular faces): per file attribute, 1^T H 1 = h area and sum b = g
    area, the area taken from the vertices alone."""
    mesh = E.Mesh(os.path.join(GOLDEN, "fichera.mesh"))
    attr, area = mesh.GetBdrAttributes(), _quad_areas(mesh)
    fes, ref = _ref(mesh, p, p + 1)
    _, lref = _ref(mesh, p, R.lf_default_q1d(p))
    one = np.ones(fes.ndofs)
    h, g = 3.0, 0.5
    for a in sorted(set(attr.tolist())):
        mk = np.zeros(attr.max(), np.int32)
        mk[a - 1] = 1
        A = area[attr == a].sum()
        assert abs(one @ ref.mult([(h, mk)], one) - h * A) < 1e-13 * h * A
        assert abs(lref.assemble([(g, mk)]).sum() - g * A) < 1e-13 * g * A


@pytest.mark.parametrize("name,p,dq", [("perturbed", 1, 1), ("perturbed", 2, 2), ("fichera", 3, 1), ("perturbed", 4, 2)])
def test_sum_factorised_mass_equals_entrywise_matrix(name, p, dq):
    """B^T D B on every face equals the face mass matrix assembled entry by entry; its diagonal is
    the PA diagonal; non-planar faces, a per-point h."""
    mesh = R.MESHES[name](E)
    q1d = p + dq
    fes, ref = _ref(mesh, p, q1d)
    pa = ref.pa_data(R.h_points(R.face_points(mesh.boundary_nodes(), q1d)))
    M = ref.face_matrix(pa)
    xf = ref.gather(R.positive_field(fes.dof_coords()))
    D = p + 1
    y_mat = np.einsum("fij,fj->fi", M, xf.reshape(-1, D * D))
    assert relerr(ref.face_apply(pa, xf).reshape(-1, D * D), y_mat) < 1e-14
    assert relerr(ref.face_diag(pa).reshape(-1, D * D), np.einsum("fii->fi", M)) < 1e-14


def test_marker_rules():
    """Mult masks each integrator by its own marker; the diagonal's shared face vector is zeroed by a
    later marked integrator on the faces that one excludes (bilinearform_ext.cpp:441-452)."""
    mesh = R.mesh_perturbed(E)
    p, q1d = 2, 3
    fes, ref = _ref(mesh, p, q1d)
    x = R.positive_field(fes.dof_coords())
    m13, m36 = [1, 0, 1, 0, 0, 0], [0, 0, 1, 0, 0, 1]
    y = ref.mult([(2.0, m13), (5.0, m36)], x)
    assert relerr(y, ref.mult([(2.0, m13)], x) + ref.mult([(5.0, m36)], x)) < 1e-14
    d = ref.diagonal([(2.0, m13), (5.0, m36)])
    # integrator 1 survives only where integrator 2 acts too: attribute 3
    only3 = [0, 0, 1, 0, 0, 0]
    assert relerr(d, ref.diagonal([(2.0, only3)]) + ref.diagonal([(5.0, m36)])) < 1e-14
    # an unmarked later integrator masks nothing
    d2 = ref.diagonal([(2.0, m13), (5.0, None)])
    assert relerr(d2, ref.diagonal([(2.0, m13)]) + ref.diagonal([(5.0, None)])) < 1e-14
    # pa_data holds zeros on excluded faces
    keep = R.marker_keep(ref.attr, m13)
    assert np.all(ref.pa_data(2.0, m13)[~keep] == 0.0) and np.all(ref.pa_data(2.0, m13)[keep] > 0.0)


@pytest.mark.parametrize("name", ["perturbed", "fichera"])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_float64_helper_error_is_far_below_the_gpu_bar(name, p):
    """The float64 checker against its np.longdouble restatement: Mult, diagonal and linear form."""
    mesh = R.MESHES[name](E)
    q1d = p + 1
    fes, r64 = _ref(mesh, p, q1d)
    _, rld = _ref(mesh, p, q1d, dtype=np.longdouble)
    x = R.positive_field(fes.dof_coords())
    hq = R.h_points(R.face_points(mesh.boundary_nodes(), q1d))
    nattr = int(mesh.GetBdrAttributes().max())
    mk = [1 if a % 2 == 0 else 0 for a in range(nattr)]
    integ = [(hq, None), (4.0, mk)]
    gaps = (relerr(r64.mult(integ, x), rld.mult(integ, x).astype(np.float64)),
            relerr(r64.diagonal(integ), rld.diagonal(integ).astype(np.float64)),
            relerr(r64.assemble(integ), rld.assemble(integ).astype(np.float64)))
    print(f"{name} p={p}: float64 vs longdouble gaps mult {gaps[0]:.2e} diag {gaps[1]:.2e} lform {gaps[2]:.2e}")
    assert max(gaps) < 1e-13
