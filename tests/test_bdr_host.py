"""CPU tests of the host side of the boundary terms: the mesh's boundary elements (Mesh::Make3D's six
sides, the v1.0 reader's `boundary` section, GenerateBoundaryElements, uniform refinement) and the
space's boundary-face dof map."""
import os

import numpy as np
import pytest

import ecm2_amd as E
import oracle as O
from helpers import GOLDEN, read_mfem_mesh, write_linear_mfem_mesh


def _make3d_boundary(nx, ny, nz):
    """numpy restatement of Mesh::Make3D's boundary loops (mesh/mesh.cpp:3815-3949)."""
    V = lambda x, y, z: x + (y + z * (ny + 1)) * (nx + 1)
    q, a = [], []
    for y in range(ny):
        for x in range(nx):
            q.append([V(x, y, 0), V(x, y + 1, 0), V(x + 1, y + 1, 0), V(x + 1, y, 0)]); a.append(1)
    for y in range(ny):
        for x in range(nx):
            q.append([V(x, y, nz), V(x + 1, y, nz), V(x + 1, y + 1, nz), V(x, y + 1, nz)]); a.append(6)
    for z in range(nz):
        for y in range(ny):
            q.append([V(0, y, z), V(0, y, z + 1), V(0, y + 1, z + 1), V(0, y + 1, z)]); a.append(5)
    for z in range(nz):
        for y in range(ny):
            q.append([V(nx, y, z), V(nx, y + 1, z), V(nx, y + 1, z + 1), V(nx, y, z + 1)]); a.append(3)
    for x in range(nx):
        for z in range(nz):
            q.append([V(x, 0, z), V(x + 1, 0, z), V(x + 1, 0, z + 1), V(x, 0, z + 1)]); a.append(2)
    for x in range(nx):
        for z in range(nz):
            q.append([V(x, ny, z), V(x, ny, z + 1), V(x + 1, ny, z + 1), V(x + 1, ny, z)]); a.append(4)
    return np.array(q, np.int32), np.array(a, np.int32)


def _file_boundary(path):
    lines = [ln.split("#")[0].strip() for ln in open(path)]
    lines = [ln for ln in lines if ln]
    i = lines.index("boundary")
    n = int(lines[i + 1])
    rows = np.array([[int(t) for t in lines[i + 2 + k].split()] for k in range(n)], np.int32)
    assert np.all(rows[:, 1] == 3)
    return rows[:, 2:], rows[:, 0]


def _faces_of_one_element(mesh):
    """For every boundary quad, the number of elements that have its vertex set as a face."""
    faces = [(3, 2, 1, 0), (0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (3, 0, 4, 7), (4, 5, 6, 7)]
    count = {}
    for el in mesh.elements():
        for f in faces:
            k = tuple(sorted(int(el[i]) for i in f))
            count[k] = count.get(k, 0) + 1
    return [count.get(tuple(sorted(int(v) for v in q)), 0) for q in mesh.boundary()]


@pytest.mark.parametrize("sfc", [False, True])
def test_cartesian_boundary_is_make3d(sfc):
    nx, ny, nz = 3, 2, 2
    m = E.Mesh.MakeCartesian3D(nx, ny, nz, sfc_ordering=sfc)
    q, a = _make3d_boundary(nx, ny, nz)
    assert m.GetNBE() == 2 * (nx * ny + ny * nz + nx * nz) == 32
    assert np.array_equal(m.GetBdrAttributes(), a)
    assert np.array_equal(m.boundary(), q)
    assert _faces_of_one_element(m) == [1] * 32


def test_fichera_boundary_and_refinement():
    path = os.path.join(GOLDEN, "fichera.mesh")
    m = E.Mesh(path)
    q, a = _file_boundary(path)
    assert m.GetNBE() == 24
    assert np.array_equal(m.boundary(), q) and np.array_equal(m.GetBdrAttributes(), a)
    assert _faces_of_one_element(m) == [1] * 24
    V0, parents = m.vertices(), m.boundary()
    m.UniformRefinement()
    assert m.GetNBE() == 96
    assert np.array_equal(m.GetBdrAttributes(), np.repeat(a, 4))
    assert _faces_of_one_element(m) == [1] * 96
    # child k of parent i keeps the parent's vertex k at position k (mesh.cpp:10749-10756), its
    # opposite corner is the parent's centre, and the four children tile the parent
    V, kids = m.vertices(), m.boundary().reshape(24, 4, 4)
    for i in range(24):
        centre = V0[parents[i]].mean(axis=0)
        for k in range(4):
            assert kids[i, k, k] == parents[i, k]
            assert np.allclose(V[kids[i, k, (k + 2) % 4]], centre)
        for k in range(4):  # the midpoint of edge (k, k + 1): child k's vertex k + 1 = child k + 1's vertex k
            mid = 0.5 * (V0[parents[i, k]] + V0[parents[i, (k + 1) % 4]])
            assert kids[i, k, (k + 1) % 4] == kids[i, (k + 1) % 4, k]
            assert np.allclose(V[kids[i, k, (k + 1) % 4]], mid)


def test_boundary_attributes_round_trip():
    m = E.Mesh.MakeCartesian3D(2, 2, 1)
    a = m.GetBdrAttributes().copy()
    a[::2] = 9
    m.SetBdrAttributes(a)
    assert np.array_equal(m.GetBdrAttributes(), a)
    a[0] = 0
    with pytest.raises(E.ECM2Error):
        m.SetBdrAttributes(a)


def test_file_without_boundary_section_gets_generated_boundary(tmp_path):
    """A v1.0 file with no `boundary` section: the faces with one element, attribute 1."""
    V, El = read_mfem_mesh(os.path.join(GOLDEN, "fichera.mesh"))
    path = os.path.join(str(tmp_path), "nobdr.mesh")
    with open(path, "w") as f:
        f.write("MFEM mesh v1.0\n\ndimension\n3\n\nelements\n%d\n" % len(El))
        for e in El:
            f.write("1 5 " + " ".join(str(int(v)) for v in e) + "\n")
        f.write("\nvertices\n%d\n3\n" % len(V))
        for v in V:
            f.write("%.17g %.17g %.17g\n" % tuple(v))
    m = E.Mesh(path)
    assert m.GetNBE() == 24 and np.all(m.GetBdrAttributes() == 1)
    assert _faces_of_one_element(m) == [1] * 24
    ref = E.Mesh(os.path.join(GOLDEN, "fichera.mesh"))
    assert sorted(tuple(sorted(q)) for q in m.boundary().tolist()) == sorted(tuple(sorted(q)) for q in ref.boundary().tolist())
    # an explicitly empty section stays empty (the file's word)
    empty = os.path.join(str(tmp_path), "empty.mesh")
    write_linear_mfem_mesh(empty, V, El)
    assert E.Mesh(empty).GetNBE() == 0


def test_boundary_section_takes_quadrilaterals_only(tmp_path):
    path = os.path.join(str(tmp_path), "tri.mesh")
    with open(path, "w") as f:
        f.write("MFEM mesh v1.0\n\ndimension\n3\n\nelements\n1\n1 5 0 1 2 3 4 5 6 7\n\nboundary\n1\n1 2 0 1 2\n\n"
                "vertices\n8\n3\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n0 0 1\n1 0 1\n1 1 1\n0 1 1\n")
    with pytest.raises(E.ECM2Error) as ei:
        E.Mesh(path)
    assert ei.value.code == 5  # ECM2_ERR_UNSUPPORTED


def _meshes():
    c = E.Mesh.MakeCartesian3D(3, 2, 2, 1.5, 1.0, 0.8)
    V = c.vertices()
    V += np.random.default_rng(3).uniform(-0.03, 0.03, V.shape)
    c.set_vertices(V)
    f = E.Mesh(os.path.join(GOLDEN, "fichera.mesh"))
    f.UniformRefinement()
    return {"cartesian": c, "fichera": f}


@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("name,numbering", [("cartesian", E.NUMBERING_ENTITY), ("cartesian", E.NUMBERING_STRUCTURED),
                                            ("fichera", E.NUMBERING_ENTITY)])
def test_boundary_map_rows_are_the_face_dofs(name, numbering, p):
    """Every row equals the dofs found geometrically: the dof coordinates are the bilinear image of
    the GLL lattice of the quad in its own frame (xi: v0 -> v1, eta: v0 -> v3), and the row is found
    again from the coordinates alone."""
    mesh = _meshes()[name]
    fes = E.H1Space(mesh, p, numbering)
    bm, X, bn = fes.boundary_map(), fes.dof_coords(), mesh.boundary_nodes()
    D = p + 1
    assert bm.shape == (mesh.GetNBE(), D * D) and bm.min() >= 0 and bm.max() < fes.ndofs
    t = O.gauss_lobatto(D)[0]
    xi, et = np.tile(t, D), np.repeat(t, D)
    N = np.stack([(1 - xi) * (1 - et), xi * (1 - et), (1 - xi) * et, xi * et], 0)    # [corner][i]
    img = np.einsum("fca,ai->fic", bn, N)                                            # [f][i][3]
    assert np.abs(X[bm] - img).max() < 1e-13
    # corners of the frame are the quad's vertices v0, v1, v3, v2
    V, Q = mesh.vertices(), mesh.boundary()
    for a, k in enumerate((0, 1, 3, 2)):
        assert np.array_equal(bn[:, :, a], V[Q[:, k]])
    # found from the coordinates alone: the nearest dof to every image point is the row's entry
    flat = img.reshape(-1, 3)
    d2 = ((flat[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    assert np.array_equal(d2.argmin(axis=1).reshape(bm.shape), bm)
    # every boundary dof of the space appears in some row, and nothing else does
    assert np.array_equal(np.unique(bm), np.sort(fes.boundary_dofs()))
