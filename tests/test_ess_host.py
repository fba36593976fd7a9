"""CPU tests of the essential-condition feature's host side: H1Space.essential_dofs (ecm2_h1space_essential_dofs:
GetEssentialVDofs + MarkerToList, fem/fespace.cpp:548-571, 622-) against a numpy restatement from the space's boundary
map and the mesh's boundary attributes; the new symbols are declared in include/ecm2_pa.h, exported and bound; and
examples/rf_electrode.cpp builds and fails loudly without a GPU (its first compute entry point returns ECM2_ERR_HIP:
no CPU fallback).  The GPU runs are tests/test_gpu_essential.py's and tests/test_gpu_example_rf_electrode.py's."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import helpers  # noqa: F401
import ecm2_amd as E
import lform_ref as LR
from helpers import ROOT

EXAMPLES = os.path.join(ROOT, "examples")
ERR_ARG = 1
ARGS = {"ecm2_operator_pcg_ex": 13, "ecm2_operator_pcg_prec_ex": 13, "ecm2_operator_pcg_mg_ex": 13,
        "ecm2_operator_bicgstab_ex": 13, "ecm2_operator_eliminate_rhs": 6, "ecm2_operator_form_linear_system": 7}


def _restated(fes, marker):
    """The dofs of the boundary elements whose attribute is marked, sorted and unique."""
    attr, bmap = fes.mesh.GetBdrAttributes(), fes.boundary_map()
    keep = np.array([marker[a - 1] != 0 for a in attr], dtype=bool)
    return np.unique(bmap[keep].ravel()).astype(np.int32)


def _meshes():
    out = [("cartesian", E.Mesh.MakeCartesian3D(3, 2, 2), p) for p in (1, 2, 3, 4)]
    m = LR.mesh_fichera(E)
    # (a file's generated boundary has attribute 1 everywhere: three attributes in turn)
    m.SetBdrAttributes(1 + (np.arange(m.GetNBE()) % 3).astype(np.int32))
    return out + [("fichera", m, 2)]


@pytest.mark.parametrize("name,mesh,p", _meshes(), ids=lambda v: v if isinstance(v, (str, int)) else "")
def test_essential_dofs_match_the_restatement(name, mesh, p):
    fes = E.H1Space(mesh, p)
    nattr = int(mesh.GetBdrAttributes().max())
    rng = np.random.default_rng(5)
    markers = [np.ones(nattr, np.int32), np.zeros(nattr, np.int32)]
    markers += [np.eye(nattr, dtype=np.int32)[a] for a in range(nattr)]          # a single attribute (a face)
    markers += [(rng.uniform(size=nattr) < 0.5).astype(np.int32) * 7 for _ in range(3)]  # any nonzero value marks
    for mk in markers:
        got = fes.essential_dofs(mk)
        assert got.dtype == np.int32 and np.array_equal(got, _restated(fes, mk)), mk
        assert np.all(np.diff(got) > 0)
    # the all-ones marker is ess_bdr = all; the empty marker marks nothing; a longer marker is fine
    assert np.array_equal(fes.essential_dofs(np.ones(nattr, np.int32)), fes.boundary_dofs())
    assert fes.essential_dofs(np.zeros(nattr, np.int32)).size == 0
    assert np.array_equal(fes.essential_dofs(np.ones(nattr + 2, np.int32)), fes.boundary_dofs())


def test_a_single_face_of_the_cartesian_mesh():
    """Make3D's attributes: 5 is the side x = 0, 3 the side x = 1 (include/ecm2_pa.h)."""
    m = E.Mesh.MakeCartesian3D(3, 2, 2)
    fes = E.H1Space(m, 2)
    X = fes.dof_coords()
    for attr, x in ((5, 0.0), (3, 1.0)):
        mk = np.zeros(6, np.int32)
        mk[attr - 1] = 1
        assert np.array_equal(fes.essential_dofs(mk), np.nonzero(X[:, 0] == x)[0])
    # the attributes are read at the call: after they change, so does the list
    m.SetBdrAttributes(np.where(m.GetBdrAttributes() == 5, 9, 1).astype(np.int32))
    mk = np.zeros(9, np.int32)
    mk[8] = 1
    assert np.array_equal(fes.essential_dofs(mk), np.nonzero(X[:, 0] == 0.0)[0])


def test_out_of_range_attribute_and_small_buffer_are_refused():
    m = E.Mesh.MakeCartesian3D(2, 2, 2)
    fes = E.H1Space(m, 1)
    with pytest.raises(E.ECM2Error) as e:
        fes.essential_dofs(np.ones(5, np.int32))       # attribute 6 has no marker entry
    assert e.value.code == ERR_ARG
    with pytest.raises(E.ECM2Error) as e:
        fes.essential_dofs(np.zeros(0, np.int32))
    assert e.value.code == ERR_ARG
    lib = E.load_library()
    mk = np.ones(6, np.int32)
    n = ctypes.c_int(3)
    out = np.full(64, -1, np.int32)
    assert lib.ecm2_h1space_essential_dofs(fes._h, E._np_ptr(mk), 6, E._np_ptr(out), ctypes.byref(n)) == ERR_ARG
    assert (out == -1).all()
    assert lib.ecm2_h1space_essential_dofs(fes._h, E._np_ptr(mk), 6, None, ctypes.byref(n)) == 0
    assert n.value == fes.boundary_dofs().size
    # the mesh refined after the space was created: its boundary no longer matches the space's map
    m.UniformRefinement()
    with pytest.raises(E.ECM2Error) as e:
        fes.essential_dofs(mk)
    assert e.value.code == ERR_ARG


def test_symbols_declared_exported_and_bound():
    declared = E.declared_symbols()
    lib = E._par_lib()
    assert "ecm2_h1space_essential_dofs" in declared and lib.ecm2_h1space_essential_dofs.argtypes is not None
    for name, nargs in ARGS.items():
        assert name in declared
        fn = getattr(lib, name)          # exported
        assert name in E._PAR_SIGS and fn.argtypes == E._PAR_SIGS[name][1]
        assert len(E._PAR_SIGS[name][1]) == nargs
    # an _ex entry point is the old one with a trailing int
    for old in ("ecm2_operator_pcg", "ecm2_operator_pcg_prec", "ecm2_operator_pcg_mg", "ecm2_operator_bicgstab"):
        assert E._PAR_SIGS[old + "_ex"][1] == E._PAR_SIGS[old][1] + [ctypes.c_int]
    for fn in (E.Operator.PCG, E.Operator.BiCGSTAB):
        assert inspect.signature(fn).parameters["iterative_mode"].default is False
    p = inspect.signature(E.Operator.FormLinearSystem).parameters
    assert list(p)[1:4] == ["ess", "x", "b"] and p["copy_interior"].default is False
    assert list(inspect.signature(E.Operator.EliminateRHS).parameters)[1:4] == ["x", "b", "ess"]
    # the header cites the reference's lines at the entry points
    txt = open(E.HEADER_PATH).read()
    for cite in ("548-571", "559-584", "114-129", "875-884", "1618-1622", "solvers.cpp:29-30", "RecoverFEMSolution"):
        assert cite in txt, cite
    # a null operator is refused before anything else
    assert lib.ecm2_operator_eliminate_rhs(None, None, 0, None, None, None) == ERR_ARG
    assert lib.ecm2_operator_form_linear_system(None, None, 0, None, None, 0, None) == ERR_ARG


def test_rf_electrode_example_builds_and_fails_loudly_without_gpu():
    """Compiles and links against the header + library; with no device the form's create returns ECM2_ERR_HIP and
    the program stops with status 2 (no CPU fallback), after the host setup -- the essential list included."""
    subprocess.run(["make", "-s", "-C", EXAMPLES], check=True, timeout=300)
    binary = os.path.join(EXAMPLES, "rf_electrode")
    assert os.access(binary, os.X_OK)
    if E.load_library().ecm2_device_count() > 0:
        return
    r = subprocess.run([binary], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, r.stdout + r.stderr
    # 17^3 dofs, two faces of 17^2 essential dofs, Make3D's attributes of x = 0 and x = 1
    assert "unit cube 8^3 elements, H1 p=2, 4913 dofs, 578 essential (attributes 5: phi = 30, 3: phi = 0)" in r.stdout
    assert "ecm2_pa_form_create" in r.stderr and "no HIP device" in r.stderr
