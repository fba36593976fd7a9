"""CPU tests of the h-multigrid's public surface: the new symbols are declared in include/ecm2_pa.h, exported by the
library and bound with their argument counts; ecm2_mesh_copy gives an equal, independent mesh;
ecm2_mesh_refinement_embedding is the embedding of ecm2_mesh_refine_uniform's children; and the h-transfer's
construction refuses on the host what it must (no GPU is needed before a plan is valid).  The GPU runs are
tests/test_gpu_htransfer.py's and tests/test_gpu_hmultigrid.py's."""
import ctypes
import inspect
import os

import numpy as np

import helpers  # noqa: F401
import ecm2_amd as E
import mg_cases as MC
from helpers import GOLDEN, LEX_TO_NATIVE

ERR_ARG, ERR_UNSUPPORTED = 1, 5


def test_symbols_declared_exported_and_bound():
    declared = E.declared_symbols()
    lib = E._par_lib()
    for name in ("ecm2_transfer_create_h", "ecm2_mesh_copy", "ecm2_mesh_refinement_embedding"):
        assert name in declared
        assert getattr(lib, name).argtypes is not None   # exported and bound
    assert len(E._PAR_SIGS["ecm2_transfer_create_h"][1]) == 10
    assert lib.ecm2_transfer_create_h.argtypes == E._PAR_SIGS["ecm2_transfer_create_h"][1]
    assert len(lib.ecm2_mesh_copy.argtypes) == 2 and len(lib.ecm2_mesh_refinement_embedding.argtypes) == 3
    assert list(inspect.signature(E.HRefinementTransfer.__init__).parameters)[1:] == ["lfes", "hfes"]
    for attr in ("Mult", "MultTranspose"):
        assert hasattr(E.HRefinementTransfer, attr)
    assert hasattr(E.Mesh, "Copy")
    # the header cites what each entry replaces
    txt = open(E.HEADER_PATH).read()
    for cite in ("1833-2120", "1786-1807", "2055-", "CoarseFineTransformations::embeddings", "Mesh(const Mesh &)"):
        assert cite in txt, cite


def test_mesh_copy_is_equal_and_independent():
    m = E.Mesh(os.path.join(GOLDEN, "fichera.mesh"))
    m.SetAttributes(np.arange(1, m.GetNE() + 1, dtype=np.int32))
    c = m.Copy()
    V, EL = m.vertices().copy(), m.elements().copy()
    for a, b in ((c.vertices(), V), (c.elements(), EL), (c.GetAttributes(), m.GetAttributes()), (c.boundary(), m.boundary()),
                 (c.GetBdrAttributes(), m.GetBdrAttributes())):
        assert np.array_equal(a, b)
    # refining or moving the copy leaves the source as it was, and the other way round
    c.UniformRefinement()
    assert c.GetNE() == 8 * m.GetNE() and np.array_equal(m.elements(), EL) and np.array_equal(m.vertices(), V)
    m.set_vertices(V + 1.0)
    assert np.array_equal(c.vertices()[:V.shape[0]], V)
    del m
    assert c.GetNE() == 8 * EL.shape[0]
    # a Cartesian mesh keeps its lattice: the structured numbering is still available on the copy
    s = MC.lattice((3, 2, 2), True)
    a, b = E.H1Space(s, 2, E.NUMBERING_STRUCTURED), E.H1Space(s.Copy(), 2, E.NUMBERING_STRUCTURED)
    assert np.array_equal(a.gather_map(), b.gather_map())


def test_refinement_embedding_places_every_child_at_its_corner():
    """Child e has parent e / 8; its corner `octant` (lexicographic) is the parent's corner vertex `octant`: child
    k's native vertex k is the parent's native vertex k."""
    for m in (E.Mesh(os.path.join(GOLDEN, "fichera.mesh")), MC.lattice((3, 2, 2), True, sfc=True)):
        parent, octant = m.refinement_embedding()
        f = m.Copy()
        f.UniformRefinement()
        EC, EF = m.elements(), f.elements()
        assert parent.shape == octant.shape == (EF.shape[0],)
        assert np.array_equal(parent, np.arange(EF.shape[0]) // 8)
        native = np.asarray(LEX_TO_NATIVE)[octant]
        assert np.array_equal(native, np.arange(EF.shape[0]) % 8)
        assert np.array_equal(EF[np.arange(EF.shape[0]), native], EC[parent, native])
        # and geometrically: the child's lexicographic corner `octant` coincides with the parent's
        NC, NF = m.element_nodes(), f.element_nodes()
        e = np.arange(EF.shape[0])
        assert np.array_equal(NF[e, :, octant], NC[parent, :, octant])
        # every parent has one child per octant
        assert np.array_equal(np.sort(octant.reshape(-1, 8), axis=1), np.tile(np.arange(8), (EC.shape[0], 1)))


def _code(fn):
    try:
        fn()
    except E.ECM2Error as e:
        return e.code
    return 0


def test_htransfer_refusals_on_the_host():
    """Every refusal is made by the host construction, before a device is asked for."""
    m = E.Mesh.MakeCartesian3D(2, 2, 1)
    f = m.Copy()
    f.UniformRefinement()
    c1, c2, f1, f2 = E.H1Space(m, 1), E.H1Space(m, 2), E.H1Space(f, 1), E.H1Space(f, 2)
    assert _code(lambda: E.HRefinementTransfer(c1, f2)) == ERR_ARG     # unequal orders
    assert _code(lambda: E.HRefinementTransfer(c2, f1)) == ERR_ARG
    assert _code(lambda: E.HRefinementTransfer(c1, c1)) == ERR_ARG     # hfes.ne != 8 lfes.ne
    assert _code(lambda: E.HRefinementTransfer(f1, c1)) == ERR_ARG
    assert _code(lambda: E.HRefinementTransfer(E.H1Space(m, 5), E.H1Space(f, 5))) == ERR_UNSUPPORTED
    lib = E._par_lib()
    gc, gf = c1.gather_map(), f1.gather_map()
    parent, octant = m.refinement_embedding()
    h = ctypes.c_void_p()

    def create(gc=gc, gf=gf, parent=parent, octant=octant, nc=c1.ndofs, nf=f1.ndofs):
        return lib.ecm2_transfer_create_h(1, c1.ne, nc, E._np_ptr(gc), f1.ne, nf, E._np_ptr(gf), E._np_ptr(parent),
                                          E._np_ptr(octant), ctypes.byref(h))
    signed = gf.copy()
    signed[1, 3] = -1 - signed[1, 3]
    assert create(gf=signed) == ERR_UNSUPPORTED and not h.value
    assert create(nf=f1.ndofs - 1) == ERR_ARG       # an entry >= ndofs
    assert create(nf=f1.ndofs + 1) == ERR_ARG       # a fine dof that no element holds
    assert create(nc=c1.ndofs - 1) == ERR_ARG
    bad = parent.copy()
    bad[3] = c1.ne
    assert create(parent=bad) == ERR_ARG
    bad = octant.copy()
    bad[3] = 8
    assert create(octant=bad) == ERR_ARG
    bad = octant.copy()
    bad[3] = bad[2]                                  # parent 0: two children at one octant, none at another
    assert create(octant=bad) == ERR_UNSUPPORTED and not h.value
    assert b"h-transfer" in lib.ecm2_last_error()
    assert np.array_equal(gf, f1.gather_map())
