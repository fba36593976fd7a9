"""CPU tests of the p-multigrid's public surface: the new symbols are declared in include/ecm2_pa.h, exported by the
library and bound in _PAR_SIGS with their argument counts, the Python classes have the documented signatures, and
the transfer's construction refuses on the host what it must (no GPU is needed before a plan is valid).  The GPU
runs are tests/test_gpu_transfer.py's and tests/test_gpu_multigrid.py's."""
import inspect

import numpy as np

import helpers  # noqa: F401
import ecm2_amd as E

ARGS = {"ecm2_transfer_create": 8, "ecm2_transfer_mult": 4, "ecm2_transfer_mult_transpose": 4, "ecm2_transfer_info": 7,
        "ecm2_transfer_destroy": 1, "ecm2_multigrid_create": 9, "ecm2_multigrid_set_coarse_pcg": 3,
        "ecm2_multigrid_mult": 4, "ecm2_multigrid_destroy": 1, "ecm2_operator_pcg_mg": 12}
ERR_ARG, ERR_UNSUPPORTED = 1, 5


def test_symbols_declared_exported_and_bound():
    declared = E.declared_symbols()
    lib = E._par_lib()
    for name, nargs in ARGS.items():
        assert name in declared
        fn = getattr(lib, name)          # exported
        assert name in E._PAR_SIGS and fn.argtypes == E._PAR_SIGS[name][1]
        assert len(E._PAR_SIGS[name][1]) == nargs
    # ecm2_operator_pcg_mg has ecm2_operator_pcg_prec's argument list
    assert E._PAR_SIGS["ecm2_operator_pcg_mg"] == E._PAR_SIGS["ecm2_operator_pcg_prec"]
    p = inspect.signature(E.Multigrid.__init__).parameters
    assert list(p)[1:5] == ["ops", "smoothers", "transfers", "ess"]
    assert [p[k].default for k in ("pre", "post", "coarse_pcg")] == [1, 1, None]
    assert list(inspect.signature(E.PRefinementTransfer.__init__).parameters)[1:] == ["lfes", "hfes"]
    assert hasattr(E.PRefinementTransfer, "Mult") and hasattr(E.PRefinementTransfer, "MultTranspose")
    p = inspect.signature(E.Operator.PCG).parameters
    assert list(p)[-2:] == ["stream", "prec"] and p["prec"].default is None
    # the header cites the reference's lines at the entry points
    txt = open(E.HEADER_PATH).read()
    for cite in ("2223-2287", "2338-2423", "2470-2539", "248-283", "106-145", "147-232", "296-309"):
        assert cite in txt, cite


def _code(fn):
    try:
        fn()
    except E.ECM2Error as e:
        return e.code
    return 0


def test_multigrid_list_lengths_are_checked_before_the_call():
    assert _code(lambda: E.Multigrid([], [], [], [])) == ERR_ARG
    assert _code(lambda: E.Multigrid([], [], [], None)) == ERR_ARG


def test_transfer_refusals_on_the_host():
    """Every refusal is made by the host construction, before a device is asked for."""
    m = E.Mesh.MakeCartesian3D(2, 2, 1)
    f1, f2 = E.H1Space(m, 1), E.H1Space(m, 2)
    assert _code(lambda: E.PRefinementTransfer(f2, f1)) == ERR_ARG
    assert _code(lambda: E.PRefinementTransfer(f2, f2)) == ERR_ARG
    assert _code(lambda: E.PRefinementTransfer(f1, E.H1Space(E.Mesh.MakeCartesian3D(2, 2, 2), 2))) == ERR_ARG  # unequal ne
    assert _code(lambda: E.PRefinementTransfer(f1, E.H1Space(m, 5))) == ERR_UNSUPPORTED
    lib = E._par_lib()
    import ctypes
    g1, g2 = f1.gather_map(), f2.gather_map()
    h = ctypes.c_void_p()

    def create(gl, gh, nl=f1.ndofs, nh=f2.ndofs):
        return lib.ecm2_transfer_create(f1.ne, 1, nl, E._np_ptr(gl), 2, nh, E._np_ptr(gh), ctypes.byref(h))
    signed = g2.copy()
    signed[1, 3] = -1 - signed[1, 3]
    assert create(g1, signed) == ERR_UNSUPPORTED and not h.value
    assert create(g1, g2, nh=f2.ndofs - 1) == ERR_ARG       # an entry >= ndofs
    assert create(g1, g2, nh=f2.ndofs + 1) == ERR_ARG       # a fine dof that no element holds
    assert create(g1, g2, nl=f1.ndofs - 1) == ERR_ARG
    assert b"transfer" in lib.ecm2_last_error()
    assert np.array_equal(g2, f2.gather_map())
