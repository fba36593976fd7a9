"""CPU tests of the cell-death feature's host side: the update of csrc/celldeath_math.hpp (the function the device
kernel calls per entry) in a program of its own under ASan + UBSan (the library Makefile's celldeath_check target;
the sanitizers are linked into that program only) over the case matrix, the near-double-eigenvalue cases and the hazards, against a long
double closed form evaluated in the program and against tests/celldeath_ref.py's 80-bit run; the new symbols are
declared in include/ecm2_pa.h, exported and bound; the Python names exist; create's argument checks return
ECM2_ERR_ARG and create fails loudly without a GPU.  The GPU runs are tests/test_gpu_celldeath.py's."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import helpers  # noqa: F401
import ecm2_amd as E
import celldeath_cases as CC
import celldeath_ref as CR
from helpers import ROOT
from test_celldeath_reference import C_SUM, c_cd

PKG = os.path.join(ROOT, "cardiac-ablation-ecm2_amd")
SYMBOLS = ["ecm2_celldeath_create", "ecm2_celldeath_step", "ecm2_celldeath_measure", "ecm2_celldeath_info",
           "ecm2_celldeath_destroy"]


def _hx(v):
    v = float(v)
    return v.hex() if np.isfinite(v) else repr(v)


@pytest.fixture(scope="module")
def checked(tmp_path_factory):
    """Every case's entries through the C++ program once: [(case, ok, N, U, D, errN, errU, errD)]."""
    tmp = tmp_path_factory.mktemp("celldeath")
    exe = os.path.join(str(tmp), "celldeath_check")
    subprocess.run(["make", "-s", "-C", PKG, f"OBJ={tmp}", exe], check=True, timeout=600)
    cases = list(CC.measured_cases()) + CC.hazard_cases()
    lines = []
    for c in cases:
        T1 = c["T1"]
        head = " ".join([str(c["model"])] + [_hx(v) for i in range(3) for v in (c["A"][i], c["dE"][i])]
                        + [_hx(c["t_offset"])])
        for i in range(c["T0"].size):
            dT = (T1[i] - c["T0"][i]) if T1 is not None else 0.0
            lines.append(f"{head} {_hx(c['T0'][i])} {_hx(dT)} {_hx(c['dt'])} {c['nsub']} {_hx(c['N'][i])} "
                         f"{_hx(c['U'][i])} {_hx(c['D'][i])}\n")
    r = subprocess.run([exe], input="".join(lines) + "end\n", capture_output=True, text=True, timeout=600)
    print(r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = r.stdout.split("\n")
    assert rows[len(lines)] == f"cases {len(lines)}"
    out, k = [], 0
    for c in cases:
        n = c["T0"].size
        f = [rows[k + i].split() for i in range(n)]
        k += n
        ok = np.array([t[0] == "1" for t in f])
        vals = [np.array([float.fromhex(t[j]) for t in f]) for j in (1, 2, 3)]
        errs = [np.array([float(t[j]) for t in f]) for j in (4, 5, 6)]
        out.append((c, ok, *vals, *errs))
    return out


def test_header_update_against_closed_form_and_reference(checked):
    worst = 0.0
    for c, ok, N, U, D, eN, eU, eD in checked:
        C = c_cd(c["model"])
        tol = CC.tolerance(c, C)
        hp = CR.step(c["model"], c["A"], c["dE"], c["t_offset"], c["T0"], c["T1"], c["dt"], c["nsub"], c["N"],
                     c["U"], c["D"])
        assert (ok == ~hp[3]).all(), c["name"]
        for X, got, err, ref in zip("NUD", (N, U, D), (eN, eU, eD), hp):
            assert np.isfinite(got).all(), (c["name"], X)
            scale = np.maximum(1.0, np.abs(ref)) if (c["model"] == CR.ARRHENIUS and X == "U") else 1.0
            e1 = float((err / tol).max())                                         # the program's closed form
            e2 = float((np.abs(got.astype(np.longdouble) - ref) / scale / tol).max())    # the 80-bit restatement
            worst = max(worst, e1 * C, e2 * C)
            assert e1 <= 1.0, (c["name"], X, e1 * C, C)
            assert e2 <= 1.0, (c["name"], X, e2 * C, C)
    print(f"worst error of the header's update: {worst:.3f} u (1 + x_max), bounds {c_cd(0)}, {c_cd(1)}")


def test_header_invariants_and_hazards(checked):
    names = set()
    for c, ok, N, U, D, _, _, _ in checked:
        names.add(c["name"])
        assert (D[ok] >= c["D"][ok]).all(), c["name"]                   # monotone death, exactly
        assert (N >= 0).all() and (U >= 0).all() and (D >= 0).all(), c["name"]
        bad = ~ok
        for got, old in ((N, c["N"]), (U, c["U"]), (D, c["D"])):        # invalid entries: bitwise untouched
            assert (got[bad].view(np.int64) == old[bad].view(np.int64)).all(), c["name"]
        if c["model"] == CR.THREE_STATE:
            assert (N <= 1).all() and (U <= 1).all() and (D <= 1).all(), c["name"]
            s0, s1 = c["N"] + c["U"] + c["D"], N + U + D
            assert (np.abs(s1 - 1.0) <= np.abs(s0 - 1.0) + C_SUM * CR.U_ROUND * c["nsub"]).all(), c["name"]
        if "A123=0" in c["name"] or c["name"] in ("underflow: T_K = 1", "dt = 0"):
            for got, old in ((N, c["N"]), (U, c["U"]), (D, c["D"])):    # zero rates: bitwise unchanged
                assert (got.view(np.int64) == old.view(np.int64)).all(), c["name"]
        if c["name"] == "invalid entries":
            assert list(np.flatnonzero(bad)) == [3, 7, 11, 20]
        if c["name"] == "invalid at a substep":
            assert list(np.flatnonzero(bad)) == [3, 7, 30]
        if c["name"].startswith("overflow"):
            assert ok.all() and (D > 0.999999).all()
    assert {"overflow: 95 C, dt = 300", "overflow: rate dt = inf", "double eigenvalue: a = c, b = 0",
            "invalid at a substep"} <= names
    assert sum(n.startswith("near-double") for n in names) >= 40


def test_symbols_declared_exported_and_bound():
    declared = E.declared_symbols()
    lib = E._par_lib()
    for name in SYMBOLS:
        assert name in declared
        fn = getattr(lib, name)          # exported
        assert name in E._PAR_SIGS and fn.argtypes == E._PAR_SIGS[name][1]
    assert len(E._PAR_SIGS["ecm2_celldeath_step"][1]) == 10
    assert len(E._PAR_SIGS["ecm2_celldeath_measure"][1]) == 6
    assert (E.CELLDEATH_THREE_STATE, E.CELLDEATH_ARRHENIUS) == (0, 1)
    p = inspect.signature(E.CellDeath.__init__).parameters
    assert list(p)[1:] == ["model", "A", "dE", "n", "t_offset"] and p["t_offset"].default == 273.15
    p = inspect.signature(E.CellDeath.Step).parameters
    assert list(p)[1:6] == ["T0", "dt", "N", "U", "D"]
    assert [p[k].default for k in ("T1", "nsub", "check")] == [None, 1, False]
    assert list(inspect.signature(E.CellDeath.Measure).parameters)[1:4] == ["D", "w", "theta"]
    assert callable(E.CellDeath.info)
    txt = open(E.HEADER_PATH).read()
    for word in ("ECM2_CELLDEATH_THREE_STATE 0", "ECM2_CELLDEATH_ARRHENIUS 1", "8.31446261815324",
                 "(a - c)^2 + b^2 + 2 b (a + c)", "lambda_+ = a c / lambda_-"):
        assert word in txt, word


def _create(model, params, t_offset, n):
    lib = E._par_lib()
    h = ctypes.c_void_p()
    arr = (ctypes.c_double * 6)(*params) if params is not None else None
    rc = lib.ecm2_celldeath_create(model, arr, t_offset, n, ctypes.byref(h))
    if rc == 0:
        lib.ecm2_celldeath_destroy(h)
    return rc, lib.ecm2_last_error().decode()


def test_create_argument_checks_come_before_the_device():
    good = [1.0, 1e5, 1.0, 1e5, 1.0, 1e5]
    nan, inf = float("nan"), float("inf")
    bad = [(2, good, 273.15, 8), (-1, good, 273.15, 8), (0, good, 273.15, 0), (0, good, 273.15, -3),
           (0, None, 273.15, 8), (0, good, nan, 8), (1, [-1.0] + good[1:], 273.15, 8)]
    for i in range(6):
        for v in (-1e-300, nan, inf):
            bad.append((0, good[:i] + [v] + good[i + 1:], 273.15, 8))
    bad.append((0, [1e151] + good[1:], 273.15, 8))
    for args in bad:
        rc, msg = _create(*args)
        assert rc == 1, (args, rc, msg)          # ECM2_ERR_ARG, with or without a device
        assert msg
    with pytest.raises(E.ECM2Error) as ei:
        E.CellDeath(7, (1.0, 1.0, 1.0), (1e5, 1e5, 1e5), 8)
    assert ei.value.code == 1
    with pytest.raises(E.ECM2Error):
        E.CellDeath(E.CELLDEATH_THREE_STATE, (1.0, 1.0), (1e5, 1e5, 1e5), 8)   # three of each


def test_create_fails_loudly_without_gpu():
    if E.load_library().ecm2_device_count() > 0:
        return
    rc, msg = _create(0, [1.0, 1e5, 1.0, 1e5, 1.0, 1e5], 273.15, 8)
    assert rc == 2 and "no HIP device" in msg, (rc, msg)     # ECM2_ERR_HIP: no CPU fallback
    with pytest.raises(E.ECM2Error) as ei:
        E.CellDeath(E.CELLDEATH_ARRHENIUS, (1.0, 0.0, 0.0), (1e5, 0.0, 0.0), 8)
    assert ei.value.code == 2
