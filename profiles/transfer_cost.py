#!/usr/bin/env python3
"""The transfer operator's two kernels alone (DESIGN.md sections 4f and 4g): what profiles/mg_cost.py and
profiles/hmg_cost.py report beside their solves, and a mode of its own that walks all ten (kind, orders)
combinations at one size.

transfer_times(T, lo, hi, res): ms per call of T.Mult and T.MultTranspose between the spaces lo and hi (HIP events
over 20 calls, the median of 5 groups, after 3 warm-up calls) and the bytes that must move: both vectors, both maps
(the restriction reads the fine one only), the owner words and, for an h-refinement, the children table; for
MultTranspose also its coarse E-vector written and read back and the transposed map.

Usage: python profiles/transfer_cost.py [n = 54] [--lib=path/to/libecm2pa.so]
  all six p pairs on an n^3 mesh and the four h orders from (n/2)^3 to n^3 (n even), entity numbering; one JSON line
  per combination.  Reported, not gated.  One MI355X.
Every profiles script that imports load() takes --lib=... to time another build of the library (a same-box A/B)."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import _load_pkg  # noqa: E402


def load(argv):
    """The package with the library of --lib=path loaded (default: the tree's own)."""
    E = _load_pkg()
    libs = [a[len("--lib="):] for a in argv if a.startswith("--lib=")]
    E.load_library(*[os.path.abspath(p) for p in libs[:1]])
    return E


def timed_call(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def call_ms(fn):
    """ms per call: 3 warm-up calls, then the median of 5 groups of 20."""
    for _ in range(3):
        fn()
    return round(statistics.median(timed_call(lambda: [fn() for _ in range(20)])[0] / 20 for _ in range(5)), 5)


def transfer_times(T, lo, hi, res):
    xc = torch.rand(lo.ndofs, dtype=torch.float64, device="cuda")
    xf = torch.rand(hi.ndofs, dtype=torch.float64, device="cuda")
    yc, yf = torch.empty_like(xc), torch.empty_like(xf)
    res["prolong_ms"] = call_ms(lambda: T.Mult(xc, yf))
    res["restrict_ms"] = call_ms(lambda: T.MultTranspose(xf, yc))
    vectors, owner = 8 * (lo.ndofs + hi.ndofs), 16 * hi.ne
    children = 32 * lo.ne if hi.ne != lo.ne else 0
    csr = 4 * (lo.ndofs + 1) + 4 * lo.nd * lo.ne
    res["pair"] = {"elements": [lo.ne, hi.ne], "ndofs": [lo.ndofs, hi.ndofs], "orders": [lo.order, hi.order],
                   "plan_bytes": T.plan_bytes}
    res["prolong_bytes"] = vectors + 4 * (lo.nd * lo.ne + hi.nd * hi.ne) + owner + children
    res["restrict_bytes"] = vectors + 4 * hi.nd * hi.ne + owner + children + 2 * 8 * lo.nd * lo.ne + csr
    res["prolong_tb_s"] = round(res["prolong_bytes"] / res["prolong_ms"] * 1e-9, 3)
    res["restrict_tb_s"] = round(res["restrict_bytes"] / res["restrict_ms"] * 1e-9, 3)


def all_combinations(E, n):
    assert n % 2 == 0, n
    coarse = E.Mesh.MakeCartesian3D(n // 2, n // 2, n // 2)
    fine = coarse.Copy()
    fine.UniformRefinement()
    on_fine = {p: E.H1Space(fine, p) for p in (1, 2, 3, 4)}
    combos = [("p", on_fine[pc], on_fine[pf]) for pc in (1, 2, 3) for pf in range(pc + 1, 5)]
    combos += [("h", E.H1Space(coarse, p), on_fine[p]) for p in (1, 2, 3, 4)]
    for kind, lo, hi in combos:
        T = (E.PRefinementTransfer if kind == "p" else E.HRefinementTransfer)(lo, hi)
        res = {"shape": "combinations", "kind": kind}
        transfer_times(T, lo, hi, res)
        print(json.dumps(res), flush=True)
        del T


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    all_combinations(load(sys.argv[1:]), int(args[0]) if args else 54)
