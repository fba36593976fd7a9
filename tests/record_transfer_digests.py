"""The cases of tests/test_gpu_transfer_bitwise.py and the recorder of their digests.

    python3 tests/record_transfer_digests.py <libecm2pa.so> [out.json]

loads the given build of the library (E.load_library(path)), runs every case on cuda:0 through the public Python
API, twice, and writes the SHA-256 of the float64 bytes of Mult's and of MultTranspose's result (default:
tests/golden/transfer_digests.json).  Every output is preset to NaN, so an entry that is not written changes the
digest; a case whose two runs differ is refused, not recorded.  The committed file was recorded from the build of
commit efd6d83, the last one in which the p- and the h-refinement transfer were two sets of kernels
(csrc/k_transfer.hip, csrc/k_htransfer.hip) behind a virtual base: that commit's kernels are the reference the one
pair of kernel templates must reproduce bit for bit -- per output entry the x sum, the y sum, the z sum, each
ascending from 0.0, then the children in ascending octant order, then the transposed-map sum.  The recorder ran in
two fresh processes there, and the two files were byte-identical; no case had to be dropped.

Inputs use no libm function: x_c and x_f are seeded uniform draws (default_rng(9).uniform(-1, 1, n), the coarse
vector first; hmg_cases.Pair.inputs["random"] for the h kind), and the transfers read nothing of a mesh but its
numbering.  The shapes are the smallest that reach a full workgroup, a tail workgroup and the second owner word
(local fine dofs 64..124, pf = 4) of each kernel:
  p, all six (pc, pf) on the moved 3 x 2 x 2 mesh: 12 elements; the pf = 4 prolongations take 10 elements per
     workgroup -- one full and one partial workgroup
  p, all six (pc, pf) on the moved 5 x 4 x 3 mesh: 60 elements, 693 fine dofs at p = 2 (odd); the restrictions take
     64, 31, 28 and 16 elements per workgroup -- several workgroups and a tail
  p, (1, 2) on the moved 9 x 4 x 2 mesh: 72 elements, the 1 -> 2 restriction takes 64 per workgroup
  p, (1, 2) and (2, 4) on fichera.mesh: seven elements whose shared faces have differing local orientations
  h, hmg_cases.TRANSFER_CASES as it stands (8, 3, 2, 1 parents per workgroup at p = 1..4), and (fichera, 3): 7
     parents at 2 per workgroup, the only odd tail of the p = 3 kernels
The largest case has 7,225 fine dofs (h, moved322 at p = 4: 6 x 4 x 4 fine elements)."""
import hashlib
import json
import os
import sys

import numpy as np

DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transfer_digests.json")
PAIRS = [(pc, pf) for pc in (1, 2, 3) for pf in range(pc + 1, 5)]
P_MESHES = {"moved322": (3, 2, 2), "moved543": (5, 4, 3), "moved942": (9, 4, 2), "fichera": None}
P_CASES = [("moved322", pc, pf) for pc, pf in PAIRS] + [("moved543", pc, pf) for pc, pf in PAIRS] \
    + [("moved942", 1, 2), ("fichera", 1, 2), ("fichera", 2, 4)]
_CACHE = {}


def h_cases():
    import hmg_cases as HC
    return list(HC.TRANSFER_CASES) + [("fichera", 3)]


def all_cases():
    return ["p-%s-%d-%d" % c for c in P_CASES] + ["h-%s-%d" % c for c in h_cases()]


def sha(t):
    a = np.ascontiguousarray(t.cpu().numpy(), dtype=np.float64)
    return hashlib.sha256(a.tobytes()).hexdigest()


def _p_mesh(E, name):
    if name not in _CACHE:
        import mg_cases as MC
        from helpers import GOLDEN
        dims = P_MESHES[name]
        _CACHE[name] = MC.lattice(dims, True) if dims else E.Mesh(os.path.join(GOLDEN, "fichera.mesh"))
    return _CACHE[name]


def setup(E, cid):
    """(transfer, x_c, x_f) of a case."""
    kind, name, orders = cid.split("-", 2)
    if kind == "p":
        pc, pf = map(int, orders.split("-"))
        m = _p_mesh(E, name)
        lf, hf = E.H1Space(m, pc), E.H1Space(m, pf)
        rng = np.random.default_rng(9)
        xc, xf = rng.uniform(-1, 1, lf.ndofs), rng.uniform(-1, 1, hf.ndofs)
        return E.PRefinementTransfer(lf, hf), xc, xf
    assert kind == "h", cid
    import hmg_cases as HC
    P = HC.pair(name, int(orders))
    xc, xf = P.inputs["random"]
    return E.HRefinementTransfer(P.lf, P.hf), xc, xf


def run_case(E, torch, cid):
    T, xc, xf = setup(E, cid)
    assert (T.width, T.height) == (len(xc), len(xf))
    yf = torch.full((T.height,), float("nan"), dtype=torch.float64, device="cuda")
    yc = torch.full((T.width,), float("nan"), dtype=torch.float64, device="cuda")
    T.Mult(torch.as_tensor(xc).cuda(), yf)
    T.MultTranspose(torch.as_tensor(xf).cuda(), yc)
    assert bool(torch.isfinite(yf).all()) and bool(torch.isfinite(yc).all()), cid + ": an entry was not written"
    return {"mult": sha(yf), "mult_transpose": sha(yc), "ndofs": [T.width, T.height]}


def main(argv):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tests"))
    import helpers  # noqa: F401  (registers the package as ecm2_amd)
    import torch
    import ecm2_amd as E
    assert len(argv) >= 2, __doc__
    E.load_library(os.path.abspath(argv[1]))
    out = argv[2] if len(argv) > 2 else DIGESTS
    digests, refused = {}, []
    for cid in all_cases():
        first, second = run_case(E, torch, cid), run_case(E, torch, cid)
        print(cid, first, flush=True)
        if first != second:
            refused.append(cid)
            print("  REFUSED: the second run gave", second, flush=True)
            continue
        digests[cid] = first
    with open(out, "w") as fh:
        json.dump(digests, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", out, "refused:", refused)
    return 1 if refused else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
