#!/usr/bin/env python3
"""bench.py's marginal Jacobi-PCG iteration of one source tree, repeated inside one process: the tree's own
bench.pcg_iteration_ms on its own configs[3] form (Cartesian 108^3 elements, p = 2, structured numbering), 11
times at 20 / 40 iterations and 7 times at 50 / 100.  For comparing two builds of the library -- a checkout of
the parent commit, built, against this tree -- run it once per tree, alternating the trees, in one session:
    python profiles/pcg_iteration_ab.py . ; python profiles/pcg_iteration_ab.py ../parent ; ...
bench.py itself takes the figure once per process, where the order of the processes shows (profiles/cheb_c4.txt).
One MI355X; prints one JSON line: the median, minimum and maximum of each series, ms.

Usage: python profiles/pcg_iteration_ab.py TREE_ROOT"""
import json
import os
import statistics
import sys

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
os.chdir(root)
import torch  # noqa: E402
import bench  # noqa: E402  (the tree's own)

E = bench.load_pkg()
mesh, fes = bench.cartesian_space(E, 108, 108, 108, 2, "structured", "affine")
keep = []
form = bench.bench_form(E, torch, mesh, fes, keep)
out = {"root": sys.argv[1]}
for iters, reps in ((20, 11), (50, 7)):
    v = [bench.pcg_iteration_ms(torch, form, fes.ndofs, iters) for _ in range(reps)]
    out[f"iters{iters}"] = {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}
print(json.dumps(out), flush=True)
