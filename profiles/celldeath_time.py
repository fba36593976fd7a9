#!/usr/bin/env python3
"""Time of one CellDeath.Step at C4's dof count (n = 10,218,313) for nsub = 1 and 4, with and without T1, beside
the bandwidth floor of its 7 or 8 vector streams at this run's own ecm2_stream_copy rate.  HIP
events; every configuration runs in a child process of its own under its own time limit, so a configuration that
hangs or faults ends the run there instead of the next one starting on the same card.  One MI355X; prints one JSON
line per configuration.  (The FP64 instruction count per entry per substep is read from the ISA, not here.)

Usage: python profiles/celldeath_time.py [n = 10218313] [reps = 20]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT_S = 150


def timed(torch, fn, reps):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def one(n, reps, nsub, with_T1):
    import torch
    from __graft_entry__ import _load_pkg
    E = _load_pkg()
    E.load_library()
    g = torch.Generator(device="cuda").manual_seed(1)
    T0 = torch.empty(n, dtype=torch.float64, device="cuda").uniform_(37.0, 95.0, generator=g)
    T1 = T0 + 5.0 if with_T1 else None
    # the lesion example's parameters; the warm-up and the timed steps keep advancing the same state (the step's
    # time does not depend on the data)
    cd = E.CellDeath(E.CELLDEATH_THREE_STATE, (7.39e39, 1.0e25, 3.1e98), (2.577e5, 1.6e5, 6.28e5), n)
    N, U, D = torch.ones_like(T0), torch.zeros_like(T0), torch.zeros_like(T0)
    step_ms = timed(torch, lambda: cd.Step(T0, 1.0, N, U, D, T1=T1, nsub=nsub), reps)
    assert cd.Step(T0, 1.0, N, U, D, T1=T1, nsub=nsub, check=True) == 0
    assert bool(torch.isfinite(D).all()) and float(D.max()) <= 1.0
    m = n & ~1
    a, c = T0[:m], torch.empty(m, dtype=torch.float64, device="cuda")
    copy_ms = timed(torch, lambda: E.stream_copy(a, c), reps)
    copy_gbs = 16.0 * m / copy_ms / 1e6
    streams = 8 if with_T1 else 7
    nbytes = 8 * n * streams
    floor_ms = nbytes / (copy_gbs * 1e6)
    return {"n": n, "nsub": nsub, "T1": bool(with_T1), "step_ms": round(step_ms, 4), "streams": streams,
            "bytes": nbytes, "achieved_gbs": round(nbytes / step_ms / 1e6, 1), "stream_copy_gbs": round(copy_gbs, 1),
            "stream_floor_ms": round(floor_ms, 4), "step_over_floor": round(step_ms / floor_ms, 2),
            "ns_per_entry_substep": round(step_ms * 1e6 / n / nsub, 4), "device": torch.cuda.get_device_name(0)}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        n, reps, nsub, with_T1 = (int(v) for v in sys.argv[2:6])
        print(json.dumps(one(n, reps, nsub, with_T1)))
        return 0
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10218313
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    for nsub in (1, 4):
        for with_T1 in (0, 1):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n), str(reps), str(nsub),
                                str(with_T1)], capture_output=True, text=True, timeout=LIMIT_S)
            if r.returncode != 0:   # a fault, an abort or a failed check: nothing more is started on the card
                print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
                return r.returncode if r.returncode > 0 else 1
            print(r.stdout.strip().split("\n")[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
