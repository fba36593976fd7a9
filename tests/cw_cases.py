"""The case matrix of the componentwise Mult / diagonal criterion (tests/hp_ref.py), shared by the CPU
pins of the oracle (test_hp_reference.py: c_ref) and the device tests (test_gpu_componentwise.py).

A *space* is (mesh, p, numbering): the meshes are the existing suite's, each the smallest that still
reaches its kernel path.  On it live the four states, the per-point coefficients (float64 arrays both
the device and the extended-precision reference take as exact inputs), and per form the HPRef with
y_hp, S for every state and the diagonal -- computed once, cached, left unchanged.

Forms: K (beta = k(T(P))), M (balanced alpha), MK (both), MKphys (alpha_bioheat, 1e3 - 1e5 times the
diffusion term: the headline scaling), and on the coefficient-snapshot spaces Ks / MKs / PKs with beta
the affine law of the H1 field T (PKs: the mass the perfusion law of the same field).  "Balanced":
alpha = s (1 + 0.1 sin 3x) with s = max diag K / max diag M_1 from the oracle, so that neither half of
M + K hides behind the other.
"""
import numpy as np

import ecm2_amd as E
import oracle as O
import bioheat as BH
import hp_ref as HP
from helpers import GOLDEN, alpha_bioheat, k_of_T, nonaligned, temperature

K_AFF = (0.05, 0.0012, 37.0)        # AffineGridFunctionCoefficient(T, scale, slope, t_ref)
STATES = ("random", "celsius", "kelvin", "linear")
STRUCTURED, ENTITY = E.NUMBERING_STRUCTURED, E.NUMBERING_ENTITY


def _moved(m, amp, seed):
    """Interior vertices moved: genuinely trilinear (non-affine) hexes."""
    V = m.vertices()
    inner = np.all((V > 1e-9) & (V < V.max(0) - 1e-9), axis=1)
    V[inner] += amp * np.random.default_rng(seed).uniform(-1, 1, (int(inner.sum()), 3))
    m.set_vertices(V)
    return m


def _sheared(m):
    m.set_vertices(nonaligned(m.vertices()))
    return m


def _fichera_r1():
    m = E.Mesh(f"{GOLDEN}/fichera.mesh")
    m.UniformRefinement()
    return m


MESHES = {
    "na543": lambda: _sheared(E.Mesh.MakeCartesian3D(5, 4, 3)),                  # 60 el: a ragged block
    "na885": lambda: _sheared(E.Mesh.MakeCartesian3D(8, 8, 5, 1.0, 0.8, 0.6)),   # 4 bricks + leftovers
    "fichera_r1": _fichera_r1,                                                   # 56 el, unstructured
    "tri865": lambda: _moved(E.Mesh.MakeCartesian3D(8, 6, 5), 0.02, 5),          # 240 el, trilinear
    "lat8": lambda: _moved(E.Mesh.MakeCartesian3D(8, 8, 8), 0.15 / 8, 9),        # every block a brick
    "box8": lambda: E.Mesh.MakeCartesian3D(8, 8, 8, 1.0, 0.7, 1.3),
    "box8_sfc": lambda: E.Mesh.MakeCartesian3D(8, 8, 8, 1.0, 0.7, 1.3, sfc_ordering=True),
    "na645": lambda: _sheared(E.Mesh.MakeCartesian3D(6, 4, 5)),                  # 2 x 2 x 1 bricks + leftovers
    "cart4": lambda: E.Mesh.MakeCartesian3D(4, 4, 4),                            # axis-aligned bricks
    "cart448": lambda: E.Mesh.MakeCartesian3D(4, 4, 8),                          # two z-slabs of 4 layers
}
AFFINE_MESHES = {"na543", "na885", "fichera_r1", "box8", "box8_sfc", "na645", "cart4", "cart448"}


def mid_gap_stop(Tq, lo=45.0, hi=55.0):
    """A shut-down temperature in the middle of the widest gap of the point temperatures in (lo, hi):
    no point sits on the perfusion law's discontinuity, so rounding cannot flip a side."""
    ts = np.unique(Tq.ravel())
    gaps = np.diff(ts)
    mid = np.argmax(gaps * ((ts[:-1] > lo) & (ts[1:] < hi)))
    return float(0.5 * (ts[mid] + ts[mid + 1]))


class Space:
    def __init__(self, name, p, numbering, mesh=None):
        self.name, self.p, self.numbering = name, p, numbering
        if mesh is None:
            self.mesh = MESHES[name]()
            self.fes = E.H1Space(self.mesh, p, numbering)
            self.en, self.gm, self.ndofs = self.mesh.element_nodes(), self.fes.gather_map(), self.fes.ndofs
            self.X = self.fes.dof_coords()
        else:                       # an oracle-side mesh (oracle.cartesian_mesh): no product code at all
            self.mesh = self.fes = None
            self.en, self.gm, self.ndofs, self.X = mesh
        self.ne = self.gm.shape[0]
        self.q1d = O.default_q1d(p)
        self.P = O.quad_points(self.en, self.q1d)                   # [ne][nq][3]
        T = temperature(self.X)
        self.T = T
        self.x = {"random": np.random.default_rng(1000 + p).uniform(-1, 1, self.ndofs),
                  "celsius": T,
                  "kelvin": T + 273.15,
                  "linear": 310.15 + self.X @ np.array([0.3, -1.1, 0.7])}
        self.beta_q = k_of_T(temperature(self.P))
        self._a1 = 1.0 + 0.1 * np.sin(3.0 * self.P[..., 0])
        self._forms = {}

    def _oracle(self, alpha, beta):
        return O.OracleOperator(self.en, self.gm, self.ndofs, self.p, alpha=alpha, beta=beta)

    def _balanced(self, beta):
        s = self._oracle(None, beta).diagonal().max() / self._oracle(self._a1, None).diagonal().max()
        return float(s)

    def form(self, fname):
        """dict(alpha, beta: the oracle's float64 coefficients; mass, diff: what the device form is
        given -- ("quad", values) or a law of T; hp: the HPRef; y_hp, S: per state; d_hp, dS)."""
        if fname in self._forms:
            return self._forms[fname]
        f = {"mass": None, "diff": None, "alpha": None, "beta": None}
        a_hp = b_hp = None
        if fname in ("K", "MK", "MKphys"):
            f["beta"] = b_hp = self.beta_q
            f["diff"] = ("quad", self.beta_q)
        if fname in ("M", "MK"):
            f["alpha"] = a_hp = self._balanced(self.beta_q) * self._a1
            f["mass"] = ("quad", f["alpha"])
        if fname == "MKphys":
            f["alpha"] = a_hp = alpha_bioheat(self.P)
            f["mass"] = ("quad", f["alpha"])
        if fname in ("Ks", "MKs", "PKs"):
            base = HP.HPRef(self.en, self.gm, self.ndofs, self.p, self.q1d)   # tables + geometry only
            Tq = BH.temperature_at_quadrature(self.T, self.gm, self.p, self.q1d)
            f["beta"] = BH.affine_law(Tq, *K_AFF)
            f["diff"] = ("affine",) + K_AFF
            b_hp = HP.beta_from_field(base, self.T, f["diff"])
            s = self._balanced(f["beta"])
            if fname == "MKs":
                f["alpha"] = a_hp = s * self._a1
                f["mass"] = ("quad", f["alpha"])
            elif fname == "PKs":
                par = (s, s, 0.5, 0.02, 37.0, mid_gap_stop(Tq))
                f["alpha"] = BH.perfusion_law(Tq, *par)
                f["mass"] = ("perfusion",) + par
                a_hp = HP.beta_from_field(base, self.T, f["mass"])
        assert f["mass"] is not None or f["diff"] is not None, fname
        hp = HP.HPRef(self.en, self.gm, self.ndofs, self.p, self.q1d, alpha=a_hp, beta=b_hp)
        f["hp"] = hp
        f["y_hp"] = {s: hp.mult(self.x[s]) for s in STATES}
        f["S"] = {s: hp.bound(self.x[s]) for s in STATES}
        f["d_hp"], f["dS"] = hp.diagonal(), hp.diagonal_bound()
        self._forms[fname] = f
        return f

    def oracle(self, fname):
        f = self.form(fname)
        return self._oracle(f["alpha"], f["beta"])


def space(name, p, numbering=ENTITY):
    return HP.cached(("space", name, p, numbering), lambda: Space(name, p, numbering))


def oracle_space(nx, ny, nz, p, transform=None, tag="cart"):
    """A space on the oracle's own cartesian_mesh (lattice numbering)."""
    key = ("ospace", tag, nx, ny, nz, p)
    return HP.cached(key, lambda: Space("%s%d%d%d" % (tag, nx, ny, nz), p, None,
                                        mesh=O.cartesian_mesh(nx, ny, nz, order=p, transform=transform)))


# ---- the device cases ---------------------------------------------------------------------------
VOLUME = ("K", "M", "MK")


class Case:
    def __init__(self, cid, mesh, p, forms=VOLUME, numbering=ENTITY, kernel=E.KERNEL_AUTO, resolved=None, **kw):
        self.id, self.mesh, self.p, self.forms, self.numbering = cid, mesh, p, tuple(forms), numbering
        # lattice: every block a lattice brick; snapshot: the k(T) snapshot kernel; group: n z-slabs
        self.flags = {k: kw.pop(k) for k in ("lattice", "snapshot", "group") if k in kw}
        self.kernel, self.kw = kernel, kw           # kw: BilinearForm's own arguments
        # the kernel mode AUTO resolves to, which info()["kernel"] must report
        self.resolved = resolved if resolved is not None else (
            kernel if kernel != E.KERNEL_AUTO else (E.KERNEL_TPE if p <= 2 else E.KERNEL_LINE))

    def layout(self, fname):
        """The qdata layout the form must report (PAForm::resolve_layout): the compressed layouts for
        the fused kernels whenever a DiffusionIntegrator is present; a mass-only form keeps its 8-byte
        stream; the workgroup-per-element and unfused kernels read the reference's layout."""
        if self.resolved in (E.KERNEL_WPE, E.KERNEL_UNFUSED):
            return E.QLAYOUT_NATIVE
        tpe = self.resolved == E.KERNEL_TPE
        if self.kw.get("compress_geometry", True) and fname != "M":
            if self.mesh in AFFINE_MESHES:
                return E.QLAYOUT_AFFINE if tpe else E.QLAYOUT_AFFINE_E
            return E.QLAYOUT_TRILINEAR if tpe else E.QLAYOUT_TRILINEAR_E
        return E.QLAYOUT_BLOCKED if tpe else E.QLAYOUT_NATIVE


SNAP = ("Ks", "MKs", "PKs")
CASES = [
    # thread-per-element, BLOCKED (full per-point qdata), generic map, a ragged last block
    Case("tpe-blocked-p1", "na543", 1, kernel=E.KERNEL_TPE, compress_geometry=False),
    Case("tpe-blocked-p2", "na543", 2, VOLUME + ("MKphys",), kernel=E.KERNEL_TPE, compress_geometry=False),
    # AFFINE: in-wave + cross-wave face merge, bricks + leftovers; unstructured valence
    Case("tpe-affine-bricks-p1", "na885", 1),
    Case("tpe-affine-bricks-p2", "na885", 2, VOLUME + ("MKphys",)),
    Case("tpe-affine-fichera-p1", "fichera_r1", 1),
    Case("tpe-affine-fichera-p2", "fichera_r1", 2),
    # TRILINEAR: the generic kernel, and the two-wave lattice kernel in both numberings
    Case("tpe-trilinear-p1", "tri865", 1),
    Case("tpe-trilinear-p2", "tri865", 2, VOLUME + ("MKphys",)),
    Case("tpe-trilinear-lattice-structured", "lat8", 2, numbering=STRUCTURED, lattice=True),
    Case("tpe-trilinear-lattice-entity", "lat8", 2, element_order="faces", lattice=True),
    # the coefficient-snapshot kernel (regular blocks / lattice-map blocks)
    Case("snapshot-structured", "box8", 2, SNAP, numbering=STRUCTURED, snapshot=True),
    Case("snapshot-entity-sfc", "box8_sfc", 2, SNAP, element_order="faces", snapshot=True),
    # line + brick kernels
    Case("line-affine-p3", "na645", 3, kernel=E.KERNEL_LINE),
    Case("line-affine-p4", "na645", 4, VOLUME + ("MKphys",), kernel=E.KERNEL_LINE),
    Case("line-affine-axis-p4", "cart4", 4, numbering=STRUCTURED),
    Case("line-trilinear-p3", "tri865", 3, kernel=E.KERNEL_LINE),
    Case("line-native-p3", "tri865", 3, kernel=E.KERNEL_LINE, compress_geometry=False),
    # workgroup-per-element and unfused
    Case("wpe-p2", "na543", 2, VOLUME + ("MKphys",), kernel=E.KERNEL_WPE),
    Case("wpe-p3", "na543", 3, kernel=E.KERNEL_WPE),
    Case("unfused-p2", "na543", 2, VOLUME + ("MKphys",), kernel=E.KERNEL_UNFUSED),
    Case("unfused-p3", "na543", 3, kernel=E.KERNEL_UNFUSED),
    # atomic scatter
    Case("tpe-atomic-p2", "na543", 2, ("MK",), kernel=E.KERNEL_TPE, scatter="atomic"),
    # loopback group: 2 z-slabs, OVERLAP decomposition, overlapped schedule
    Case("group-overlap-p2", "cart448", 2, VOLUME + ("MKphys",), group=2),
]
CASE_FORMS = [(c, f) for c in CASES for f in c.forms]


def case_id(v):
    return v.id if isinstance(v, Case) else str(v)


def reference_spaces():
    """Every (space, forms) c_ref is measured on: the device cases' spaces (each once) and, with no
    product code involved, the oracle's own cartesian_mesh -- the non-aligned 4^3 at p = 1, 2, 4 and the
    Cartesian 8^3 at p = 2."""
    seen = {}
    for c in CASES:
        key = (c.mesh, c.p, c.numbering)
        seen.setdefault(key, [])
        seen[key] += [f for f in c.forms if f not in seen[key]]
    out = [(space(*k), tuple(v)) for k, v in seen.items()]
    for p in (1, 2, 4):
        out.append((oracle_space(4, 4, 4, p, transform=nonaligned, tag="ona"), VOLUME + ("MKphys",)))
    out.append((oracle_space(8, 8, 8, 2), VOLUME + ("MKphys",)))
    return out
