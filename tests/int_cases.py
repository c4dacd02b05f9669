"""The case table of the integral kernel's paths (xtddft_amd/csrc/xt_int.hip), used three times:
tests/golden/make_int_ref.py computes a 40-digit reference of every case (tests/int_ref.py),
tests/test_int_cases.py checks on the host that every case runs the code it claims, that the
table is closed over what the kernel can be asked for, and the host routine against the
reference; tests/test_gpu_int_paths.py runs every case on the device against the fixture.

A case is one call of xt_int2e_cart: 1 to 4 bra shell pairs, 1 to 3 kets, 1 to 3 primitives
per shell (the thread-mapping case "map67" has 67 one-primitive pairs).  The tables are built
by hand from ints.ShellPair / ints.AuxShellSet with the packing rules of the header; inputs
are Cartesian and unnormalised, and a ket lists at most 6 of its components.  What a case
claims:
  paths   the code each of its quartets runs: "reg:lab,lc" (the compile-time instance
          quartet_cls<lab, lc>) or "rt" (the runtime path)
  bucket  8 (k_int_cart<8, 4>) or 13 (k_int_cart<13, 6>), from the *declared* lmax_orb / lket
  boys    the Boys branches its primitive quartets take: "table" (T < 30) and / or "erf"
  regime  for the one-primitive Boys cases, where T = alpha |P - C|^2 lands (REGIMES)
`twin` names the case with the same tables declared with lmax_orb = 3: the other bucket must
give the same bits.  lmax_orb and lket are never declared below what a table entry holds.
"""
from __future__ import annotations

import os
import zlib
from dataclasses import dataclass, field

import numpy as np

from xtddft_amd.qc.dints import POINT_CHARGE_EXP
from xtddft_amd.qc.gto import Shell
from xtddft_amd.qc import ints

# the 22 compile-time instances (lab, lc) of k_int_cart's switch
REGISTER = frozenset([(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (1, 0), (1, 1), (1, 2), (1, 3), (1, 4),
                      (2, 0), (2, 1), (2, 2), (2, 3), (2, 4), (3, 0), (3, 1), (3, 2), (3, 3),
                      (4, 0), (4, 1), (4, 2)])
# every (la, lb) the table uses for a bra of order lab
SPLITS = {0: [(0, 0)], 1: [(1, 0), (0, 1)], 2: [(1, 1), (2, 0), (0, 2)], 3: [(2, 1), (3, 0), (1, 2)],
          4: [(2, 2), (3, 1), (1, 3)], 5: [(3, 2), (2, 3)], 6: [(3, 3)]}
# the pair ket (l_c, l_d) of order lc
KET_SPLIT = {0: (0, 0), 1: (1, 0), 2: (1, 1), 3: (2, 1), 4: (2, 2), 5: (3, 2), 6: (3, 3)}
LAB_MAX, LC_MAX, L_MAX = 6, 7, 13
CLASSES = [(lab, lc) for lab in range(LAB_MAX + 1) for lc in range(LC_MAX + 1) if lab + lc <= L_MAX]

# Boys regimes: name -> (target T, predicate on the FP64 T the kernel computes)
BOYS_H = 0.05


def _node_dist(T):
    return abs(T - BOYS_H * np.floor(T / BOYS_H + 0.5))


REGIMES = {
    "zero": (0.0, lambda T: T == 0.0),
    "tiny": (1e-12, lambda T: 0.5e-12 < T < 2e-12),
    "node": (137 * BOYS_H, lambda T: T > 1.0 and T < 29.0 and _node_dist(T) < 1e-6),
    "mid": (57 * BOYS_H + 0.0249, lambda T: T < 29.9 and _node_dist(T) > 0.024),
    "last": (29.99, lambda T: 29.975 <= T < 30.0),
    "above": (30.05, lambda T: 30.0 <= T < 30.1),
    "t35": (35.0, lambda T: 34.0 < T < 36.0),
    "t500": (500.0, lambda T: 450.0 < T < 550.0),
    "huge": (2.5e5, lambda T: T > 1e5),
}
# classes of the regime cases: (la, lb), ket, declared (lmax_orb, lket)
REGIME_CLASSES = [
    ("r00", (0, 0), ("aux", 0), (0, 0)),          # register instance (0, 0)
    ("r22", (1, 1), ("aux", 2), (1, 2)),          # register instance (2, 2)
    ("r44", (2, 2), ("aux", 4), (2, 4)),          # runtime, bucket 8
    ("r35", (3, 0), ("aux", 5), (3, 5)),          # runtime, bucket 13
    ("r67", (3, 3), ("aux", 7), (3, 7)),          # L = 13
    ("r66", (3, 3), ("pair", 3, 3), (3, 6)),      # lab = lc = 6, the ket a shell pair
]
OMEGAS = (0.33, 1e-3, 1e3)
OMEGA_CLASSES = [("w00", (0, 0), 0, 1), ("w11", (1, 0), 1, 2), ("w44", (2, 2), 4, 2), ("w67", (3, 3), 7, 1)]
POINT_CHARGE_BRAS = [(0, 0), (1, 1), (2, 2), (3, 2), (3, 3)]          # lab = 0, 2, 4, 5, 6


def ncart(l):
    return (l + 1) * (l + 2) // 2


def ntuv(L):
    return (L + 1) * (L + 2) * (L + 3) // 6


@dataclass(frozen=True)
class Case:
    name: str
    bras: tuple                 # ((la, lb, na, nb), ...)
    kets: tuple                 # ("aux", l, nprim) | ("pair", lc, ld, nc, nd) | ("pc", Z)
    lmax_orb: int               # declared
    lket: int                   # declared
    paths: frozenset
    bucket: int
    boys: frozenset
    omega: float = 0.0
    regime: str = ""
    twin: str = ""              # same tables, declared lmax_orb = 3
    ref_of: str = ""            # a twin: the fixture entry it shares
    nc_max: int = 6
    pad: tuple = (0, 0, 0, 0)   # rows before, rows after, columns before, columns after the blocks
    spread: float = 0.8         # centres in [-spread, spread]^3
    tight: bool = False         # exponents up to ~60 (T on both sides of 30)

    @property
    def klass(self):
        """(lab, lc) of the case's first quartet: the parametrisation id."""
        la, lb = self.bras[0][:2]
        k = self.kets[0]
        lc = k[1] if k[0] == "aux" else k[1] + k[2] if k[0] == "pair" else 0
        return la + lb, lc


@dataclass
class Tables:
    pinfo: np.ndarray
    pprim: np.ndarray
    eab: np.ndarray
    kinfo: np.ndarray
    kprim: np.ndarray
    ek: np.ndarray
    nrow: int
    ldo: int
    omega: float
    lmax_orb: int
    lket: int
    blocks: list = field(default_factory=list)   # (k, j, row0, nab, col0, nc, lab, lc)

    def mask(self):
        """True where some block writes."""
        m = np.zeros((self.nrow, self.ldo), dtype=bool)
        for _, _, r0, nab, c0, nc, _, _ in self.blocks:
            m[r0:r0 + nab, c0:c0 + nc] = True
        return m


# --------------------------------------------------------------------------- the table
def _path(lab, lc):
    return f"reg:{lab},{lc}" if (lab, lc) in REGISTER else "rt"


def _ket_l(k):
    return k[1] if k[0] == "aux" else k[1] + k[2] if k[0] == "pair" else 0


def _bucket(lmax_orb, lket):
    return 8 if 2 * lmax_orb <= 4 and 2 * lmax_orb + lket <= 8 else 13


def _case(name, bras, kets, lmax_orb=None, lket=None, **kw):
    lo = max(max(b[0], b[1]) for b in bras) if lmax_orb is None else lmax_orb
    lk = max(_ket_l(k) for k in kets) if lket is None else lket
    paths = frozenset(_path(b[0] + b[1], _ket_l(k)) for b in bras for k in kets)
    kw.setdefault("boys", frozenset(["table"]))
    return Case(name, tuple(bras), tuple(kets), lo, lk, paths, _bucket(lo, lk), **kw)


def _nprim(i):
    return 1 + i % 3


def _build_table():
    cases = []
    # --- every class (lab, lc), every split, auxiliary and pair kets, both buckets
    for lab, lc in CLASSES:
        ncm = 6 if lab <= 3 else 3 if lab <= 5 else 2
        kets = [("aux", lc, _nprim(lab + lc))]
        if lc in KET_SPLIT:
            c, d = KET_SPLIT[lc]
            kets.append(("pair", c, d, 1 + (lab + lc) % 2, 1))
        lo_splits = [s for s in SPLITS[lab] if _bucket(max(s), lc) == 8]
        hi_splits = [s for s in SPLITS[lab] if _bucket(max(s), lc) == 13]

        def bras(splits):
            return [(la, lb, _nprim(la + lc), _nprim(lb + lab)) if la + lb + lc <= 9 else (la, lb, 1 + (la + lc) % 2, 1)
                    for la, lb in splits]
        if lo_splits:
            cases.append(_case(f"c{lab}{lc}_b8", bras(lo_splits), kets, nc_max=ncm, twin=f"c{lab}{lc}_b13"))
            cases.append(_case(f"c{lab}{lc}_b13", bras(lo_splits), kets, lmax_orb=3, nc_max=ncm,
                               ref_of=f"c{lab}{lc}_b8"))
        if hi_splits:
            cases.append(_case(f"c{lab}{lc}_hi", bras(hi_splits), kets, nc_max=ncm))
    # --- Boys regimes, one primitive per shell
    for tag, (la, lb), ket, (lo, lk) in REGIME_CLASSES:
        k = ("aux", ket[1], 1) if ket[0] == "aux" else ("pair", ket[1], ket[2], 1, 1)
        for reg, (T, _) in REGIMES.items():
            cases.append(_case(f"{tag}_{reg}", [(la, lb, 1, 1)], [k], lo, lk, regime=reg, nc_max=3,
                               boys=frozenset(["table" if T < 30.0 else "erf"])))
    # --- range separation: omega = 0.33 and the two limits of a' = alpha w^2 / (alpha + w^2)
    for tag, (la, lb), lc, npr in OMEGA_CLASSES:
        for w in OMEGAS:
            cases.append(_case(f"{tag}_w{w:g}", [(la, lb, npr, npr)], [("aux", lc, npr)], omega=w, nc_max=3))
    # --- point-charge kets (nuclear attraction): three charges, the first on the bra's centre A
    for la, lb in POINT_CHARGE_BRAS:
        cases.append(_case(f"pc{la + lb}", [(la, lb, 2, 1 + (la + lb) % 2)], [("pc", 8.0), ("pc", 1.0), ("pc", 6.0)],
                           boys=frozenset(["table", "erf"]), tight=True))
    # --- tight and far primitives: T on both sides of the switch inside one contraction
    cases.append(_case("far21", [(1, 1, 3, 2), (2, 0, 2, 2)], [("aux", 1, 3), ("aux", 3, 2)],
                       boys=frozenset(["table", "erf"]), tight=True, spread=2.0))
    cases.append(_case("far65", [(3, 3, 3, 2)], [("aux", 5, 3)], boys=frozenset(["table", "erf"]), tight=True,
                       spread=2.0, nc_max=3))
    # --- thread mapping: 67 quartets (a full wave and three lanes), register and runtime
    # quartets mixed inside the wave; and a block inside a larger, padded output
    cyc = [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (0, 1)]
    cases.append(_case("map67", [cyc[i % 7] + (1, 1) for i in range(67)], [("aux", 3, 1)], nc_max=3))
    cases.append(_case("ldo_pad", [(1, 1, 2, 1), (2, 1, 1, 2)], [("aux", 2, 2), ("pair", 1, 0, 2, 1)],
                       pad=(2, 3, 3, 4)))
    return cases


CASES = _build_table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# the cases that own a fixture entry (a twin shares its partner's)
REF_CASES = [c for c in CASES if not c.ref_of]
# the fixed subset the CPU suite regenerates with mpmath and compares with the committed file
REGEN = [c.name for c in REF_CASES if c.name.endswith("_b8") and c.klass[1] in (0, 3, 6)] + \
        [c.name for c in REF_CASES if c.regime and c.name[:3] in ("r00", "r35", "r66")] + \
        ["w11_w0.33", "w44_w0.001", "w44_w1000", "pc0", "pc5", "far21", "ldo_pad"]


# --------------------------------------------------------------------------- builders
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _shell(rng, l, nprim, center, tight=False):
    base = rng.uniform(0.35, 0.6)
    ratio = rng.uniform(2.2, 3.0) * (4.0 if tight else 1.0)
    exps = base * ratio ** np.arange(nprim)[::-1]
    coefs = rng.uniform(0.3, 1.0, nprim) * rng.choice([-1.0, 1.0], nprim)
    return Shell(0, l, np.asarray(center, dtype=np.float64), exps, coefs)


def _pick(ncomp, nc_max):
    """At most nc_max component indices of a ket, spread over the shell."""
    if ncomp <= nc_max:
        return np.arange(ncomp)
    return np.unique(np.round(np.linspace(0, ncomp - 1, nc_max)).astype(int))


def kernel_T(p, P, s, C, omega):
    """T of one primitive quartet in FP64, as k_int_cart writes it."""
    alpha = p * s / (p + s)
    if omega > 0.0:
        w2 = omega * omega
        alpha = alpha * w2 / (alpha + w2)
    X, Y, Z = P[0] - C[0], P[1] - C[1], P[2] - C[2]
    return alpha * (X * X + Y * Y + Z * Z)


def _regime_shells(c, rng):
    """One-primitive bra pair and ket whose T lands in the case's regime."""
    (la, lb, _, _), k = c.bras[0], c.kets[0]
    T = REGIMES[c.regime][0]
    if c.regime == "zero":
        # everything on one centre with dyadic coordinates and exponents: P = A = C exactly
        A = np.array([0.5, -0.25, 0.75])
        sa = Shell(0, la, A, np.array([1.5]), np.array([0.8]))
        sb = Shell(0, lb, A, np.array([0.75]), np.array([-0.6]))
        if k[0] == "aux":
            return sa, sb, (Shell(0, k[1], A, np.array([1.25]), np.array([0.7])),)
        return sa, sb, (Shell(0, k[1], A, np.array([2.0]), np.array([0.7])),
                        Shell(0, k[2], A, np.array([0.5]), np.array([0.9])))
    big = T > 100.0
    sa = _shell(rng, la, 1, rng.uniform(-0.6, 0.6, 3))
    sb = _shell(rng, lb, 1, sa.center + rng.uniform(-0.5, 0.5, 3))
    if big:     # tight primitives far apart
        sa.exps *= 6.0
        sb.exps *= 6.0
    bp = ints.ShellPair(sa, sb)
    u = np.array([0.48, -0.6, 0.64])
    u /= np.linalg.norm(u)
    if k[0] == "aux":
        sc = _shell(rng, k[1], 1, np.zeros(3))
        if big:
            sc.exps *= 6.0
        s = sc.exps[0]
        alpha = bp.p[0] * s / (bp.p[0] + s)
        sc.center = bp.P[0] + np.sqrt(T / alpha) * u
        return sa, sb, (sc,)
    sc = _shell(rng, k[1], 1, rng.uniform(-0.3, 0.3, 3))
    sd = _shell(rng, k[2], 1, sc.center + rng.uniform(-0.4, 0.4, 3))
    if big:
        sc.exps *= 6.0
        sd.exps *= 6.0
    kp = ints.ShellPair(sc, sd)
    alpha = bp.p[0] * kp.p[0] / (bp.p[0] + kp.p[0])
    shift = bp.P[0] + np.sqrt(T / alpha) * u - kp.P[0]
    sc.center = sc.center + shift
    sd.center = sd.center + shift
    return sa, sb, (sc, sd)


def build(c: Case) -> Tables:
    """The kernel tables of a case (deterministic: the geometry is seeded by the tables' name,
    so a case and its twin get the same numbers)."""
    rng = _rng(c.ref_of or c.name)
    pinfo, pprim, eab, kinfo, kprim, ek = [], [], [], [], [], []
    regime_ket = None
    row, q0, e0 = c.pad[0], 0, 0
    first_A = None
    rows = []
    for la, lb, na, nb in c.bras:
        if c.regime:
            sa, sb, regime_ket = _regime_shells(c, rng)
        else:
            sa = _shell(rng, la, na, rng.uniform(-c.spread, c.spread, 3), c.tight)
            sb = _shell(rng, lb, nb, sa.center + rng.uniform(-0.7, 0.7, 3), c.tight)
        first_A = sa.center if first_A is None else first_A
        sp = ints.ShellPair(sa, sb)
        nab = ncart(la) * ncart(lb)
        pinfo.append([la, lb, sp.p.size, q0, e0, row, 0, 0])
        pprim.append(np.column_stack([sp.p, sp.P]))
        eab.append(sp.Eab.ravel())
        rows.append((row, nab, la + lb))
        row += nab
        q0 += sp.p.size
        e0 += sp.Eab.size
    col, r0, e0 = c.pad[2], 0, 0
    cols = []
    for ik, k in enumerate(c.kets):
        if k[0] == "pc":
            ctr = first_A if ik == 0 else first_A + rng.uniform(-2.5, 2.5, 3)
            lc, p_k, P_k = 0, np.array([POINT_CHARGE_EXP]), ctr[None, :]
            E_k = np.array([[[-k[1] * (POINT_CHARGE_EXP / np.pi) ** 1.5]]])
        elif k[0] == "aux":
            sc = regime_ket[0] if c.regime else _shell(rng, k[1], k[2], rng.uniform(-c.spread, c.spread, 3), c.tight)
            a = ints.AuxShellSet([sc])
            lc, p_k, P_k = k[1], a.p, a.P
            E_k = a.Ek[_pick(ncart(lc), c.nc_max)]
        else:
            if c.regime:
                sc, sd = regime_ket
            else:
                sc = _shell(rng, k[1], k[3], rng.uniform(-c.spread, c.spread, 3), c.tight)
                sd = _shell(rng, k[2], k[4], sc.center + rng.uniform(-0.7, 0.7, 3), c.tight)
            kp = ints.ShellPair(sc, sd)
            lc, p_k, P_k = k[1] + k[2], kp.p, kp.P
            full = kp.Eab.reshape(ncart(k[1]) * ncart(k[2]), ntuv(lc), kp.p.size)
            E_k = full[_pick(full.shape[0], c.nc_max)]
        nc = E_k.shape[0]
        kinfo.append([lc, p_k.size, r0, e0, col, nc, 0, 0])
        kprim.append(np.column_stack([p_k, P_k]))
        ek.append(np.ascontiguousarray(E_k).ravel())
        cols.append((col, nc, lc))
        col += nc
        r0 += p_k.size
        e0 += E_k.size
    tb = Tables(np.array(pinfo, dtype=np.int32), np.concatenate(pprim), np.concatenate(eab),
                np.array(kinfo, dtype=np.int32), np.concatenate(kprim), np.concatenate(ek),
                row + c.pad[1], col + c.pad[3], c.omega, c.lmax_orb, c.lket)
    for j, (c0, nc, lc) in enumerate(cols):
        for k, (rw, nab, lab) in enumerate(rows):
            tb.blocks.append((k, j, rw, nab, c0, nc, lab, lc))
    return tb


def quartet_T(tb: Tables):
    """The FP64 T of every primitive quartet of the call."""
    out = []
    for k, j, *_ in tb.blocks:
        _, _, npp, pq0 = tb.pinfo[k][:4]
        _, nr, ar0 = tb.kinfo[j][:3]
        for q in range(pq0, pq0 + npp):
            for r in range(ar0, ar0 + nr):
                out.append(kernel_T(tb.pprim[q, 0], tb.pprim[q, 1:], tb.kprim[r, 0], tb.kprim[r, 1:], tb.omega))
    return np.array(out)


# --------------------------------------------------------------------------- the host routine
def host_int2e(tb: Tables, diag=False):
    """The host FP64 path on the same tables: the formula of ints.eri_quartet / ints.eri3c
    (ints.hermite_r, ints._attenuate, ints._sum_table and their two contractions), applied
    block by block to hand-built tables -- which may list a subset of a ket's components or
    a point charge, so the shell objects those routines take do not exist."""
    out = np.zeros((tb.nrow, tb.ldo))
    for k, j, row0, nab, col0, nc, lab, lc in tb.blocks:
        if diag and k != j:
            continue
        _, _, npp, pq0, pe0 = (int(x) for x in tb.pinfo[k][:5])
        _, nr, ar0, ae0 = (int(x) for x in tb.kinfo[j][:4])
        E = tb.eab[pe0:pe0 + nab * ntuv(lab) * npp].reshape(nab, ntuv(lab), npp)
        K = tb.ek[ae0:ae0 + nc * ntuv(lc) * nr].reshape(nc, ntuv(lc), nr)
        p = tb.pprim[pq0:pq0 + npp, 0][:, None]
        s = tb.kprim[ar0:ar0 + nr, 0][None, :]
        alpha, scale = ints._attenuate(p * s / (p + s), tb.omega)
        d = tb.pprim[pq0:pq0 + npp, None, 1:] - tb.kprim[None, ar0:ar0 + nr, 1:]
        R = ints.hermite_r(lab + lc, alpha, d[..., 0], d[..., 1], d[..., 2])
        pref = 2.0 * np.pi ** 2.5 / (p * s * np.sqrt(p + s)) * scale
        idx, sign = ints._sum_table(lab, lc)
        X = np.einsum('tsPQ,s,csQ->tcP', R[idx] * pref, sign, K, optimize=True)
        out[row0:row0 + nab, col0:col0 + nc] += np.einsum('atP,tcP->ac', E, X, optimize=True)
    return out


# --------------------------------------------------------------------------- the fixture
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE_MAX_BYTES = 464 * 1000


def fixture_files():
    return sorted(os.path.join(GOLDEN, f) for f in os.listdir(GOLDEN)
                  if f.startswith("int_ref") and f.endswith(".npz"))


def load_fixture():
    """Every array of tests/golden/int_ref*.npz (the fixture is split to keep each file small)."""
    d = {}
    for f in fixture_files():
        with np.load(f, allow_pickle=False) as z:
            d.update({k: z[k] for k in z.files})
    return d


# --------------------------------------------------------------------------- the bound
U = 2.0 ** -53
KAPPA_FACTOR, KAPPA_FLOOR = 8.0, 64.0


def measured_ratio(val, ref, sabs, Lmap):
    """Largest |val - ref| / (2^-53 sabs) per total order L (length L_MAX + 1; 0 where no
    element has that order); elements with sabs == 0 must be exact zeros."""
    out = np.zeros(L_MAX + 1)
    live = (Lmap >= 0) & (sabs > 0)
    assert np.all(val[(Lmap >= 0) & (sabs == 0)] == 0.0)
    r = np.abs(val[live] - ref[live]) / (U * sabs[live])
    np.maximum.at(out, Lmap[live], r)
    return out


def kappa_from(measured):
    return np.maximum(KAPPA_FLOOR, KAPPA_FACTOR * np.asarray(measured))


# --------------------------------------------------------------------------- xt_eval_ao
AO_BASIS = {
    "O": [[0, [11.0, 0.3], [2.4, 0.6], [0.55, 0.5]], [1, [1.3, 1.0]], [2, [6.0, 0.2], [1.7, 0.7], [0.5, 0.4]],
          [3, [0.9, 1.0]], [4, [3.1, 0.3], [1.2, 0.6], [0.6, 0.4]]],
    "H": [[0, [0.7, 1.0]], [1, [4.0, 0.25], [1.1, 0.6], [0.5, 0.5]], [2, [0.8, 1.0]],
          [3, [2.6, 0.3], [1.0, 0.7], [0.5, 0.3]], [4, [0.75, 1.0]]],
}
AO_CENTRES = [("O", (0.25, -0.5, 0.125)), ("H", (1.5, 0.75, -0.625))]
AO_C_FACTOR, AO_C_FLOOR = 8.0, 16.0


def ao_mol():
    """s to g shells of 1 and 3 primitives on two centres (10 shells, 50 AOs)."""
    from xtddft_amd.qc import M
    return M(AO_CENTRES, basis=AO_BASIS, spin=1, unit="Bohr")


def ao_points():
    """301 points (301 x 10 shells is no multiple of 256): both centres, the axes and planes
    through them, 1e-8 from them, a cloud, and points where every exponential underflows.
    Returns (coords, index array of the underflow points)."""
    ctr = np.array([c for _, c in AO_CENTRES])
    pts = []
    e = np.eye(3)
    for c in ctr:
        pts.append(c)
        for a in range(3):
            for h in (0.75, -1.5):
                pts.append(c + h * e[a])                         # on an axis: two offsets vanish
            b, d = (a + 1) % 3, (a + 2) % 3
            pts.append(c + 0.5 * e[b] - 1.25 * e[d])             # in a plane: one offset vanishes
            pts.append(c - 0.875 * e[b] + 0.375 * e[d])
            pts.append(c + 1e-8 * e[a])
        pts.append(c + 1e-8 * np.array([0.6, -0.64, 0.48]))
    rng = np.random.default_rng(20240607)
    far = []
    for v in rng.normal(size=(8, 3)):
        far.append(ctr[0] + 60.0 * v / np.linalg.norm(v))         # 0.5 x 58^2 > 745: exp underflows
    ncloud = 301 - len(pts) - len(far)
    cloud = ctr[rng.integers(0, 2, ncloud)] + rng.normal(size=(ncloud, 3)) * rng.choice([0.3, 1.5, 5.0], (ncloud, 1))
    coords = np.concatenate([np.array(pts), cloud, np.array(far)])
    assert coords.shape == (301, 3)
    return np.ascontiguousarray(coords), np.arange(301 - len(far), 301)


# --------------------------------------------------------------------------- diag / screening
def pair_ket_tables():
    """Five mixed shell pairs as bra and as ket -- the tables of the integral-direct Cholesky
    (qc/dints.py ket_info_pairs): ket_info rows built from the pair entries, ket_prim = pair_prim,
    ek = eab.  Returns (Tables of the full (pairs | pairs) call, ket_info of the diag = 1 call
    with column offset 0, ldo of the diagonal call).  Declared lmax_orb = 2, lket = 4: register
    quartets ((0 0|0 0) ...) and runtime ones ((2 2|2 2), L = 8) in k_int_cart<8, 4>."""
    c = _case("pairs5", [(0, 0, 2, 1), (1, 0, 1, 2), (1, 1, 2, 2), (2, 1, 1, 1), (2, 2, 1, 2)], [("aux", 0, 1)])
    tb = build(c)
    nab = np.array([ncart(r[0]) * ncart(r[1]) for r in tb.pinfo])
    kinfo = np.zeros((5, 8), dtype=np.int32)
    kinfo[:, 0] = tb.pinfo[:, 0] + tb.pinfo[:, 1]
    kinfo[:, 1:4] = tb.pinfo[:, 2:5]
    kinfo[:, 4] = np.concatenate([[0], np.cumsum(nab)[:-1]])
    kinfo[:, 5] = nab
    nrow = int(nab.sum())
    full = Tables(tb.pinfo, tb.pprim, tb.eab, kinfo, tb.pprim, tb.eab, nrow, nrow, 0.0, 2, 4)
    for j in range(5):
        for k in range(5):
            full.blocks.append((k, j, int(tb.pinfo[k, 5]), int(nab[k]), int(kinfo[j, 4]), int(nab[j]),
                                int(kinfo[k, 0]), int(kinfo[j, 0])))
    kdiag = kinfo.copy()
    kdiag[:, 4] = 0
    return full, kdiag, int(nab.max())


# Schwarz bounds of the five pairs (powers of two: every product is exact) and the threshold:
# products below 0.25 are skipped, products equal to it (0.5 x 0.5, 1 x 0.25, 2 x 0.125) are kept
SCREEN_Q = np.array([1.0, 0.5, 0.25, 2.0, 0.125])
SCREEN_THR = 0.25
