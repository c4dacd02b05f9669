"""The case table of the derivative-ERI gradient kernel (xtddft_amd/csrc/xt_grad.hip), used three
times: tests/golden/make_grad_kappa.py measures the multiplier of the bound from the host
restatement of every case, tests/test_grad_cases.py checks on the host that every case runs the
code it claims and that the table is closed over what ``grad_jk`` can launch, and
tests/test_gpu_grad_paths.py runs every case on the device against ``hint_ref.ref_grad``.

A case is one raw call of ``xt_grad_jk`` built by hand: bra rows are ordered DerivPair entries of
shells from ``hint_ref.shell`` (Cartesian, 1 or 3 primitives, the four centres of that module,
some coincident), kets are plain ShellPair entries; equal rows share one prim / E block.  The
"atom" column of ``bra_ao`` is only an output row index: unless a case says otherwise row k goes
to output row k (natm = nbra), so every bra entry is resolved on its own.  Every bra row and
every ket owns a disjoint range of Cartesian AOs in P / Q (``nao`` is larger than what is used),
and every element of P and Q the kernel has no reason to read is NaN.  P, Q hold integers in
[-4, 4] divided by 4 and the weights are from {+-1, +-0.5, +-2, 0}: every Gamma element is exact
in float64 in any summation order.

What a case claims (checked by tests/test_grad_cases.py against a restatement of the dispatch):
  inst    the template instance (MAXL, MAXLB), from the *declared* (lbra, lket)
  cache   "c" where a (bra row, ket) block is kept in the per-thread Gamma cache (nab ncol <= 81),
          "u" where Gamma is recomputed per element
  image   "i" where a ket adds its (d, c) image, "n" where it does not
  strips  (number of strips, kets of the last strip)
  blocks  thread blocks of 64
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from hint_ref import shell

CACHE = 81                      # kGradCache
INSTANCES = ((6, 4), (10, 6), (14, 8))
WEIGHTS = (1.0, -1.0, 0.5, -0.5, 2.0, -2.0)
GAP = 1                         # unused AOs between two ranges


def ncart(l):
    return (l + 1) * (l + 2) // 2


@dataclass(frozen=True)
class Bra:
    la: int
    lb: int
    na: int = 1
    nb: int = 1
    ca: int = 0
    cb: int = 1
    atom: int = -1              # -1: the row's own index
    ncb0: bool = False          # write 0 into bra_ao[..][2] (the kernel's ncb <= 0 -> 1 fallback)

    @property
    def order(self):
        return self.la + self.lb + 1

    @property
    def nab(self):
        return ncart(self.la) * ncart(self.lb)

    @property
    def block(self):
        return (self.la, self.lb, self.na, self.nb, self.ca, self.cb)


@dataclass(frozen=True)
class Ket:
    lc: int
    ld: int
    nc: int = 1
    nd: int = 1
    cc: int = 2
    cd: int = 3
    same: bool = False          # c and d are one shell (a diagonal pair): no image
    image: int = -1             # -1: the pair table's rule (1 when c != d)
    ncd0: bool = False

    @property
    def order(self):
        return self.lc + self.ld

    @property
    def ncol(self):
        return ncart(self.lc) * ncart(self.ld)

    @property
    def flag(self):
        return int(not self.same) if self.image < 0 else self.image

    @property
    def block(self):
        return (self.lc, self.ld, self.nc, self.nd, self.cc, self.cd, self.same)


@dataclass(frozen=True)
class Case:
    name: str
    bras: tuple
    kets: tuple
    lbra: int                   # declared
    lket: int                   # declared
    nterm: int
    strip: int
    natm: int
    inst: tuple
    cache: frozenset
    image: frozenset
    strips: tuple
    blocks: int
    zero_w: tuple = ()          # (term, "j" | "k"): weights set to 0
    out0: bool = False          # `out` starts from non-zero values
    kets_first: bool = False    # the kets' AO ranges come before the bras'
    ref_of: str = ""            # same tables, densities and reference as that case
    probe: bool = False         # a class case: four rows of one block against one ket

    @property
    def klass(self):
        return self.bras[0].order, self.kets[0].order


@dataclass
class Call:
    """The arrays of one xt_grad_jk call."""
    binfo: np.ndarray
    bprim: np.ndarray
    eb: np.ndarray
    bra_ao: np.ndarray
    kinfo: np.ndarray
    kprim: np.ndarray
    ek: np.ndarray
    ket_ao: np.ndarray
    lbra: int
    lket: int
    wj: np.ndarray
    wk: np.ndarray
    P: np.ndarray
    Q: np.ndarray
    nao: int
    strip: int
    natm: int
    out0: np.ndarray
    pmask: np.ndarray = field(repr=False, default=None)     # where the kernel may read P / Q
    qmask: np.ndarray = field(repr=False, default=None)

    @property
    def nstrip(self):
        return (len(self.kinfo) + self.strip - 1) // self.strip

    @property
    def nwork(self):
        return 3 * len(self.binfo) * (self.nstrip + 1)


# --------------------------------------------------------------------------- the dispatch, as claimed
def _inst(lbra, lket):
    if lbra <= 4 and lbra + lket <= 6:
        return (6, 4)
    if lbra <= 6 and lbra + lket <= 10:
        return (10, 6)
    return (14, 8)


def _strips(nket, strip):
    nstrip = (nket + strip - 1) // strip
    return nstrip, len(range(nstrip - 1, nket, nstrip))


def _case(name, bras, kets, lbra=None, lket=None, nterm=2, strip=None, natm=None, claim=None, **kw):
    bras, kets = tuple(bras), tuple(kets)
    lbra = max(b.order for b in bras) if lbra is None else lbra
    lket = max(k.order for k in kets) if lket is None else lket
    strip = len(kets) if strip is None else strip
    natm = len(bras) if natm is None else natm
    nstrip, last = _strips(len(kets), strip)
    c = Case(name, bras, kets, lbra, lket, nterm, strip, natm, _inst(lbra, lket),
             frozenset("c" if b.nab * k.ncol <= CACHE else "u" for b in bras for k in kets),
             frozenset("i" if k.flag else "n" for k in kets), (nstrip, last),
             (len(bras) * nstrip + 63) // 64, **kw)
    for key, want in (claim or {}).items():      # the claims written out by hand, where a case is about them
        got = getattr(c, key)
        assert got == (frozenset(want) if isinstance(got, frozenset) else want), (name, key, got, want)
    return c


# (la, lb) of a bra of order la + lb + 1 and (lc, ld) of a ket of order lc + ld; a class (ob, ok)
# takes bra split ok mod n and ket split ob mod n, which puts every l at every position
BRA_SPLITS = {1: [(0, 0)], 2: [(1, 0), (0, 1)], 3: [(1, 1), (2, 0), (0, 2)], 4: [(2, 1), (3, 0), (1, 2), (0, 3)],
              5: [(2, 2), (3, 1), (1, 3)], 6: [(3, 2), (2, 3)], 7: [(3, 3)]}
KET_SPLITS = {0: [(0, 0)], 1: [(1, 0), (0, 1)], 2: [(1, 1), (2, 0), (0, 2)], 3: [(2, 1), (3, 0), (1, 2), (0, 3)],
              4: [(2, 2), (3, 1), (1, 3)], 5: [(3, 2), (2, 3)], 6: [(3, 3)]}
CLASSES = [(ob, ok) for ob in range(1, 8) for ok in range(7)]
CENTRE_SETS = [(0, 1, 2, 3), (0, 0, 1, 2), (1, 0, 3, 2), (2, 3, 3, 0)]


def _class_case(ob, ok):
    la, lb = BRA_SPLITS[ob][ok % len(BRA_SPLITS[ob])]
    lc, ld = KET_SPLITS[ok][ob % len(KET_SPLITS[ok])]
    L = ob + ok
    # 1 and 3 primitives on both sides up to L = 7, one contracted shell up to 10, none above
    if L <= 7:
        npr = [(3, 1, 1, 3), (1, 3, 3, 1)][L % 2]
    elif L <= 10:
        npr = [(1, 1, 3, 1), (3, 1, 1, 1)][L % 2]
    else:
        npr = (1, 1, 1, 1)
    ca, cb, cc, cd = CENTRE_SETS[(ob + 2 * ok) % 4]
    same = lc == ld and (ob + ok) % 2 == 0          # a diagonal pair (c = d, no image) on every other class
    ket = Ket(lc, ld, npr[2], npr[2] if same else npr[3], cc, cc if same else cd, same=same)
    return _case(f"c{ob}{ok}", [Bra(la, lb, npr[0], npr[1], ca, cb)] * 4, [ket], nterm=1 + (ob + ok) % 2,
                 zero_w=((0, "k"),) if (ob + ok) % 3 == 0 else (), kets_first=bool(ok % 2), probe=True)


def _build_table():
    cases = [_class_case(ob, ok) for ob, ok in CLASSES]
    # --- a small class declared with larger bounds: the other two instances, cached, with and without image
    for ob, ok in ((2, 1), (2, 0)):
        for tag, (lb_, lk_) in (("d", (6, 4)), ("f", (8, 6))):
            base = cases[CLASSES.index((ob, ok))]
            cases.append(_case(f"c{ob}{ok}_{tag}", base.bras, base.kets, lb_, lk_, nterm=base.nterm, zero_w=base.zero_w,
                               kets_first=base.kets_first, probe=True, ref_of=base.name,
                               claim=dict(inst=(10, 6) if tag == "d" else (14, 8), cache="c")))
    # --- the cache threshold nab ncol <= 81, and twins whose strip alternates cached and uncached kets
    pp, pp2 = Ket(1, 1, 3, 1, 2, 3), Ket(1, 1, 1, 1, 3, 3, same=True)
    dp_ket, ds_ket = Ket(2, 1, 1, 1, 3, 1), Ket(2, 0, 1, 3, 2, 3)
    ds_bra, pp_bra, dp_bra = Bra(2, 0, 1, 3, 0, 1), Bra(1, 1, 3, 1, 0, 1), Bra(2, 1, 1, 1, 0, 1)
    cases += [
        _case("cth54", [ds_bra, ds_bra], [pp], claim=dict(inst=(6, 4), cache="c", image="i")),
        _case("cth81", [pp_bra, pp_bra], [pp], claim=dict(inst=(6, 4), cache="c")),
        _case("cth108", [dp_bra, dp_bra], [ds_ket], claim=dict(inst=(6, 4), cache="u")),
        _case("cth162", [dp_bra, dp_bra], [pp], claim=dict(inst=(6, 4), cache="u")),
        _case("cth54_twin", [ds_bra, ds_bra], [pp, dp_ket, pp2], strip=3,
              claim=dict(inst=(6, 4), cache="cu", strips=(1, 3))),
        _case("cth81_twin", [pp_bra, pp_bra], [pp, dp_ket, pp2], strip=3, nterm=1,
              claim=dict(inst=(6, 4), cache="cu", strips=(1, 3))),
    ]
    # --- the image: c != d with the flag cleared gives the one-sided sum
    cases.append(_case("img_off", [Bra(1, 0, 1, 3, 0, 1), Bra(0, 1, 3, 1, 1, 0)], [Ket(1, 0, 3, 1, 2, 3, image=0)],
                       claim=dict(image="n")))
    # --- ncb / ncd written as 0 on s-s entries
    cases.append(_case("ncb0", [Bra(0, 0, 3, 1, 0, 1, ncb0=True), Bra(0, 0, 1, 1, 2, 2)],
                       [Ket(0, 0, 1, 3, 2, 3, ncd0=True), Ket(0, 0, 1, 1, 1, 1, same=True, ncd0=True)]))
    # --- nterm = 1, 2, 8 with zero weights
    tb, tk = [Bra(1, 0, 1, 3, 0, 1), Bra(1, 1, 1, 1, 2, 0)], [Ket(1, 0, 3, 1, 2, 3), Ket(1, 1, 1, 1, 1, 1, same=True)]
    cases += [
        _case("nterm1", tb, tk, nterm=1),
        _case("nterm2", tb, tk, nterm=2, zero_w=((0, "j"), (1, "k"))),
        _case("nterm8", tb, tk, nterm=8, zero_w=((1, "j"), (2, "k"), (5, "j"), (6, "k"))),
    ]
    # --- centres: a, b on one centre; all four shells on one centre (the origin: exact zeros)
    cases += [
        _case("ab_one", [Bra(1, 2, 1, 3, 1, 1), Bra(2, 0, 1, 1, 3, 3)], [Ket(1, 0, 1, 1, 2, 0)]),
        _case("onec_s", [Bra(0, 0, 3, 1, 0, 0)] * 2, [Ket(0, 0, 1, 3, 0, 0)]),
        _case("onec_pd", [Bra(1, 2, 1, 1, 0, 0), Bra(2, 1, 1, 3, 0, 0)], [Ket(1, 1, 1, 1, 0, 0, same=True), Ket(2, 0, 1, 1, 0, 0)]),
    ]
    # --- the thread map: 70 rows of four shared s / p blocks against 5 kets
    cyc = [Bra(0, 0, 3, 1, 0, 1), Bra(1, 0, 1, 1, 1, 2), Bra(0, 1, 1, 3, 2, 0), Bra(1, 1, 1, 1, 3, 1)]
    rows = [cyc[(i * i + i // 7) % 4] for i in range(70)]
    mk = [Ket(0, 0, 3, 3, 1, 1, same=True), Ket(1, 0, 1, 1, 2, 3), Ket(1, 1, 1, 1, 0, 0, same=True), Ket(0, 1, 1, 3, 3, 0),
          Ket(1, 1, 1, 1, 2, 1)]
    cases.append(_case("map70", rows, mk, strip=2, nterm=2,
                       claim=dict(inst=(6, 4), cache="c", strips=(3, 1), blocks=4)))
    for strip, nst, last, nblk in ((1, 5, 1, 6), (5, 1, 5, 2), (1000, 1, 5, 2)):
        cases.append(_case(f"map70_s{strip}", rows, mk, strip=strip, nterm=2, ref_of="map70",
                           claim=dict(strips=(nst, last), blocks=nblk)))
    # --- the fold: rows sharing an atom, atoms without a row, natm above every index, out += from non-zero
    fb = [Bra(1, 0, 1, 1, 0, 1, atom=2), Bra(0, 0, 3, 1, 1, 2, atom=0), Bra(1, 1, 1, 1, 2, 3, atom=2),
          Bra(2, 0, 1, 1, 3, 0, atom=5), Bra(0, 1, 1, 3, 0, 2, atom=0), Bra(0, 0, 1, 1, 1, 3, atom=2)]
    fk = [Ket(1, 0, 1, 1, 2, 3), Ket(0, 0, 3, 1, 0, 0, same=True), Ket(1, 1, 1, 1, 1, 3)]
    cases.append(_case("fold", fb, fk, strip=2, natm=8, out0=True, claim=dict(strips=(2, 1))))
    return cases


CASES = _build_table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
REF_CASES = [c for c in CASES if not c.ref_of]
PROBE_CASES = [c for c in CASES if c.probe]


# --------------------------------------------------------------------------- builders
def _seed(name):
    import zlib
    return zlib.crc32(name.encode())


def build(c: Case) -> Call:
    """The arrays of a case (deterministic; a case with ``ref_of`` gets that case's numbers)."""
    from xtddft_amd.qc.ints import DerivPair, ShellPair
    rng = np.random.default_rng(_seed(c.ref_of or c.name))
    # AO ranges: every bra row and every ket its own
    nxt = [2]

    def alloc(n):
        s = nxt[0]
        nxt[0] += n + GAP
        return s
    ket_ao, bra_ao = [None] * len(c.kets), [None] * len(c.bras)

    def place_kets():
        for j, k in enumerate(c.kets):
            c0 = alloc(ncart(k.lc))
            d0 = c0 if k.same else alloc(ncart(k.ld))
            ket_ao[j] = [c0, d0, 0 if k.ncd0 else ncart(k.ld), k.flag]

    def place_bras():
        for i, b in enumerate(c.bras):
            a0 = alloc(ncart(b.la))
            b0 = alloc(ncart(b.lb))
            bra_ao[i] = [a0, b0, 0 if b.ncb0 else ncart(b.lb), i if b.atom < 0 else b.atom]
    for f in ((place_kets, place_bras) if c.kets_first else (place_bras, place_kets)):
        f()
    nao = nxt[0] + 12           # above every range by more than the widest shell (10 components)
    # tables: equal rows share one block
    binfo, bprim, eb, blocks = [], [], [], {}
    q0 = e0 = 0
    for b in c.bras:
        if b.block not in blocks:
            sa = shell(b.la, b.na, b.ca, 11 + b.la)
            sb = shell(b.lb, b.nb, b.cb, 23 + b.lb)
            dp = DerivPair(sa, sb)
            tab = dp.Eab[:, 0]
            blocks[b.block] = [dp.L, tab.shape[0], dp.p.size, q0, e0, 0, 0, 0]
            bprim.append(np.column_stack([dp.p, dp.P]))
            eb.append(tab.ravel())
            q0 += dp.p.size
            e0 += tab.size
        binfo.append(blocks[b.block])
    kinfo, kprim, ek, blocks = [], [], [], {}
    q0 = e0 = 0
    for k in c.kets:
        if k.block not in blocks:
            sc = shell(k.lc, k.nc, k.cc, 37 + k.lc)
            sd = sc if k.same else shell(k.ld, k.nd, k.cd, 41 + k.ld)
            sp = ShellPair(sc, sd)
            tab = sp.Eab.reshape(k.ncol, sp.Eab.shape[2], sp.p.size)
            blocks[k.block] = [sp.L, sp.p.size, q0, e0, 0, k.ncol, 0, 0]
            kprim.append(np.column_stack([sp.p, sp.P]))
            ek.append(tab.ravel())
            q0 += sp.p.size
            e0 += tab.size
        kinfo.append(blocks[k.block])
    bra_ao, ket_ao = np.array(bra_ao, dtype=np.int32), np.array(ket_ao, dtype=np.int32)
    pmask, qmask = read_masks(c, bra_ao, ket_ao, nao)
    wj, wk = rng.choice(WEIGHTS, c.nterm), rng.choice(WEIGHTS, c.nterm)
    for t, which in c.zero_w:
        (wj if which == "j" else wk)[t] = 0.0
    P = np.where(pmask[None], rng.integers(-4, 5, (c.nterm, nao, nao)) / 4.0, np.nan)
    Q = np.where(qmask[None], rng.integers(-4, 5, (c.nterm, nao, nao)) / 4.0, np.nan)
    out0 = rng.choice([-1.0, 1.0], (c.natm, 3)) * rng.integers(1, 65, (c.natm, 3)) / 16.0 if c.out0 \
        else np.zeros((c.natm, 3))
    return Call(np.array(binfo, dtype=np.int32), np.concatenate(bprim), np.concatenate(eb), bra_ao,
                np.array(kinfo, dtype=np.int32), np.concatenate(kprim), np.concatenate(ek), ket_ao, c.lbra, c.lket,
                wj, wk, P, Q, nao, c.strip, c.natm, out0, pmask, qmask)


def read_masks(c, bra_ao, ket_ao, nao):
    """Where grad_gamma reads: P[a, b], P[a, c] (image: P[a, d]); Q[c, d], Q[b, d] (image: Q[d, c],
    Q[b, c]) for every bra row against every ket.  A term reads all of them whatever its weights."""
    pm = np.zeros((nao, nao), dtype=bool)
    qm = np.zeros((nao, nao), dtype=bool)
    for b, (a0, b0, _, _) in zip(c.bras, bra_ao):
        ra, rb = slice(a0, a0 + ncart(b.la)), slice(b0, b0 + ncart(b.lb))
        pm[ra, rb] = True
        for k, (c0, d0, _, image) in zip(c.kets, ket_ao):
            rc, rd = slice(c0, c0 + ncart(k.lc)), slice(d0, d0 + ncart(k.ld))
            pm[ra, rc] = True
            qm[rc, rd] = True
            qm[rb, rd] = True
            if image:
                pm[ra, rd] = True
                qm[rd, rc] = True
                qm[rb, rc] = True
    return pm, qm


# --------------------------------------------------------------------------- selector probes
SELECTORS = ("J", "K", "Jimg", "Jsum")


def probes(c: Case, call: Call):
    """Seeded (ab, cd) per bra row of a class case (one ket): distinct pairs, the first and the
    last element of the block among them."""
    rng = np.random.default_rng(_seed(c.ref_of or c.name) + 1)
    nab, ncol = c.bras[0].nab, c.kets[0].ncol
    out = [(0, ncol - 1), (nab - 1, 0)]
    while len(out) < len(c.bras):
        out.append((int(rng.integers(nab)), int(rng.integers(ncol))))
    return out[:len(c.bras)]


def selector(c: Case, call: Call, kind: str) -> Call:
    """The call with Gamma a selector: term t picks element (ab_t, cd_t) of bra row t against the
    one ket.  "J": P_t = e_a e_b^T, Q_t = e_c e_d^T, wj = 1, wk = 0.  "K": the exchange mapping,
    P_t = e_a e_c^T, Q_t = e_b e_d^T, wj = 0, wk = 1.  "Jimg": Q_t = e_d e_c^T (reaches Gamma only
    through an image ket).  "Jsum": Q_t = e_c e_d^T + e_d e_c^T (twice the value on an image ket)."""
    import copy
    assert c.probe and len(c.kets) == 1 and kind in SELECTORS
    n = len(c.bras)
    P = np.where(call.pmask[None], 0.0, np.nan).repeat(n, axis=0)
    Q = np.where(call.qmask[None], 0.0, np.nan).repeat(n, axis=0)
    c0, d0, ncd, _ = (int(x) for x in call.ket_ao[0])
    ncd = max(ncd, 1)
    for t, (ab, cd) in enumerate(probes(c, call)):
        a0, b0, ncb, _ = (int(x) for x in call.bra_ao[t])
        ncb = max(ncb, 1)
        ia, ib, ic, idd = a0 + ab // ncb, b0 + ab % ncb, c0 + cd // ncd, d0 + cd % ncd
        if kind == "K":
            P[t, ia, ic] = 1.0
            Q[t, ib, idd] = 1.0
            continue
        P[t, ia, ib] = 1.0
        if kind in ("J", "Jsum"):
            Q[t, ic, idd] += 1.0
        if kind in ("Jimg", "Jsum"):
            Q[t, idd, ic] += 1.0
    out = copy.copy(call)
    out.P, out.Q = P, Q
    out.wj = np.full(n, 0.0 if kind == "K" else 1.0)
    out.wk = np.full(n, 1.0 if kind == "K" else 0.0)
    return out


# --------------------------------------------------------------------------- the bound
U = 2.0 ** -53
L_MAX = 13                      # bra order 7 + ket order 6
KAPPA_FACTOR, KAPPA_FLOOR = 8.0, 64.0


def kappa_file():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grad_kappa.json")


def load_kappa():
    """(host error, kappa_g) per total order L = 0 .. L_MAX of tests/golden/grad_kappa.json."""
    import json
    with open(kappa_file()) as f:
        d = json.load(f)
    return np.array(d["host_error"], dtype=np.float64), np.array(d["kappa_g"], dtype=np.float64)


def units(val, ref, sabs, Lrow):
    """|val - ref| / (2^-53 sabs) per element of the rows that have a bra entry; 0 where sabs = 0,
    where the value must be an exact zero."""
    live = (Lrow >= 0)[:, None] & (sabs > 0)
    assert np.all(val[(Lrow >= 0)[:, None] & (sabs == 0)] == 0.0), "sabs = 0 but the value is not an exact zero"
    out = np.zeros(val.shape)
    out[live] = np.abs(val[live] - ref[live]) / (U * sabs[live])
    return out


def measured_ratio(val, ref, sabs, Lrow):
    """Largest units() per total order L (length L_MAX + 1)."""
    out = np.zeros(L_MAX + 1)
    r = units(val, ref, sabs, Lrow).max(axis=1)
    np.maximum.at(out, Lrow[Lrow >= 0], r[Lrow >= 0])
    return out


def kappa_from(measured):
    return np.maximum(KAPPA_FLOOR, KAPPA_FACTOR * np.asarray(measured))
