"""The case table of the GEMM engine's planned paths (xtddft_amd/csrc/xt_gemm.hip), used twice:
tests/test_gemm_plan.py checks on the host (xt_gemm_plan) that every case takes the path it
claims and that the table is closed over the paths the engine can launch;
tests/test_gpu_gemm_paths.py runs every case on the device (xt_gemm_run) against an exact
host product.

A case is a shape, a reduce count, a batch, the operand layouts and what the planner must
make of them:
  cfg      tile configuration (kCfg index: 2 128x64, 3 64x128, 4 64x64, 5 / 8 128x128 BK 16,
           9 128x128 BK 32)
  la, lb   contiguous axis of A ("k" or "m") and of B ("k" or "n")
  staging  "whole" (K % bk == 0), "ragged_first" (R == 1, K % bk != 0: the ragged K tile is
           staged by the prologue) or "masked" (R > 1, K % bk != 0: every tile masked)
  split    split-K (nsplit > 1) or not
  tiles    "full" (bm | M and bn | N), "ragged" (neither) or "mixed"
  tall     more than 8 row tiles, not a multiple of 8 (a partial last GROUP_M sweep of the
           tile walk), and at least 2 column tiles
Operands sit inside larger allocations (layout() / pack()): leading dimensions larger than
the extents and gaps between reduce slabs and batches, so that a load or a store outside the
operand shows.
"""
from __future__ import annotations

import ctypes
import itertools
from dataclasses import dataclass

import numpy as np

# (bm, bn, bk) of the plain-mode tile configurations
CFG_TILE = {2: (128, 64, 32), 3: (64, 128, 32), 4: (64, 64, 32), 5: (128, 128, 16), 8: (128, 128, 16),
            9: (128, 128, 32)}
LAYOUTS = [("k", "k"), ("k", "n"), ("m", "k"), ("m", "n")]
STAGINGS = ["whole", "ragged_first", "masked"]
ALPHAS = (1.0, -2.0, 0.5)
BETAS = (0.0, 1.0, -0.5)


@dataclass(frozen=True)
class Case:
    name: str
    m: int
    n: int
    k: int
    r: int
    la: str
    lb: str
    cfg: int
    staging: str
    split: bool
    nb1: int = 1
    nb2: int = 1
    rdiv: int = 0
    tag: int = 0
    bcast: str = ""        # batch strides set to 0, e.g. "sBb2"
    alpha: float = 1.0
    beta: float = 0.0

    @property
    def tiles(self):
        bm, bn, _ = CFG_TILE[self.cfg]
        fm, fn = self.m % bm == 0, self.n % bn == 0
        return "full" if fm and fn else "ragged" if not fm and not fn else "mixed"

    @property
    def tall(self):
        bm, bn, _ = CFG_TILE[self.cfg]
        tm, tn = -(-self.m // bm), -(-self.n // bn)
        return tm > 8 and tm % 8 != 0 and tn >= 2


# shapes that plan each configuration (first: ragged in M and N; cfg 8 exists only with a
# ragged column edge, so its "most full" shape is full in M alone)
SHAPES = {
    2: [(100, 40), (128, 64), (1153, 70)],
    3: [(40, 100), (64, 128)],
    4: [(40, 40), (64, 64)],
    5: [(130, 260), (256, 256), (257, 257), (1153, 256)],
    8: [(97, 130), (128, 133), (1153, 130)],
    9: [(130, 260), (256, 256), (257, 257), (1153, 130)],
}


def _k_r(staging, split):
    """(K, R) of a staging / split combination: K = 64 is whole K tiles of every bk, 37 is
    ragged for every bk; 2048 / 2001 / 777 x 3 are the same with enough K tiles to split."""
    if staging == "whole":
        return (2048, 1) if split else (64, 1)
    if staging == "ragged_first":
        return (2001, 1) if split else (37, 1)
    return (777, 3) if split else (37, 3)


def _build():
    cases = []
    count = itertools.count()

    def add(cfg, shape, la, lb, staging, split, **kw):
        i = next(count)
        k, r = kw.pop("kr", None) or _k_r(staging, split)
        m, n = shape
        name = f"c{cfg}-{la}{lb}-{staging}-{'split' if split else 'one'}-{m}x{n}x{k}"
        if kw.get("rdiv"):
            name += "-rdiv"
        if kw.get("tag"):
            name += f"-tag{kw['tag']}"
        if kw.get("nb1", 1) * kw.get("nb2", 1) > 1:
            name += f"-b{kw.get('nb1', 1)}x{kw.get('nb2', 1)}"
        cases.append(Case(name, m, n, k, r, la, lb, cfg, staging, split,
                          alpha=ALPHAS[i % 3], beta=BETAS[(i + i // 3) % 3], **kw))

    for cfg in (2, 3, 4, 5, 8, 9):
        layouts = LAYOUTS if cfg in (2, 3, 4) else LAYOUTS[:3] if cfg in (5, 8) else LAYOUTS[3:]
        shapes = itertools.cycle(SHAPES[cfg])
        for (la, lb), staging, split in itertools.product(layouts, STAGINGS, (False, True)):
            add(cfg, next(shapes), la, lb, staging, split)
    # neither operand k-contiguous on the BK 16 tiles: only with two-level rows
    for cfg, shape in ((5, (256, 256)), (5, (257, 257)), (8, (128, 133)), (8, (97, 130))):
        for staging in ("whole", "ragged_first"):
            add(cfg, shape, "m", "n", staging, False, rdiv=13)
    # two-level batch, distinct strides, B broadcast over the inner batch index
    add(2, (100, 40), "k", "n", "ragged_first", False, nb1=2, nb2=3, bcast="sBb2")
    add(4, (40, 40), "m", "k", "masked", False, nb1=3, nb2=2, bcast="sAb1")
    # planning rules of the tagged call sites
    add(5, (40, 100), "k", "n", "ragged_first", False, tag=1)     # stored exchange: M < 96 <= N
    add(4, (130, 147), "m", "n", "ragged_first", False, tag=3)    # XC back L, N = 147: 64 x 64
    return cases


CASES = _build()


def required_paths():
    """Every (cfg, la, lb, staging, split, rdiv) the table must hold."""
    req = set()
    for cfg in (2, 3, 4):
        for (la, lb), st, sp in itertools.product(LAYOUTS, STAGINGS, (False, True)):
            req.add((cfg, la, lb, st, sp, False))
    for cfg in (5, 8):
        for (la, lb), st, sp in itertools.product(LAYOUTS[:3], STAGINGS, (False, True)):
            req.add((cfg, la, lb, st, sp, False))
        for st in ("whole", "ragged_first"):
            req.add((cfg, "m", "n", st, False, True))
    for st, sp in itertools.product(STAGINGS, (False, True)):
        req.add((9, "m", "n", st, sp, False))
    return req


# ---- operands inside larger allocations -------------------------------------------------
PAD = 3          # extra elements per row (ld = extent + PAD)
GAP = 5          # extra elements between reduce slabs and between batches
TAIL = 4096      # allocation tail past the last element


def layout(c: Case):
    """Strides of the three operands (xt_gemm_desc names) and the allocation sizes."""
    s = {}
    if c.rdiv:
        # row m = (hi, lo) = (m / rdiv, m % rdiv) at hi sAm_hi + lo, k-stride over all hi
        nhi = -(-c.m // c.rdiv)
        s["sAm"], s["sAm_hi"] = 1, c.rdiv + PAD
        s["sAk"] = nhi * s["sAm_hi"] + GAP
        s["sAr"] = c.k * s["sAk"] + GAP
    elif c.la == "k":
        s["sAk"], s["sAm"] = 1, c.k + PAD
        s["sAr"] = c.m * s["sAm"] + GAP
    else:
        s["sAm"], s["sAk"] = 1, c.m + PAD
        s["sAr"] = c.k * s["sAk"] + GAP
    s["sAb2"] = c.r * s["sAr"] + GAP
    s["sAb1"] = c.nb2 * s["sAb2"] + GAP
    if c.lb == "k":
        s["sBk"], s["sBn"] = 1, c.k + PAD
        s["sBr"] = c.n * s["sBn"] + GAP
    else:
        s["sBn"], s["sBk"] = 1, c.n + PAD
        s["sBr"] = c.k * s["sBk"] + GAP
    s["sBb2"] = c.r * s["sBr"] + GAP
    s["sBb1"] = c.nb2 * s["sBb2"] + GAP
    s["ldc"] = c.n + PAD
    if c.rdiv:
        s["sC_hi"] = c.rdiv * s["ldc"] + GAP
        crows = -(-c.m // c.rdiv) * s["sC_hi"]
    else:
        crows = c.m * s["ldc"]
    s["sCb2"] = crows + GAP
    s["sCb1"] = c.nb2 * s["sCb2"] + GAP
    sizes = {"A": c.nb1 * s["sAb1"] + TAIL, "B": c.nb1 * s["sBb1"] + TAIL, "C": c.nb1 * s["sCb1"] + TAIL}
    for name in c.bcast.split(","):
        if name:
            s[name] = 0
    return s, sizes


def logical_shapes(c: Case):
    """Shapes of A (b1, b2, r, m, k), B (b1, b2, r, k, n) and C (b1, b2, m, n); a broadcast
    batch index has extent 1."""
    bc = set(c.bcast.split(","))
    a = (1 if "sAb1" in bc else c.nb1, 1 if "sAb2" in bc else c.nb2, c.r, c.m, c.k)
    b = (1 if "sBb1" in bc else c.nb1, 1 if "sBb2" in bc else c.nb2, c.r, c.k, c.n)
    return a, b, (c.nb1, c.nb2, c.m, c.n)


def _offsets(c: Case, s, which, shape):
    ix = np.ix_(*[np.arange(e, dtype=np.int64) for e in shape])
    if which == "A":
        b1, b2, r, m, k = ix
        row = (m // c.rdiv) * s["sAm_hi"] + m % c.rdiv if c.rdiv else m * s["sAm"]
        return b1 * s["sAb1"] + b2 * s["sAb2"] + r * s["sAr"] + row + k * s["sAk"]
    if which == "B":
        b1, b2, r, k, n = ix
        return b1 * s["sBb1"] + b2 * s["sBb2"] + r * s["sBr"] + k * s["sBk"] + n * s["sBn"]
    b1, b2, m, n = ix
    row = (m // c.rdiv) * s["sC_hi"] + (m % c.rdiv) * s["ldc"] if c.rdiv else m * s["ldc"]
    return b1 * s["sCb1"] + b2 * s["sCb2"] + row + n


def pack(c: Case, which, values, fill):
    """Flat allocation of operand `which` holding `values` (logical shape) at the case's
    strides, `fill` everywhere else; and the flat offsets of the values."""
    s, sizes = layout(c)
    off = _offsets(c, s, which, values.shape)
    assert off.min() >= 0 and off.max() + TAIL // 2 < sizes[which]
    assert np.unique(off).size == off.size, "operand elements overlap"
    flat = np.full(sizes[which], fill, dtype=np.float64)
    flat[off] = values
    return flat, off


def host_product(a, b, dtype=np.float64):
    """sum_r sum_k A B of logical operands (batch indices broadcast): (b1, b2, m, n).  The
    reduce index is folded into k (one product over r k)."""
    a = np.asarray(a, dtype=dtype)
    b = np.asarray(b, dtype=dtype)
    am = np.moveaxis(a, 2, 3).reshape(a.shape[0], a.shape[1], a.shape[3], a.shape[2] * a.shape[4])
    bm = b.reshape(b.shape[0], b.shape[1], b.shape[2] * b.shape[3], b.shape[4])
    return np.matmul(am, bm)


def fill_desc(desc, c: Case, **over):
    """Fill an XtGemmDesc (xtddft_amd._capi) from a case."""
    s, _ = layout(c)
    desc.m, desc.n, desc.k, desc.r, desc.nb1, desc.nb2 = c.m, c.n, c.k, c.r, c.nb1, c.nb2
    desc.alpha, desc.beta = c.alpha, c.beta
    for name in ("sAm", "sAk", "sAr", "sAb1", "sAb2", "sBk", "sBn", "sBr", "sBb1", "sBb2", "ldc", "sCb1", "sCb2"):
        setattr(desc, name, s[name])
    desc.rdiv, desc.sAm_hi, desc.sC_hi = c.rdiv, s.get("sAm_hi", 0), s.get("sC_hi", 0)
    desc.max_split, desc.tag, desc.ws_bytes = 0, c.tag, 0
    for name, v in over.items():
        setattr(desc, name, v)
    return desc


def plan(lib, desc):
    """xt_gemm_plan -> dict(cfg, bm, bn, bk, nsplit, masked); raises on a rejected descriptor."""
    out = [ctypes.c_int() for _ in range(6)]
    rc = lib.xt_gemm_plan(ctypes.byref(desc), *[ctypes.byref(o) for o in out])
    if rc != 0:
        raise ValueError(f"xt_gemm_plan: {lib.xt_last_error().decode()} (code {rc})")
    return dict(zip(("cfg", "bm", "bn", "bk", "nsplit", "masked"), (o.value for o in out)))


def gaussian_cases():
    """One case per configuration, unsplit and split-K, for the rounding-error check: the
    configuration's ragged shape with a ragged K, 777 being the smallest K of the table's that
    every configuration splits (3 to 6 ways)."""
    out = []
    for cfg, (la, lb) in ((2, "kn"), (3, "mk"), (4, "kk"), (5, "kn"), (8, "mk"), (9, "mn")):
        for k, split, alpha, beta in ((37, False, 0.5, 0.0), (777, True, -2.0, -0.5)):
            m, n = SHAPES[cfg][0]
            out.append(Case(f"gauss-c{cfg}-{la}{lb}-{m}x{n}x{k}", m, n, k, 1, la, lb, cfg, "ragged_first", split,
                            alpha=alpha, beta=beta))
    return out


def gaussian_operands(c: Case):
    """Seeded standard-normal logical operands of a case."""
    rng = np.random.default_rng(1000 * c.cfg + c.m + 3 * c.n + 7 * c.k + c.r)
    sa, sb, sc = logical_shapes(c)
    return rng.standard_normal(sa), rng.standard_normal(sb), rng.standard_normal(sc)


def higham_bound(c: Case, a, b, cc):
    """Elementwise bound gamma_n (|alpha| |A||B| + |beta| |C|), n = R K + 2, u = 2^-53 on the
    error of any float64 evaluation of alpha sum A B + beta C (R K products and additions in
    any order, the scaling by alpha, the beta C term and its addition)."""
    n = c.r * c.k + 2
    u = np.longdouble(2.0) ** -53
    gamma = n * u / (1 - n * u)
    ab = host_product(np.abs(a), np.abs(b), np.longdouble)
    return gamma * (abs(np.longdouble(c.alpha)) * ab + abs(np.longdouble(c.beta)) * np.abs(cc).astype(np.longdouble))


def reference_ld(c: Case, a, b, cc):
    """alpha sum A B + beta C in np.longdouble."""
    return np.longdouble(c.alpha) * host_product(a, b, np.longdouble) + np.longdouble(c.beta) * cc.astype(np.longdouble)
