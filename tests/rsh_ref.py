"""References of the long-range (erf(omega r12) / r12) derivative-ERI gradient, ``xt_grad_jk2_lr`` of
xtddft_amd/csrc/xt_grad.hip, and of the range-separated UKS gradient (TEST INFRASTRUCTURE ONLY; not
a test file).  Shared by tests/test_rshgrad_host.py, tests/test_gpu_grad_lr.py, tests/test_gpu_rshgrad.py
and tests/golden/make_rsh_kappa.py.

* ``grad_integrals_lr`` -- the 40-digit derivative integrals of every distinct (bra block, ket block) of a
  raw call over the attenuated operator: the loop of ``hint_ref.ref_hint`` in plain mode with, per
  primitive quartet, alpha = p s / (p + s), a2 = alpha w^2 / (alpha + w^2), the Hermite integrals at a2 and
  the factor sqrt(a2 / alpha), all in mpmath at ``int_ref.DPS`` digits.  It returns what
  ``hint_ref.ref_grad(call, blocks=...)`` accepts, so Gamma, the fold and sabs are that module's.
  ``drop_scale`` leaves the factor out: one of the two deliberately wrong references.
* ``host_grad_lr`` -- the host FP64 restatement (``hint_ref.host_integrals`` with ``ints._attenuate``), from
  which the multiplier kappa_lr(L) of the bound is measured (tests/golden/make_rsh_kappa.py).
* ``deriv_eri_lr`` -- ``grad_ref.deriv_eri`` over the attenuated operator.
* ``uks_grad_rsh`` -- ``ksgrad_ref.uks_grad`` plus the long-range exchange -(alpha - hyb) K_LR[D_s] . D_s.
* ``far_case`` -- s and p shells, 1 and 3 primitives, on two centres 20 Bohr apart: at omega = 0.33 the Boys
  argument a2 R^2 of its primitive quartets lies on both sides of 30, where ``hint_boys`` changes regime.
"""
from __future__ import annotations

import json
import os

import numpy as np

import grad_cases as gc
import grad_ref as R
import hint_ref
import int_ref
import ksgrad_ref as K

OMEGA = 0.33                     # CAM-B3LYP's; wB97X-D has 0.2
LIMIT_OMEGAS = (0.2, 2.0 ** -4, 16.0)
LIMIT_CASES = ("nterm8", "c21_d", "c21_f")      # one per template instance
STRUCTURE_CASES = ("cth81", "cth108", "cth54_twin", "img_off", "map70", "map70_s1", "fold")
CAM_HYB, CAM_ALPHA = 0.19, 0.65  # hyb and alpha of CAM-B3LYP: k_lr = alpha - hyb = 0.46


# --------------------------------------------------------------------------- 40 digits
def grad_integrals_lr(call, omega, drop_scale=False):
    """(ref, sabs, brow, kcol) as ``hint_ref.grad_integrals``, over erf(omega r12) / r12."""
    import mpmath as mp
    LD, WIDE = int_ref.LD, int_ref.WIDE
    binfo, kinfo, brow, kcol, nrow_tot, ncol_tot = hint_ref._unique_blocks(call)
    zero = LD(0) if WIDE else mp.mpf(0)
    ref = np.full((nrow_tot, ncol_tot), zero, dtype=LD if WIDE else object)
    sab = ref.copy()
    bprim, kprim = np.asarray(call.bprim).reshape(-1, 4), np.asarray(call.kprim).reshape(-1, 4)
    with mp.workdps(int_ref.DPS):
        w2 = mp.mpf(float(omega)) ** 2
        for j in range(len(kinfo)):
            for k in range(len(binfo)):
                lb, nrow, npp, bq0, be0, row0 = (int(x) for x in binfo[k][:6])
                lk, nr, kr0, ke0, col0, ncol = (int(x) for x in kinfo[j][:6])
                L, nt, nu = lb + lk, int_ref.ntuv(lb), int_ref.ntuv(lk)
                E = int_ref._wide_array(np.asarray(call.eb[be0:be0 + nrow * nt * npp]).reshape(nrow, nt, npp))
                Kt = int_ref._wide_array(np.asarray(call.ek[ke0:ke0 + ncol * nu * nr]).reshape(ncol, nu, nr))
                idx, sign = int_ref._sum_index(lb, lk)
                Ks = Kt * (sign[None, :, None].astype(LD) if WIDE else sign[None, :, None].astype(int).astype(object))
                blk = np.full((nrow, ncol), zero, dtype=ref.dtype)
                blka = blk.copy()
                for q in range(npp):
                    p = mp.mpf(float(bprim[bq0 + q, 0]))
                    P = [mp.mpf(float(x)) for x in bprim[bq0 + q, 1:]]
                    for r in range(nr):
                        s = mp.mpf(float(kprim[kr0 + r, 0]))
                        C = [mp.mpf(float(x)) for x in kprim[kr0 + r, 1:]]
                        alpha = p * s / (p + s)
                        a2 = alpha * w2 / (alpha + w2)
                        scale = mp.mpf(1) if drop_scale else mp.sqrt(a2 / alpha)
                        Rt = int_ref.hermite_r_mp(L, a2, P[0] - C[0], P[1] - C[1], P[2] - C[2])
                        pref = int_ref._wide(2 * mp.pi ** 2.5 / (p * s * mp.sqrt(p + s)) * scale)
                        Rg = np.array([int_ref._wide(x) for x in Rt], dtype=ref.dtype)[idx]
                        blk += pref * (E[:, :, q] @ (Rg @ Ks[:, :, r].T))
                        blka += abs(pref) * (np.abs(E[:, :, q]) @ (np.abs(Rg) @ np.abs(Kt[:, :, r]).T))
                ref[row0:row0 + nrow, col0:col0 + ncol] = blk
                sab[row0:row0 + nrow, col0:col0 + ncol] = blka

    def f64(a):
        return a.astype(np.float64) if WIDE else np.array([float(x) for x in a.ravel()]).reshape(a.shape)
    ref, sab = f64(ref), f64(sab)
    for x in (ref, sab):
        x.setflags(write=False)
    return ref, sab, brow, kcol


def boys_arguments(call, omega):
    """a2 R^2 of every primitive quartet of the call: what ``hint_boys`` is called with."""
    bprim, kprim = np.asarray(call.bprim).reshape(-1, 4), np.asarray(call.kprim).reshape(-1, 4)
    p, s = bprim[:, None, 0], kprim[None, :, 0]
    alpha = p * s / (p + s)
    a2 = alpha * omega ** 2 / (alpha + omega ** 2)
    return a2 * ((bprim[:, None, 1:] - kprim[None, :, 1:]) ** 2).sum(axis=2)


# --------------------------------------------------------------------------- host FP64
def host_integrals_lr(call, omega):
    """``hint_ref.host_integrals`` with the exponent and scale of ``ints._attenuate``."""
    from xtddft_amd.qc import ints
    binfo, kinfo, brow, kcol, nrow, ncol = hint_ref._unique_blocks(call)
    out = np.zeros((nrow, ncol))
    bprim, kprim = call.bprim.reshape(-1, 4), call.kprim.reshape(-1, 4)
    for lb, nr_b, npp, bq0, be0, row0 in (tuple(int(x) for x in r[:6]) for r in binfo):
        for lk, nr, kr0, ke0, col0, nc in (tuple(int(x) for x in r[:6]) for r in kinfo):
            E = call.eb[be0:be0 + nr_b * int_ref.ntuv(lb) * npp].reshape(nr_b, int_ref.ntuv(lb), npp)
            Kt = call.ek[ke0:ke0 + nc * int_ref.ntuv(lk) * nr].reshape(nc, int_ref.ntuv(lk), nr)
            p = bprim[bq0:bq0 + npp, 0][:, None]
            s = kprim[kr0:kr0 + nr, 0][None, :]
            d = bprim[bq0:bq0 + npp, None, 1:] - kprim[None, kr0:kr0 + nr, 1:]
            a2, scale = ints._attenuate(p * s / (p + s), omega)
            Rt = ints.hermite_r(lb + lk, a2, d[..., 0], d[..., 1], d[..., 2])
            pref = 2.0 * np.pi ** 2.5 / (p * s * np.sqrt(p + s)) * scale
            idx, sign = ints._sum_table(lb, lk)
            X = np.einsum('tsPQ,s,csQ->tcP', Rt[idx] * pref, sign, Kt, optimize=True)
            out[row0:row0 + nr_b, col0:col0 + nc] = np.einsum('atP,tcP->ac', E, X, optimize=True)
    return out, brow, kcol


def host_grad_lr(call, omega):
    """The host FP64 restatement of one ``xt_grad_jk2_lr`` call: float64 integrals times Gamma, in float64."""
    val, brow, kcol = host_integrals_lr(call, omega)
    g, _, _, _ = hint_ref.contract(call, val, brow, kcol, wide=False)
    return hint_ref.fold(call, g)


# --------------------------------------------------------------------------- the bound
def kappa_file():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rsh_kappa.json")


def load_kappa():
    """(host error, kappa_lr) per total order L = 0 .. grad_cases.L_MAX of tests/golden/rsh_kappa.json."""
    with open(kappa_file()) as f:
        d = json.load(f)
    return np.array(d["host_error"], dtype=np.float64), np.array(d["kappa_lr"], dtype=np.float64)


# --------------------------------------------------------------------------- the far pair
_FAR = {}


def far_case():
    """(case, call): the bra pair (s of 3 primitives, p of 1) on the origin, the ket pairs (p of 1, s of 3)
    and a diagonal (s s) 20 Bohr away along z, built from ``gto.Shell`` directly.  With ``OMEGA`` the
    smallest primitive quartets have a2 R^2 near 28 and the largest above 40."""
    if "far" in _FAR:
        return _FAR["far"]
    from xtddft_amd.qc.gto import Shell, gto_norm
    from xtddft_amd.qc.ints import DerivPair, ShellPair
    A, B = np.zeros(3), np.array([0.0, 0.0, 20.0])

    def sh(atom, l, centre, exps, coefs):
        e = np.asarray(exps, dtype=np.float64)
        return Shell(atom, l, centre.copy(), e, np.asarray(coefs, dtype=np.float64) * gto_norm(l, e))
    s3a, p1a = sh(0, 0, A, [0.15, 0.6, 2.5], [0.5, 0.7, 0.3]), sh(0, 1, A, [0.3], [1.0])
    s3b, p1b = sh(1, 0, B, [0.1, 0.5, 2.0], [0.6, 0.6, 0.2]), sh(1, 1, B, [0.25], [1.0])
    bras = (gc.Bra(0, 1, 3, 1, 0, 0), gc.Bra(1, 0, 1, 3, 0, 0))
    kets = (gc.Ket(1, 0, 1, 3, 1, 1), gc.Ket(0, 0, 3, 3, 1, 1, same=True))
    c = gc._case("far", bras, kets, nterm=2, strip=1, claim=dict(inst=(6, 4), cache="c", image="in", strips=(2, 1)))
    bshells = [(s3a, p1a), (p1a, s3a)]
    kshells = [(p1b, s3b), (s3b, s3b)]
    nxt = [2]

    def alloc(n):
        s = nxt[0]
        nxt[0] += n + gc.GAP
        return s
    bra_ao, ket_ao = [], []
    for i, b in enumerate(bras):
        bra_ao.append([alloc(gc.ncart(b.la)), alloc(gc.ncart(b.lb)), gc.ncart(b.lb), i])
    for k in kets:
        c0 = alloc(gc.ncart(k.lc))
        ket_ao.append([c0, c0 if k.same else alloc(gc.ncart(k.ld)), gc.ncart(k.ld), k.flag])
    nao = nxt[0] + 12
    binfo, bprim, eb = [], [], []
    q0 = e0 = 0
    for sa, sb in bshells:
        dp = DerivPair(sa, sb)
        tab = dp.Eab[:, 0]
        binfo.append([dp.L, tab.shape[0], dp.p.size, q0, e0, 0, 0, 0])
        bprim.append(np.column_stack([dp.p, dp.P]))
        eb.append(tab.ravel())
        q0 += dp.p.size
        e0 += tab.size
    kinfo, kprim, ek = [], [], []
    q0 = e0 = 0
    for k, (sc, sd) in zip(kets, kshells):
        sp = ShellPair(sc, sd)
        tab = sp.Eab.reshape(k.ncol, sp.Eab.shape[2], sp.p.size)
        kinfo.append([sp.L, sp.p.size, q0, e0, 0, k.ncol, 0, 0])
        kprim.append(np.column_stack([sp.p, sp.P]))
        ek.append(tab.ravel())
        q0 += sp.p.size
        e0 += tab.size
    bra_ao, ket_ao = np.array(bra_ao, dtype=np.int32), np.array(ket_ao, dtype=np.int32)
    pmask, qmask = gc.read_masks(c, bra_ao, ket_ao, nao)
    rng = np.random.default_rng(gc._seed("far"))
    wj, wk = rng.choice(gc.WEIGHTS, c.nterm), rng.choice(gc.WEIGHTS, c.nterm)
    P = np.where(pmask[None], rng.integers(-4, 5, (c.nterm, nao, nao)) / 4.0, np.nan)
    Q = np.where(qmask[None], rng.integers(-4, 5, (c.nterm, nao, nao)) / 4.0, np.nan)
    call = gc.Call(np.array(binfo, dtype=np.int32), np.concatenate(bprim), np.concatenate(eb), bra_ao,
                   np.array(kinfo, dtype=np.int32), np.concatenate(kprim), np.concatenate(ek), ket_ao, c.lbra, c.lket,
                   wj, wk, P, Q, nao, c.strip, c.natm, np.zeros((c.natm, 3)), pmask, qmask)
    _FAR["far"] = (c, call)
    return _FAR["far"]


def bound_cases():
    """[(name, case, call, omega)]: every raw call the bound of ``xt_grad_jk2_lr`` is measured and tested on --
    the 49 classes and the structure cases at ``OMEGA``, the far pair, and one case per template instance at
    ``LIMIT_OMEGAS`` (cases with ``ref_of`` have the integrals of the case they name)."""
    out = [(c.name, c, gc.build(c), OMEGA) for c in gc.CASES
           if (c.probe and not c.ref_of) or c.name in STRUCTURE_CASES]
    c, call = far_case()
    out.append((c.name, c, call, OMEGA))
    for name in LIMIT_CASES:
        for w in LIMIT_OMEGAS:
            out.append((f"{name}@{w:g}", gc.BY_NAME[name], gc.build(gc.BY_NAME[name]), w))
    return out


# --------------------------------------------------------------------------- molecules
def deriv_eri_lr(mol, omega):
    """``grad_ref.deriv_eri`` with (nabla_x i j|k l) over erf(omega r12) / r12."""
    from xtddft_amd.qc.gto import _sph_transform
    from xtddft_amd.qc.ints import DerivPair, ShellPair, eri_quartet
    n = mol.nao
    sh, loc = mol.shells, mol.ao_loc
    out = np.zeros((3, n, n, n, n))
    T = [_sph_transform(s.l) * mol._norm[p0:p0 + s.nsph, None] for s, p0 in zip(sh, loc[:-1])]
    kets = {(k, l): ShellPair(sh[k], sh[l]) for k in range(len(sh)) for l in range(k + 1)}
    for i in range(len(sh)):
        for j in range(len(sh)):
            bra = DerivPair(sh[i], sh[j])
            for (k, l), ket in kets.items():
                g = -eri_quartet(bra, ket, omega)[:, 0].reshape(3, sh[i].ncart, sh[j].ncart, sh[k].ncart, sh[l].ncart)
                g = np.einsum('xabcd,ia,jb,kc,ld->xijkl', g, T[i], T[j], T[k], T[l], optimize=True)
                out[:, loc[i]:loc[i + 1], loc[j]:loc[j + 1], loc[k]:loc[k + 1], loc[l]:loc[l + 1]] = g
                if k != l:
                    out[:, loc[i]:loc[i + 1], loc[j]:loc[j + 1], loc[l]:loc[l + 1], loc[k]:loc[k + 1]] = \
                        g.transpose(0, 1, 2, 4, 3)
    return out


def uks_grad_rsh(mf, ip=None, ip_lr=None):
    """dE/dR (natm, 3) of a converged range-separated UKS on the grid held fixed: ``ksgrad_ref.uks_grad``
    (one-electron, J - hyb K, XC and nuclear parts) plus -(alpha - hyb) K_LR[D_s] with D_s per spin."""
    mol = mf.mol
    assert mf.omega != 0
    ip = R.deriv_eri(mol) if ip is None else ip
    ip_lr = deriv_eri_lr(mol, mf.omega) if ip_lr is None else ip_lr
    g = K.uks_grad(mf, ip)[0]
    k_lr = float(mf.alpha) - float(mf.hyb)
    d = [mf.mo_coeff[s][:, mf.mo_occ[s] > 0] @ mf.mo_coeff[s][:, mf.mo_occ[s] > 0].T for s in range(2)]
    return g + R._de_2e(mol, ip_lr, [(0, -k_lr, d[0], d[0]), (0, -k_lr, d[1], d[1])])
