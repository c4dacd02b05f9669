"""NumPy restatement of the reference's spin-orbit state interaction: the rank-1 tables of
x2c_hamiltonian/driver/si_driver.py:520-867 (``interact_*``), its H_eff assembly
(``make_heff``, si_driver.py:393-470) and the moments ``TDM_S_1`` / ``TDM_GSS`` / ``TDM_S`` /
``TDM_S1`` of x2c_hamiltonian/driver/tdm.py, written state by state and pair by pair as the
reference loops, one contraction per reference line with its Kronecker deltas carried out.

The reference stores no output of this driver, so this restatement is what ``xt_si_couple``
and ``xtddft_amd.soc.SI_driver`` are pinned to, together with the exactly solvable limits
below (``limit``), which pin the restatement itself.  It shares no code with the device
algorithm (which never forms an image per state on the host, addresses the operator's blocks
by strides and takes one Gram product per pair of manifolds).

Two places where the reference's text is easy to misread: in ``interact_SS`` every line-3 case
(50, 54, 57, 59) sits inside ``if self.S != 0``; case 54 at si_driver.py:795 indexes with the
S-1 slice name, which is the same slice as the CO(0) block.
"""
from functools import lru_cache
from math import sqrt

import numpy as np

R2 = sqrt(2.0)
GROUPS = ('|S->', '|GS>', '|So>', '|S+>')
es = np.einsum


def op_blocks(d, nc, no, nv):
    """Blocks of an operator (nmo, nmo, ncomp) over [c|o|v], keyed 'cc', 'co', ..., 'vv'."""
    sl = {'c': slice(0, nc), 'o': slice(nc, nc + no), 'v': slice(nc + no, nc + no + nv)}
    return {p + q: d[sl[p], sl[q], :] for p in 'cov' for q in 'cov'}


def split_sm(x, nc, no, nv):
    """|S-> vector -> CV(1), CO(1), OV(1), O1O2, O1O1."""
    cv, co, ov, oo = nc * nv, nc * no, no * nv, no * no
    a, b, c, d = cv, cv + co, cv + co + ov, cv + co + ov + oo
    return (x[:a].reshape(nc, nv), x[a:b].reshape(nc, no), x[b:c].reshape(no, nv),
            x[c:d].reshape(no, no), x[d:d + no])


def split_so(x, nc, no, nv):
    """|So> vector -> CV(0), CO(0), OV(0), CV(1)."""
    cv, co, ov = nc * nv, nc * no, no * nv
    a, b, c = cv, cv + co, cv + co + ov
    return x[:a].reshape(nc, nv), x[a:b].reshape(nc, no), x[b:c].reshape(no, nv), x[c:c + cv].reshape(nc, nv)


def join(parts):
    m = parts[0].shape[-1]
    return np.concatenate([p.reshape(-1, m) for p in parts], axis=0)


# ---- images h X_R in the layout of the left manifold (rows) x components --------
def img_sm_sm(b, S, n, xr):
    """interact_S_1S_1, cases 1-35."""
    nc, no, nv = n
    r0, r1, r2, r3, r4 = split_sm(xr, *n)
    f1 = (1 - S) / (S * R2)
    f2 = sqrt((2 * S + 1) / S) * (1 - S) / (2 * S)
    f11 = -(S - 1) / (S * R2)
    k11 = (2 * S + 1) / (2 * S - 1)
    f13 = -(S - 1) / sqrt(S * (2 * S - 1))
    f14 = -1.0 / (2 * sqrt(S * (2 * S - 1)))
    f21 = (1 - S) / sqrt(S * (2 * S - 1))
    f28 = -1 / R2
    g4 = (1 - S) / S * r4.sum() + 2 * (S - 1) * r4            # ((1-S)/S + 2(S-1) delta) X
    y0 = f1 * (es('abm,ib->iam', b['vv'], r0) + es('jim,ja->iam', b['cc'], r0))             # (1)
    y0 += f2 * es('atm,it->iam', b['vo'], r1)                                               # (2)
    y0 += f2 * es('tim,ta->iam', b['oc'], r2)                                               # (3)
    y1 = -f2 * es('ia,atm->itm', r0, b['vo'])                                               # (2)
    y1 += f11 * (es('jim,ju->ium', b['cc'], r1) + k11 * es('utm,it->ium', b['oo'], r1))     # (11)
    y1 += f13 * es('wim,wu->ium', b['oc'], r3)                                              # (13)
    y1 += f14 * es('uim,u->ium', b['oc'], g4)                                               # (14)
    y2 = -f2 * es('ia,tim->tam', r0, b['oc'])                                               # (3)
    y2 += f11 * (es('abm,ub->uam', b['vv'], r2) + k11 * es('tum,ta->uam', b['oo'], r2))     # (20)
    y2 += f21 * es('atm,ut->uam', b['vo'], r3)                                              # (21)
    y2 += f14 * es('aum,u->uam', b['vo'], g4)                                               # (22)
    y3 = -f13 * es('it,wim->wtm', r1, b['oc'])                                              # (13)
    y3 -= f21 * es('wa,atm->wtm', r2, b['vo'])                                              # (21)
    y3 += f28 * (es('wvm,wu->vum', b['oo'], r3) + es('utm,vt->vum', b['oo'], r3))           # (28)
    y3 += f28 * (es('uvm,u->vum', b['oo'], r4) + es('uvm,v->vum', b['oo'], r4 - r4.sum() / S))   # (29)
    q = es('iu,uim->um', r1, b['oc']) + es('ua,aum->um', r2, b['vo'])                       # (14), (22)
    y4 = -f14 * ((1 - S) / S * q.sum(axis=0)[None, :] + 2 * (S - 1) * q)
    y4 -= f28 * (es('vt,tvm->tm', r3, b['oo']) + es('tu,utm->tm', r3, b['oo'])
                 - es('vu,uvm->m', r3, b['oo'])[None, :] / S)                               # (29)
    return join([y0, y1, y2, y3, y4])


def img_sm_gs(b, S, n):
    """interact_S_1GS, cases 6, 15, 23, 30 (36 is zero)."""
    m = b['cc'].shape[-1]
    return join([sqrt((2 * S - 1) / (2 * S + 1)) * b['vc'].transpose(1, 0, 2),
                 sqrt((2 * S - 1) / (2 * S)) * b['oc'].transpose(1, 0, 2),
                 sqrt((2 * S - 1) / (2 * S)) * b['vo'].transpose(1, 0, 2),
                 b['oo'].transpose(1, 0, 2), np.zeros((n[1], m), dtype=b['cc'].dtype)])


def img_sm_so(b, S, n, xr):
    """interact_S_1S, cases 7-40."""
    r0, r1, r2, r3 = split_so(xr, *n)
    q = sqrt((2 * S - 1) / (2 * S + 1))
    f10 = -sqrt((1 + S) * (2 * S - 1) / (2 * S * (2 * S + 1)))
    f16 = sqrt((2 * S - 1) / S) / 2
    f17 = -sqrt((2 * S - 1) / (2 * S))
    f19 = -sqrt((1 + S) * (2 * S - 1)) / (2 * S)
    y0 = q / R2 * (es('abm,ib->iam', b['vv'], r0) - es('jim,ja->iam', b['cc'], r0))         # (7)
    y0 -= q / (2 * S) * es('atm,it->iam', b['vo'], r1)                                      # (8)
    y0 += q / (2 * S) * es('tim,ta->iam', b['oc'], r2)                                      # (9)
    y0 += f10 * (es('abm,ib->iam', b['vv'], r3) + es('jim,ja->iam', b['cc'], r3))           # (10)
    y1 = f16 * es('ubm,ib->ium', b['ov'], r0)                                               # (16)
    y1 += f17 * (es('jim,ju->ium', b['cc'], r1) + es('utm,it->ium', b['oo'], r1) / (2 * S - 1))   # (17)
    y1 += f19 * es('ubm,ib->ium', b['ov'], r3)                                              # (19)
    y2 = -f16 * es('jum,ja->uam', b['co'], r0)                                              # (24)
    y2 -= f17 * (es('abm,ub->uam', b['vv'], r2) + es('tum,ta->uam', b['oo'], r2) / (2 * S - 1))   # (26)
    y2 += f19 * es('jum,ja->uam', b['co'], r3)                                              # (27)
    y3 = -es('jvm,ju->vum', b['co'], r1) + es('ubm,vb->vum', b['ov'], r2)                   # (32), (33)
    p = -es('jtm,jt->tm', b['co'], r1) + es('tbm,tb->tm', b['ov'], r2)                      # (38), (39)
    y4 = p - p.sum(axis=0)[None, :] / (2 * S)
    return join([y0, y1, y2, y3, y4])


def row_gs_so(b, S, n, xr):
    """interact_GSS, cases 42-45."""
    _, r1, r2, r3 = split_so(xr, *n)
    t = -es('jvm,jv->m', b['co'], r1) / R2 + es('vbm,vb->m', b['ov'], r2) / R2              # (43), (44)
    if S != 0:
        t = t - sqrt(S / (1 + S)) * es('jbm,jb->m', b['cv'], r3)                            # (45)
    return t


def row_gs_sp(b, S, n, xr):
    """interact_GSS1, case 46."""
    return -es('jbm,jb->m', b['cv'], xr.reshape(n[0], n[2]))


def img_so_so(b, S, n, xr):
    """interact_SS, cases 47-59."""
    r0, r1, r2, r3 = split_so(xr, *n)
    y0 = -0.5 * es('avm,iv->iam', b['vo'], r1) - 0.5 * es('vim,va->iam', b['oc'], r2)       # (48), (49)
    y1 = 0.5 * es('ia,avm->ivm', r0, b['vo'])                                               # (48)
    y1 -= (es('uvm,iv->ium', b['oo'], r1) - es('jim,ju->ium', b['cc'], r1)) / R2            # (52)
    y2 = 0.5 * es('ib,vim->vbm', r0, b['oc'])                                               # (49)
    y2 += (es('abm,ub->uam', b['vv'], r2) - es('vum,va->uam', b['oo'], r2)) / R2            # (56)
    y3 = np.zeros(r3.shape + (b['cc'].shape[-1],), dtype=y0.dtype)
    if S != 0:
        f50 = -sqrt(S / (2 * (1 + S)))
        f54 = (1 - S) / (2 * sqrt(S * (S + 1)))
        f59 = 1 / (R2 * (1 + S))
        y0 += f50 * (es('abm,ib->iam', b['vv'], r3) - es('jim,ja->iam', b['cc'], r3))       # (50)
        y1 += f54 * es('ubm,ib->ium', b['ov'], r3)                                          # (54)
        y2 -= f54 * es('jum,ja->uam', b['co'], r3)                                          # (57)
        y3 += f50 * (-es('ja,abm->jbm', r0, b['vv']) + es('ib,jim->jbm', r0, b['cc']))      # (50)
        y3 -= f54 * es('ju,ubm->jbm', r1, b['ov'])                                          # (54)
        y3 += f54 * es('ub,jum->jbm', r2, b['co'])                                          # (57)
        y3 += f59 * (es('abm,ib->iam', b['vv'], r3) + es('jim,ja->iam', b['cc'], r3))       # (59)
    return join([y0, y1, y2, y3])


def img_so_sp(b, S, n, xr):
    """interact_SS1, cases 51, 55, 58, 60."""
    r = xr.reshape(n[0], n[2])
    y0 = (es('jim,ja->iam', b['cc'], r) - es('abm,ib->iam', b['vv'], r)) / R2               # (51)
    y1 = -es('ubm,ib->ium', b['ov'], r)                                                     # (55)
    y2 = es('jum,ja->uam', b['co'], r)                                                      # (58)
    y3 = np.zeros_like(y0)
    if S != 0:
        y3 = -sqrt(S / (2 * (S + 1))) * (es('jim,ja->iam', b['cc'], r) + es('abm,ib->iam', b['vv'], r))   # (60)
    return join([y0, y1, y2, y3])


def img_sp_sp(b, S, n, xr):
    """interact_S1S1, case 61."""
    r = xr.reshape(n[0], n[2])
    return ((es('abm,ib->iam', b['vv'], r) + es('jim,ja->iam', b['cc'], r)) / R2).reshape(-1, b['cc'].shape[-1])


# ---- moments (tdm.py), operator symmetric --------------------------------------------
def tdm_sm(b, S, n, xl, xr):
    """TDM_S_1 (tdm.py:156-238) for one pair."""
    l0, l1, l2, l3, l4 = split_sm(xl, *n)
    r0, r1, r2, r3, r4 = split_sm(xr, *n)
    t = es('ia,abm,ib->m', l0, b['vv'], r0) - es('ia,jim,ja->m', l0, b['cc'], r0)           # 1
    t += es('iu,utm,it->m', l1, b['oo'], r1) - es('iu,jim,ju->m', l1, b['cc'], r1)          # 2
    t += es('ua,abm,ub->m', l2, b['vv'], r2) - es('ua,tum,ta->m', l2, b['oo'], r2)          # 3
    t += es('vu,utm,vt->m', l3, b['oo'], r3) - es('vu,wvm,wu->m', l3, b['oo'], r3)          # 4
    f = sqrt((2 * S + 1) / (2 * S))
    t += f * (es('ia,atm,it->m', l0, b['vo'], r1) + es('it,atm,ia->m', l1, b['vo'], r0))    # 6, 7
    t -= f * (es('ia,tim,ta->m', l0, b['oc'], r2) + es('tb,tim,ib->m', l2, b['oc'], r0))    # 8, 9
    f = -sqrt(2 * S / (2 * S - 1))
    t += f * (es('iu,wim,wu->m', l1, b['oc'], r3) + es('wt,wim,it->m', l3, b['oc'], r1))    # 16, 17
    t -= f * (es('ua,atm,ut->m', l2, b['vo'], r3) + es('ut,atm,ua->m', l3, b['vo'], r2))    # 20, 21
    f = -2 * S / sqrt(2 * S * (2 * S - 1))
    t += f * (es('iu,uim,u->m', l1, b['oc'], r4) + es('u,uim,iu->m', l4, b['oc'], r1))      # 18, 19
    t -= f * (es('ua,aum,u->m', l2, b['vo'], r4) + es('u,aum,ua->m', l4, b['vo'], r2))      # 22, 23
    t += es('vu,uvm,v->m', l3, b['oo'], r4) - es('vu,uvm,u->m', l3, b['oo'], r4)            # 24
    t += es('t,utm,tu->m', l4, b['oo'], r3) - es('t,tvm,vt->m', l4, b['oo'], r3)            # 25
    return t


def tdm_gs_so(b, S, n, xr):
    """TDM_GSS (tdm.py:14-42)."""
    r0, r1, r2, _ = split_so(xr, *n)
    return R2 * es('bjm,jb->m', b['vc'], r0) + es('jtm,jt->m', b['co'], r1) + es('tbm,tb->m', b['ov'], r2)


def tdm_so(b, S, n, xl, xr):
    """TDM_S (tdm.py:61-126) for one pair, in tdm.py's own CV(1) phase (+g)."""
    l0, l1, l2, l3 = split_so(xl, *n)
    r0, r1, r2, r3 = split_so(xr, *n)
    t = es('ia,bam,ib->m', l0, b['vv'], r0) - es('ia,jim,ja->m', l0, b['cc'], r0)           # (21)
    if S != 0:
        t += es('iu,vum,iv->m', l1, b['oo'], r1) - es('iu,jim,ju->m', l1, b['cc'], r1)      # (25)
        t += es('ua,abm,ub->m', l2, b['vv'], r2) - es('ua,uvm,va->m', l2, b['oo'], r2)      # (28)
        t += es('ia,abm,ib->m', l3, b['vv'], r3) - es('ia,jim,ja->m', l3, b['cc'], r3)      # (30)
        t += (es('ia,atm,it->m', l0, b['vo'], r1) + es('it,atm,ia->m', l1, b['vo'], r0)) / R2    # (22)
        t -= (es('ia,tim,ta->m', l0, b['oc'], r2) + es('tb,tim,ib->m', l2, b['oc'], r0)) / R2    # (23)
        g = sqrt((1 + S) / (2 * S))
        t += g * (es('iu,ubm,ib->m', l1, b['ov'], r3) + es('ib,ubm,iu->m', l3, b['ov'], r1))     # (24)
        t += g * (es('ua,jum,ja->m', l2, b['co'], r3) + es('jb,jum,ub->m', l3, b['co'], r2))     # (24)
    return t


def tdm_sp(b, S, n, xl, xr):
    """TDM_S1 (tdm.py:128-154)."""
    l, r = xl.reshape(n[0], n[2]), xr.reshape(n[0], n[2])
    return es('ia,abm,ib->m', l, b['vv'], r) - es('ia,jim,ja->m', l, b['cc'], r)


# ---- all pairs, in the layout of xt_si_couple ---------------------------------------
def couple(op, s, nc, no, nv, x_sm=None, x_so=None, x_sp=None, with_ground=True, mode="soc", device=None):
    """(ncomp, n, n) with the groups |S->, |GS>, |So>, |S+>: what ``xt_si_couple`` returns
    (``xtddft_amd.soc.si_couple`` has this signature).  ``op`` (ncomp, nmo, nmo), real or
    complex.  'soc': same-manifold blocks in full, the others with L before R; 'dipole': the
    same-S blocks."""
    op = np.asarray(op)
    d = np.ascontiguousarray(op.transpose(1, 2, 0))
    b = op_blocks(d, nc, no, nv)
    n = (nc, no, nv)
    S = float(s)
    xs = {'|S->': np.zeros((0, 0)) if x_sm is None else np.asarray(x_sm),
          '|GS>': np.ones((1 if with_ground else 0, 1)),
          '|So>': np.zeros((0, 0)) if x_so is None else np.asarray(x_so),
          '|S+>': np.zeros((0, 0)) if x_sp is None else np.asarray(x_sp)}
    first, k = {}, 0
    for g in GROUPS:
        first[g] = k
        k += xs[g].shape[0]
    out = np.zeros((op.shape[0], k, k), dtype=op.dtype)

    def put(gl, i, gr, j, val):
        out[:, first[gl] + i, first[gr] + j] = val
    images = {('|S->', '|S->'): img_sm_sm, ('|S->', '|So>'): img_sm_so, ('|So>', '|So>'): img_so_so,
              ('|So>', '|S+>'): img_so_sp, ('|S+>', '|S+>'): img_sp_sp}
    if mode == "soc":
        for (gl, gr), fn in images.items():
            for j, xr in enumerate(xs[gr] if xs[gl].shape[0] else ()):
                y = fn(b, S, n, xr)
                for i, xl in enumerate(xs[gl]):
                    put(gl, i, gr, j, xl @ y)
        if with_ground:
            if xs['|S->'].shape[0]:
                y = img_sm_gs(b, S, n)
                for i, xl in enumerate(xs['|S->']):
                    put('|S->', i, '|GS>', 0, xl @ y)
            for j, xr in enumerate(xs['|So>']):
                put('|GS>', 0, '|So>', j, row_gs_so(b, S, n, xr))
            for j, xr in enumerate(xs['|S+>']):
                put('|GS>', 0, '|S+>', j, row_gs_sp(b, S, n, xr))
    elif mode == "dipole":
        for g, fn in (('|S->', tdm_sm), ('|So>', tdm_so), ('|S+>', tdm_sp)):
            for i, xl in enumerate(xs[g]):
                for j, xr in enumerate(xs[g]):
                    put(g, i, g, j, fn(b, S, n, xl, xr))
        if with_ground:
            for j, xr in enumerate(xs['|So>']):
                put('|GS>', 0, '|So>', j, tdm_gs_so(b, S, n, xr))
    else:
        raise ValueError(mode)
    return out


# ---- H_eff as the reference assembles it ------------------------------------------------
@lru_cache(maxsize=None)
def w_sympy(S, M, Sp, Mp):
    """si_driver.py:46-65 with sympy's 3j symbols."""
    from sympy import Rational
    from sympy.physics.wigner import wigner_3j
    S, M, Sp, Mp = (Rational(int(round(2 * float(v))), 2) for v in (S, M, Sp, Mp))
    den = wigner_3j(S, 1, Sp, -S, S - Sp, Sp)
    if abs(float(den)) < 1e-9:
        return 0.0
    return float((-1) ** int(S - M) * wigner_3j(S, 1, Sp, -M, M - Mp, Mp) / den)


def hm_of(vso):
    """(3, nmo, nmo) complex: h^-1, h^0, h^+1 (cal_hm's reversed order)."""
    return np.array([-1j * vso[0] - vso[1], 1j * R2 * vso[2], 1j * vso[0] - vso[1]])


def heff(vso, S, nc, no, nv, states, ngs=1, wfun=None):
    """(heff, hso, Omega) by the reference's loops over (L, R, ML, MR): upper triangle,
    Hermitian completion, zero diagonal of hso, Omega on the diagonal.  ``states`` maps
    '|S->', '|So>', '|S+>' to lists of (e, X)."""
    wfun = wfun or w_sympy
    st = {g: list(states.get(g, [])) for g in GROUPS}
    st['|GS>'] = [(0.0, np.ones(1))] if ngs else []
    rows = {g: np.array([np.asarray(x, dtype=float) for _, x in st[g]]) if st[g] else np.zeros((0, 0))
            for g in GROUPS}
    spin = {'|S->': S - 1, '|GS>': S, '|So>': S, '|S+>': S + 1}
    h = couple(hm_of(np.asarray(vso)), S, nc, no, nv, rows['|S->'], rows['|So>'], rows['|S+>'], bool(ngs), "soc")
    first, off, k, p = {}, {}, 0, 0
    for g in GROUPS:
        first[g], off[g] = k, p
        k += len(st[g])
        p += int(round(2 * spin[g] + 1)) * len(st[g]) if spin[g] >= 0 else 0
    hso = np.zeros((p, p), dtype=complex)
    omega = np.zeros((p, p))
    for gl in GROUPS:
        for li, (el, _) in enumerate(st[gl]):
            for gr in GROUPS:
                for ri in range(len(st[gr])):
                    sl, sr = spin[gl], spin[gr]
                    for ml in np.arange(-sl, sl + 1):
                        for mr in np.arange(-sr, sr + 1):
                            lp = int(off[gl] + (ml + sl) * len(st[gl]) + li)
                            rp = int(off[gr] + (mr + sr) * len(st[gr]) + ri)
                            if lp <= rp and abs(mr - ml) <= 1 and abs(sr - sl) <= 1:
                                hso[lp, rp] = h[int(mr - ml) + 1, first[gl] + li, first[gr] + ri] * wfun(sl, ml, sr, mr)
                            if lp == rp:
                                omega[lp, rp] = el
    hso = np.triu(hso) + np.triu(hso, 1).T.conj()
    hso = hso - np.diag(np.diag(hso))
    return hso + omega, hso, omega


# ---- random inputs ------------------------------------------------------------------------
def dims(nc, no, nv):
    cv, co, ov = nc * nv, nc * no, no * nv
    return cv + co + ov + no * no + no, 2 * cv + co + ov, cv


def random_problem(nc, no, nv, counts, seed=0, scale=1.0):
    """Seeded orthonormal states per manifold (an O1O2 block has a zero diagonal), sorted
    random energies, an antisymmetric ``vso`` and a symmetric ``dip`` (3, nmo, nmo)."""
    rng = np.random.default_rng(seed)
    nmo = nc + no + nv
    a = rng.standard_normal((3, nmo, nmo))
    vso = scale * (a - a.transpose(0, 2, 1))
    a = rng.standard_normal((3, nmo, nmo))
    dip = a + a.transpose(0, 2, 1)
    states = {}
    for key, dim, cnt in zip(('|S->', '|So>', '|S+>'), dims(nc, no, nv), counts):
        x = rng.standard_normal((cnt, dim))
        if key == '|S->' and cnt:
            o0 = nc * nv + nc * no + no * nv
            x[:, o0 + np.arange(no) * (no + 1)] = 0.0
        if key == '|So>' and no == 0 and cnt:
            x[:, nc * nv:] = 0.0                      # S = 0: no CV(1) amplitudes (reformat_S)
        if cnt:
            q, _ = np.linalg.qr(x.T)
            x = q.T
            if key == '|S->':
                x[:, o0 + np.arange(no) * (no + 1)] = 0.0
        e = np.sort(rng.random(cnt)) + 0.1
        states[key] = [(float(e[i]), x[i].copy()) for i in range(cnt)]
    return vso, dip, states


def rows_of(states, key, dim):
    return np.array([x for _, x in states.get(key, [])], dtype=float).reshape(len(states.get(key, [])), dim)


# ---- exactly solvable limits -----------------------------------------------------------------
PAULI = np.array([[[0, 1], [1, 0]], [[0, -1j], [1j, 0]], [[1, 0], [0, -1]]], dtype=complex)


def one_body(vso):
    """sum_k (i Vso_k) (x) sigma_k over spin orbitals 2 p + sigma (0 up, 1 down)."""
    return sum(np.kron(1j * vso[k], PAULI[k]) for k in range(3))


def two_electron(h1):
    """h (x) 1 + 1 (x) h on the product space of two spin orbitals."""
    eye = np.eye(h1.shape[0])
    return np.kron(h1, eye) + np.kron(eye, h1)


def det(nso, p, q):
    """The normalised determinant |p q| of two spin orbitals in the product space."""
    v = np.zeros((nso, nso))
    v[p, q], v[q, p] = 1.0, -1.0
    return v.ravel() / R2


def singlet(nso, p, q):
    return det(nso, 2 * p, 2 * p + 1) if p == q else (det(nso, 2 * p, 2 * q + 1) - det(nso, 2 * p + 1, 2 * q)) / R2


def triplet(nso, p, q):
    return [det(nso, 2 * p + 1, 2 * q + 1), (det(nso, 2 * p, 2 * q + 1) + det(nso, 2 * p + 1, 2 * q)) / R2,
            det(nso, 2 * p, 2 * q)]


def unit(dim, k):
    v = np.zeros(dim)
    v[k] = 1.0
    return v


def limit(name, k=2, seed=0):
    """One exactly solvable limit: ``dict(nc, no, nv, S, vso, states, exact)``; ``exact`` are
    the eigenvalues of H_so + diag(energies) projected on the explicitly written spin
    eigenfunctions, H_so = sum_electrons sum_k (i Vso_k) (x) sigma_k.
      'a' one particle  nc=0, no=1, nv=k, S=1/2, |So> = unit vectors on OV(0)
      'b' one hole      nc=k, no=1, nv=0, S=1/2, |So> = unit vectors on CO(0)
      'c' closed shell  nc=1, no=0, nv=k, S=0, singlets (c,a) in |So>, triplets in |S+>
      'd' triplet       nc=0, no=2, nv=k, S=1, triplets (o_other, v_a) in |So>; in |S-> their
          singlets (OV(1)), the closed shells o_v^2 (off-diagonal O1O2) and the open-shell
          singlet (O1O1 = (1, -1)/sqrt 2)"""
    rng = np.random.default_rng(seed)
    nc, no, nv, S = {'a': (0, 1, k, 0.5), 'b': (k, 1, 0, 0.5), 'c': (1, 0, k, 0.0), 'd': (0, 2, k, 1.0)}[name]
    nmo = nc + no + nv
    a = rng.standard_normal((3, nmo, nmo))
    vso = a - a.transpose(0, 2, 1)
    dsm, dso, dsp = dims(nc, no, nv)
    states = {'|S->': [], '|So>': [], '|S+>': []}
    if name == 'a':
        e = np.sort(rng.random(k)) + 0.5
        states['|So>'] = [(e[a_], unit(dso, a_)) for a_ in range(k)]
        exact = np.linalg.eigvalsh(np.kron(np.diag(np.concatenate([[0.0], e])), np.eye(2)) + one_body(vso))
    elif name == 'b':
        e = np.sort(rng.random(k)) + 0.5
        states['|So>'] = [(e[j], unit(dso, j)) for j in range(k)]        # CO(0): cv = 0, so offset 0
        order = [nc] + list(range(nc))                                   # [o, c...]
        v = vso[:, order][:, :, order]
        exact = np.linalg.eigvalsh(np.kron(np.diag(np.concatenate([[0.0], e])), np.eye(2)) - one_body(v))
    else:
        nso = 2 * nmo
        h2 = two_electron(one_body(vso))
        basis, energy = [], []
        if name == 'c':
            es_, et = np.sort(rng.random(k)) + 0.5, np.sort(rng.random(k)) + 0.3
            states['|So>'] = [(es_[a_], unit(dso, a_)) for a_ in range(k)]
            states['|S+>'] = [(et[a_], unit(dsp, a_)) for a_ in range(k)]
            basis.append(singlet(nso, 0, 0)); energy.append(0.0)
            for a_ in range(k):
                basis.append(singlet(nso, 0, 1 + a_)); energy.append(es_[a_])
                for t in triplet(nso, 0, 1 + a_):
                    basis.append(t); energy.append(et[a_])
        else:
            et = np.sort(rng.random(2 * k)) + 0.5
            eov, eoo, e11 = rng.random(2 * k) + 0.3, rng.random(2) + 0.2, float(rng.random()) + 0.1
            for t in triplet(nso, 0, 1):
                basis.append(t); energy.append(0.0)
            ov0, ov1 = nc * nv + nc * no, nc * nv + nc * no            # both layouts: OV after CV, CO
            o12 = ov1 + no * nv
            for u in range(2):
                for a_ in range(k):
                    idx = u * nv + a_
                    states['|So>'].append((et[idx], unit(dso, ov0 + idx)))
                    for t in triplet(nso, 1 - u, 2 + a_):
                        basis.append(t); energy.append(et[idx])
                    states['|S->'].append((eov[idx], unit(dsm, ov1 + idx)))
                    basis.append(singlet(nso, 1 - u, 2 + a_)); energy.append(eov[idx])
            for u, v_ in ((0, 1), (1, 0)):                               # X[u,v], u != v: o_v^2
                states['|S->'].append((eoo[u], unit(dsm, o12 + u * no + v_)))
                basis.append(singlet(nso, v_, v_)); energy.append(eoo[u])
            x = np.zeros(dsm)
            x[o12 + no * no:] = np.array([1.0, -1.0]) / R2
            states['|S->'].append((e11, x))
            basis.append(singlet(nso, 0, 1)); energy.append(e11)
        p = np.array(basis).T
        exact = np.linalg.eigvalsh(p.conj().T @ h2 @ p + np.diag(energy))
    return dict(nc=nc, no=no, nv=nv, S=S, vso=vso, states=states, exact=np.sort(exact))
