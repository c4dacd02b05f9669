"""NumPy restatement of the simplified open-shell TDA (sX-TDA / sU-TDA) of the reference's
``xtddft/sTDA/os_sTDA.py``, term by term, as the oracle of ``xt_stda_*`` and ``xtddft_amd.OSsTDA``.

The device generates matrix elements of a CSF list one 16 x 16 tile at a time from pair-major
operands; this file works the other way round: dense ``(atom, orbital, orbital)`` charge
tensors as the reference builds them (os_sTDA.py:644-670), whole-list products, and for the
driver the full active space at once (every CSF's diagonal, the whole P x N block of B), from
which the selected A is cut.

A problem is a dict:
  natm, nc, no, nv, nocc (2), nvir (2)
  qoo, qov, qvv   per spin, (natm, nocc, nocc) / (natm, nocc, nvir) / (natm, nvir, nvir)
  gk, gj          gamma^K, gamma^J (natm, natm)
  foo, fvv        per spin, KS Fock blocks
  hoo, hvv        per spin, ROHF-type Fock blocks, or None (spin-orbital)
  sa, si          spin_adapted and S
  correct, dmax, sigk
A CSF list is an int array (n, 3) of (spin, i, a) in the spin's own numbering.
"""
import numpy as np

HA2EV = 27.2113834          # xtddft/utils/unit.py (ORCA's value)
TP = 1e-4                   # the reference's hard-coded selection threshold (os_sTDA.py:951)


# --------------------------------------------------------------------------- operands
def sqrt_overlap(s):
    """S^1/2 by diagonalisation (os_sTDA.py:637-638)."""
    w, u = np.linalg.eigh(s)
    return (u * np.sqrt(w)) @ u.T


def gamma(dist, eta_ev, hyb, paramtype="os"):
    """(gamma^J, gamma^K): Mataga-Nishimoto-Ohno-Klopman damped Coulomb matrices
    (OSsTDA.gamma, os_sTDA.py:408-433).  dist: inter-atomic distances in Bohr; eta_ev: the
    chemical hardness of every atom in eV."""
    eta = 2.0 * np.asarray(eta_ev, dtype=np.float64) / HA2EV
    eta = 0.5 * (eta[:, None] + eta[None, :])
    if paramtype == "cs":
        beta = 0.20 + hyb * 1.83
        gj = (1.0 / (dist ** beta + (hyb * eta) ** (-beta))) ** (1.0 / beta)
    elif paramtype == "os":
        beta = hyb + 0.3
        gj = (1.0 / (dist ** beta + (1.4 * hyb * eta) ** (-beta))) ** (1.0 / beta)
    else:
        raise ValueError(paramtype)
    alpha = 1.42 + hyb * 0.48
    gk = (1.0 / (dist ** alpha + eta ** (-alpha))) ** (1.0 / alpha)
    return gj, gk


def charges(cprime, ao_off, nocc):
    """q_oo, q_ov, q_vv of one spin, (natm, ., .): q^A_pq = sum_{mu in A} C'_mu,p C'_mu,q
    (os_sTDA.py:650-662)."""
    natm = len(ao_off) - 1
    nmo = cprime.shape[1]
    q = np.zeros((natm, nmo, nmo))
    for a in range(natm):
        blk = cprime[ao_off[a]:ao_off[a + 1]]
        q[a] = blk.T @ blk
    return q[:, :nocc, :nocc], q[:, :nocc, nocc:], q[:, nocc:, nocc:]


def x_coefficients(si):
    """c1, c2, c3 of the spin-adapted correction (os_sTDA.py:277-283, 294, 316-322)."""
    rt = np.sqrt((si + 1.0) / si)
    return 0.5 * (1 - rt + 1 / (2 * si)), 0.5 * (-1 + rt + 1 / (2 * si)), 1 / (4 * si)


# --------------------------------------------------------------------------- the generator
def generator(pr, rows, cols, full=True, same=False):
    """The (len(rows), len(cols)) block of A between two CSF lists.  full=False: the first two
    lines only (the selection's B, the active iajb_f of os_sTDA.py:235-260).  same: the two
    lists are one list, so the correction sits where row = column."""
    rows = np.asarray(rows).reshape(-1, 3)
    cols = np.asarray(cols).reshape(-1, 3)
    sp, ip, ap = rows.T
    sq, iq, aq = cols.T
    nc, no = pr["nc"], pr["no"]
    out = np.zeros((len(rows), len(cols)))
    kline = np.zeros_like(out)
    # line 1: every spin pair
    for s in (0, 1):
        for t in (0, 1):
            r, c = np.where(sp == s)[0], np.where(sq == t)[0]
            if r.size == 0 or c.size == 0:
                continue
            ql = pr["qov"][s][:, ip[r], ap[r]]                      # (natm, nr)
            qr = pr["qov"][t][:, iq[c], aq[c]]
            kline[np.ix_(r, c)] = np.einsum('np,nm,mq->pq', ql, pr["gk"], qr)
    out += kline
    for s in (0, 1):
        r, c = np.where(sp == s)[0], np.where(sq == s)[0]
        if r.size == 0 or c.size == 0:
            continue
        i, j = ip[r][:, None], iq[c][None, :]
        a, b = ap[r][:, None], aq[c][None, :]
        # line 2: same spin
        out[np.ix_(r, c)] -= np.einsum('npq,nm,mpq->pq', pr["qoo"][s][:, i, j], pr["gj"], pr["qvv"][s][:, a, b])
        if full:   # line 3
            out[np.ix_(r, c)] += (i == j) * pr["fvv"][s][a, b] - (a == b) * pr["foo"][s][i, j]
    if full and pr["sa"] and no > 0:   # line 4: both CSFs of class CV
        c1, c2, c3 = x_coefficients(pr["si"])
        cvr = np.where(sp == 0, ip < nc, ap >= no)
        cvc = np.where(sq == 0, iq < nc, aq >= no)
        r, c = np.where(cvr)[0], np.where(cvc)[0]
        if r.size and c.size:
            i, j = ip[r][:, None], iq[c][None, :]
            a = np.where(sp[r] == 0, ap[r], ap[r] - no)[:, None]     # alpha virtual index
            b = np.where(sq[c] == 0, aq[c], aq[c] - no)[None, :]
            dab = pr["hvv"][1][no + a, no + b] - pr["hvv"][0][a, b]
            dij = pr["hoo"][1][i, j] - pr["hoo"][0][i, j]
            s1, s2 = sp[r][:, None], sq[c][None, :]
            cij = np.where(s1 != s2, c3, np.where(s1 == 0, c1, c2))
            cab = np.where(s1 != s2, c3, np.where(s1 == 0, c2, c1))
            out[np.ix_(r, c)] += cij * (i == j) * dab + cab * (a == b) * dij
    if full and pr["correct"] and same:   # line 5
        k = np.diag(kline)
        out[np.diag_indices(len(rows))] += pr["dmax"] / (1.0 + (k / pr["sigk"]) ** 4)
    return out, kline


def matrix(pr, csf):
    return generator(pr, csf, csf, full=True, same=True)[0]


def diag(pr, csf):
    """(E_p, K_pp) of a list, one CSF at a time."""
    csf = np.asarray(csf).reshape(-1, 3)
    e, k = np.empty(len(csf)), np.empty(len(csf))
    for n, c in enumerate(csf):
        a, kl = generator(pr, c[None], c[None], full=True, same=True)
        e[n], k[n] = a[0, 0], kl[0, 0]
    return e, k


def weights(pr, csf_p, e_p, csf_n, e_n):
    """w_q = sum_{p in P} B[p,q]^2 / (E_q - E_p + 1e-10) (os_sTDA.py:259, 752-793)."""
    b = generator(pr, csf_p, csf_n, full=False)[0]
    return (b ** 2 / (np.asarray(e_n)[None, :] - np.asarray(e_p)[:, None] + 1e-10)).sum(axis=0)


# --------------------------------------------------------------------------- the driver
def active_window(mo_occ, mo_energy, hyb, emax):
    """First and last orbital (inclusive) of the CAS window (os_sTDA.py:504-548)."""
    upe = np.nonzero(mo_occ[0] - mo_occ[1])[0]
    if upe.size == 0:
        raise ValueError("the CAS window is defined by the open shells: there are none")
    somo_lo, somo_hi = mo_energy[0, upe[0]], mo_energy[0, upe[-1]]
    sumo_lo, sumo_hi = mo_energy[1, upe[0]], mo_energy[1, upe[-1]]
    deps = (1.0 + 0.8 * hyb) * emax / HA2EV
    nc = max(np.count_nonzero((mo_energy[0] > somo_lo - 2 * deps) & (mo_energy[0] < somo_lo)),
             np.count_nonzero((mo_energy[1] > sumo_lo - 2 * deps) & (mo_energy[1] < sumo_lo)))
    nv = max(np.count_nonzero((mo_energy[0] < somo_hi + 2 * deps) & (mo_energy[0] > somo_hi)),
             np.count_nonzero((mo_energy[1] < sumo_hi + 2 * deps) & (mo_energy[1] > sumo_hi)))
    return int(upe[0] - nc), int(upe[-1] + nv)


def class_lists(nc, no, nv):
    """Every CSF of the active space, class by class in the reference's order
    CV(aa) | OV(aa) | CO(bb) | CV(bb), each (i, a) row-major in the class's own local indices
    (os_sTDA.py:733-736, 989-1000)."""
    def grid(ni, na):
        i, a = np.indices((ni, na))
        return i.ravel(), a.ravel()
    return [grid(nc, nv), grid(no, nv), grid(nc, no), grid(nc, nv)]


def to_triples(cls, i, a, nc, no):
    """Class-local (i, a) -> (spin, i, a) in the spin's numbering: OV(aa) occupied nc + i,
    CV(bb) virtual no + a."""
    i, a = np.asarray(i, dtype=np.int64), np.asarray(a, dtype=np.int64)
    s = np.full(i.shape, 0 if cls < 2 else 1, dtype=np.int64)
    if cls == 1:
        i = i + nc
    if cls == 3:
        a = a + no
    return np.stack([s, i, a], axis=1).reshape(-1, 3)


def _merge(nc, x, y, op):
    """Per occupied index, the union / intersection of the virtual indices of two (i, a)
    lists, sorted (union / intersec, os_sTDA.py:66-87)."""
    oi, oa = [], []
    for i in range(nc):
        v = op(x[1][x[0] == i], y[1][y[0] == i])
        oi.append(np.full(v.size, i, dtype=np.int64))
        oa.append(v.astype(np.int64))
    return np.concatenate(oi) if oi else np.zeros(0, np.int64), np.concatenate(oa) if oa else np.zeros(0, np.int64)


def select(pr, emax, union=True, tp=TP):
    """The P / S selection over the whole active space (os_sTDA.py:682-985).  Returns the four
    class-local index lists [(i, a)] of P u S in the final order, the counts the reference
    prints, and every selection weight with its N list."""
    nc, no, nv = pr["nc"], pr["no"], pr["nv"]
    shapes = [(nc, nv), (no, nv), (nc, no), (nc, nv)]
    cls = class_lists(nc, no, nv)
    e_cls = [diag(pr, to_triples(k, *cls[k], nc, no))[0].reshape(shapes[k]) for k in range(4)]
    p = [tuple(np.where(e * HA2EV <= emax)) for e in e_cls]
    n = [tuple(np.where(e * HA2EV > emax)) for e in e_cls]
    counts = {"p_cva_before_union": len(p[0][0]), "p_cvb_before_union": len(p[3][0])}
    if union:
        p[0] = p[3] = _merge(nc, p[0], p[3], np.union1d)
        n[0] = n[3] = _merge(nc, n[0], n[3], np.intersect1d)
    p_tr = np.concatenate([to_triples(k, *p[k], nc, no) for k in range(4)])
    n_tr = np.concatenate([to_triples(k, *n[k], nc, no) for k in range(4)])
    e_p = np.concatenate([e_cls[k][p[k]] for k in range(4)])
    e_n = np.concatenate([e_cls[k][n[k]] for k in range(4)])
    w = weights(pr, p_tr, e_p, n_tr, e_n) if len(n_tr) else np.zeros(0)
    hit = w >= tp
    ps, off = [], 0
    for k in range(4):
        m = len(n[k][0])
        sel = np.where(hit[off:off + m])[0]
        off += m
        i = np.concatenate([p[k][0], n[k][0][sel]])
        a = np.concatenate([p[k][1], n[k][1][sel]])
        order = np.argsort(i, kind="stable")
        ps.append((i[order], a[order]))
    counts["s_cva_before_union"] = len(ps[0][0]) - len(p[0][0])
    counts["s_cvb_before_union"] = len(ps[3][0]) - len(p[3][0])
    if union:
        ps[0] = _merge(nc, ps[0], ps[3], np.union1d)
    ps[3] = ps[0]          # the reference sets CV(bb) = CV(aa) with and without union (os_sTDA.py:963-965)
    counts["pcsf"] = [len(x[0]) for x in p]
    counts["pscsf"] = [len(x[0]) for x in ps]
    counts["ncsf"] = len(w) - (sum(counts["pscsf"]) - sum(counts["pcsf"]))
    return ps, counts, w


def solve(pr, emax, union=True, tp=TP, nstates=10):
    """(e, v, A, index lists, counts, weights): the reference's kernel() from the selection to
    the roots (os_sTDA.py:682-1282); emax None / 0 takes every CSF."""
    nc, no, nv = pr["nc"], pr["no"], pr["nv"]
    if emax:
        ps, counts, w = select(pr, emax, union, tp)
    else:
        ps, counts, w = class_lists(nc, no, nv), {}, np.zeros(0)
    csf = np.concatenate([to_triples(k, *ps[k], nc, no) for k in range(4)])
    a = matrix(pr, csf)
    a = np.triu(a) + np.triu(a, 1).T          # the reference mirrors the upper triangle
    e, v = np.linalg.eigh(a)
    return e[:nstates], v[:, :nstates], a, ps, counts, w


# --------------------------------------------------------------------------- properties
def split(v, ps):
    """Rows of v.T per class: xycv_a, xyov_a, xyco_b, xycv_b (os_sTDA.py:1283-1292)."""
    ends = np.cumsum([0] + [len(x[0]) for x in ps])
    vt = v.T
    return [vt[:, ends[k]:ends[k + 1]] for k in range(4)]


def osc_str(e, v, ps, dip_ao, co_a, cv_a, co_b, cv_b, nc, no):
    """Length-form oscillator strengths (os_sTDA.py:1388-1418)."""
    da = np.einsum('xpq,pi,qj->xij', dip_ao, co_a, cv_a)
    db = np.einsum('xpq,pi,qj->xij', dip_ao, co_b, cv_b)
    x = split(v, ps)
    t = (np.einsum('xi,yi->yx', da[:, ps[0][0], ps[0][1]], x[0])
         + np.einsum('xi,yi->yx', da[:, nc + ps[1][0], ps[1][1]], x[1])
         + np.einsum('xi,yi->yx', db[:, ps[2][0], ps[2][1]], x[2])
         + np.einsum('xi,yi->yx', db[:, ps[3][0], no + ps[3][1]], x[3]))
    return 2.0 / 3.0 * np.einsum('s,sx,sx->s', e, t, t)


def delta_s2_sa(v, ps):
    """Spin-adapted Delta<S^2> on the aligned CV lists (os_sTDA.py:1337-1340)."""
    x = split(v, ps)
    return (x[0] ** 2).sum(1) + (x[3] ** 2).sum(1) - 2 * (x[0] * x[3]).sum(1)


def delta_s2_so(v, ps, s_ao, co_a, cv_a, co_b, cv_b, nc, no, nv):
    """Spin-orbital Delta<S^2> (os_sTDA.py:1342-1385), the sixteen terms in the reference's
    order on amplitudes scattered back to the untruncated blocks."""
    n = v.shape[1]
    x = split(v, ps)
    cva, ova = np.zeros((n, nc, nv)), np.zeros((n, no, nv))
    cob, cvb = np.zeros((n, nc, no)), np.zeros((n, nc, nv))
    cva[:, ps[0][0], ps[0][1]] = x[0]
    ova[:, ps[1][0], ps[1][1]] = x[1]
    cob[:, ps[2][0], ps[2][1]] = x[2]
    cvb[:, ps[3][0], ps[3][1]] = x[3]
    sccba = co_b.T @ s_ao @ co_a
    sccab = co_a.T @ s_ao @ co_b
    svcab = cv_a.T @ s_ao @ co_b
    svcba = cv_b.T @ s_ao @ co_a
    svvab = cv_a.T @ s_ao @ cv_b
    e = np.einsum
    return (e('nia,nja,ki,jk->n', cva, cva, sccba[:, :nc], sccba.T[:nc, :])
            + e('nia,nja,ki,jk->n', ova, ova, sccba[:, nc:], sccba.T[nc:, :])
            + e('nia,nja,ki,jk->n', ova, cva, sccba[:, nc:], sccba.T[:nc, :])
            + e('nia,nja,ki,jk->n', cva, ova, sccba[:, :nc], sccba.T[nc:, :])
            - e('nia,nib,ak,kb->n', cva, cva, svcab, svcab.T)
            - e('nia,nib,ak,kb->n', ova, ova, svcab, svcab.T)
            + e('nia,nja,ki,jk->n', cvb, cvb, sccab, sccab.T)
            + e('nia,nja,ki,jk->n', cob, cob, sccab, sccab.T)
            - e('nia,nib,ak,kb->n', cob, cob, svcba[:no, :], svcba.T[:, :no])
            - e('nia,nib,ak,kb->n', cvb, cvb, svcba[no:, :], svcba.T[:, no:])
            - e('nia,nib,ak,kb->n', cob, cvb, svcba[:no, :], svcba.T[:, no:])
            - e('nia,nib,ak,kb->n', cvb, cob, svcba[no:, :], svcba.T[:, :no])
            - 2 * e('nia,njb,ji,ab->n', cva, cvb, sccba[:, :nc], svvab[:, no:])
            - 2 * e('nia,njb,ji,ab->n', cva, cob, sccba[:, :nc], svvab[:, :no])
            - 2 * e('nia,njb,ji,ab->n', ova, cvb, sccba[:, nc:], svvab[:, no:])
            - 2 * e('nia,njb,ji,ab->n', ova, cob, sccba[:, nc:], svvab[:, :no]))


# --------------------------------------------------------------------------- from a mean field
def problem_from_mf(mf, spinadapt, emax, cas, correct, paramtype, eta_ev, ao_off, dist):
    """The problem dict of a ``MeanField`` the way OSsTDA.kernel prepares it
    (os_sTDA.py:435-681): occupations (ROKS mask rule :449-455), Fock matrices, the CAS window on
    the orbital energies (sorted Fock diagonals when spin-adapted, :485), S^1/2, charges, gamma.
    Also returns what the properties need: the active orbitals per spin and the first orbital."""
    h1e, veff = mf.get_hcore(), mf.get_veff()
    if spinadapt:
        c = np.array((mf.mo_coeff, mf.mo_coeff))
        occ = np.zeros((2, mf.mo_occ.size))
        occ[0, mf.mo_occ >= 1] = 1
        occ[1, mf.mo_occ == 2] = 1
    else:
        c, occ = np.asarray(mf.mo_coeff), np.asarray(mf.mo_occ, dtype=np.float64)
    fa_ao, fb_ao = h1e + veff[0], h1e + veff[1]
    if spinadapt:
        energy = np.array((np.sort(np.diag(c[0].T @ fa_ao @ c[0])), np.sort(np.diag(c[1].T @ fb_ao @ c[1]))))
    else:
        energy = np.asarray(mf.mo_energy)
    nmo = occ.shape[1]
    lo, hi = (active_window(occ, energy, mf.hyb, emax) if cas and emax else (0, nmo - 1))
    occ_a, occ_b = occ[0, lo:hi + 1], occ[1, lo:hi + 1]
    ca, cb = c[0][:, lo:hi + 1], c[1][:, lo:hi + 1]
    nocc = [int((occ_a > 0.999).sum()), int((occ_b > 0.999).sum())]
    nvir = [int((occ_a < 0.001).sum()), int((occ_b < 0.001).sum())]
    nc, no, nv = nocc[1], nocc[0] - nocc[1], nvir[0]
    fa, fb = ca.T @ fa_ao @ ca, cb.T @ fb_ao @ cb
    pr = dict(natm=len(ao_off) - 1, nc=nc, no=no, nv=nv, nocc=nocc, nvir=nvir, sa=bool(spinadapt),
              si=0.5 * mf.mol.spin, correct=bool(correct), dmax=0.5 / HA2EV if correct else 0.0,
              sigk=0.1 / HA2EV if correct else 1.0)
    pr["foo"] = [fa[:nocc[0], :nocc[0]], fb[:nocc[1], :nocc[1]]]
    pr["fvv"] = [fa[nocc[0]:, nocc[0]:], fb[nocc[1]:, nocc[1]:]]
    if spinadapt:
        vhf = mf.get_veff_hf()
        ha, hb = ca.T @ (h1e + vhf[0]) @ ca, cb.T @ (h1e + vhf[1]) @ cb
        pr["hoo"] = [ha[:nocc[0], :nocc[0]], hb[:nocc[1], :nocc[1]]]
        pr["hvv"] = [ha[nocc[0]:, nocc[0]:], hb[nocc[1]:, nocc[1]:]]
    else:
        pr["hoo"] = pr["hvv"] = None
    pr["gj"], pr["gk"] = gamma(dist, eta_ev, mf.hyb, paramtype)
    s_half = sqrt_overlap(mf.get_ovlp())
    pr["qoo"], pr["qov"], pr["qvv"] = [], [], []
    for s, cs in enumerate((ca, cb)):
        qoo, qov, qvv = charges(s_half @ cs, ao_off, nocc[s])
        pr["qoo"].append(qoo); pr["qov"].append(qov); pr["qvv"].append(qvv)
    orbitals = (ca[:, :nocc[0]], ca[:, nocc[0]:], cb[:, :nocc[1]], cb[:, nocc[1]:])
    return pr, orbitals, lo
