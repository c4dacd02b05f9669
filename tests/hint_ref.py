"""The 40-digit reference of the Hermite-form Coulomb kernels (xtddft_amd/csrc/xt_hint.hip and
xt_grad.hip), shared by tests/test_gpu_somf.py, tests/test_grad_cases.py and
tests/test_gpu_grad_paths.py.

``shell`` / ``tables`` / ``as_ket`` build the tables of DerivPair entries the kernels take, and
``ref_hint`` generalises ``int_ref.ref_int2e`` to stated orders, row counts and the cross mode.

``ref_grad`` is the reference of one raw ``xt_grad_jk`` call (tests/grad_cases.py): for every
distinct (bra block, ket block) the (3 nab) x ncol derivative integrals and their sabs from
``ref_hint``, multiplied by Gamma and summed over the kets in np.longdouble.  ``host_grad`` is the
host FP64 restatement of the same call (the formula of ``ints.eri_quartet`` on the tables, times
Gamma, summed in float64) from which the multiplier kappa_g(L) of the bound is measured
(tests/golden/make_grad_kappa.py).  Gamma is the kernel's formula

    Gamma[ab, c] = sum_t wj_t P_t[ia, ib] Q_t[ic, id] + wk_t P_t[ia, ic] Q_t[ib, id]   (+ ic <-> id: image)

over dyadic P, Q, wj, wk, so float64 holds every Gamma element exactly in any order.
"""
import numpy as np

import int_ref

CENTRES = np.array([[0.0, 0.0, 0.0], [0.9, -0.4, 0.3], [-0.5, 0.7, 1.1], [0.2, 1.3, -0.8]])


def shell(l, nprim, centre, seed):
    from xtddft_amd.qc.gto import Shell, gto_norm
    rng = np.random.default_rng(seed)
    exps = 0.4 * 3.1 ** np.arange(nprim) * (1.0 + 0.3 * rng.random(nprim))
    coefs = (0.5 + rng.random(nprim)) * gto_norm(l, exps)
    return Shell(int(centre), l, CENTRES[centre].copy(), exps, coefs)


def tables(pairs, unit):
    """xt_hint_cart tables of DerivPair entries; a pair's output offset advances by unit * nab
    (unit 3: plain mode, its rows are (m, a, b); unit 1: cross mode)."""
    from xtddft_amd.qc.ints import DerivPair
    info, prim, e = [], [], []
    q0 = e0 = o0 = 0
    for sa, sb in pairs:
        dp = DerivPair(sa, sb)
        tab = dp.Eab[:, 0]
        info.append([dp.L, tab.shape[0], dp.p.size, q0, e0, o0, 0, 0])
        prim.append(np.column_stack([dp.p, dp.P]))
        e.append(tab.ravel())
        q0 += dp.p.size
        e0 += tab.size
        o0 += unit * dp.nab
    return np.array(info, dtype=np.int32), np.concatenate(prim), np.concatenate(e), o0


def as_ket(info):
    """bra rows (order, nrow, npp, prim0, e0, row0) -> ket rows (order, nprim, prim0, e0, col0, ncol)."""
    out = np.zeros_like(info)
    out[:, 0], out[:, 1:4], out[:, 4], out[:, 5] = info[:, 0], info[:, 2:5], info[:, 5], info[:, 1]
    return out


def ref_hint(binfo, bprim, eb, kinfo, kprim, ek, cross, nrow_tot, ldo):
    """int_ref.ref_int2e for xt_hint_cart: orders and row counts read from the tables, and in
    cross mode the eps_lmn combination of the (m | n) blocks.  (ref, sabs, L) of shape
    (ncomp, nrow_tot, ldo), ncomp = 3 (cross) or 1."""
    import mpmath as mp
    LD, WIDE = int_ref.LD, int_ref.WIDE
    ncomp = 3 if cross else 1
    zero = LD(0) if WIDE else mp.mpf(0)
    ref = np.full((ncomp, nrow_tot, ldo), zero, dtype=LD if WIDE else object)
    sab = ref.copy()
    Lmap = np.full((ncomp, nrow_tot, ldo), -1, dtype=np.int64)
    bprim, kprim = np.asarray(bprim).reshape(-1, 4), np.asarray(kprim).reshape(-1, 4)
    with mp.workdps(int_ref.DPS):
        for j in range(len(kinfo)):
            for k in range(len(binfo)):
                lb, nrow, npp, bq0, be0, row0 = (int(x) for x in binfo[k][:6])
                lk, nr, kr0, ke0, col0, ncol = (int(x) for x in kinfo[j][:6])
                L, nt, nu = lb + lk, int_ref.ntuv(lb), int_ref.ntuv(lk)
                E = int_ref._wide_array(np.asarray(eb[be0:be0 + nrow * nt * npp]).reshape(nrow, nt, npp))
                K = int_ref._wide_array(np.asarray(ek[ke0:ke0 + ncol * nu * nr]).reshape(ncol, nu, nr))
                idx, sign = int_ref._sum_index(lb, lk)
                Ks = K * (sign[None, :, None].astype(LD) if WIDE else sign[None, :, None].astype(int).astype(object))
                blk = np.full((nrow, ncol), zero, dtype=ref.dtype)
                blka = blk.copy()
                for q in range(npp):
                    p = mp.mpf(float(bprim[bq0 + q, 0]))
                    P = [mp.mpf(float(x)) for x in bprim[bq0 + q, 1:]]
                    for r in range(nr):
                        s = mp.mpf(float(kprim[kr0 + r, 0]))
                        C = [mp.mpf(float(x)) for x in kprim[kr0 + r, 1:]]
                        Rt = int_ref.hermite_r_mp(L, p * s / (p + s), P[0] - C[0], P[1] - C[1], P[2] - C[2])
                        pref = int_ref._wide(2 * mp.pi ** 2.5 / (p * s * mp.sqrt(p + s)))
                        Rg = np.array([int_ref._wide(x) for x in Rt], dtype=ref.dtype)[idx]
                        blk += pref * (E[:, :, q] @ (Rg @ Ks[:, :, r].T))
                        blka += abs(pref) * (np.abs(E[:, :, q]) @ (np.abs(Rg) @ np.abs(K[:, :, r]).T))
                if not cross:
                    ref[0, row0:row0 + nrow, col0:col0 + ncol] = blk
                    sab[0, row0:row0 + nrow, col0:col0 + ncol] = blka
                    Lmap[0, row0:row0 + nrow, col0:col0 + ncol] = L
                    continue
                nab, ncd = nrow // 3, ncol // 3
                b4 = blk.reshape(3, nab, 3, ncd)
                a4 = blka.reshape(3, nab, 3, ncd)
                for l, m, n in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
                    ref[l, row0:row0 + nab, col0:col0 + ncd] = b4[m, :, n] - b4[n, :, m]
                    sab[l, row0:row0 + nab, col0:col0 + ncd] = a4[m, :, n] + a4[n, :, m]
                    Lmap[l, row0:row0 + nab, col0:col0 + ncd] = L

    def f64(a):
        return a.astype(np.float64) if WIDE else np.array([float(x) for x in a.ravel()]).reshape(a.shape)
    return f64(ref), f64(sab), Lmap


# --------------------------------------------------------------------------- xt_grad_jk
def _unique_blocks(call):
    """The distinct bra and ket blocks of a call (table rows may share one prim / E block): info
    tables with consecutive row0 / col0, and per table row the offset of its block."""
    bkeys, kkeys, brow, kcol = {}, {}, [], []
    binfo, kinfo = [], []
    r0 = c0 = 0
    for row in call.binfo:
        key = tuple(int(x) for x in row[:5])
        if key not in bkeys:
            bkeys[key] = r0
            binfo.append(list(key) + [r0, 0, 0])
            r0 += key[1]
        brow.append(bkeys[key])
    for row in call.kinfo:
        key = tuple(int(x) for x in row[:4]) + (int(row[5]),)
        if key not in kkeys:
            kkeys[key] = c0
            kinfo.append(list(key[:4]) + [c0, key[4], 0, 0])
            c0 += key[4]
        kcol.append(kkeys[key])
    return np.array(binfo, dtype=np.int32), np.array(kinfo, dtype=np.int32), brow, kcol, r0, c0


def grad_integrals(call):
    """40-digit derivative integrals of every distinct (bra block, ket block) of a call:
    (ref, sabs) of shape (rows, cols) and the block offsets of the table rows.  A pure function
    of the tables: the selector probes and the dense Gamma of one case share it."""
    binfo, kinfo, brow, kcol, nrow, ncol = _unique_blocks(call)
    ref, sabs, _ = ref_hint(binfo, call.bprim, call.eb, kinfo, call.kprim, call.ek, 0, nrow, ncol)
    for x in (ref, sabs):
        x.setflags(write=False)
    return ref[0], sabs[0], brow, kcol


def host_integrals(call):
    """The same blocks from the host FP64 path: the formula of ints.eri_quartet (ints.hermite_r,
    ints._sum_table and its two contractions) applied to the tables."""
    from xtddft_amd.qc import ints
    binfo, kinfo, brow, kcol, nrow, ncol = _unique_blocks(call)
    out = np.zeros((nrow, ncol))
    bprim, kprim = call.bprim.reshape(-1, 4), call.kprim.reshape(-1, 4)
    for lb, nr_b, npp, bq0, be0, row0 in (tuple(int(x) for x in r[:6]) for r in binfo):
        for lk, nr, kr0, ke0, col0, nc in (tuple(int(x) for x in r[:6]) for r in kinfo):
            E = call.eb[be0:be0 + nr_b * int_ref.ntuv(lb) * npp].reshape(nr_b, int_ref.ntuv(lb), npp)
            K = call.ek[ke0:ke0 + nc * int_ref.ntuv(lk) * nr].reshape(nc, int_ref.ntuv(lk), nr)
            p = bprim[bq0:bq0 + npp, 0][:, None]
            s = kprim[kr0:kr0 + nr, 0][None, :]
            d = bprim[bq0:bq0 + npp, None, 1:] - kprim[None, kr0:kr0 + nr, 1:]
            R = ints.hermite_r(lb + lk, p * s / (p + s), d[..., 0], d[..., 1], d[..., 2])
            pref = 2.0 * np.pi ** 2.5 / (p * s * np.sqrt(p + s))
            idx, sign = ints._sum_table(lb, lk)
            X = np.einsum('tsPQ,s,csQ->tcP', R[idx] * pref, sign, K, optimize=True)
            out[row0:row0 + nr_b, col0:col0 + nc] = np.einsum('atP,tcP->ac', E, X, optimize=True)
    return out, brow, kcol


def gamma_block(call, k, j, drop_image=False, swap_ncb=False):
    """Gamma[ab, c] of bra row k and ket row j in float64 (exact for the dyadic inputs of
    tests/grad_cases.py), the image of a flagged ket included.  ``drop_image`` and ``swap_ncb``
    are the two deliberately wrong references of tests/test_grad_cases.py."""
    a0, b0, ncb, _ = (int(x) for x in call.bra_ao[k])
    c0, d0, ncd, image = (int(x) for x in call.ket_ao[j])
    ncb, ncd = max(ncb, 1), max(ncd, 1)
    if swap_ncb:
        ncb, ncd = ncd, ncb
    nab, ncol = int(call.binfo[k][1]) // 3, int(call.kinfo[j][5])
    ab, c = np.arange(nab)[:, None], np.arange(ncol)[None, :]
    ia, ib, ic, idd = a0 + ab // ncb, b0 + ab % ncb, c0 + c // ncd, d0 + c % ncd
    g = np.zeros((nab, ncol))
    for t in range(len(call.wj)):
        P, Q = call.P[t], call.Q[t]
        g += call.wj[t] * P[ia, ib] * Q[ic, idd] + call.wk[t] * P[ia, ic] * Q[ib, idd]
        if image and not drop_image:
            g += call.wj[t] * P[ia, ib] * Q[idd, ic] + call.wk[t] * P[ia, idd] * Q[ib, ic]
    return g


def contract(call, ints_, brow, kcol, sabs=None, wide=True, **wrong):
    """Per bra row k: g[k][m] = sum_j sum_{ab, c} Gamma[ab, c] I[(m, ab), c]; with ``sabs`` also
    sum |Gamma| sabs, the largest total order L met and the number of products summed."""
    T = int_ref.LD if wide else np.float64
    nb, nk = len(call.binfo), len(call.kinfo)
    g = np.zeros((nb, 3), dtype=T)
    sa = np.zeros((nb, 3), dtype=T)
    L = np.zeros(nb, dtype=np.int64)
    nsum = np.zeros(nb, dtype=np.int64)
    for k in range(nb):
        nrow = int(call.binfo[k][1])
        nab = nrow // 3
        for j in range(nk):
            ncol = int(call.kinfo[j][5])
            gam = gamma_block(call, k, j, **wrong)
            blk = ints_[brow[k]:brow[k] + nrow, kcol[j]:kcol[j] + ncol].reshape(3, nab, ncol)
            if wide:
                g[k] += (blk.astype(T) * gam.astype(T)[None]).sum(axis=(1, 2))
            else:
                g[k] += (blk * gam[None]).sum(axis=(1, 2))
            if sabs is not None:
                sb = sabs[brow[k]:brow[k] + nrow, kcol[j]:kcol[j] + ncol].reshape(3, nab, ncol)
                sa[k] += (sb.astype(T) * np.abs(gam).astype(T)[None]).sum(axis=(1, 2))
            L[k] = max(L[k], int(call.binfo[k][0]) + int(call.kinfo[j][0]))
            nsum[k] += nab * ncol * int(call.binfo[k][2]) * int(call.kinfo[j][1])
    return g, sa, L, nsum


def fold(call, per_entry, absolute=False):
    """(natm, 3) = out0 + sum of the bra rows of every atom, in the type of ``per_entry``."""
    out = np.abs(call.out0).astype(per_entry.dtype) if absolute else call.out0.astype(per_entry.dtype)
    for k in range(len(call.binfo)):
        out[int(call.bra_ao[k][3])] += per_entry[k]
    return out


def ref_grad(call, blocks=None, **wrong):
    """(ref, sabs, L, nsum), each per output row: the value of ``out`` after the call in
    np.longdouble rounded to float64, the sum of the absolute values of every term (|Gamma
    element| x the integral's sabs, and |out0|), the largest total order that contributes to
    the row (-1: no bra entry, the row keeps its bits) and the number of products summed."""
    ref, sabs, brow, kcol = blocks if blocks is not None else grad_integrals(call)
    g, sa, L, nsum = contract(call, ref, brow, kcol, sabs=sabs, **wrong)
    natm = call.out0.shape[0]
    Lrow = np.full(natm, -1, dtype=np.int64)
    nrow = np.zeros(natm, dtype=np.int64)
    for k in range(len(call.binfo)):
        A = int(call.bra_ao[k][3])
        Lrow[A] = max(Lrow[A], L[k])
        nrow[A] += nsum[k]
    return fold(call, g).astype(np.float64), fold(call, sa, absolute=True).astype(np.float64), Lrow, nrow


def host_grad(call):
    """The host FP64 restatement of the call: float64 integrals times Gamma, summed in float64."""
    val, brow, kcol = host_integrals(call)
    g, _, _, _ = contract(call, val, brow, kcol, wide=False)
    return fold(call, g)
