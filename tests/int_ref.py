"""Independent references for xtddft_amd/csrc/xt_int.hip.

ref_int2e: the quartic part of xt_int2e_cart from the same FP64 tables the kernel is handed
(pair_info / pair_prim / eab, ket_info / ket_prim / ek, omega), taken as exact inputs.  The
Boys function comes from mpmath's lower incomplete gamma function at 40 digits (1/(2n+1) at
T = 0), the Hermite integrals R_tuv from the McMurchie-Davidson recursion in mpmath --
restated here, reducing v, then u, then t (the kernel and qc/ints.py reduce t first) -- and
the prefactor and the two contractions run in np.longdouble (in mpmath where long double is
no wider than double).  Next to every element's value it returns sabs, the same sum with the
absolute value of every factor: the natural scale of that element's rounding.  Only the index
order (hermite_index, cart_comps) is shared with qc/ints.py.

ref_eval_ao: AO values and gradients of xt_eval_ao in np.longdouble straight from the
definition, combined with the spherical tables and norms the kernel is handed.

mpmath is imported inside the functions that need it: the GPU tests import this module for
ref_eval_ao only and run without it.
"""
from __future__ import annotations

import numpy as np

from xtddft_amd.qc.ints import cart_comps, hermite_index

LD = np.longdouble
WIDE = bool(np.finfo(LD).eps < 1e-18)
U = 2.0 ** -53
DPS = 40


def ncart(l):
    return (l + 1) * (l + 2) // 2


def ntuv(L):
    return (L + 1) * (L + 2) * (L + 3) // 6


# --------------------------------------------------------------------------- integrals
def boys_mp(nmax, T):
    """[F_0(T) .. F_nmax(T)] as mpf: F_n = gamma_lower(n + 1/2, T) / (2 T^(n + 1/2))."""
    import mpmath as mp
    if T == 0:
        return [mp.mpf(1) / (2 * n + 1) for n in range(nmax + 1)]
    half = mp.mpf(1) / 2
    return [mp.gammainc(n + half, 0, T) / (2 * T ** (n + half)) for n in range(nmax + 1)]


def hermite_r_mp(L, alpha, X, Y, Z):
    """R^0_tuv(alpha, X, Y, Z) for hermite_index(L), as a list of mpf:
    R^n_000 = (-2 alpha)^n F_n(alpha |XYZ|^2), R^n_{..,v} = Z R^{n+1}_{..,v-1} + (v-1) R^{n+1}_{..,v-2}
    (and the same in u, t)."""
    F = boys_mp(L, alpha * (X * X + Y * Y + Z * Z))
    m2a = -2 * alpha
    memo = {}

    def R(n, t, u, v):
        key = (n, t, u, v)
        if key in memo:
            return memo[key]
        if v > 0:
            r = Z * R(n + 1, t, u, v - 1)
            if v > 1:
                r += (v - 1) * R(n + 1, t, u, v - 2)
        elif u > 0:
            r = Y * R(n + 1, t, u - 1, 0)
            if u > 1:
                r += (u - 1) * R(n + 1, t, u - 2, 0)
        elif t > 0:
            r = X * R(n + 1, t - 1, 0, 0)
            if t > 1:
                r += (t - 1) * R(n + 1, t - 2, 0, 0)
        else:
            r = m2a ** n * F[n]
        memo[key] = r
        return r

    return [R(0, t, u, v) for (t, u, v) in hermite_index(L)[0]]


def _wide(x):
    """mpf -> the contraction's number type (long double from a two-term split, or mpf)."""
    if not WIDE:
        return x
    hi = float(x)
    return LD(hi) + LD(float(x - hi))


def _wide_array(a):
    if WIDE:
        return np.asarray(a, dtype=LD)
    import mpmath as mp
    out = np.empty(a.shape, dtype=object)
    for i, x in np.ndenumerate(a):
        out[i] = mp.mpf(float(x))
    return out


def _sum_index(lab, lc):
    """pos[t, u] of t + u in hermite_index(lab + lc), and (-1)^|u|."""
    tab, _ = hermite_index(lab)
    tc, _ = hermite_index(lc)
    _, pos = hermite_index(lab + lc)
    idx = np.array([[pos[(a + d, b + e, c + f)] for (d, e, f) in tc] for (a, b, c) in tab], dtype=np.int64)
    sign = np.array([-1.0 if (d + e + f) % 2 else 1.0 for (d, e, f) in tc])
    return idx, sign


def ref_int2e(pair_info, pair_prim, eab, ket_info, ket_prim, ek, omega, nrow, ldo, diag=False):
    """(ref, sabs, L): (nrow, ldo) float64 values and scales of every output element of one
    xt_int2e_cart call on a zeroed `out`, and the total Hermite order of the block an element
    belongs to (-1: outside every block)."""
    import mpmath as mp
    zero = LD(0) if WIDE else mp.mpf(0)
    ref = np.full((nrow, ldo), zero, dtype=LD if WIDE else object)
    sab = ref.copy()
    Lmap = np.full((nrow, ldo), -1, dtype=np.int64)
    pair_prim = np.asarray(pair_prim).reshape(-1, 4)
    ket_prim = np.asarray(ket_prim).reshape(-1, 4)
    npair, nket = len(pair_info), len(ket_info)
    quartets = [(k, k) for k in range(npair)] if diag else [(k, j) for j in range(nket) for k in range(npair)]
    with mp.workdps(DPS):
        for k, j in quartets:
            la, lb, npp, pq0, pe0, row0 = (int(x) for x in pair_info[k][:6])
            lc, nr, ar0, ae0, col0, nc = (int(x) for x in ket_info[j][:6])
            lab, L = la + lb, la + lb + lc
            nab, nt, nu = ncart(la) * ncart(lb), ntuv(lab), ntuv(lc)
            E = _wide_array(np.asarray(eab[pe0:pe0 + nab * nt * npp]).reshape(nab, nt, npp))
            K = _wide_array(np.asarray(ek[ae0:ae0 + nc * nu * nr]).reshape(nc, nu, nr))
            idx, sign = _sum_index(lab, lc)
            Ks = K * (sign[None, :, None].astype(LD) if WIDE else sign[None, :, None].astype(int).astype(object))
            blk = ref[row0:row0 + nab, col0:col0 + nc]
            blka = sab[row0:row0 + nab, col0:col0 + nc]
            Lmap[row0:row0 + nab, col0:col0 + nc] = L
            for q in range(npp):
                p = mp.mpf(float(pair_prim[pq0 + q, 0]))
                P = [mp.mpf(float(x)) for x in pair_prim[pq0 + q, 1:]]
                for r in range(nr):
                    s = mp.mpf(float(ket_prim[ar0 + r, 0]))
                    C = [mp.mpf(float(x)) for x in ket_prim[ar0 + r, 1:]]
                    alpha, scale = p * s / (p + s), mp.mpf(1)
                    if omega > 0:
                        w2 = mp.mpf(float(omega)) ** 2
                        a2 = alpha * w2 / (alpha + w2)
                        scale = mp.sqrt(a2 / alpha)
                        alpha = a2
                    Rt = hermite_r_mp(L, alpha, P[0] - C[0], P[1] - C[1], P[2] - C[2])
                    pref = _wide(2 * mp.pi ** 2.5 / (p * s * mp.sqrt(p + s)) * scale)
                    Rv = np.array([_wide(x) for x in Rt], dtype=LD if WIDE else object)
                    Rg = Rv[idx]                                        # (nt, nu)
                    blk += pref * (E[:, :, q] @ (Rg @ Ks[:, :, r].T))
                    blka += abs(pref) * (np.abs(E[:, :, q]) @ (np.abs(Rg) @ np.abs(K[:, :, r]).T))

    def f64(a):
        return a.astype(np.float64) if WIDE else np.array([[float(x) for x in row] for row in a]).reshape(a.shape)
    return f64(ref), f64(sab), Lmap


# --------------------------------------------------------------------------- AO on the grid
def ref_eval_ao(coords, shell_info, shell_data, sph, norm, nao):
    """(ref, sabs, amp), each (4, ngrid, nao) np.longdouble: value, d/dx, d/dy, d/dz of the
    normalised spherical AOs; sabs sums the absolute values of every term (primitives,
    Cartesian components, the two gradient terms); amp is sabs with every exponential
    replaced by 1 -- what an absolute error of the exponential (its FP64 underflow) is
    multiplied by on the way to the output."""
    coords = np.asarray(coords, dtype=np.float64)
    ng = coords.shape[0]
    out = [np.zeros((4, ng, nao), dtype=LD) for _ in range(3)]
    for info in shell_info:
        l, npr, off, ao0 = (int(x) for x in info[:4])
        ex = shell_data[off:off + npr].astype(LD)
        cf = shell_data[off + npr:off + 2 * npr].astype(LD)
        ctr = shell_data[off + 2 * npr:off + 2 * npr + 3].astype(LD)
        d = coords.astype(LD) - ctr
        r2 = (d * d).sum(1)
        toff = sum((2 * k + 1) * ncart(k) for k in range(l))
        T = np.asarray(sph[toff:toff + (2 * l + 1) * ncart(l)]).reshape(2 * l + 1, ncart(l)).astype(LD)
        nm = np.asarray(norm[ao0:ao0 + 2 * l + 1]).astype(LD)
        e_true = cf * np.exp(-ex * r2[:, None])                         # (ng, npr)
        variants = [(e_true, False), (np.abs(e_true), True), (np.abs(cf) * np.ones((ng, 1), dtype=LD), True)]
        for dst, (e, absolute) in zip(out, variants):
            g0 = e.sum(1)
            g1 = (2 * ex * e).sum(1) if absolute else (-2 * ex * e).sum(1)
            dd = np.abs(d) if absolute else d
            cart = np.zeros((4, ng, ncart(l)), dtype=LD)
            for c, (ix, iy, iz) in enumerate(cart_comps(l)):
                pw = (ix, iy, iz)
                poly = dd[:, 0] ** ix * dd[:, 1] ** iy * dd[:, 2] ** iz
                cart[0, :, c] = poly * g0
                for a in range(3):
                    g = poly * dd[:, a] * g1
                    if pw[a] > 0:
                        low = [pw[b] - (1 if b == a else 0) for b in range(3)]
                        g = g + pw[a] * dd[:, 0] ** low[0] * dd[:, 1] ** low[1] * dd[:, 2] ** low[2] * g0
                    cart[1 + a, :, c] = g
            Tm = np.abs(T) if absolute else T
            dst[:, :, ao0:ao0 + 2 * l + 1] = (cart @ Tm.T) * (np.abs(nm) if absolute else nm)
    return tuple(out)


def ao_bound(c, sabs, amp):
    """Elementwise bound of |dev - ref| for xt_eval_ao: c 2^-53 sabs, plus the FP64 underflow
    of the exponentials (an absolute error up to the smallest normal number each) times amp."""
    return LD(c) * LD(U) * sabs + LD(np.finfo(np.float64).tiny) * amp
