"""NumPy restatement of the reference's state-to-state transition moments
(``XSF_TDA.calculate_TDM_U`` / ``calculate_TDM_R``, XSF_TDA.py:435-592), term by term.

Test infrastructure: the device entry ``xt_tdm`` evaluates the same quantity as one
linear map per state and a Gram product; here every one of the reference's trace terms is
written out as its own ``einsum`` over all ordered pairs (s, t) of states at once, so the
two forms are independent.  The reference's notebooks print no transition-dipole table,
so this restatement of its formula is what the feature is pinned to.
"""
import numpy as np


def split_blocks(vecs, nc, no, nv, vects=None):
    """cv (N,nc,nv), co (N,nc,no), ov (N,no,nv), oo (N,no,no) of state rows in the
    reference's cv|co|ov|oo order; a compressed OO block is expanded, oo = vects w
    (XSF_TDA.py:509-515)."""
    vecs = np.asarray(vecs)
    n = vecs.shape[0]
    d1 = nc * nv
    d2 = d1 + nc * no
    d3 = d2 + no * nv
    oo = vecs[:, d3:]
    if vects is not None:
        oo = oo @ np.asarray(vects).T
    return (vecs[:, :d1].reshape(n, nc, nv), vecs[:, d1:d2].reshape(n, nc, no),
            vecs[:, d2:d3].reshape(n, no, nv), oo.reshape(n, no, no))


def blocks_to_rows(c, nc, no, nv):
    """Amplitude matrices c (N, nc+no, no+nv) (rows [c|o], columns [o|v], XSF_TDA.py:456-460)
    -> rows in cv|co|ov|oo order (OO un-compressed)."""
    n = c.shape[0]
    return np.hstack([c[:, :nc, no:].reshape(n, -1), c[:, :nc, :no].reshape(n, -1),
                      c[:, nc:, no:].reshape(n, -1), c[:, nc:, :no].reshape(n, -1)])


def spin_factors(sa, si):
    """factor1, factor2, factor3 of XSF_TDA.py:500-507."""
    if sa == 0:
        return 1.0, 1.0, 0.0
    return (np.sqrt((2 * si + 1) / (2 * si)), np.sqrt((2 * si) / (2 * si - 1)),
            1.0 / np.sqrt(2 * si * (2 * si - 1)))


def tdm_roks(vecs, ints_mo, nc, no, nv, sa, si, vects=None):
    """T (ncomp, N, N) of calculate_TDM_R (XSF_TDA.py:481-592): ``ints_mo`` (ncomp, nmo, nmo)
    the operator in the ROKS MO basis (core | open | virtual)."""
    cv, co, ov, oo = split_blocks(vecs, nc, no, nv, vects)
    f1, f2, f3 = spin_factors(sa, si)
    c_, o_, v_ = slice(0, nc), slice(nc, nc + no), slice(nc + no, nc + no + nv)
    d = np.asarray(ints_mo)
    dcc, dco, doo = d[:, c_, c_], d[:, c_, o_], d[:, o_, o_]
    dvo, dvv, dov = d[:, v_, o_], d[:, v_, v_], d[:, o_, v_]
    tr_oo = np.einsum('suu->s', oo)
    t = np.zeros((d.shape[0], vecs.shape[0], vecs.shape[0]))
    # CV-CV (:528-529)
    t += np.einsum('sia,xab,tib->xst', cv, dvv, cv) - np.einsum('sia,xij,tja->xst', cv, dcc, cv)
    # CV-CO (:534, :537)
    t += f1 * np.einsum('sia,xav,tiv->xst', cv, dvo, co)
    t += f1 * np.einsum('siu,xbu,tib->xst', co, dvo, cv)
    # CV-OV (:541, :544)
    t += -f1 * np.einsum('sia,xiv,tva->xst', cv, dco, ov)
    t += -f1 * np.einsum('sua,xju,tja->xst', ov, dco, cv)
    # CO-CO (:548-549)
    t += np.einsum('siu,xuv,tiv->xst', co, doo, co) - np.einsum('siu,xij,tju->xst', co, dcc, co)
    # CO-OO (:554, :557, :560, :563)
    t += -f2 * np.einsum('siu,xiv,tvu->xst', co, dco, oo)
    t += f3 * np.einsum('siu,xiu,t->xst', co, dco, tr_oo)
    t += -f2 * np.einsum('sut,xju,rjt->xsr', oo, dco, co)
    t += f3 * np.einsum('s,xjv,tjv->xst', tr_oo, dco, co)
    # OV-OV (:567-568)
    t += np.einsum('sua,xab,tub->xst', ov, dvv, ov) - np.einsum('sua,xuv,tva->xst', ov, doo, ov)
    # OV-OO (:573, :576, :579, :582)
    t += f2 * np.einsum('sua,xaw,tuw->xst', ov, dvo, oo)
    t += -f3 * np.einsum('sua,xua,t->xst', ov, dov, tr_oo)
    t += f2 * np.einsum('sut,xbt,rub->xsr', oo, dvo, ov)
    t += -f3 * np.einsum('s,xvb,tvb->xst', tr_oo, dov, ov)
    # OO-OO (:586-587)
    t += np.einsum('sut,xtv,ruv->xsr', oo, doo, oo) - np.einsum('sut,xuw,rwt->xsr', oo, doo, oo)
    return t


def tdm_uks(vecs, ints_occ, ints_vir, nc, no, nv, vects=None):
    """T (ncomp, N, N) of calculate_TDM_U (XSF_TDA.py:435-478): ``ints_occ`` (ncomp, nc+no,
    nc+no) the operator over the occupied orbitals of the amplitude rows (``ints_aa[:, :nc+no,
    :nc+no]``), ``ints_vir`` (ncomp, no+nv, no+nv) over the virtuals of its columns
    (``ints_bb[:, nc:, nc:]``); c assembled as :456-460."""
    cv, co, ov, oo = split_blocks(vecs, nc, no, nv, vects)
    c = np.concatenate([np.concatenate([co, cv], axis=2), np.concatenate([oo, ov], axis=2)], axis=1)
    # :476  trace(c0 D_vir c1^T) - trace(c0^T D_occ c1)
    return (np.einsum('sia,xab,tib->xst', c, np.asarray(ints_vir), c)
            - np.einsum('sia,xij,tja->xst', c, np.asarray(ints_occ), c))


def osc(e, t):
    """(2/3) |e_i - e_j| (T_x^2 + T_y^2 + T_z^2) (XSF_TDA.py:591)."""
    e = np.asarray(e)
    return 2.0 / 3.0 * np.abs(e[:, None] - e[None, :]) * (t ** 2).sum(axis=0)
