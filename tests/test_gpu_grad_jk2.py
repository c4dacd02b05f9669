"""GPU: ``xt_grad_jk2`` (xtddft_amd/csrc/xt_grad.hip), the derivative-ERI gradient kernel with a
Coulomb list and an exchange list of their own, through raw calls of the C entry on the case table of
tests/grad_cases.py.

Same body, same bits: every case of the table is sent to ``xt_grad_jk2`` as the Coulomb list of its
terms with wj != 0 and the exchange list of those with wk != 0.  Gamma is dense and dyadic there
(entries multiples of 1/16, weights +-1/2, +-1, +-2, at most 16 summands and the image), so it is
exact in FP64 in any summation order, and everything after Gamma is the one kernel body: the result
must have the bits of ``xt_grad_jk`` on the same call.

New ground: both lists full (nj = nk = 8, sixteen distinct matrices from two seeded builds on the same
tables), one case per template instance, against ``hint_ref.ref_grad`` of the two calls summed inside
kappa_g 2^-53 (sabs_1 + sabs_2); and nj = 0 / nk = 0 with the empty list's pointers null.

Every call: NaN slack behind every float table, NaN wherever a list's P / Q are not to be read (a
Coulomb pair reads P[a,b], Q[c,d] and the image Q[d,c] only; an exchange pair P[a,c], Q[b,d] and the
image P[a,d], Q[b,c] only), sentinel guards around `out` and behind `work[nwork]`, `work` NaN before
the call, nwork exactly 3 nbra (nstrip + 1), the same call with nwork - 1 refused with nothing
written, and two calls give equal bits.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

import grad_cases as gc
import hint_ref

pytestmark = pytest.mark.gpu

SENTINEL = -7777.25
GUARD = 64
U = 2.0 ** -53


@pytest.fixture(scope="module")
def torch(hiplib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def list_masks(c, call):
    """(pj, qj, pk, qk) boolean (nao, nao): where a Coulomb pair and an exchange pair read."""
    n = call.nao
    pj, qj, pk, qk = (np.zeros((n, n), dtype=bool) for _ in range(4))
    for b, (a0, b0, _, _) in zip(c.bras, call.bra_ao):
        ra, rb = slice(a0, a0 + gc.ncart(b.la)), slice(b0, b0 + gc.ncart(b.lb))
        pj[ra, rb] = True
        for k, (c0, d0, _, image) in zip(c.kets, call.ket_ao):
            rc, rd = slice(c0, c0 + gc.ncart(k.lc)), slice(d0, d0 + gc.ncart(k.ld))
            qj[rc, rd] = True
            pk[ra, rc] = True
            qk[rb, rd] = True
            if image:
                qj[rd, rc] = True
                pk[ra, rd] = True
                qk[rb, rc] = True
    return pj, qj, pk, qk


def lists_of(c, call, jcall=None, kcall=None):
    """The two lists of a case: (wj, PJ, QJ) of the terms of ``jcall`` with wj != 0, (wk, PK, QK) of the
    terms of ``kcall`` with wk != 0 (both default to ``call``), NaN outside what the list reads; an
    empty list is (None, None, None)."""
    jcall, kcall = jcall or call, kcall or call
    mpj, mqj, mpk, mqk = list_masks(c, call)
    tj = [t for t in range(len(jcall.wj)) if jcall.wj[t] != 0.0]
    tk = [t for t in range(len(kcall.wk)) if kcall.wk[t] != 0.0]

    def pick(src, ts, w, mp, mq):
        if not ts:
            return None, None, None
        return (np.array([w[t] for t in ts]), np.stack([np.where(mp, src.P[t], np.nan) for t in ts]),
                np.stack([np.where(mq, src.Q[t], np.nan) for t in ts]))
    return pick(jcall, tj, jcall.wj, mpj, mqj), pick(kcall, tk, kcall.wk, mpk, mqk)


def _device_tables(torch, call):
    def up(a):
        a = np.ascontiguousarray(a)
        if a.dtype == np.float64:
            a = np.concatenate([a.ravel(), np.full(GUARD, np.nan)])
        return torch.from_numpy(a).cuda()
    return [up(x) for x in (call.binfo, call.bprim, call.eb, call.bra_ao, call.kinfo, call.kprim, call.ek, call.ket_ao)], up


def _guarded(torch, hiplib, call, run_entry):
    """The memory discipline around one entry: refused at nwork - 1 with nothing written, then the call."""
    flat = np.concatenate([np.full(GUARD, SENTINEL), call.out0.ravel(), np.full(GUARD, SENTINEL)])
    nwork = call.nwork
    wflat = np.concatenate([np.full(nwork, np.nan), np.full(GUARD, SENTINEL)])

    def run(nw):
        d_out, d_work = torch.from_numpy(flat.copy()).cuda(), torch.from_numpy(wflat.copy()).cuda()
        rc = run_entry(d_work.data_ptr(), nw, d_out.data_ptr() + 8 * GUARD)
        torch.cuda.synchronize()
        return rc, d_out.cpu().numpy(), d_work.cpu().numpy()
    rc, got, work = run(nwork - 1)
    assert rc == -1 and b"workspace" in hiplib.xt_last_error()
    assert np.array_equal(_bits(got), _bits(flat)) and np.array_equal(_bits(work), _bits(wflat)), "a refused call wrote"
    rc, got, work = run(nwork)
    assert rc == 0, hiplib.xt_last_error()
    assert np.array_equal(_bits(got[:GUARD]), _bits(flat[:GUARD])), "write before out"
    assert np.array_equal(_bits(got[-GUARD:]), _bits(flat[-GUARD:])), "write past out"
    assert np.array_equal(_bits(work[nwork:]), _bits(wflat[nwork:])), "write past work[nwork]"
    assert np.all(np.isfinite(work[:nwork])), \
        "a workspace element is NaN: not written, or summed from an element of P / Q outside what the list reads"
    return got[GUARD:-GUARD].reshape(call.natm, 3)


def launch_jk(torch, hiplib, call):
    """One xt_grad_jk call (the entry the bits are compared with)."""
    dev, up = _device_tables(torch, call)
    dp, dq = up(call.P), up(call.Q)
    wj, wk = np.ascontiguousarray(call.wj, dtype=np.float64), np.ascontiguousarray(call.wk, dtype=np.float64)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def entry(work, nw, out):
        return hiplib.xt_grad_jk(len(call.binfo), *[x.data_ptr() for x in dev[:4]], len(call.kinfo),
                                 *[x.data_ptr() for x in dev[4:8]], call.lbra, call.lket, len(wj), wj.ctypes.data,
                                 wk.ctypes.data, dp.data_ptr(), dq.data_ptr(), call.nao, call.strip, call.natm,
                                 work, nw, out, st)
    return _guarded(torch, hiplib, call, entry)


def launch_jk2(torch, hiplib, call, jl, kl):
    """One xt_grad_jk2 call with the lists jl = (wj, PJ, QJ), kl = (wk, PK, QK); an empty list is sent
    as three null pointers."""
    dev, up = _device_tables(torch, call)
    keep = []

    def side(lst):
        w, p, q = lst
        if w is None:
            return 0, None, None, None
        w = np.ascontiguousarray(w, dtype=np.float64)
        dp, dq = up(p), up(q)
        keep.extend([w, dp, dq])
        return len(w), w.ctypes.data, dp.data_ptr(), dq.data_ptr()
    nj, wj, pj, qj = side(jl)
    nk, wk, pk, qk = side(kl)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def entry(work, nw, out):
        return hiplib.xt_grad_jk2(len(call.binfo), *[x.data_ptr() for x in dev[:4]], len(call.kinfo),
                                  *[x.data_ptr() for x in dev[4:8]], call.lbra, call.lket, nj, wj, pj, qj, nk, wk, pk,
                                  qk, call.nao, call.strip, call.natm, work, nw, out, st)
    return _guarded(torch, hiplib, call, entry)


# --------------------------------------------------------------------------- same body, same bits
@pytest.mark.parametrize("c", gc.CASES, ids=[c.name for c in gc.CASES])
def test_two_lists_give_the_bits_of_xt_grad_jk(torch, hiplib, c):
    call = gc.build(c)
    jl, kl = lists_of(c, call)
    assert jl[0] is not None or kl[0] is not None
    want = launch_jk(torch, hiplib, call)
    got = launch_jk2(torch, hiplib, call, jl, kl)
    assert np.all(np.isfinite(got))
    same = np.array_equal(_bits(got), _bits(want))
    print(f"JK2BITS {c.name} <{c.inst[0]},{c.inst[1]}> nj {0 if jl[0] is None else len(jl[0])} nk "
          f"{0 if kl[0] is None else len(kl[0])}: bits {'identical' if same else 'differ'}, max difference "
          f"{np.abs(got - want).max():.3e}")
    assert same, "xt_grad_jk2 does not reproduce the bits of xt_grad_jk on an exact Gamma"
    again = launch_jk2(torch, hiplib, call, jl, kl)
    assert np.array_equal(_bits(again), _bits(got)), "two calls differ"


# --------------------------------------------------------------------------- full lists, empty lists
FULL = {"nterm8": (6, 4), "c21_d": (10, 6), "c21_f": (14, 8)}      # one case per template instance
_FULL = {}


def full_case(name):
    """(case, call of the Coulomb side, call of the exchange side, 40-digit blocks): two builds of eight
    terms each on the tables of ``name``, seeded by their own names."""
    if name not in _FULL:
        base = gc.BY_NAME[name]
        assert base.inst == FULL[name]
        ca = dataclasses.replace(base, name=name + "_jk2a", nterm=8, zero_w=(), ref_of="")
        cb = dataclasses.replace(base, name=name + "_jk2b", nterm=8, zero_w=(), ref_of="")
        a, b = gc.build(ca), gc.build(cb)
        for x in ("binfo", "bprim", "eb", "bra_ao", "kinfo", "kprim", "ek", "ket_ao"):
            assert np.array_equal(getattr(a, x), getattr(b, x))
        assert np.all(a.wj != 0) and np.all(b.wk != 0)
        assert not np.array_equal(np.nan_to_num(a.P), np.nan_to_num(b.P))
        _FULL[name] = (ca, a, b, hint_ref.grad_integrals(a))
    return _FULL[name]


def _only(call, which):
    """The call with the other kind of weight set to zero (the reference of one list)."""
    out = dataclasses.replace(call)
    if which == "j":
        out.wk = np.zeros_like(call.wk)
    else:
        out.wj = np.zeros_like(call.wj)
    return out


@pytest.fixture(scope="module")
def kappa_g():
    return gc.load_kappa()[1]


@pytest.mark.parametrize("name", list(FULL))
def test_full_lists_against_40_digits(torch, hiplib, kappa_g, name):
    """nj = nk = 8 with sixteen distinct matrices: |dev - (ref_1 + ref_2)| <= kappa_g 2^-53 (sabs_1 + sabs_2)
    elementwise; then each list alone with the other's pointers null, against its own reference."""
    c, a, b, blocks = full_case(name)
    jl, _ = lists_of(c, a, jcall=a, kcall=a)
    _, kl = lists_of(c, a, jcall=b, kcall=b)
    assert len(jl[0]) == 8 and len(kl[0]) == 8
    rj, sj, Lrow, _ = hint_ref.ref_grad(_only(a, "j"), blocks=blocks)
    rk, sk, Lk, _ = hint_ref.ref_grad(_only(b, "k"), blocks=blocks)
    assert np.array_equal(Lrow, Lk) and np.all(Lrow >= 0)
    none = (None, None, None)
    for tag, lj, lk_, ref, sabs in (("both", jl, kl, rj + rk, sj + sk), ("nk = 0", jl, none, rj, sj),
                                    ("nj = 0", none, kl, rk, sk)):
        out = launch_jk2(torch, hiplib, a, lj, lk_)
        assert np.all(np.isfinite(out)) and np.any(ref != 0.0)
        ratio = gc.units(out, ref, sabs, Lrow) / kappa_g[Lrow][:, None]
        print(f"JK2RATIO {name} <{c.inst[0]},{c.inst[1]}> {tag}: worst |dev - ref| / bound {ratio.max():.4f}, "
              f"max|ref| {np.abs(ref).max():.3e}")
        assert np.all(ratio <= 1.0), (name, tag, float(ratio.max()))
        again = launch_jk2(torch, hiplib, a, lj, lk_)
        assert np.array_equal(_bits(again), _bits(out)), "two calls differ"
