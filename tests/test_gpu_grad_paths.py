"""GPU: the derivative-ERI gradient kernel ``xt_grad_jk`` (xtddft_amd/csrc/xt_grad.hip) per quartet
class against 40 digits, through raw calls of the C entry (tests/grad_cases.py; the claims of the
table are checked on the host by tests/test_grad_cases.py).

Both tiers are elementwise, |dev - ref| <= kappa 2^-53 sabs, with ref and sabs (the same sum over
the absolute values of every factor) from hint_ref.ref_grad.

Tier 1, selector probes: Gamma picks one (ab, cd) per bra row, so g[k][m] is a single derivative
integral and the bound is the one tests/test_gpu_somf.py holds xt_hint_cart to: kappa(L) of
tests/golden/int_ref.npz.  The exchange mapping and the image must reproduce the Coulomb
selector's bits (twice them for Q = e_c e_d^T + e_d e_c^T).

Tier 2, dense dyadic Gamma: every case of the table against ref_grad with kappa_g(L) of
tests/golden/grad_kappa.json (8 x the host restatement's error, floor 64).  Where sabs = 0 the
output is an exact zero, output rows without a bra entry keep their bits, two calls give the same
bits, and every strip length stays inside the same bound.

Every call: NaN slack behind every float table, NaN wherever P / Q are not to be read, sentinel
guards around `out` and behind `work[nwork]`, `work` NaN before the call, nwork exactly
3 nbra (nstrip + 1), and the same call with nwork - 1 refused with `out` untouched.
"""
import ctypes

import numpy as np
import pytest

import grad_cases as gc
import hint_ref
import int_cases as ic

pytestmark = pytest.mark.gpu

SENTINEL = -7777.25
GUARD = 64
U = 2.0 ** -53
_BLOCKS, _DEV = {}, {}


@pytest.fixture(scope="module")
def torch(hiplib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def kappa():
    k = ic.load_fixture()["kappa"]
    return np.concatenate([k, [k.max()] * (15 - len(k))])


@pytest.fixture(scope="module")
def kappa_g():
    return gc.load_kappa()[1]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def tables_of(c):
    """(call, 40-digit integral blocks) of a case, once per set of tables in this module."""
    name = c.ref_of or c.name
    if name not in _BLOCKS:
        call = gc.build(gc.BY_NAME[name])
        _BLOCKS[name] = (call, hint_ref.grad_integrals(call))
    call, blocks = _BLOCKS[name]
    return (call if name == c.name else gc.build(c)), blocks


def launch(torch, hiplib, call):
    """One xt_grad_jk call under the memory discipline of the module docstring: `out` after it."""
    def up(a):
        a = np.ascontiguousarray(a)
        if a.dtype == np.float64:
            a = np.concatenate([a.ravel(), np.full(GUARD, np.nan)])
        return torch.from_numpy(a).cuda()
    dev = [up(x) for x in (call.binfo, call.bprim, call.eb, call.bra_ao, call.kinfo, call.kprim, call.ek, call.ket_ao,
                           call.P, call.Q)]
    flat = np.concatenate([np.full(GUARD, SENTINEL), call.out0.ravel(), np.full(GUARD, SENTINEL)])
    nwork = call.nwork
    wflat = np.concatenate([np.full(nwork, np.nan), np.full(GUARD, SENTINEL)])
    wj, wk = np.ascontiguousarray(call.wj, dtype=np.float64), np.ascontiguousarray(call.wk, dtype=np.float64)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(nw):
        d_out, d_work = torch.from_numpy(flat.copy()).cuda(), torch.from_numpy(wflat.copy()).cuda()
        rc = hiplib.xt_grad_jk(len(call.binfo), *[x.data_ptr() for x in dev[:4]], len(call.kinfo),
                               *[x.data_ptr() for x in dev[4:8]], call.lbra, call.lket, len(wj), wj.ctypes.data,
                               wk.ctypes.data, dev[8].data_ptr(), dev[9].data_ptr(), call.nao, call.strip, call.natm,
                               d_work.data_ptr(), nw, d_out.data_ptr() + 8 * GUARD, st)
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
        "a workspace element is NaN: not written, or summed from an element of P / Q outside the case's ranges"
    return got[GUARD:-GUARD].reshape(call.natm, 3)


def check(tag, call, out, ref, sabs, Lrow, kap):
    """The elementwise bound; returns the largest error / bound."""
    rows = Lrow >= 0
    assert np.array_equal(_bits(out[~rows]), _bits(call.out0[~rows])), "a row without a bra entry changed"
    assert np.all(np.isfinite(out)), tag
    un = gc.units(out, ref, sabs, Lrow)                           # asserts exact zeros where sabs = 0
    ratio = un / kap[np.maximum(Lrow, 0)][:, None]
    by_l = {int(L): float(ratio[Lrow == L].max()) for L in sorted(set(Lrow[rows]))}
    print(f"GRADRATIO {tag} L={int(Lrow.max())} worst |dev - ref| / bound {ratio.max():.4f}  by L "
          + " ".join(f"{L}:{r:.4f}" for L, r in by_l.items()) + f"  max|ref| {np.abs(ref).max():.3e}")
    assert np.all(ratio <= 1.0), (tag, float(ratio.max()))
    return float(ratio.max())


def inst_tag(c):
    return f"{c.name} <{c.inst[0]},{c.inst[1]}>"


# --------------------------------------------------------------------------- tier 1
@pytest.mark.parametrize("c", gc.PROBE_CASES, ids=[c.name for c in gc.PROBE_CASES])
def test_selector_probes_are_single_integrals(torch, hiplib, kappa, c):
    call, blocks = tables_of(c)
    sel = gc.selector(c, call, "J")
    ref, sabs, Lrow, _ = hint_ref.ref_grad(sel, blocks=blocks)
    assert np.all(Lrow == c.klass[0] + c.klass[1])
    out = launch(torch, hiplib, sel)
    check(inst_tag(c) + " selector", sel, out, ref, sabs, Lrow, kappa)
    assert np.any(ref != 0.0) and np.any(out != 0.0)
    exch = launch(torch, hiplib, gc.selector(c, call, "K"))
    assert np.array_equal(_bits(exch), _bits(out)), "P[a,c] Q[b,d] does not pick the integral P[a,b] Q[c,d] picks"
    if call.ket_ao[0, 3]:
        img = launch(torch, hiplib, gc.selector(c, call, "Jimg"))
        assert np.array_equal(_bits(img), _bits(out)), "the (d, c) image is not the (c, d) integral"
        both = launch(torch, hiplib, gc.selector(c, call, "Jsum"))
        assert np.array_equal(_bits(both), _bits(2.0 * out)), "Q + Q^T on an image ket is not twice the integral"


# --------------------------------------------------------------------------- tier 2
def dense(torch, hiplib, c):
    if c.name not in _DEV:
        call, _ = tables_of(c)
        out = launch(torch, hiplib, call)
        out.setflags(write=False)
        _DEV[c.name] = out
    return _DEV[c.name]


@pytest.mark.parametrize("c", gc.CASES, ids=[c.name for c in gc.CASES])
def test_dense_gamma_against_40_digits(torch, hiplib, kappa_g, c):
    call, blocks = tables_of(c)
    ref, sabs, Lrow, _ = hint_ref.ref_grad(call, blocks=blocks)
    out = dense(torch, hiplib, c)
    check(inst_tag(c) + f" cache {''.join(sorted(c.cache))} image {''.join(sorted(c.image))} strips {c.strips}", call, out,
          ref, sabs, Lrow, kappa_g)
    assert np.any(ref[Lrow >= 0] != 0.0) or c.name == "onec_s"
    if c.name == "onec_s":
        assert not np.any(sabs) and not np.any(out)               # every term an exact zero by parity
    again = launch(torch, hiplib, call)
    assert np.array_equal(_bits(again), _bits(out)), "two calls differ"
    if c.ref_of:
        base = dense(torch, hiplib, gc.BY_NAME[c.ref_of])
        same = np.array_equal(_bits(base), _bits(out))
        print(f"{c.name} against {c.ref_of}: bits {'identical' if same else 'differ'}, "
              f"max difference {np.abs(base - out).max():.3e}")
    if c.out0:
        assert np.any(call.out0 != 0.0) and np.any(Lrow < 0)
