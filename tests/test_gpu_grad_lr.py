"""GPU: ``xt_grad_jk2_lr`` (xtddft_amd/csrc/xt_grad.hip), the derivative-ERI gradient kernel over
erf(omega r12) / r12, through raw calls of the C entry against the 40-digit reference of
tests/rsh_ref.py: elementwise |dev - ref| <= kappa_lr(L) 2^-53 sabs with kappa_lr of
tests/golden/rsh_kappa.json (measured from the host FP64 restatement by the rule of make_grad_kappa.py).

* per class: the 49 cases ``c{ob}{ok}`` of tests/grad_cases.py at omega = 0.33, each with its own lists;
* limits: one case per template instance at omega = 0.2, 2^-4 and 16 with both lists full (sixteen
  distinct matrices, ``test_gpu_grad_jk2.full_case``), then nj = 0 and nk = 0 with null pointers;
* structure: the Gamma cache on both sides of its threshold, the image flag, the strips and the fold at
  omega = 0.33, and the far pair (two centres 20 Bohr apart: a2 R^2 on both sides of 30, both regimes of
  ``hint_boys`` under attenuation);
* linearity: ``xt_grad_jk2`` with the exchange weights hyb wk plus ``xt_grad_jk2_lr`` with (alpha - hyb) wk
  against hyb ref + (alpha - hyb) ref_lr inside the sum of the two bounds, with CAM-B3LYP's 0.19 and 0.46:
  how the gradient drivers use the pair (``qc.grad.grad_jk_rsh``).

Every call carries the memory discipline of tests/test_gpu_grad_jk2.py (``_guarded``, ``lists_of``): NaN slack
behind every float table, NaN wherever a list's P / Q are not to be read, sentinel guards around `out` and
behind `work[nwork]`, the call with nwork - 1 refused with nothing written, and two calls give equal bits.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

import grad_cases as gc
import hint_ref
import rsh_ref
import test_gpu_grad_jk2 as J

pytestmark = pytest.mark.gpu

NONE = (None, None, None)


@pytest.fixture(scope="module")
def torch(hiplib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def kappa_lr():
    return rsh_ref.load_kappa()[1]


_BLOCKS = {}


def blocks_lr(key, call, omega):
    """The 40-digit long-range integrals of a call's tables, computed once per (tables, omega)."""
    if (key, omega) not in _BLOCKS:
        _BLOCKS[key, omega] = rsh_ref.grad_integrals_lr(call, omega)
    return _BLOCKS[key, omega]


def launch_lr(torch, hiplib, call, jl, kl, omega):
    """One xt_grad_jk2_lr call with the lists jl = (wj, PJ, QJ), kl = (wk, PK, QK); an empty list is sent as
    three null pointers."""
    dev, up = J._device_tables(torch, call)
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
        return hiplib.xt_grad_jk2_lr(len(call.binfo), *[x.data_ptr() for x in dev[:4]], len(call.kinfo),
                                     *[x.data_ptr() for x in dev[4:8]], call.lbra, call.lket, nj, wj, pj, qj, nk, wk,
                                     pk, qk, call.nao, call.strip, call.natm, work, nw, out, st, float(omega))
    return J._guarded(torch, hiplib, call, entry)


def check(torch, hiplib, kappa, tag, call, jl, kl, omega, ref, sabs, Lrow):
    out = launch_lr(torch, hiplib, call, jl, kl, omega)
    assert np.all(np.isfinite(out))
    ratio = gc.units(out, ref, sabs, Lrow) / kappa[np.maximum(Lrow, 0)][:, None]
    print(f"LRRATIO {tag} omega {omega:g}: worst |dev - ref| / bound {ratio.max():.4f}, max|ref| "
          f"{np.abs(ref).max():.3e}")
    assert np.all(ratio <= 1.0), (tag, omega, float(ratio.max()))
    again = launch_lr(torch, hiplib, call, jl, kl, omega)
    assert np.array_equal(J._bits(again), J._bits(out)), "two calls differ"
    return out


def own_lists(torch, hiplib, kappa, c, call, omega):
    jl, kl = J.lists_of(c, call)
    assert jl[0] is not None or kl[0] is not None
    ref, sabs, Lrow, _ = hint_ref.ref_grad(call, blocks=blocks_lr(c.ref_of or c.name, call, omega))
    assert np.any(ref != call.out0) or c.name.startswith("onec")
    return check(torch, hiplib, kappa, c.name, call, jl, kl, omega, ref, sabs, Lrow)


# --------------------------------------------------------------------------- per class
CLASS_CASES = [c for c in gc.CASES if c.probe and not c.ref_of]
assert len(CLASS_CASES) == 49


@pytest.mark.parametrize("c", CLASS_CASES, ids=[c.name for c in CLASS_CASES])
def test_every_class_against_40_digits(torch, hiplib, kappa_lr, c):
    own_lists(torch, hiplib, kappa_lr, c, gc.build(c), rsh_ref.OMEGA)


# --------------------------------------------------------------------------- limits
@pytest.mark.parametrize("omega", rsh_ref.LIMIT_OMEGAS)
@pytest.mark.parametrize("name", rsh_ref.LIMIT_CASES)
def test_full_lists_at_small_and_large_omega(torch, hiplib, kappa_lr, name, omega):
    """nj = nk = 8 with sixteen distinct matrices, then each list alone with the other's pointers null."""
    c, a, b, _ = J.full_case(name)
    blocks = blocks_lr(name + "_full", a, omega)
    jl, _ = J.lists_of(c, a, jcall=a, kcall=a)
    _, kl = J.lists_of(c, a, jcall=b, kcall=b)
    assert len(jl[0]) == 8 and len(kl[0]) == 8
    rj, sj, Lrow, _ = hint_ref.ref_grad(J._only(a, "j"), blocks=blocks)
    rk, sk, Lk, _ = hint_ref.ref_grad(J._only(b, "k"), blocks=blocks)
    assert np.array_equal(Lrow, Lk) and np.all(Lrow >= 0)
    for tag, lj, lk_, ref, sabs in (("both", jl, kl, rj + rk, sj + sk), ("nk = 0", jl, NONE, rj, sj),
                                    ("nj = 0", NONE, kl, rk, sk)):
        assert np.any(ref != 0.0)
        check(torch, hiplib, kappa_lr, f"{name} <{c.inst[0]},{c.inst[1]}> {tag}", a, lj, lk_, omega, ref, sabs, Lrow)


# --------------------------------------------------------------------------- structure
@pytest.mark.parametrize("name", rsh_ref.STRUCTURE_CASES)
def test_cache_image_strips_and_fold(torch, hiplib, kappa_lr, name):
    c = gc.BY_NAME[name]
    own_lists(torch, hiplib, kappa_lr, c, gc.build(c), rsh_ref.OMEGA)


def test_far_pair_runs_both_boys_regimes(torch, hiplib, kappa_lr):
    c, call = rsh_ref.far_case()
    T = rsh_ref.boys_arguments(call, rsh_ref.OMEGA)
    assert T.min() < 30.0 < T.max()
    own_lists(torch, hiplib, kappa_lr, c, call, rsh_ref.OMEGA)


# --------------------------------------------------------------------------- linearity
def test_full_range_plus_long_range_as_the_drivers_call_them(torch, hiplib, kappa_lr):
    """Call 1: xt_grad_jk2 with the Coulomb list and hyb wk; call 2: xt_grad_jk2_lr with nj = 0 and
    (alpha - hyb) wk; their sum against the sum of the two references inside the sum of the two bounds."""
    c = gc.BY_NAME["nterm8"]
    call = gc.build(c)
    hyb, k_lr = rsh_ref.CAM_HYB, rsh_ref.CAM_ALPHA - rsh_ref.CAM_HYB
    assert abs(k_lr - 0.46) < 1e-15
    full = dataclasses.replace(call)
    full.wk = hyb * call.wk
    lr = dataclasses.replace(call)
    lr.wj, lr.wk = np.zeros_like(call.wj), k_lr * call.wk
    jl, kl_full = J.lists_of(c, full)
    _, kl_lr = J.lists_of(c, lr)
    r1, s1, Lrow, _ = hint_ref.ref_grad(full, blocks=hint_ref.grad_integrals(call))
    r2, s2, L2, _ = hint_ref.ref_grad(lr, blocks=blocks_lr(c.name, call, rsh_ref.OMEGA))
    assert np.array_equal(Lrow, L2)
    out1 = J.launch_jk2(torch, hiplib, full, jl, kl_full)
    out2 = launch_lr(torch, hiplib, lr, NONE, kl_lr, rsh_ref.OMEGA)
    kg = gc.load_kappa()[1]
    bound = gc.U * (kg[Lrow][:, None] * s1 + kappa_lr[Lrow][:, None] * s2)
    err = np.abs(out1 + out2 - (r1 + r2))
    print(f"LRSUM nterm8: worst |dev - ref| / bound {(err / bound).max():.4f}, max|ref| {np.abs(r1 + r2).max():.3e}, "
          f"long-range share {np.abs(r2).max() / np.abs(r1 + r2).max():.3f}")
    assert np.any(r2 != 0.0) and np.all(err <= bound)
    assert np.array_equal(J._bits(J.launch_jk2(torch, hiplib, full, jl, kl_full)), J._bits(out1)), "two calls differ"
    assert np.array_equal(J._bits(launch_lr(torch, hiplib, lr, NONE, kl_lr, rsh_ref.OMEGA)), J._bits(out2)), \
        "two calls differ"
