"""GPU: every dispatch path and Boys regime of the integral kernel, and xt_eval_ao at its edges
(xtddft_amd/csrc/xt_int.hip), one case of tests/int_cases.py at a time against the 40-digit
fixture tests/golden/int_ref*.npz (tests/golden/make_int_ref.py; no mpmath here).

Bound, elementwise: |dev - ref| <= kappa(L) 2^-53 sabs, where sabs is the reference's sum of the
absolute values of every term of that element and kappa(L) is 8 x the error the *host* FP64
routine shows against the same reference at total Hermite order L (floor 64), measured by the
generator and stored in the fixture -- never taken from the device.  Elements whose terms all
vanish (sabs == 0) must be exact zeros.

Isolation: every input table is followed by NaN slack (a read past a table poisons the result),
`out` is a window inside a larger allocation, and everything outside the case's blocks -- the
padding rows and columns of the window and the guard zones around it -- holds a sentinel that
must come back bit-identical.
"""
import numpy as np
import pytest

import int_cases as ic
import int_ref

pytestmark = pytest.mark.gpu

SENTINEL = -7777.25
GUARD = 64
XT_ERR_ARG = -1
PARAMS = [pytest.param(c.name, id=f"lab{c.klass[0]}-lc{c.klass[1]}-{c.name}") for c in ic.CASES]


@pytest.fixture(scope="module")
def torch(hiplib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def fixture():
    return ic.load_fixture()


@pytest.fixture(scope="module")
def results():
    """Device results by case name, shared between the per-case test and the twin test."""
    return {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _up(torch, a, slack=True):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64 and slack:
        a = np.concatenate([a.ravel(), np.full(GUARD, np.nan)])
    return torch.from_numpy(a).cuda()


def call(torch, hiplib, tb, out0=None, *, entry="int2e", kinfo=None, npair=None, nket=None, lmax_orb=None,
         lket=None, omega=None, q_bra=None, q_ket=None, thr=0.0, diag=0, nrow=None, ldo=None):
    """One library call on the tables `tb` (overrides by keyword).  `out0` (nrow, ldo) is the
    initial window (default: zeros inside the blocks, the sentinel elsewhere).  Returns
    (return code, window after the call, window before the call); asserts the guard zones."""
    nrow = tb.nrow if nrow is None else nrow
    ldo_ = tb.ldo if ldo is None else ldo
    if out0 is None:
        out0 = np.where(tb.mask(), 0.0, SENTINEL)
    assert out0.shape == (nrow, abs(ldo_))
    flat = np.concatenate([np.full(GUARD, SENTINEL), out0.ravel(), np.full(GUARD, SENTINEL)])
    d_out = torch.from_numpy(flat).cuda()
    dev = [_up(torch, x) for x in (tb.pinfo, tb.pprim, tb.eab, tb.kinfo if kinfo is None else kinfo, tb.kprim,
                                   tb.ek)]
    dq = [None if q is None else _up(torch, q, slack=False) for q in (q_bra, q_ket)]
    ptr = [x.data_ptr() for x in dev]
    np_ = len(tb.pinfo) if npair is None else npair
    nk = len(tb.kinfo) if nket is None else nket
    lo = tb.lmax_orb if lmax_orb is None else lmax_orb
    lk = tb.lket if lket is None else lket
    om = float(tb.omega if omega is None else omega)
    st = torch.cuda.current_stream().cuda_stream
    optr = d_out.data_ptr() + 8 * GUARD
    if entry == "int3c2e":
        rc = hiplib.xt_int3c2e_cart(np_, ptr[0], ptr[1], ptr[2], nk, ptr[3], ptr[4], ptr[5], lo, lk, om, optr,
                                    ldo_, st)
    else:
        rc = hiplib.xt_int2e_cart(np_, ptr[0], ptr[1], ptr[2], nk, ptr[3], ptr[4], ptr[5], lo, lk, om,
                                  None if dq[0] is None else dq[0].data_ptr(),
                                  None if dq[1] is None else dq[1].data_ptr(), float(thr), int(diag), optr,
                                  ldo_, st)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert np.array_equal(_bits(got[:GUARD]), _bits(flat[:GUARD])), "write before out"
    assert np.array_equal(_bits(got[-GUARD:]), _bits(flat[-GUARD:])), "write past out"
    return rc, got[GUARD:-GUARD].reshape(out0.shape), out0


def _lmap(tb):
    L = np.full((tb.nrow, tb.ldo), -1, dtype=np.int64)
    for _, _, r0, nab, c0, nc, lab, lc in tb.blocks:
        L[r0:r0 + nab, c0:c0 + nc] = lab + lc
    return L


def _bound(fixture, tb, name):
    m = tb.mask()
    kap = np.where(m, fixture["kappa"][np.maximum(_lmap(tb), 0)], 0.0)
    return kap * ic.U * fixture[name + "/sabs"]


def _report(tag, tb, err, bound):
    """Largest |dev - ref| / bound per total order (printed: the figures of the commit message)."""
    L = _lmap(tb)
    for order in np.unique(L[L >= 0]):
        sel = (L == order) & (bound > 0)
        if sel.any():
            print(f"INTRATIO {tag} L={order} {float((err[sel] / bound[sel]).max()):.4f}")


# --------------------------------------------------------------------------- every case
@pytest.mark.parametrize("name", PARAMS)
def test_case_against_the_reference(torch, hiplib, fixture, results, name):
    c = ic.BY_NAME[name]
    tb = ic.build(c)
    rc, out, out0 = call(torch, hiplib, tb)
    assert rc == 0
    results[name] = out
    m = tb.mask()
    assert np.array_equal(_bits(out[~m]), _bits(out0[~m])), "output outside the blocks was touched"
    key = c.ref_of or name
    ref, bound = fixture[key + "/ref"], _bound(fixture, tb, key)
    err = np.abs(out - ref)
    _report(name, tb, np.where(m, err, 0.0), bound)
    assert np.all(np.isfinite(out[m]))
    assert np.all(err[m] <= bound[m]), (name, float((err[m] / np.maximum(bound[m], 1e-300)).max()))


@pytest.mark.parametrize("name", [c.name for c in ic.CASES if c.twin])
def test_both_buckets_give_the_same_bits(torch, hiplib, results, name):
    """k_int_cart<8, 4> (true bounds) and k_int_cart<13, 6> (declared lmax_orb = 3)."""
    outs = []
    for n in (name, ic.BY_NAME[name].twin):
        if n not in results:
            rc, results[n], _ = call(torch, hiplib, ic.build(ic.BY_NAME[n]))
            assert rc == 0
        outs.append(results[n])
    assert ic.BY_NAME[name].bucket == 8 and ic.BY_NAME[ic.BY_NAME[name].twin].bucket == 13
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))


@pytest.mark.parametrize("name", ["far21", "c67_hi", "pc4"])
def test_both_three_index_entries_give_the_same_bits(torch, hiplib, name):
    tb = ic.build(ic.BY_NAME[name])
    rc_a, a, _ = call(torch, hiplib, tb, entry="int3c2e")
    rc_b, b, _ = call(torch, hiplib, tb)
    assert rc_a == 0 and rc_b == 0 and np.array_equal(_bits(a), _bits(b)) and np.any(a[tb.mask()] != 0.0)


# --------------------------------------------------------------------------- flags
def test_diag_blocks_are_the_diagonal_of_the_full_call(torch, hiplib):
    full, kdiag, ldd = ic.pair_ket_tables()
    rc, big, _ = call(torch, hiplib, full)
    assert rc == 0
    out0 = np.full((full.nrow, ldd), SENTINEL)
    for k, j, r0, nab, c0, nc, _, _ in full.blocks:
        if k == j:
            out0[r0:r0 + nab, :nc] = 0.0
    rc, dg, _ = call(torch, hiplib, full, out0, kinfo=kdiag, diag=1, ldo=ldd)
    assert rc == 0
    for k, j, r0, nab, c0, nc, _, _ in full.blocks:
        if k == j:
            assert np.array_equal(_bits(dg[r0:r0 + nab, :nc]), _bits(big[r0:r0 + nab, c0:c0 + nc]))
            assert np.all(dg[r0:r0 + nab, :nc].diagonal() > 0.0)            # (ab|ab) > 0
            assert np.array_equal(_bits(dg[r0:r0 + nab, nc:]), _bits(out0[r0:r0 + nab, nc:]))


def test_screening_skips_strictly_below_the_threshold(torch, hiplib):
    full, _, _ = ic.pair_ket_tables()
    rng = np.random.default_rng(11)
    out0 = rng.uniform(-1.0, 1.0, (full.nrow, full.ldo))
    rc, plain, _ = call(torch, hiplib, full, out0)
    assert rc == 0
    rc, scr, _ = call(torch, hiplib, full, out0, q_bra=ic.SCREEN_Q, q_ket=ic.SCREEN_Q, thr=ic.SCREEN_THR)
    assert rc == 0
    kinds = set()
    for k, j, r0, nab, c0, nc, _, _ in full.blocks:
        prod = ic.SCREEN_Q[k] * ic.SCREEN_Q[j]
        blk = (slice(r0, r0 + nab), slice(c0, c0 + nc))
        if prod < ic.SCREEN_THR:
            kinds.add("below")
            assert np.array_equal(_bits(scr[blk]), _bits(out0[blk])), (k, j)
        else:
            kinds.add("equal" if prod == ic.SCREEN_THR else "above")
            assert np.array_equal(_bits(scr[blk]), _bits(plain[blk])), (k, j)
            assert not np.array_equal(_bits(scr[blk]), _bits(out0[blk]))
    assert kinds == {"below", "equal", "above"}


@pytest.mark.parametrize("name", ["ldo_pad", "c45_hi"])
def test_accumulation_into_a_nonzero_out(torch, hiplib, fixture, name):
    """out += integrals: within the bound of initial + ref, where every primitive quartet's
    update of an element adds one rounding of at most 2^-53 (|initial| + sabs); the same bits
    in two runs."""
    tb = ic.build(ic.BY_NAME[name])
    m = tb.mask()
    rng = np.random.default_rng(3)
    out0 = np.where(m, rng.uniform(-2.0, 2.0, m.shape), SENTINEL)
    rc, a, _ = call(torch, hiplib, tb, out0)
    rc2, b, _ = call(torch, hiplib, tb, out0)
    assert rc == 0 and rc2 == 0 and np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(_bits(a[~m]), _bits(out0[~m]))
    nupd = np.zeros(m.shape)
    for k, j, r0, nab, c0, nc, _, _ in tb.blocks:
        nupd[r0:r0 + nab, c0:c0 + nc] = int(tb.pinfo[k, 2]) * int(tb.kinfo[j, 1])
    sabs = fixture[name + "/sabs"]
    bound = _bound(fixture, tb, name) + nupd * ic.U * (np.abs(out0) + sabs)
    want = out0.astype(np.longdouble) + fixture[name + "/ref"].astype(np.longdouble)
    assert np.all(np.abs(a.astype(np.longdouble) - want)[m] <= bound[m])
    assert np.all(a[m] != out0[m])


# --------------------------------------------------------------------------- arguments
BAD_ARGS = {
    "lmax_orb=4": dict(lmax_orb=4, lket=0),
    "2lmax_orb+lket=14": dict(lmax_orb=3, lket=8),
    "omega<0": dict(omega=-0.25),
    "q_bra alone": dict(q_bra=np.ones(4)),
    "q_ket alone": dict(q_ket=np.ones(4)),
    "diag with nket != npair": dict(diag=1),
    "npair<0": dict(npair=-1),
    "nket<0": dict(nket=-1),
    "ldo<0": dict(ldo="negative"),
}


@pytest.mark.parametrize("what", list(BAD_ARGS))
def test_argument_errors_leave_out_untouched(torch, hiplib, what):
    tb = ic.build(ic.BY_NAME["c21_b8"])
    assert len(tb.pinfo) == 3 and len(tb.kinfo) == 2
    out0 = np.random.default_rng(1).uniform(-1.0, 1.0, (tb.nrow, tb.ldo))
    kw = dict(BAD_ARGS[what])
    if kw.get("ldo") == "negative":
        kw["ldo"] = -tb.ldo
    rc, out, _ = call(torch, hiplib, tb, out0, **kw)
    assert rc == XT_ERR_ARG
    assert np.array_equal(_bits(out), _bits(out0))


@pytest.mark.parametrize("empty", [dict(npair=0), dict(nket=0), dict(npair=0, nket=0, diag=1)])
def test_empty_calls_touch_nothing(torch, hiplib, empty):
    tb = ic.build(ic.BY_NAME["ldo_pad"])
    out0 = np.random.default_rng(2).uniform(-1.0, 1.0, (tb.nrow, tb.ldo))
    rc, out, _ = call(torch, hiplib, tb, out0, **empty)
    assert rc == 0 and np.array_equal(_bits(out), _bits(out0))


# --------------------------------------------------------------------------- xt_eval_ao
@pytest.fixture(scope="module")
def ao(fixture):
    """The s-to-g molecule, its kernel tables, the 301 points and the long double reference."""
    from xtddft_amd.qc.dints import _sph_table, ao_shell_tables
    mol = ic.ao_mol()
    coords, far = ic.ao_points()
    info, dat = ao_shell_tables(mol)
    sph = _sph_table()
    ref, sabs, amp = int_ref.ref_eval_ao(coords, info, dat, sph, mol._norm, mol.nao)
    return dict(mol=mol, coords=coords, far=far, info=info, dat=dat, sph=sph, ref=ref,
                bound=int_ref.ao_bound(float(fixture["ao_c"]), sabs, amp), sabs=sabs)


def _eval_ao(torch, hiplib, ao, deriv):
    """xt_eval_ao into ldo = nao + 3, comp_stride = ngrid ldo + 11 inside a sentinel-filled
    allocation; returns (planes (4, ngrid, ldo), the whole allocation, mask of the elements the
    call may write)."""
    n, ng = ao["mol"].nao, ao["coords"].shape[0]
    ldo, cs = n + 3, ng * (n + 3) + 11
    flat = np.full(2 * GUARD + 4 * cs, SENTINEL)
    d_out = torch.from_numpy(flat).cuda()
    dev = [_up(torch, x) for x in (ao["coords"], ao["info"], ao["dat"], ao["sph"], ao["mol"]._norm)]
    rc = hiplib.xt_eval_ao(ng, dev[0].data_ptr(), len(ao["info"]), dev[1].data_ptr(), dev[2].data_ptr(),
                           dev[3].data_ptr(), dev[4].data_ptr(), deriv, d_out.data_ptr() + 8 * GUARD, ldo, cs,
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    got = d_out.cpu().numpy()
    may = np.zeros(flat.shape, dtype=bool)
    for c in range(4 if deriv else 1):
        w = may[GUARD + c * cs:GUARD + c * cs + ng * ldo].reshape(ng, ldo)
        w[:, :n] = True
    assert np.array_equal(_bits(got[~may]), _bits(flat[~may])), "xt_eval_ao wrote outside its output"
    planes = np.stack([got[GUARD + c * cs:GUARD + c * cs + ng * ldo].reshape(ng, ldo) for c in range(4)])
    return planes, got, may


def test_eval_ao_values_and_gradients_to_g_shells(torch, hiplib, ao):
    n = ao["mol"].nao
    assert (ao["coords"].shape[0] * len(ao["info"])) % 256 != 0 and ao["info"][:, 0].max() == 4
    planes, _, _ = _eval_ao(torch, hiplib, ao, 1)
    dev = planes[:, :, :n]
    assert np.all(np.isfinite(dev))
    err = np.abs(dev.astype(np.longdouble) - ao["ref"])
    live = ao["sabs"] > 1e-290
    print(f"AORATIO {float((err[live] / ao['bound'][live]).max()):.4f}")
    assert np.all(err <= ao["bound"])
    assert np.all(dev[:, ao["far"]] == 0.0)              # every exponential underflows: exact zeros
    # on a centre the p gradient is the radial part alone (every ix px[ix - 1] guard is taken)
    assert np.all(np.abs(np.diagonal(dev[1:, 0, 1:4])) > 0.1) and np.all(dev[0, 0, 1:4] == 0.0)


def test_eval_ao_deriv0_writes_the_value_plane_only(torch, hiplib, ao):
    n = ao["mol"].nao
    p0, _, _ = _eval_ao(torch, hiplib, ao, 0)
    p1, _, _ = _eval_ao(torch, hiplib, ao, 1)
    assert np.array_equal(_bits(p0[0]), _bits(p1[0]))
    assert np.all(p0[1:] == SENTINEL) and not np.any(p1[:, :, :n] == SENTINEL)
