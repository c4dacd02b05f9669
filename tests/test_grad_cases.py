"""CPU: the case table of the gradient kernel (tests/grad_cases.py) runs what it claims, is closed
over what ``grad_jk`` (xtddft_amd/csrc/xt_grad.hip) can launch, stays inside its arrays, and its
reference (hint_ref.ref_grad, 40 digits) agrees with the host FP64 restatement inside the bound
the GPU test uses -- while a deliberately wrong reference falls outside it.  Needs mpmath.

The dispatch restated here from the kernel source, independently of grad_cases._inst:
  instance   the first of <6,4>, <10,6>, <14,8> with declared lbra <= MAXLB and lbra + lket <= MAXL
  cache      a (bra row, ket) block is cached iff nab * ncol <= 81; G is a stack array of 81 doubles
  threads    id -> (strip, row) = (id / nbra, id % nbra), nstrip = ceil(nket / strip), blocks of 64;
             strip s takes the kets s, s + nstrip, ...
"""
import numpy as np
import pytest

import grad_cases as gc
import hint_ref
import int_cases as ic

IDS = [c.name for c in gc.CASES]
_CALLS, _REF = {}, {}


def call_of(c):
    if c.name not in _CALLS:
        _CALLS[c.name] = gc.build(c)
    return _CALLS[c.name]


def ref_of(c):
    name = c.ref_of or c.name
    if name not in _REF:
        _REF[name] = hint_ref.ref_grad(call_of(gc.BY_NAME[name]))
        for x in _REF[name]:
            x.setflags(write=False)
    return _REF[name]


def ntuv(L):
    return (L + 1) * (L + 2) * (L + 3) // 6


def restated_instance(lbra, lket):
    for maxl, maxlb in ((6, 4), (10, 6), (14, 8)):
        if lbra <= maxlb and lbra + lket <= maxl:
            return maxl, maxlb
    raise AssertionError("XT_ERR_ARG")


# --------------------------------------------------------------------------- claims
@pytest.mark.parametrize("c", gc.CASES, ids=IDS)
def test_case_runs_what_it_claims(c):
    call = call_of(c)
    nbra, nket = len(call.binfo), len(call.kinfo)
    assert c.inst == restated_instance(call.lbra, call.lket)
    # no entry above the declared bounds (the kernel would skip it silently), none above the instance's arrays
    assert call.binfo[:, 0].max() <= call.lbra and call.kinfo[:, 0].max() <= call.lket
    assert call.binfo[:, 0].max() + call.kinfo[:, 0].max() <= c.inst[0] and call.binfo[:, 0].max() <= c.inst[1]
    cache = set()
    for k in range(nbra):
        nab = call.binfo[k, 1] // 3
        assert 3 * nab == call.binfo[k, 1] == 3 * c.bras[k].nab and call.binfo[k, 0] == c.bras[k].order
        for j in range(nket):
            ncol = call.kinfo[j, 5]
            assert ncol == c.kets[j].ncol and call.kinfo[j, 0] == c.kets[j].order
            cached = nab * ncol <= 81
            cache.add("c" if cached else "u")
            if cached:
                assert (ncol - 1) * nab + nab - 1 < 81          # the last element of G
    assert c.cache == cache
    assert c.image == {"i" if f else "n" for f in call.ket_ao[:, 3]}
    nstrip = -(-nket // call.strip)
    owner = [[j for j in range(s, nket, nstrip)] for s in range(nstrip)]
    assert sorted(sum(owner, [])) == list(range(nket)) and all(len(o) <= call.strip for o in owner)
    assert c.strips == (nstrip, len(owner[-1]))
    assert c.blocks == -(-nbra * nstrip // 64)
    assert call.nwork == 3 * nbra * (nstrip + 1)
    if c.probe:
        assert nbra == 4 and nket == 1 and len({tuple(r) for r in call.binfo}) == 1
        assert len({(r[0], r[1], r[3]) for r in call.bra_ao}) == 4


def test_table_is_closed_and_covers_what_the_issue_lists():
    combos = {(c.inst, "c" if b.nab * k.ncol <= 81 else "u", "i" if k.flag else "n")
              for c in gc.CASES for b in c.bras for k in c.kets}
    assert combos == {(i, cu, im) for i in gc.INSTANCES for cu in "cu" for im in "in"}
    # every (bra order, ket order) pair that s..f shells form, with its own case
    assert {c.klass for c in gc.PROBE_CASES if not c.ref_of} == {(ob, ok) for ob in range(1, 8) for ok in range(7)}
    pos = [set(), set(), set(), set()]
    prims = [set(), set()]
    for c in gc.CASES:
        for b in c.bras:
            for k in c.kets:
                for s, l in zip(pos, (b.la, b.lb, k.lc, k.ld)):
                    s.add(l)
                prims[0] |= {b.na, b.nb}
                prims[1] |= {k.nc, k.nd}
    assert all(s == {0, 1, 2, 3} for s in pos) and prims == [{1, 3}, {1, 3}]
    ls = {(c.bras[0].la, c.bras[0].lb, c.kets[0].lc, c.kets[0].ld) for c in gc.CASES}
    assert (0, 0, 0, 0) in ls and (3, 3, 3, 3) in ls
    assert any(b.ca == b.cb for c in gc.CASES for b in c.bras)
    assert any({b.ca, b.cb, k.cc, k.cd} == {0} for c in gc.CASES for b in c.bras for k in c.kets)
    # both sides of the four dispatch edges, by the declared orders
    decl = {(c.lbra, c.lket) for c in gc.CASES}
    assert {4, 5, 6, 7} <= {lb for lb, _ in decl}
    for lo, hi, cap in ((6, 7, 4), (10, 11, 6)):
        assert any(lb + lk == lo and lb <= cap for lb, lk in decl) and any(lb + lk == hi and lb <= cap for lb, lk in decl)
    # a class again in the two larger instances
    for base, tags in (("c21", ("c21_d", "c21_f")), ("c20", ("c20_d", "c20_f"))):
        assert gc.BY_NAME[base].inst == (6, 4)
        assert [gc.BY_NAME[t].inst for t in tags] == [(10, 6), (14, 8)] and all(gc.BY_NAME[t].ref_of == base for t in tags)
    # the cache threshold
    sizes = {n: {b.nab * k.ncol for b in gc.BY_NAME[n].bras for k in gc.BY_NAME[n].kets}
             for n in ("cth54", "cth81", "cth108", "cth162", "cth54_twin", "cth81_twin")}
    assert sizes["cth54"] == {54} and sizes["cth81"] == {81} and sizes["cth108"] == {108} and sizes["cth162"] == {162}
    assert any(2 in (b.la, b.lb) for b in gc.BY_NAME["cth54"].bras)
    assert all(gc.BY_NAME[n].inst == (6, 4) for n in sizes)
    for n, small in (("cth54_twin", 54), ("cth81_twin", 81)):
        c = gc.BY_NAME[n]
        per_ket = [c.bras[0].nab * k.ncol for k in c.kets]
        assert c.strips[0] == 1 and per_ket[0] == small and per_ket[1] > 81 and per_ket[2] <= 81
    # image, ncb fallback, nterm, weights
    assert any(k.flag and not k.same for c in gc.CASES for k in c.kets)
    assert any(k.same and not k.flag for c in gc.CASES for k in c.kets)
    assert [(k.same, k.flag) for k in gc.BY_NAME["img_off"].kets] == [(False, 0)]
    z = call_of(gc.BY_NAME["ncb0"])
    assert z.bra_ao[0, 2] == 0 and z.ket_ao[0, 2] == 0 and (z.binfo[0, 0], z.kinfo[0, 0]) == (1, 0)
    assert {1, 2, 8} <= {c.nterm for c in gc.CASES}
    w = [call_of(c) for c in gc.CASES if c.zero_w]
    assert any(np.any(x.wj == 0) for x in w) and any(np.any(x.wk == 0) for x in w)
    # the thread map and the fold
    m = gc.BY_NAME["map70"]
    assert len(m.bras) == 70 and len(m.kets) == 5 and m.strip == 2 and m.strips == (3, 1) and m.blocks == 4
    assert 70 * 3 % 64 != 0 and len({b.block for b in m.bras}) == 4 and len(call_of(m).eb) < 2000
    assert len({b.block for b in m.bras[:64]}) > 1                       # waves of mixed classes
    assert {gc.BY_NAME[f"map70_s{s}"].strip for s in (1, 5, 1000)} == {1, 5, 1000}
    f = call_of(gc.BY_NAME["fold"])
    atoms = f.bra_ao[:, 3]
    assert len(set(atoms)) < len(atoms) and f.natm > atoms.max() + 1 and set(range(f.natm)) - set(atoms)
    assert np.all(f.out0 != 0.0) and all(not np.any(call_of(c).out0) for c in gc.CASES if not c.out0)


# --------------------------------------------------------------------------- bounds of every array
@pytest.mark.parametrize("c", gc.CASES, ids=IDS)
def test_case_stays_inside_its_arrays(c):
    call = call_of(c)
    assert call.bprim.size % 4 == 0 and call.kprim.size % 4 == 0
    for lb, nrow, npp, q0, e0 in call.binfo[:, :5]:
        assert 0 <= q0 and q0 + npp <= call.bprim.size // 4 and 0 <= e0 and e0 + nrow * ntuv(lb) * npp <= call.eb.size
    for lk, nr, r0, e0, _, ncol in call.kinfo[:, :6]:
        assert 0 <= r0 and r0 + nr <= call.kprim.size // 4 and 0 <= e0 and e0 + ncol * ntuv(lk) * nr <= call.ek.size
    assert np.all((call.bra_ao[:, 3] >= 0) & (call.bra_ao[:, 3] < call.natm)) and call.out0.shape == (call.natm, 3)
    assert call.P.shape == call.Q.shape == (len(call.wj), call.nao, call.nao) and 1 <= len(call.wj) <= 8
    # every AO range inside nao, all ranges disjoint, and what grad_gamma reads is exactly the non-NaN part
    ranges = []
    for b, (a0, b0, ncb, _) in zip(c.bras, call.bra_ao):
        ranges += [(a0, a0 + gc.ncart(b.la)), (b0, b0 + gc.ncart(b.lb))]
        assert ncb == (0 if b.ncb0 else gc.ncart(b.lb))
    for k, (c0, d0, ncd, _) in zip(c.kets, call.ket_ao):
        ranges += [(c0, c0 + gc.ncart(k.lc))] + ([] if k.same else [(d0, d0 + gc.ncart(k.ld))])
        assert ncd == (0 if k.ncd0 else gc.ncart(k.ld)) and (c0 == d0) == k.same
    ranges.sort()
    assert ranges[0][0] >= 0 and ranges[-1][1] < call.nao
    assert all(hi < lo2 for (_, hi), (lo2, _) in zip(ranges, ranges[1:]))
    calls = [call] + ([gc.selector(c, call, kind) for kind in gc.SELECTORS] if c.probe else [])
    for x in calls:
        assert np.array_equal(np.isfinite(x.P), np.broadcast_to(call.pmask, x.P.shape))
        assert np.array_equal(np.isfinite(x.Q), np.broadcast_to(call.qmask, x.Q.shape))
        assert 0 < call.pmask.sum() < call.nao ** 2 and 0 < call.qmask.sum() < call.nao ** 2
        for k in range(len(call.binfo)):
            for j in range(len(call.kinfo)):
                assert np.all(np.isfinite(hint_ref.gamma_block(x, k, j)))
    # the dyadic inputs: every Gamma element exact in float64
    assert np.all(np.isin(call.wj, gc.WEIGHTS + (0.0,))) and np.all(np.isin(call.wk, gc.WEIGHTS + (0.0,)))
    for M in (call.P[np.isfinite(call.P)], call.Q[np.isfinite(call.Q)]):
        assert np.all(M * 4 == np.round(M * 4)) and np.abs(M).max() <= 1.0


def test_selectors_pick_single_integrals():
    for c in gc.PROBE_CASES:
        call = call_of(c)
        pr = gc.probes(c, call)
        assert len(pr) >= 4
        for kind in gc.SELECTORS:
            x = gc.selector(c, call, kind)
            on_image = bool(call.ket_ao[0, 3])
            for k, (ab, cd) in enumerate(pr):
                g = hint_ref.gamma_block(x, k, 0)
                want = np.zeros_like(g)
                diag = c.kets[0].same and cd // gc.ncart(c.kets[0].ld) == cd % gc.ncart(c.kets[0].ld)
                want[ab, cd] = {"J": 1.0, "K": 1.0, "Jimg": float(on_image or diag), "Jsum": 1.0 + float(on_image or diag)}[kind]
                if kind in ("Jimg", "Jsum") and c.kets[0].same and not diag:
                    continue                                    # (d, c) is another element of a diagonal pair's block
                assert np.array_equal(g, want), (c.name, kind, k)


# --------------------------------------------------------------------------- the reference and the bound
def test_kappa_file_follows_the_protocol():
    host, kg = gc.load_kappa()
    kappa = ic.load_fixture()["kappa"]
    assert host.shape == kg.shape == (gc.L_MAX + 1,) and len(kappa) >= gc.L_MAX + 1
    assert np.allclose(kg, gc.kappa_from(host), rtol=0, atol=1e-3)
    assert np.all(host[1:] > 0)                                  # every total order 1 .. 13 was measured


@pytest.mark.parametrize("c", gc.REF_CASES, ids=[c.name for c in gc.REF_CASES])
def test_reference_against_the_host_restatement(c):
    call = call_of(c)
    ref, sabs, Lrow, nsum = ref_of(c)
    host = hint_ref.host_grad(call)
    stored, kg = gc.load_kappa()
    kappa = ic.load_fixture()["kappa"]
    un = gc.units(host, ref, sabs, Lrow)
    rows = Lrow >= 0
    print(f"{c.name}: host {un.max():.2f} units, L {Lrow.max()}")
    assert np.all(un[rows].max(axis=1) <= stored[Lrow[rows]] * (1 + 1e-3) + 1e-3)     # the stored figures are these
    assert np.all(un[rows] <= kg[Lrow[rows]][:, None])
    assert np.all(kg[Lrow[rows]] <= kappa[Lrow[rows]] + nsum[rows])                    # Higham's gamma_n ceiling
    assert np.array_equal(host[~rows], call.out0[~rows]) and np.array_equal(ref[~rows], call.out0[~rows])
    assert np.any(ref[rows] != 0.0) or c.name == "onec_s"
    if c.name == "onec_s":                                       # every term vanishes by parity: exact zeros
        assert not np.any(sabs) and not np.any(ref) and not np.any(host)


@pytest.mark.parametrize("name,wrong", [("c21", "drop_image"), ("cth54", "drop_image"), ("c32", "swap_ncb"),
                                        ("cth108", "swap_ncb"), ("map70", "drop_image")])
def test_a_wrong_reference_falls_outside_the_bound(name, wrong):
    c = gc.BY_NAME[name]
    call = call_of(c)
    ref, sabs, Lrow, _ = ref_of(c)
    if wrong == "swap_ncb":
        assert any(b.lb != k.ld for b in c.bras for k in c.kets)
    else:
        assert any(k.flag for k in c.kets)
    bad, _, _, _ = hint_ref.ref_grad(call, blocks=hint_ref.grad_integrals(call), **{wrong: True})
    _, kg = gc.load_kappa()
    bound = kg[np.maximum(Lrow, 0)][:, None] * gc.U * sabs
    outside = ~(np.abs(bad - ref) <= bound)                      # a NaN (an AO outside the case's ranges) is outside
    factor = (np.abs(bad - ref)[bound > 0] / bound[bound > 0]).max()
    print(f"{name} {wrong}: {outside.sum()} of {outside.size} elements outside, {factor:.3e} x the bound")
    assert outside.any()
    if wrong == "drop_image":
        assert factor > 1e6


# --------------------------------------------------------------------------- the wrapper's launches
def test_wrapper_buckets_on_an_s_to_f_shell_set(hiplib):
    import grad_ref as R
    from xtddft_amd import qc
    from xtddft_amd.qc import grad as G
    S = qc.gto.Shell
    sh = [S(i % 3, l, R.CENTRES[i % 3].copy(), np.array([0.5 + 0.2 * i]), np.array([1.0])) for i, l in enumerate((0, 1, 2, 3, 0, 1))]
    tab = G.grad_tables(R.ShellMol(sh, 3))
    assert [r[2] for r in tab.bra_ranges] == [4, 6, 7] and [r[2] for r in tab.ket_ranges] == [2, 4, 6]
    assert tab.bra_ranges[0][0] == 0 and tab.bra_ranges[-1][1] == len(tab.bra.info)
    assert tab.ket_ranges[0][0] == 0 and tab.ket_ranges[-1][1] == len(tab.ket_info)
    buf, ibuf = np.zeros(8), np.zeros(8, dtype=np.int32)
    d, i = buf.ctypes.data, ibuf.ctypes.data
    seen = set()
    for b0, b1, lb in tab.bra_ranges:
        for k0, k1, lk in tab.ket_ranges:
            assert tab.bra.info[b0:b1, 0].max() == lb and tab.ket_info[k0:k1, 0].max() == lk
            inst = restated_instance(lb, lk)
            seen.add(inst)
            smaller = [x for x in gc.INSTANCES if x[0] < inst[0]]
            assert all(lb > mb or lb + lk > ml for ml, mb in smaller)          # no smaller instance holds the launch
            assert np.all(tab.bra.info[b0:b1, 0] + lk <= inst[0]) and np.all(tab.bra.info[b0:b1, 0] <= inst[1])
            # the wrapper's workspace is what the entry asks for: one double less is refused
            for strip in (G.default_strip(b1 - b0, k1 - k0), 2, 3, 1000):
                n = G.work_size(b1 - b0, k1 - k0, strip)
                assert n == 3 * (b1 - b0) * (-(-(k1 - k0) // strip) + 1)
                rc = hiplib.xt_grad_jk(b1 - b0, i, d, d, i, k1 - k0, i, d, d, i, lb, lk, 1, d, d, d, d, 1, strip, 3, d, n - 1,
                                       d, None)
                assert rc == -1 and b"workspace" in hiplib.xt_last_error()
    assert seen == set(gc.INSTANCES)
    assert G.default_strip(10, 10) == 1 and G.default_strip(7056, 3570) == 64 and G.default_strip(1000, 131) == 1
    assert G.default_strip(1024, 128) == 2
