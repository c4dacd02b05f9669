"""Host: the case table of the integral kernel (tests/int_cases.py) and its fixture
(tests/golden/int_ref*.npz, written by tests/golden/make_int_ref.py).

* every case runs what it claims -- the dispatch conditions of xt_int.hip (int2e_cart's two
  buckets, k_int_cart's switch, boys_all's T < 30) are restated here and applied to the built
  tables -- and reads and writes inside its arrays;
* the table is closed: all 22 register instances, the runtime path of both buckets, every Boys
  regime, every class (lab, lc), the range-separation limits, point charges, both thread-mapping
  cases;
* the fixture is current: a fixed subset is regenerated with mpmath and equals the file;
* the host routine (the formula of ints.eri_quartet / eri3c) meets the elementwise bound
  |host - ref| <= kappa(L) 2^-53 sabs on every case, and kappa(L) is 8 x the host's measured
  error with a floor of 64; the same for Mole.eval_ao and its constant c.
"""
import os

import numpy as np
import pytest

import int_cases as ic
import int_ref

CASE_IDS = [c.name for c in ic.CASES]


@pytest.fixture(scope="module")
def fixture():
    return ic.load_fixture()


@pytest.fixture(scope="module")
def tables():
    return {c.name: ic.build(c) for c in ic.CASES}


# --------------------------------------------------------------------------- the dispatch, restated
def dispatch_bucket(lmax_orb, lket):
    """int2e_cart: (MAXL, MAXLAB) of the kernel it launches, None for XT_ERR_ARG."""
    if 2 * lmax_orb <= 4 and 2 * lmax_orb + lket <= 8:
        return 8
    if 2 * lmax_orb <= 6 and 2 * lmax_orb + lket <= 13:
        return 13
    return None


def dispatch_path(lab, lc):
    """k_int_cart: the switch over 5 lab + lc behind L <= 6, lab <= 4, lc <= 4."""
    if lab + lc <= 6 and lab <= 4 and lc <= 4:
        return f"reg:{lab},{lc}"
    return "rt"


def test_register_set_is_the_switch():
    want = {(a, c) for a in range(5) for c in range(5) if a + c <= 6}
    assert ic.REGISTER == want and len(want) == 22


@pytest.mark.parametrize("name", CASE_IDS)
def test_case_runs_what_it_claims(tables, name):
    c, tb = ic.BY_NAME[name], tables[name]
    # the declared bounds cover every table entry (below them the kernel's private arrays overrun)
    assert tb.pinfo[:, :2].max() <= c.lmax_orb <= 3
    assert tb.kinfo[:, 0].max() <= c.lket and 2 * c.lmax_orb + c.lket <= 13
    assert dispatch_bucket(c.lmax_orb, c.lket) == c.bucket
    assert {dispatch_path(lab, lc) for *_, lab, lc in tb.blocks} == set(c.paths)
    T = ic.quartet_T(tb)
    assert {"table" if t < 30.0 else "erf" for t in T} == set(c.boys)
    if c.regime:
        assert len(T) == 1 and ic.REGIMES[c.regime][1](T[0]), T
    # the shape of a case
    assert 1 <= len(c.kets) <= 3 and (1 <= len(c.bras) <= 4 or name == "map67")
    assert tb.kinfo[:, 5].max() <= 6 and tb.pinfo[:, 2].max() <= 9 and tb.kinfo[:, 1].max() <= 9


@pytest.mark.parametrize("name", CASE_IDS)
def test_case_stays_inside_its_arrays(tables, name):
    tb = tables[name]
    seen = np.zeros((tb.nrow, tb.ldo), dtype=int)
    for k, j, row0, nab, col0, nc, lab, lc in tb.blocks:
        la, lb, npp, pq0, pe0, r0 = (int(x) for x in tb.pinfo[k][:6])
        lcc, nr, ar0, ae0, c0, ncc = (int(x) for x in tb.kinfo[j][:6])
        assert (la + lb, lcc, r0, c0, ncc) == (lab, lc, row0, col0, nc)
        assert nab == ic.ncart(la) * ic.ncart(lb)
        assert 0 <= pq0 and pq0 + npp <= len(tb.pprim) and 0 <= ar0 and ar0 + nr <= len(tb.kprim)
        assert 0 <= pe0 and pe0 + nab * ic.ntuv(lab) * npp <= tb.eab.size
        assert 0 <= ae0 and ae0 + nc * ic.ntuv(lc) * nr <= tb.ek.size
        assert 0 <= row0 and row0 + nab <= tb.nrow and 0 <= col0 and col0 + nc <= tb.ldo
        seen[row0:row0 + nab, col0:col0 + nc] += 1
    assert seen.max() == 1                       # blocks do not overlap
    assert len(tb.blocks) == len(tb.pinfo) * len(tb.kinfo)
    for a in (tb.pprim, tb.eab, tb.kprim, tb.ek):
        assert a.dtype == np.float64 and np.all(np.isfinite(a))


# --------------------------------------------------------------------------- closure
def test_table_is_closed(tables):
    claimed = {(p, c.bucket) for c in ic.CASES for p in c.paths}
    for lab, lc in ic.REGISTER:
        assert any(p == f"reg:{lab},{lc}" for p, _ in claimed), (lab, lc)
    assert ("rt", 8) in claimed and ("rt", 13) in claimed
    assert {c.regime for c in ic.CASES if c.regime} == set(ic.REGIMES)
    assert {b for c in ic.CASES for b in c.boys} == {"table", "erf"}
    # every class the kernel can be asked for, with an auxiliary ket; a pair ket for every lc <= 6
    aux = {(b[0] + b[1], k[1]) for c in ic.CASES for b in c.bras for k in c.kets if k[0] == "aux"}
    want = {(lab, lc) for lab in range(7) for lc in range(8) if lab + lc <= 13}
    assert want == set(ic.CLASSES) and want <= aux
    pair = {(b[0] + b[1], k[1] + k[2]) for c in ic.CASES for b in c.bras for k in c.kets if k[0] == "pair"}
    assert {(lab, lc) for lab in range(7) for lc in range(7)} <= pair
    # at least two splits (la, lb) at lab = 2, 3, 4; la, lb <= 3 throughout
    splits = {}
    for c in ic.CASES:
        for la, lb, *_ in c.bras:
            assert la <= 3 and lb <= 3
            splits.setdefault(la + lb, set()).add((la, lb))
    assert all(len(splits[lab]) >= 2 for lab in (2, 3, 4)) and set(splits) == set(range(7))


def test_bucket_twins(tables):
    """Every class whose shells fit k_int_cart<8, 4> appears with its true bounds and declared
    with lmax_orb = 3, on the same tables."""
    twins = [c for c in ic.CASES if c.twin]
    fit = {(lab, lc) for lab, lc in ic.CLASSES
           if any(dispatch_bucket(max(s), lc) == 8 for s in ic.SPLITS[lab])}
    assert {c.klass for c in twins} == fit and len(fit) >= 20
    for c in twins:
        t = ic.BY_NAME[c.twin]
        assert (c.bucket, t.bucket, t.lmax_orb, t.ref_of) == (8, 13, 3, c.name)
        a, b = tables[c.name], tables[t.name]
        for x in ("pinfo", "pprim", "eab", "kinfo", "kprim", "ek"):
            assert np.array_equal(getattr(a, x), getattr(b, x))


def test_regime_omega_charge_and_mapping_cases(tables):
    reg = {}
    for c in ic.CASES:
        if c.regime:
            reg.setdefault(c.name.split("_")[0], set()).add(c.regime)
    assert len(reg) >= 6 and all(v == set(ic.REGIMES) for v in reg.values())
    firsts = {tag: ic.BY_NAME[tag + "_mid"] for tag in reg}
    kinds = [(c.klass, c.paths, c.bucket) for c in firsts.values()]
    assert ((0, 0), frozenset(["reg:0,0"]), 8) in kinds
    assert sum(1 for _, p, _ in kinds if next(iter(p)).startswith("reg")) >= 2
    assert any(p == frozenset(["rt"]) and b == 8 for _, p, b in kinds)
    assert any(p == frozenset(["rt"]) and b == 13 and k[0] + k[1] < 12 for k, p, b in kinds)
    assert any(k == (6, 7) for k, _, _ in kinds) and any(k == (6, 6) for k, _, _ in kinds)
    assert firsts["r66"].kets[0][0] == "pair"
    # omega: 0 everywhere else, 0.33 and the two limits on four classes
    om = {}
    for c in ic.CASES:
        if c.omega:
            om.setdefault(c.klass, set()).add(c.omega)
    assert len(om) == 4 and all(v == {0.33, 1e-3, 1e3} for v in om.values())
    # point charges: exponent POINT_CHARGE_EXP, coefficient -Z (s / pi)^1.5, lab = 0, 2, 4, 5, 6
    labs = set()
    for c in ic.CASES:
        if c.kets[0][0] == "pc":
            tb = tables[c.name]
            labs.add(c.klass[0])
            assert np.all(tb.kprim[:, 0] == ic.POINT_CHARGE_EXP) and np.all(tb.kinfo[:, 0] == 0)
            z = np.array([k[1] for k in c.kets])
            assert np.array_equal(tb.ek, -z * (ic.POINT_CHARGE_EXP / np.pi) ** 1.5)
    assert labs == {0, 2, 4, 5, 6}
    # 67 threads: one full wave and three lanes, register and runtime quartets in the first wave
    tb = tables["map67"]
    assert len(tb.pinfo) * len(tb.kinfo) == 67
    first_wave = {dispatch_path(lab, lc) for k, j, *_, lab, lc in tb.blocks if j * len(tb.pinfo) + k < 64}
    assert "rt" in first_wave and len(first_wave) >= 4
    # a block inside a larger output
    tb = tables["ldo_pad"]
    m = tb.mask()
    assert not m[:2].any() and not m[-3:].any() and not m[:, :3].any() and not m[:, -4:].any() and m.any()


# --------------------------------------------------------------------------- the fixture
def test_fixture_files_are_small_and_complete(fixture):
    files = ic.fixture_files()
    assert files and all(os.path.getsize(f) <= ic.FIXTURE_MAX_BYTES for f in files)
    for c in ic.REF_CASES:
        tb = ic.build(c)
        for part in ("ref", "sabs", "host"):
            a = fixture[f"{c.name}/{part}"]
            assert a.shape == (tb.nrow, tb.ldo) and a.dtype == np.float64
    assert set(fixture) == {f"{c.name}/{p}" for c in ic.REF_CASES for p in ("ref", "sabs", "host")} | \
        {"host_units", "kappa", "ao_host_units", "ao_c"}


@pytest.mark.parametrize("name", ic.REGEN)
def test_fixture_is_current(fixture, tables, name):
    """The committed reference is what tests/int_ref.py computes today, bit for bit."""
    pytest.importorskip("mpmath")
    tb = tables[name]
    ref, sabs, _ = int_ref.ref_int2e(tb.pinfo, tb.pprim, tb.eab, tb.kinfo, tb.kprim, tb.ek, tb.omega,
                                     tb.nrow, tb.ldo)
    assert np.array_equal(ref, fixture[name + "/ref"])
    assert np.array_equal(sabs, fixture[name + "/sabs"])
    assert np.array_equal(ic.host_int2e(tb), fixture[name + "/host"])


def test_regen_subset():
    assert 35 <= len(ic.REGEN) <= 50 and all(n in ic.BY_NAME and not ic.BY_NAME[n].ref_of for n in ic.REGEN)


# --------------------------------------------------------------------------- the bound and the host
def _lmap(tb):
    L = np.full((tb.nrow, tb.ldo), -1, dtype=np.int64)
    for _, _, r0, nab, c0, nc, lab, lc in tb.blocks:
        L[r0:r0 + nab, c0:c0 + nc] = lab + lc
    return L


def test_kappa_is_measured_from_the_host(fixture, tables):
    measured = np.zeros(ic.L_MAX + 1)
    for c in ic.REF_CASES:
        f = {p: fixture[f"{c.name}/{p}"] for p in ("ref", "sabs", "host")}
        measured = np.maximum(measured, ic.measured_ratio(f["host"], f["ref"], f["sabs"], _lmap(tables[c.name])))
    assert np.all(measured > 0)                              # every total order 0..13 is measured
    assert np.array_equal(measured, fixture["host_units"])
    assert np.array_equal(fixture["kappa"], np.maximum(64.0, 8.0 * measured))


@pytest.mark.parametrize("name", [c.name for c in ic.REF_CASES])
def test_host_routine_meets_the_bound(fixture, tables, name):
    """|host - ref| <= kappa(L) 2^-53 sabs elementwise, with the host recomputed here (its bits
    may differ from the fixture's between machines; the bound holds for both); untouched
    output stays zero; and the reference is not vacuous."""
    tb = tables[name]
    ref, sabs = fixture[name + "/ref"], fixture[name + "/sabs"]
    L, m = _lmap(tb), tb.mask()
    kap = np.where(m, fixture["kappa"][np.maximum(L, 0)], 0.0)
    for host in (ic.host_int2e(tb), fixture[name + "/host"]):
        assert np.all(np.abs(host - ref) <= kap * ic.U * sabs)
        assert np.all(host[~m] == 0.0)
    assert np.all(ref[~m] == 0.0) and np.all(sabs[~m] == 0.0)
    assert np.all(np.abs(ref) <= sabs)
    c = ic.BY_NAME[name]
    if c.regime == "zero" and sum(c.klass) % 2:       # a one-centre integral of odd parity: exact zeros
        assert not ref.any() and not sabs.any()
    else:
        assert np.count_nonzero(ref[m]) >= 0.2 * m.sum()


def test_host_formula_is_the_library_routine():
    """int_cases.host_int2e on whole shells gives what ints.eri3c and ints.eri_quartet give."""
    from xtddft_amd.qc import ints
    rng = np.random.default_rng(5)
    sh = [ic._shell(rng, l, n, rng.uniform(-1, 1, 3)) for l, n in ((2, 2), (1, 3), (3, 1), (2, 2), (1, 1))]
    bra, aux, ket = ints.ShellPair(sh[0], sh[1]), ints.AuxShellSet([sh[2]]), ints.ShellPair(sh[3], sh[4])
    pinfo = np.array([[2, 1, bra.p.size, 0, 0, 0, 0, 0]], dtype=np.int32)
    kinfo = np.array([[3, 1, 0, 0, 0, 10, 0, 0], [3, ket.p.size, 1, aux.Ek.size, 10, 18, 0, 0]], dtype=np.int32)
    tb = ic.Tables(pinfo, np.column_stack([bra.p, bra.P]), bra.Eab.ravel(), kinfo,
                   np.concatenate([np.column_stack([aux.p, aux.P]), np.column_stack([ket.p, ket.P])]),
                   np.concatenate([aux.Ek.ravel(), ket.Eab.ravel()]), 18, 28, 0.33, 2, 3,
                   [(0, 0, 0, 18, 0, 10, 3, 3), (0, 1, 0, 18, 10, 18, 3, 3)])
    out = ic.host_int2e(tb)
    a = ints.eri3c(bra, aux, omega=0.33).reshape(18, 10)
    b = ints.eri_quartet(bra, ket, omega=0.33).reshape(18, 18)
    assert np.abs(out[:, :10] - a).max() <= 1e-14 * np.abs(a).max()
    assert np.abs(out[:, 10:] - b).max() <= 1e-14 * np.abs(b).max()


# --------------------------------------------------------------------------- xt_eval_ao
def test_host_eval_ao_meets_the_bound(fixture):
    """Mole.eval_ao (s to g) against the long double reference within c 2^-53 sabs; c is 8 x the
    host's measured error, floor 16; exact zeros where every exponential underflows."""
    from xtddft_amd.qc.dints import _sph_table, ao_shell_tables
    mol = ic.ao_mol()
    coords, far = ic.ao_points()
    info, dat = ao_shell_tables(mol)
    assert sorted(set(info[:, 0])) == [0, 1, 2, 3, 4] and set(info[:, 1]) == {1, 3}
    assert (coords.shape[0] * len(info)) % 256 != 0
    ref, sabs, amp = int_ref.ref_eval_ao(coords, info, dat, _sph_table(), mol._norm, mol.nao)
    host = mol.eval_ao(coords, deriv=1)
    c = float(fixture["ao_c"])
    assert c == max(16.0, 8.0 * float(fixture["ao_host_units"]))
    assert np.all(np.abs(host.astype(int_ref.LD) - ref) <= int_ref.ao_bound(c, sabs, amp))
    assert np.all(host[:, far] == 0.0)
    # the p gradient at its own centre is the radial part: nonzero, and the reference has it
    ctr = 0
    p_aos = slice(1, 4)
    assert np.all(np.abs(np.diagonal(ref[1:, ctr, p_aos])) > 0.1)
    assert np.all(ref[0, ctr, p_aos] == 0)
