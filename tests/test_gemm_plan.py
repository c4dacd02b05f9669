"""CPU: the GEMM engine's planner through xt_gemm_plan (host only, no HIP call) -- every
case of tests/gemm_cases.py takes the path it claims, the table is closed over the paths
the engine can launch, no planned split-K range is empty, and the rounding bound the GPU
test uses holds for a host float64 product of the same data."""
import ctypes

import numpy as np
import pytest

import gemm_cases as gc


@pytest.fixture(scope="module")
def capi(hiplib):
    from xtddft_amd import _capi
    return _capi


def _plan(hiplib, capi, c, **over):
    return gc.plan(hiplib, gc.fill_desc(capi.XtGemmDesc(), c, **over))


@pytest.mark.parametrize("c", gc.CASES + gc.gaussian_cases(), ids=lambda c: c.name)
def test_case_takes_the_path_it_claims(hiplib, capi, c):
    p = _plan(hiplib, capi, c)
    assert (p["bm"], p["bn"], p["bk"]) == gc.CFG_TILE[p["cfg"]]
    assert p["cfg"] == c.cfg, p
    ragged_k = c.k % p["bk"] != 0
    staging = "whole" if not ragged_k else "ragged_first" if c.r == 1 else "masked"
    assert staging == c.staging
    assert p["masked"] == (1 if staging == "masked" else 0)
    assert (p["nsplit"] > 1) == c.split, p
    if c.split:
        assert p["nsplit"] <= 64 and (p["nsplit"] >= 7 or c.name.startswith("gauss"))
        units = c.r * -(-c.k // p["bk"])
        assert (p["nsplit"] - 1) * -(-units // p["nsplit"]) < units


def test_case_table_is_closed():
    """A planner change that drops a path makes a case above fail; a table edit that drops
    one fails here."""
    have = {(c.cfg, c.la, c.lb, c.staging, c.split, c.rdiv > 0) for c in gc.CASES}
    missing = gc.required_paths() - have
    assert not missing, sorted(missing)
    plain = [c for c in gc.CASES if not c.rdiv and not c.tag and c.nb1 * c.nb2 == 1]
    for cfg in gc.CFG_TILE:
        tiles = {c.tiles for c in plain if c.cfg == cfg}
        assert "ragged" in tiles, cfg
        # the planner takes cfg 8 only for a ragged column edge: full in M is all it can be
        if cfg == 8:
            assert any(c.cfg == 8 and c.m % 128 == 0 for c in plain)
        else:
            assert "full" in tiles, cfg
    for cfg in (2, 5, 8, 9):
        assert any(c.tall for c in plain if c.cfg == cfg), cfg
    # both staging paths of the tile walk's partial last group run split and unsplit somewhere
    assert {c.split for c in plain if c.tall} == {False, True}
    # a two-level batch with distinct strides and one broadcast stride
    two = [c for c in gc.CASES if c.nb1 > 1 and c.nb2 > 1]
    assert two and all(c.bcast for c in two)
    for c in two:
        s, _ = gc.layout(c)
        strides = [s[k] for k in ("sAb1", "sAb2", "sBb1", "sBb2", "sCb1", "sCb2")]
        assert sorted(strides).count(0) == 1 and len(set(strides)) == 6
    assert any(c.tag == 1 and c.m < 96 <= c.n and c.cfg == 5 for c in gc.CASES)
    assert any(c.tag == 3 and c.n == 147 and c.cfg == 4 for c in gc.CASES)
    # every alpha and beta of the exact comparison is used, beta == 0 on every configuration
    assert {c.alpha for c in gc.CASES} == set(gc.ALPHAS) and {c.beta for c in gc.CASES} == set(gc.BETAS)
    for cfg in gc.CFG_TILE:
        assert {c.beta for c in gc.CASES if c.cfg == cfg} == set(gc.BETAS), cfg
    assert len({c.name for c in gc.CASES}) == len(gc.CASES)


def test_cfg8_needs_a_ragged_column_edge(hiplib, capi):
    """Why the table has no all-full-tiles case on cfg 8: with full column tiles the planner
    keeps cfg 5, whatever the row edge."""
    for m, n in ((128, 128), (256, 256), (97, 256), (1153, 128)):
        c = gc.Case("probe", m, n, 64, 1, "k", "n", 5, "whole", False)
        assert _plan(hiplib, capi, c)["cfg"] == 5, (m, n)


def test_workspace_cap_takes_fewer_splits(hiplib, capi):
    """(256, 256, 4096) plans 32 splits; a workspace of 3 slabs + 8 bytes takes 3, one of a
    single slab none (dgemm()'s fallback); max_split caps the count."""
    c = gc.Case("ws", 256, 256, 4096, 1, "k", "n", 5, "whole", True)
    slab = 8 * 256 * 256
    assert _plan(hiplib, capi, c)["nsplit"] == 32
    assert _plan(hiplib, capi, c, ws_bytes=3 * slab + 8)["nsplit"] == 3
    assert _plan(hiplib, capi, c, ws_bytes=slab)["nsplit"] == 1
    assert _plan(hiplib, capi, c, ws_bytes=32 * slab)["nsplit"] == 32
    assert _plan(hiplib, capi, c, max_split=5)["nsplit"] == 5


def test_plan_edge_sizes(hiplib, capi):
    c = gc.Case("k0", 100, 40, 0, 1, "k", "n", 2, "whole", False)
    assert _plan(hiplib, capi, c) == dict(cfg=2, bm=128, bn=64, bk=32, nsplit=1, masked=0)
    c = gc.Case("m0", 0, 40, 64, 1, "k", "n", 2, "whole", False)
    assert _plan(hiplib, capi, c) == dict(cfg=-1, bm=0, bn=0, bk=0, nsplit=0, masked=0)


def _sweep_rows(hiplib, capi, la, lb, m):
    """One (layout, M) slice of the sweep below; returns the violations."""
    desc = capi.XtGemmDesc()
    out = [ctypes.c_int() for _ in range(6)]
    refs = [ctypes.byref(o) for o in out]
    dref = ctypes.byref(desc)
    fn = hiplib.xt_gemm_plan
    bad = []
    for n in range(1, 301, 7):
        # fill_desc's strides depend on k only through the padded leading dimensions; the
        # planner reads which stride is 1, not their size
        gc.fill_desc(desc, gc.Case("sweep", m, n, 1, 1, la, lb, 4, "whole", False))
        for r in (1, 3):
            desc.r = r
            for k in range(1, 6001, 13):
                desc.k = k
                if fn(dref, *refs) != 0:
                    bad.append((m, n, k, r, la, lb, "rejected"))
                    continue
                ns = out[4].value
                if ns == 1:
                    continue
                bm, bn, bk = out[1].value, out[2].value, out[3].value
                units = r * -(-k // bk)
                tiles = -(-m // bm) * -(-n // bn)
                if not (ns > 1 and (ns - 1) * -(-units // ns) < units and units // ns >= 8 and tiles * ns <= 32768):
                    bad.append((m, n, k, r, la, lb, ns))
    return bad


def test_no_planned_split_range_is_empty(hiplib, capi):
    """Sweep M, N in {1..300 step 7}, K in {1..6000 step 13}, R in {1, 3} and the four
    layouts: a planned split count leaves no split without K tiles ((nsplit - 1)
    ceil(units / nsplit) < units), keeps >= 8 tile units per split and <= 32768 blocks.
    (6.8 million plans; the planner's list-scheduling model runs once per distinct shape,
    outside the interpreter lock, so the slices run on a few threads.)"""
    import os
    from concurrent.futures import ThreadPoolExecutor
    jobs = [(la, lb, m) for la, lb in gc.LAYOUTS for m in range(1, 301, 7)]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        bad = [v for res in ex.map(lambda j: _sweep_rows(hiplib, capi, *j), jobs) for v in res]
    assert not bad, bad[:20]


@pytest.mark.parametrize("c", gc.gaussian_cases(), ids=lambda c: c.name)
def test_rounding_bound_holds_for_a_host_float64_product(c):
    """The bound of the GPU rounding test is derived (Higham, gamma_n with n = R K + 2), not
    measured: a plain float64 host product of the same data stays inside it."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble must be wider than float64"
    a, b, cc = gc.gaussian_operands(c)
    got = c.alpha * gc.host_product(a, b) + c.beta * np.broadcast_to(cc, (c.nb1, c.nb2, c.m, c.n))
    err = np.abs(got.astype(np.longdouble) - gc.reference_ld(c, a, b, cc))
    bound = gc.higham_bound(c, a, b, cc)
    assert (err <= bound).all(), float((err / bound).max())
    # the bound is tight enough to mean something: a single dropped term breaks it
    a2 = a.copy()
    a2[0, 0, 0, 0, 0] = 0.0
    got2 = c.alpha * gc.host_product(a2, b) + c.beta * cc
    err2 = np.abs(got2.astype(np.longdouble) - gc.reference_ld(c, a, b, cc))
    assert (err2 > bound).any()


def test_gaussian_cases_cover_every_cfg_split_and_unsplit():
    assert {(c.cfg, c.split) for c in gc.gaussian_cases()} == {(cfg, s) for cfg in gc.CFG_TILE for s in (False, True)}
