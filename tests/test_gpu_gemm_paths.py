"""GPU: every planned path of the FP64 MFMA GEMM engine (xtddft_amd/csrc/xt_gemm.hip) through
xt_gemm_run, one case of tests/gemm_cases.py at a time.

Exact comparison: A and B hold integers in [-3, 3], C integers in [-8, 8], alpha in
{1, -2, 0.5}, beta in {0, 1, -0.5}.  Every partial sum of products, in any order and under
any split of the reduction, is an integer of magnitude <= 9 R K < 2^53, and alpha times it
plus beta C is a multiple of 1/2 far below 2^53: every intermediate of every evaluation order
is exactly representable, so the device result must equal a host float64 product bit for bit.
A single missing, doubled or misplaced term fails.  Integers this small are exact in lower
precision too, so Gaussian data against an np.longdouble reference and the derived bound of
gemm_cases.higham_bound check the arithmetic's width.

Isolation: the operands sit inside larger allocations (leading dimensions larger than the
extents, gaps between reduce slabs and batches); all slack of A and B is NaN, with beta == 0
C itself starts as NaN, and C's slack holds a sentinel that must come back bit-identical.
"""
import ctypes
import zlib

import numpy as np
import pytest

import gemm_cases as gc

pytestmark = pytest.mark.gpu

SENTINEL = -7777.25


@pytest.fixture(scope="module")
def torch(hiplib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def capi(hiplib):
    from xtddft_amd import _capi
    return _capi


def _integer_operands(c):
    rng = np.random.default_rng(zlib.crc32(c.name.encode()))
    sa, sb, sc = gc.logical_shapes(c)
    return (rng.integers(-3, 4, sa).astype(np.float64), rng.integers(-3, 4, sb).astype(np.float64),
            rng.integers(-8, 9, sc).astype(np.float64))


def _run(torch, hiplib, capi, c, a, b, cc, **over):
    """Pack the logical operands at the case's strides (NaN slack in A and B, NaN over C when
    beta == 0, the sentinel in C's slack), run xt_gemm_run, return (C values, flat C, offsets)."""
    fa, _ = gc.pack(c, "A", a, np.nan)
    fb, _ = gc.pack(c, "B", b, np.nan)
    c0 = cc if c.beta != 0.0 else np.full_like(cc, np.nan)
    fc, coff = gc.pack(c, "C", c0, SENTINEL)
    da, db, dc = (torch.from_numpy(x).cuda() for x in (fa, fb, fc))
    desc = gc.fill_desc(capi.XtGemmDesc(), c, **over)
    st = torch.cuda.current_stream().cuda_stream
    capi.check(hiplib.xt_gemm_run(ctypes.byref(desc), da.data_ptr(), db.data_ptr(), dc.data_ptr(),
                                  ctypes.c_void_p(st)), "xt_gemm_run")
    torch.cuda.synchronize()
    out = dc.cpu().numpy()
    # A and B are inputs: untouched
    assert torch.equal(da.cpu().view(torch.int64), torch.from_numpy(fa).view(torch.int64))
    assert torch.equal(db.cpu().view(torch.int64), torch.from_numpy(fb).view(torch.int64))
    return out[coff], out, coff


def _assert_slack_untouched(flat, coff):
    mask = np.ones(flat.size, dtype=bool)
    mask[coff.ravel()] = False
    assert np.array_equal(flat[mask].view(np.int64), np.full(int(mask.sum()), SENTINEL).view(np.int64)), \
        "a store landed outside C"


def _assert_exact(c, got, a, b, cc):
    """Bit-identical to the host float64 product, evaluated as the kernels' epilogue does:
    alpha times the sum (a sum that cancels is +0 on the device: the accumulators start at
    +0), then beta C added only when beta != 0."""
    assert 9 * c.r * c.k < 2 ** 53
    ref = c.alpha * (gc.host_product(a, b) + 0.0)
    if c.beta != 0.0:
        ref = ref + c.beta * cc
    ref = np.ascontiguousarray(np.broadcast_to(ref, got.shape))
    assert np.abs(ref).max() <= 2 * 9 * c.r * c.k + 8
    bad = got.view(np.int64) != ref.view(np.int64)
    assert not bad.any(), (int(bad.sum()), int((got != ref).sum()), np.argwhere(bad)[:5].tolist(),
                           got[bad][:5], ref[bad][:5])


@pytest.mark.parametrize("c", gc.CASES, ids=lambda c: c.name)
def test_every_planned_path_is_exact(torch, hiplib, capi, c):
    a, b, cc = _integer_operands(c)
    got, flat, coff = _run(torch, hiplib, capi, c, a, b, cc)
    _assert_exact(c, got, a, b, cc)
    _assert_slack_untouched(flat, coff)


@pytest.mark.parametrize("c", gc.gaussian_cases(), ids=lambda c: c.name)
def test_rounding_error_within_the_derived_bound(torch, hiplib, capi, c):
    """Gaussian data against np.longdouble, elementwise within gamma_n (|alpha| |A||B| +
    |beta| |C|), n = R K + 2, u = 2^-53 (gemm_cases.higham_bound; tests/test_gemm_plan.py shows
    a host float64 product inside the same bound and a dropped term outside it).  The split-K
    cases run twice: the slab reduction has a fixed order, so the bits repeat."""
    a, b, cc = gc.gaussian_operands(c)
    got, flat, coff = _run(torch, hiplib, capi, c, a, b, cc)
    _assert_slack_untouched(flat, coff)
    err = np.abs(got.astype(np.longdouble) - gc.reference_ld(c, a, b, cc))
    bound = gc.higham_bound(c, a, b, cc)
    ratio = float((err / bound).max())
    print(f"{c.name}: max error / bound = {ratio:.3e}")
    assert (err <= bound).all(), ratio
    if c.split:
        again, _, _ = _run(torch, hiplib, capi, c, a, b, cc)
        assert np.array_equal(got.view(np.int64), again.view(np.int64))


@pytest.mark.parametrize("slabs,extra,nsplit", [(3, 8, 3), (1, 0, 1)])
def test_workspace_fallback_is_exact(torch, hiplib, capi, slabs, extra, nsplit):
    """(256, 256, 4096) plans 32 splits; with a workspace of 3 slabs + 8 bytes dgemm() takes
    3, with a single slab none -- both exact."""
    c = gc.Case("ws", 256, 256, 4096, 1, "k", "n", 5, "whole", True, alpha=-2.0, beta=-0.5)
    ws = slabs * 8 * c.m * c.n + extra
    assert gc.plan(hiplib, gc.fill_desc(capi.XtGemmDesc(), c))["nsplit"] == 32
    assert gc.plan(hiplib, gc.fill_desc(capi.XtGemmDesc(), c, ws_bytes=ws))["nsplit"] == nsplit
    a, b, cc = _integer_operands(c)
    got, flat, coff = _run(torch, hiplib, capi, c, a, b, cc, ws_bytes=ws)
    _assert_exact(c, got, a, b, cc)
    _assert_slack_untouched(flat, coff)


def test_max_split_is_exact(torch, hiplib, capi):
    c = gc.Case("ms", 100, 40, 2001, 1, "m", "k", 2, "ragged_first", True, alpha=0.5, beta=1.0)
    assert gc.plan(hiplib, gc.fill_desc(capi.XtGemmDesc(), c, max_split=2))["nsplit"] == 2
    a, b, cc = _integer_operands(c)
    got, flat, coff = _run(torch, hiplib, capi, c, a, b, cc, max_split=2)
    _assert_exact(c, got, a, b, cc)
    _assert_slack_untouched(flat, coff)


@pytest.mark.parametrize("m,n,k", [(100, 40, 2001), (40, 100, 37)])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_xt_dgemm_padded_leading_dimensions(torch, hiplib, capi, m, n, k, ta, tb):
    """xt_dgemm on the Davidson project_out tiles (128 x 64 and 64 x 128) with lda, ldb, ldc
    larger than the stored rows: exact, NaN slack never read, C's slack untouched."""
    c = gc.Case("dgemm", m, n, k, 1, "m" if ta else "k", "k" if tb else "n", 2 if m > n else 3,
                "ragged_first", k > 1000, alpha=-2.0, beta=1.0)
    p = gc.plan(hiplib, gc.fill_desc(capi.XtGemmDesc(), c))
    assert p["cfg"] == c.cfg and (p["nsplit"] > 1) == c.split
    s, _ = gc.layout(c)
    a, b, cc = _integer_operands(c)
    fa, _ = gc.pack(c, "A", a, np.nan)
    fb, _ = gc.pack(c, "B", b, np.nan)
    fc, coff = gc.pack(c, "C", cc, SENTINEL)
    da, db, dc = (torch.from_numpy(x).cuda() for x in (fa, fb, fc))
    lda = s["sAk"] if ta else s["sAm"]
    ldb = s["sBn"] if tb else s["sBk"]
    st = torch.cuda.current_stream().cuda_stream
    capi.check(hiplib.xt_dgemm(ta, tb, m, n, k, c.alpha, da.data_ptr(), lda, db.data_ptr(), ldb, c.beta,
                               dc.data_ptr(), s["ldc"], ctypes.c_void_p(st)), "xt_dgemm")
    torch.cuda.synchronize()
    out = dc.cpu().numpy()
    _assert_exact(c, out[coff], a, b, cc)
    _assert_slack_untouched(out, coff)
