"""Device timing of the sTDA element generator (``xt_stda_select``, ``xt_stda_matrix``) on a
synthetic case sized like a real use of sX-TDA / sU-TDA.

    python tools/stda_bench.py [--natm 60] [--nocc 150] [--nvir 600] [--np-side 32] [--nmat 8192]
                               [--warmup 1] [--reps 3] [--out profiles/stda_bench.json]

natm atoms with 15 AOs each; active space (nocc, nocc - 1) occupied x (nvir, nvir + 1) virtual;
P = the (np_side x np_side) frontier block of every spin (about 2 000 CSFs), N = every other CSF
(a few 10^5), both in the driver's class order; the A matrix is built for the first nmat CSFs of
P followed by N.  Operands are random and come from ``xt_stda_charges`` / ``xt_stda_half``, which
are timed too.  HIP events around each whole call (list upload and final synchronise included).

Next to the milliseconds the JSON carries a model of what each call moves:
  flops            2 natm per pair (line 1, on the FP64 MFMA) + 2 natm per same-spin pair (line 2)
  bytes_requested  what the lanes load: per 16 x 16 tile 32 natm-vectors for line 1, per
                   same-spin pair two natm-vectors for line 2 (mostly cache hits: the operand
                   arrays are far smaller)
  bytes_compulsory operands once + lists + output
and the fractions of the roofs they bear on: FP64 peak 78.6 TFLOP/s, HBM 8 TB/s for the compulsory
bytes, and the L2's about 34.5 TB/s for the requested bytes, which is the one the kernel leans on.
There is no earlier time to compare with: the number is recorded, not gated.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_PEAK, HBM_PEAK, L2_PEAK = 78.6e12, 8.0e12, 34.5e12


def class_order(nc, no, nv, pmask_a, pmask_b, want_p):
    """(spin, i, a) of the CSFs inside (want_p) or outside the frontier masks, CV(aa) | OV(aa) |
    CO(bb) | CV(bb), each row-major."""
    out = []
    ia, aa = np.where(pmask_a == want_p)
    for sel in (ia < nc, ia >= nc):
        out.append(np.stack([np.zeros(sel.sum(), np.int64), ia[sel], aa[sel]], axis=1))
    ib, ab = np.where(pmask_b == want_p)
    for sel in (ab < no, ab >= no):
        out.append(np.stack([np.ones(sel.sum(), np.int64), ib[sel], ab[sel]], axis=1))
    return np.ascontiguousarray(np.concatenate(out), dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--natm", type=int, default=60)
    ap.add_argument("--nocc", type=int, default=150)
    ap.add_argument("--nvir", type=int, default=600)
    ap.add_argument("--np-side", type=int, default=32)
    ap.add_argument("--nmat", type=int, default=8192)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from xtddft_amd import _capi, build
    build.build()
    L = _capi.lib()
    if not torch.cuda.is_available():
        raise SystemExit("stda_bench needs the GPU: a timing taken elsewhere says nothing")
    natm, no = a.natm, 1
    nc, nv = a.nocc - no, a.nvir
    nocc, nvir = (nc + no, nc), (nv, no + nv)
    nmo, nao = nc + no + nv, 15 * natm
    g = torch.Generator(device="cuda").manual_seed(0)
    rand = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=g)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    desc = _capi.XtStdaDesc(natm=natm, nocc_a=nocc[0], nvir_a=nvir[0], nocc_b=nocc[1], nvir_b=nvir[1], nc=nc, no=no,
                            nv=nv, spin_adapted=1, si=0.5, correct=0, delta_max=0.0, sigma_k=0.0)
    off = np.ascontiguousarray(np.arange(natm + 1) * 15, dtype=np.int32)
    ip = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    xyz = rand(natm, 3) * 6.0
    gam = (1.0 / (torch.cdist(xyz, xyz) ** 1.5 + 0.3 ** -1.5)) ** (1 / 1.5)
    ops, keep = _capi.XtStdaOps(), []

    def timed(f, reps):
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms
    setup_ms = {"xt_stda_charges": 0.0, "xt_stda_half": 0.0}
    for s, tag in enumerate("ab"):
        o, v = nocc[s], nvir[s]
        t = dict(cp=rand(nao, nmo) / np.sqrt(15.0), q_oo=rand(o * o * natm), q_ov=rand(o * v * natm),
                 q_vv=rand(v * v * natm), k_ov=rand(o * v * natm), j_vv=rand(v * v * natm))
        for name, n in (("f_oo", o), ("f_vv", v), ("h_oo", o), ("h_vv", v)):
            m = rand(n, n)
            t[name] = (m + m.T).contiguous()
        setup_ms["xt_stda_charges"] += timed(lambda: _capi.check(L.xt_stda_charges(
            ctypes.byref(desc), s, nao, ip(off), t["cp"].data_ptr(), t["q_oo"].data_ptr(), t["q_ov"].data_ptr(),
            t["q_vv"].data_ptr(), st), "xt_stda_charges"), 1)[0]
        setup_ms["xt_stda_half"] += timed(lambda: _capi.check(L.xt_stda_half(
            ctypes.byref(desc), s, gam.data_ptr(), gam.data_ptr(), t["q_ov"].data_ptr(), t["q_vv"].data_ptr(),
            t["k_ov"].data_ptr(), t["j_vv"].data_ptr(), st), "xt_stda_half"), 1)[0]
        for name in _capi.STDA_OPS:
            setattr(ops, f"{name}_{tag}", t[name].data_ptr())
        keep.append(t)

    # frontier masks: the highest np_side occupied x the lowest np_side virtual orbitals of each spin
    k = a.np_side
    pm_a = np.zeros((nocc[0], nvir[0]), bool)
    pm_a[nocc[0] - k:, :k] = True
    pm_b = np.zeros((nocc[1], nvir[1]), bool)
    pm_b[nocc[1] - k:, :k] = True
    csf_p = class_order(nc, no, nv, pm_a, pm_b, True)
    csf_n = class_order(nc, no, nv, pm_a, pm_b, False)
    n_p, n_n = len(csf_p), len(csf_n)
    csf_m = np.ascontiguousarray(np.concatenate([csf_p, csf_n])[:a.nmat])
    n_m = len(csf_m)
    rng = np.random.default_rng(0)
    e_p = torch.from_numpy(rng.uniform(0.1, 0.3, n_p)).cuda()
    e_n = torch.from_numpy(rng.uniform(0.35, 1.5, n_n)).cuda()
    w = torch.empty(n_n, dtype=torch.float64, device="cuda")
    amat = torch.empty(n_m, n_m, dtype=torch.float64, device="cuda")

    def select():
        _capi.check(L.xt_stda_select(ctypes.byref(desc), ctypes.byref(ops), n_p, ip(csf_p), e_p.data_ptr(), n_n,
                                     ip(csf_n), e_n.data_ptr(), w.data_ptr(), st), "xt_stda_select")

    def matrix():
        _capi.check(L.xt_stda_matrix(ctypes.byref(desc), ctypes.byref(ops), n_m, ip(csf_m), amat.data_ptr(), st),
                    "xt_stda_matrix")

    def model(rows, cols, out_doubles):
        pairs = float(len(rows)) * len(cols)
        same = sum(float((rows[:, 0] == s).sum()) * float((cols[:, 0] == s).sum()) for s in (0, 1))
        tiles = np.ceil(len(rows) / 16) * np.ceil(len(cols) / 16)
        operands = sum(8.0 * natm * (2 * nocc[s] * nvir[s] + nocc[s] ** 2 + nvir[s] ** 2) for s in (0, 1))
        return dict(pairs=pairs, same_spin_pairs=same, flops=2.0 * natm * (pairs + same),
                    bytes_requested=8.0 * natm * (32 * tiles + 2 * same),
                    bytes_compulsory=operands + 12.0 * (len(rows) + len(cols)) + 8.0 * out_doubles)
    res = dict(what="xt_stda_select / xt_stda_matrix: one call each, HIP events around it", natm=natm, nocc=nocc,
               nvir=nvir, n_p=n_p, n_n=n_n, n_matrix=n_m, setup_ms=setup_ms, warmup=a.warmup, reps=a.reps,
               device=torch.cuda.get_device_name(0),
               roofs=dict(fp64_flops=FP64_PEAK, hbm_bytes=HBM_PEAK, l2_bytes=L2_PEAK))
    for name, f, out, m in (("xt_stda_select", select, w, model(csf_p, csf_n, n_n)),
                            ("xt_stda_matrix", matrix, amat, model(csf_m, csf_m, n_m * n_m))):
        timed(f, a.warmup)
        first = out.clone()
        ms = timed(f, a.reps)
        t = float(np.median(ms)) * 1e-3
        m.update(ms_median=float(np.median(ms)), ms_all=[round(x, 3) for x in ms],
                 bit_identical_over_calls=bool(torch.equal(first, out)), finite=bool(torch.isfinite(out).all()),
                 tflops=m["flops"] / t / 1e12, frac_fp64_peak=m["flops"] / t / FP64_PEAK,
                 requested_tb_per_s=m["bytes_requested"] / t / 1e12, frac_l2_roof=m["bytes_requested"] / t / L2_PEAK,
                 frac_hbm_roof_compulsory=m["bytes_compulsory"] / t / HBM_PEAK)
        res[name] = m
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
