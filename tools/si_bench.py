"""Device timing of the state-interaction couplings (``xt_si_couple``, both modes) at a
porphyrin-like shape, next to the per-pair cost of the loop-written restatement.

    python tools/si_bench.py [--nc 119] [--no 2] [--nv 285] [--nstates 40] [--warmup 1] [--reps 3]
                             [--pairs 6] [--out profiles/si_bench.json]

nstates seeded random orthonormal vectors per manifold (|S->, |So>, |S+>), a seeded antisymmetric
``Vso`` and a symmetric dipole-like operator, all resident on the device; HIP events around each
whole call (allocation of the call's workspace and the final synchronise included).  The
restatement (tests/si_ref.py, the reference's way: one image per right-hand state, one
contraction per pair) is timed on ``--pairs`` pairs of |So> states per mode and scaled to all
n^2 pairs of the device call.  The flop model counts the engine GEMMs only: per right-hand state
and component 2 rows cols k per term, and 2 n_L n_R dim per Gram product.
There is no earlier time to compare with: the numbers are recorded, not gated.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FP64_PEAK = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nc", type=int, default=119)
    ap.add_argument("--no", type=int, default=2)
    ap.add_argument("--nv", type=int, default=285)
    ap.add_argument("--nstates", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import si_ref as ref
    from xtddft_amd import _capi, build
    build.build()
    L = _capi.lib()
    nc, no, nv, n = a.nc, a.no, a.nv, a.nstates
    s = no / 2
    counts = (n if s >= 1 else 0, n, n)
    vso, dip, states = ref.random_problem(nc, no, nv, counts, seed=0)
    xs = [ref.rows_of(states, k, d) for k, d in zip(('|S->', '|So>', '|S+>'), ref.dims(nc, no, nv))]
    ntot = sum(counts) + 1
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in
           dict(vso=vso, dip=dip, sm=xs[0], so=xs[1], sp=xs[2]).items()}
    out = torch.empty((3, ntot, ntot), dtype=torch.float64, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(mode):
        d = _capi.XtSiDesc(nc=nc, no=no, nv=nv, ncomp=3, s=s, n_sm=counts[0], n_so=counts[1], n_sp=counts[2],
                           with_ground=1, mode=_capi.SI_MODE[mode])
        op = dev["vso" if mode == "soc" else "dip"]
        _capi.check(L.xt_si_couple(ctypes.byref(d), op.data_ptr(), dev["sm"].data_ptr() if counts[0] else None,
                                   dev["so"].data_ptr(), dev["sp"].data_ptr(), out.data_ptr(), _capi.XT_PTR_DEVICE,
                                   st), "xt_si_couple")

    def timed(mode, reps):
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(mode)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    dsm, dso, dsp = ref.dims(nc, no, nv)
    gram = {"soc": 2.0 * 3 * (counts[0] ** 2 * dsm + counts[0] * n * dsm + n * n * dso + n * n * dso + n * n * dsp),
            "dipole": 2.0 * 3 * (counts[0] ** 2 * dsm + n * n * dso + n * n * dsp)}
    res = dict(what="xt_si_couple: one call per mode, HIP events around it; one run", nc=nc, no=no, nv=nv, s=s,
               states=dict(sm=counts[0], so=counts[1], sp=counts[2], ground=1), n=ntot, dims=dict(sm=dsm, so=dso, sp=dsp),
               warmup=a.warmup, reps=a.reps, device=torch.cuda.get_device_name(0))
    bvs = ref.op_blocks(np.ascontiguousarray(vso.transpose(1, 2, 0)), nc, no, nv)
    bdp = ref.op_blocks(np.ascontiguousarray(dip.transpose(1, 2, 0)), nc, no, nv)
    for mode in ("soc", "dipole"):
        timed(mode, a.warmup)
        first = out.clone()
        ms = timed(mode, a.reps)
        t = float(np.median(ms)) * 1e-3
        # the restatement, per pair of |So> states as the reference loops
        t0 = time.perf_counter()
        for k in range(a.pairs):
            xl, xr = xs[1][k % n], xs[1][(k + 1) % n]
            if mode == "soc":
                _ = xl @ ref.img_so_so(bvs, s, (nc, no, nv), xr)
            else:
                _ = ref.tdm_so(bdp, s, (nc, no, nv), xl, xr)
        per_pair = (time.perf_counter() - t0) / max(1, a.pairs)
        res[mode] = dict(ms_median=float(np.median(ms)), ms_all=[round(x, 3) for x in ms],
                         bit_identical_over_calls=bool(torch.equal(first, out)), finite=bool(torch.isfinite(out).all()),
                         gram_flops=gram[mode], gram_tflops=gram[mode] / t / 1e12,
                         gram_frac_fp64_peak=gram[mode] / t / FP64_PEAK,
                         restatement_s_per_pair=per_pair, restatement_s_all_pairs=per_pair * ntot * ntot,
                         speedup_vs_restatement=per_pair * ntot * ntot / t)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
