"""Device timing of ``xt_tdm`` (state-to-state transition moments) at a bench.py shape.

    python tools/tdm_bench.py [--config C4] [--nstates 40] [--ncomp 3] [--warmup 3] [--reps 10]
                              [--out profiles/tdm_C4_timing.json]
    python tools/tdm_bench.py --sc [--restatement] [--dump out.npy] [--out profiles/tdm_sc_headline_timing.json]

``--sc`` times ``xt_tdm_sc`` (spin-conserving roots, reference state included) at the headline
X-TDA shape instead; see ``main_sc``.

Random device-resident inputs (the timing does not depend on the values), device pointers,
HIP events around each whole call -- workspace allocation, the AO->MO transforms, the pack,
D for every state and component, the Gram product and the final synchronise included.
Warm-up calls first (code-object load, split-K plans).  Next to the time the JSON records the
per-A.x time of the same configuration from its recorded benchmark, so the property step can
be read against one matvec of the solve that precedes it.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# nao, nc, no, sa, OO compressed: the XSF configurations of bench.py
SHAPES = {"C4": dict(nao=840, nc=179, no=3, sa=3, compressed=True),
          "C4d": dict(nao=840, nc=180, no=1, sa=0, compressed=True)}


def sc_data(nao, nc, no, nstates, ncomp):
    """Host inputs of the spin-conserving mode (NumPy generator: the same on every machine)."""
    rng = np.random.default_rng(0)
    nv = nao - nc - no
    op = rng.standard_normal((ncomp, nao, nao))
    op = op + op.transpose(0, 2, 1)
    c = np.eye(nao) + rng.standard_normal((nao, nao)) / np.sqrt(nao)
    vecs = rng.standard_normal((nstates, (nc + no) * nv + nc * (no + nv)))
    vecs /= np.sqrt((vecs ** 2).sum(axis=1))[:, None]
    return op, c, vecs, nv


def main_sc(a):
    """``xt_tdm_sc`` at the headline X-TDA shape (nao 1000, nc 99, no 2: blocks 101 x 899 and
    99 x 901, dim 179 998), spin-adapted, with the ground row.  ``--restatement`` times the NumPy
    restatement (tests/xtda_tdm_ref.py) on the same data instead, on the host alone; ``--dump``
    saves either result as .npy so that the two can be compared."""
    nao, nc, no = 1000, 99, 2
    op, c, vecs, nv = sc_data(nao, nc, no, a.nstates, a.ncomp)
    dim = vecs.shape[1]
    res = dict(nao=nao, nc=nc, no=no, nv=nv, nstates=a.nstates, ncomp=a.ncomp, dim=dim, spin_adapted=1, with_ground=1)
    if a.restatement:
        import time
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import xtda_tdm_ref
        t0 = time.perf_counter()
        d = np.einsum('xpq,pi,qj->xij', op, c, c, optimize=True)
        out = xtda_tdm_ref.tdm_xtda(vecs, d, nc, no, nv, no / 2)
        res.update(what="tests/xtda_tdm_ref.py on the host, AO->MO transform included", s_restatement=time.perf_counter() - t0)
    else:
        import torch
        from xtddft_amd import _capi, build
        build.build()
        L = _capi.lib()
        if not torch.cuda.is_available():
            raise SystemExit("tdm_bench needs the GPU: a timing taken elsewhere says nothing")
        oa = nc + no
        dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda()
               for x in (op, c[:, :oa], c[:, oa:], c[:, :nc], c[:, nc:], vecs)]
        o = torch.empty(a.ncomp, a.nstates + 1, a.nstates + 1, dtype=torch.float64, device="cuda")
        desc = _capi.XtTdmScDesc(nao=nao, nocc_a=oa, nvir_a=nv, nocc_b=nc, nvir_b=no + nv, ncomp=a.ncomp,
                                 nstates=a.nstates, spin_adapted=1, no=no, si=no / 2, with_ground=1)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def call():
            _capi.check(L.xt_tdm_sc(ctypes.byref(desc), *[t.data_ptr() for t in dev], o.data_ptr(),
                                    _capi.XT_PTR_DEVICE, st), "xt_tdm_sc")
        for _ in range(a.warmup):
            call()
        first = o.clone()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        out = o.cpu().numpy()
        res.update(what="xt_tdm_sc: one call, HIP events around it (device pointers)", warmup=a.warmup, reps=a.reps,
                   ms_median=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)),
                   ms_all=[round(m, 4) for m in ms], bit_identical_over_calls=bool(torch.equal(first, o)),
                   device=torch.cuda.get_device_name(0))
    if a.dump:
        os.makedirs(os.path.dirname(os.path.abspath(a.dump)), exist_ok=True)
        np.save(a.dump, out)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4", choices=sorted(SHAPES))
    ap.add_argument("--nstates", type=int, default=None)
    ap.add_argument("--ncomp", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sc", action="store_true", help="xt_tdm_sc at the headline X-TDA shape (20 states)")
    ap.add_argument("--restatement", action="store_true", help="--sc: time the NumPy restatement on the host")
    ap.add_argument("--dump", default=None, help="--sc: save the moments as .npy")
    a = ap.parse_args()
    if a.nstates is None:
        a.nstates = 20 if a.sc else 40
    if a.sc:
        return main_sc(a)

    import torch
    from xtddft_amd import _capi, build
    build.build()
    L = _capi.lib()
    if not torch.cuda.is_available():
        raise SystemExit("tdm_bench needs the GPU: a timing taken elsewhere says nothing")
    s = SHAPES[a.config]
    nao, nc, no = s["nao"], s["nc"], s["no"]
    nv = nao - nc - no
    O, V = nc + no, no + nv
    dim = O * V - (1 if s["compressed"] else 0)
    g = torch.Generator(device="cuda").manual_seed(0)

    def rand(*shape):
        return torch.randn(*shape, dtype=torch.float64, device="cuda", generator=g)
    op = rand(a.ncomp, nao, nao)
    op = (op + op.transpose(1, 2)).contiguous()
    c = torch.linalg.qr(rand(nao, nao))[0]
    c_occ, c_vir = c[:, :O].contiguous(), c[:, nc:].contiguous()
    vecs = rand(a.nstates, dim)
    vecs /= vecs.norm(dim=1, keepdim=True)
    vects = None
    if s["compressed"] and no > 1:
        from xtddft_amd.xsf_tda import get_vect
        vects = torch.from_numpy(get_vect(no)).cuda()
    out = torch.empty(a.ncomp, a.nstates, a.nstates, dtype=torch.float64, device="cuda")
    d = _capi.XtTdmDesc(nao=nao, nc=nc, no=no, nv=nv, ncomp=a.ncomp, nstates=a.nstates, sa=s["sa"],
                        si=no / 2, layout=_capi.TDM_LAYOUT["blocks"], oo_compressed=int(s["compressed"]))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        _capi.check(L.xt_tdm(ctypes.byref(d), op.data_ptr(), c_occ.data_ptr(), c_vir.data_ptr(), vecs.data_ptr(),
                             None if vects is None else vects.data_ptr(), out.data_ptr(), _capi.XT_PTR_DEVICE, st),
                    "xt_tdm")
    for _ in range(a.warmup):
        call()
    first = out.clone()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    res = dict(what="xt_tdm: one call, HIP events around it (device pointers)", config=a.config, nao=nao, nc=nc,
               no=no, nv=nv, nstates=a.nstates, ncomp=a.ncomp, sa=s["sa"], oo_compressed=s["compressed"], dim=dim,
               warmup=a.warmup, reps=a.reps, ms_median=float(np.median(ms)), ms_min=float(min(ms)),
               ms_max=float(max(ms)), ms_all=[round(m, 4) for m in ms],
               bit_identical_over_calls=bool(torch.equal(first, out)),
               streamed_gib=8.0 * a.nstates * O * V * (2 * a.ncomp + 2) / 2 ** 30,
               device=torch.cuda.get_device_name(0))
    bench = os.path.join(ROOT, "profiles", f"r06_{a.config}_bench.json")
    if os.path.exists(bench):
        with open(bench) as f:
            b = json.load(f)
        res["ax_ms_per_matvec"] = b["ms_per_step"] / b["config"]["nvec"]
        res["ax_source"] = f"profiles/r06_{a.config}_bench.json (ms_per_step / nvec)"
        res["tdm_over_one_ax"] = res["ms_median"] / res["ax_ms_per_matvec"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
