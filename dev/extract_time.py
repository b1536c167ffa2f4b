#!/usr/bin/env python3
"""Beyn's eigenpair extraction on moments that are already in HBM: `moments2eigs_native` (wae_tall_* behind the C ABI, numpy for the
small problems) against `moments2eigs_device(gram_rel_tol=1e-6)` (torch: bmm / rocSOLVER / rocBLAS) on the SAME buffer in the same
process, random moments of the shapes (d, l, 2K) the comments of nlevp/distributed.py quote, rel_tol = 1e-6.  Both after a warm-up
(`warm_up_dense_linalg` for torch, one un-timed run each), best of 5, alternating, every timed run ending in a device synchronise.
Also: each primitive alone at the shape the extraction uses (best of 5, achieved GB/s over its algorithmic bytes) and the algorithmic
bytes of one extraction, counted call by call.  Writes one JSON object (and prints it).

    python dev/extract_time.py --out profiles/extract_tail.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
import wae_amd  # noqa
from wae_amd.nlevp import TallMatrix, moments2eigs_native
from wae_amd.nlevp.distributed import moments2eigs_device, warm_up_dense_linalg

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="995328x8x4,200000x16x4")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rel-tol", type=float, default=1e-6)
ap.add_argument("--out", default="")
a = ap.parse_args()
dev = torch.device("cuda", 0)


class _Raw:
    """a TallMatrix's storage as a flat float64 CUDA tensor (no copy): torch reads the very buffer the library owns"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2}


def best(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        ts.append(time.perf_counter() - t)
    return min(ts), ts


def count_bytes(fn):
    """algorithmic bytes of the tall-matrix calls fn makes: every operand column read once, every result column written once"""
    tot = {"gram": 0, "mul": 0, "hankel": 0, "calls": 0}
    orig = (TallMatrix.gram, TallMatrix.mul, TallMatrix.hankel)

    def gram(self, other=None, a_col0=0, na=None, b_col0=0, nb=None):
        o = self if other is None else other
        wa, wb = (self.ncols - a_col0 if na is None else na), (o.ncols - b_col0 if nb is None else nb)
        same = o is self and a_col0 == b_col0 and wa == wb
        tot["gram"] += 16 * self.rows * (wa if same else wa + wb)
        tot["calls"] += 1
        return orig[0](self, other, a_col0, na, b_col0, nb)

    def mul(self, src, Cm, dst_col0=0, src_col0=0, src_row0=0, alpha=1.0, beta=0.0):
        ns, nc = np.shape(Cm)
        tot["mul"] += 16 * self.rows * (ns + nc * (2 if beta != 0 else 1))
        tot["calls"] += 1
        return orig[1](self, src, Cm, dst_col0, src_col0, src_row0, alpha, beta)

    def hankel(self, moments, l, K, shift):
        tot["hankel"] += 2 * 16 * self.rows * self.ncols
        tot["calls"] += 1
        return orig[2](self, moments, l, K, shift)

    TallMatrix.gram, TallMatrix.mul, TallMatrix.hankel = gram, mul, hankel
    try:
        fn()
    finally:
        TallMatrix.gram, TallMatrix.mul, TallMatrix.hankel = orig
    tot["total"] = tot["gram"] + tot["mul"] + tot["hankel"]
    return tot


out = {"device": torch.cuda.get_device_name(0), "rel_tol": a.rel_tol, "reps": a.reps, "shapes": []}
for spec in a.shapes.split(","):
    d, l, K2 = (int(v) for v in spec.split("x"))
    K, n, R = K2 // 2, l * (K2 // 2), d * (K2 // 2)
    M = TallMatrix.create(d, l * K2)
    try:
        buf = torch.as_tensor(_Raw(M.ptr, d * l * K2 * 2), device=dev)
        shared = True
    except Exception as e:      # noqa: BLE001  (no array-interface import in this torch: a copy of the same numbers instead)
        print("sharing the buffer failed (%s): torch works on a copy" % e, file=sys.stderr)
        buf = torch.empty(d * l * K2 * 2, dtype=torch.float64, device=dev)
        shared = False
    gen = torch.Generator(device=dev).manual_seed(7)
    buf.normal_(generator=gen)
    torch.cuda.synchronize(dev)
    if not shared:
        M.write(buf.cpu().numpy().view(np.complex128).reshape(d, l * K2, order="F"))
    warm_up_dense_linalg(dev, rows=65536, cols=l, K=K)

    def native():
        Om, P, S = moments2eigs_native(M, (d, l, K2), rel_tol=a.rel_tol)
        P.release()
        return Om, S

    def torch_tail():
        Om, P, S = moments2eigs_device(buf, (d, l, K2), gram_rel_tol=a.rel_tol)
        return Om, S

    Om_n, S_n = native()                      # un-timed: first launches, torch's caching allocator
    Om_t, S_t = torch_tail()
    tn0, tt = [], []
    for _ in range(a.reps):                   # alternating; scratch allocated and freed inside every native call
        tn0.append(best(native, 1)[0])
        tt.append(best(torch_tail, 1)[0])
    TallMatrix.POOL_LIMIT = 16 << 30          # the opt-in pool: released scratch is reused (what torch's caching allocator does for torch)
    native()
    tn = [best(native, 1)[0] for _ in range(a.reps)]
    TallMatrix.POOL_LIMIT = 0
    TallMatrix.trim_pool()
    rec = {"d": d, "l": l, "K": K, "shared_buffer": shared,
           "native_ms": 1e3 * min(tn0), "native_all_ms": [1e3 * t for t in tn0],
           "native_pooled_ms": 1e3 * min(tn), "native_pooled_all_ms": [1e3 * t for t in tn],
           "torch_ms": 1e3 * min(tt), "torch_all_ms": [1e3 * t for t in tt],
           "native_over_torch": min(tn0) / min(tt), "native_pooled_over_torch": min(tn) / min(tt),
           "native_not_slower_within_10pct": bool(min(tn0) <= 1.1 * min(tt)),
           "native_pooled_not_slower_within_10pct": bool(min(tn) <= 1.1 * min(tt)),
           "sigma_rel_diff": float(np.max(np.abs(S_n - S_t) / S_t[0])),
           "omega_max_diff": float(max(np.min(np.abs(Om_t - w)) for w in Om_n)),
           "algorithmic_bytes": count_bytes(native)}
    rec["native_GBps_over_algorithmic_bytes"] = rec["algorithmic_bytes"]["total"] / min(tn) / 1e9      # (pooled run)
    # the primitives alone, at the shapes of the extraction
    B0 = M.new(R, n).hankel(M, l, K, 0) if K > 1 else M
    U, U2 = M.new(R, n), M.new(R, n)
    Cm = np.linalg.qr(np.random.default_rng(0).standard_normal((n, n)))[0]
    prim = {}
    for name, fn, nbytes in (("gram_XhX", lambda: B0.gram(B0, 0, n, 0, n), 16 * R * n),
                             ("mul_beta0", lambda: U.mul(B0, Cm), 16 * R * 2 * n),
                             ("mul_identity_copy", lambda: U.mul(B0, np.eye(n)), 16 * R * 2 * n),
                             ("gram_XhY", lambda: U.gram(B0, 0, n, 0, n), 16 * R * 2 * n),
                             ("mul_beta1", lambda: U2.mul(U, Cm, alpha=-1.0, beta=1.0), 16 * R * 3 * n),
                             ("hankel", (lambda: U2.hankel(M, l, K, 1)) if K > 1 else None, 16 * R * 2 * n)):
        if fn is None:
            continue
        fn()
        t, _ = best(fn, a.reps)
        prim[name] = {"ms": 1e3 * t, "bytes": nbytes, "GBps": nbytes / t / 1e9}
    rec["primitives"] = prim
    out["shapes"].append(rec)
    for m in (U, U2) + ((B0,) if K > 1 else ()):
        m.destroy()
    del buf
    M.destroy()
    TallMatrix.trim_pool()
    torch.cuda.empty_cache()
    print(json.dumps(rec), flush=True)

txt = json.dumps(out, indent=1)
if a.out:
    with open(a.out, "w") as f:
        f.write(txt + "\n")
print(txt)
