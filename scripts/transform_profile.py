"""Device time of one raw-count Pca::transform (srx_pca_transform with normalise + log1p on the fly) by kernel class, beside the
same classes of a pipeline step on the same matrix, and the wall time of the transform including the D2H of its scores.

    python scripts/transform_profile.py [--cells 1300000] [--genes 28000] [--density 0.03] [--n-hvg 2000] [--n-pc 50] [--reps 5]

Prints one JSON line.  The matrix is srx_synth's (the bench's c3 shape by default), f32 storage."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import singlerust_amd as sr                                         # noqa: E402
from singlerust_amd import _ffi as F                                # noqa: E402
from singlerust_amd.memory.processing import dim_red               # noqa: E402

CLASSES = {"rowsum": F.K_ROWSUM, "compact": F.K_COMPACT, "spmm_fwd": F.K_SPMM_FWD}


def by_class(ctx):
    out = {}
    for name, c in CLASSES.items():
        ms, n, _ = ctx.prof_get(c)
        out[name] = {"ms": round(ms, 4), "launches": int(n)}
    out["sum_ms"] = round(sum(v["ms"] for v in out.values()), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1_300_000)
    ap.add_argument("--genes", type=int, default=28_000)
    ap.add_argument("--density", type=float, default=0.03)
    ap.add_argument("--n-hvg", type=int, default=2000)
    ap.add_argument("--n-pc", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ctx = sr.Context.default()
    lib = F.lib()
    p = F.SynthParams()
    lib.srx_synth_defaults(C.byref(p), 3003, a.cells, a.genes, a.density)
    h = C.c_void_p()
    F.check(lib.srx_synth_generate(ctx.handle, C.byref(p), 0, a.cells, F.F32, F.STORE_F32, C.byref(h)), ctx.handle)
    raw = sr.IMAnnData(sr.DeviceCsr(ctx, h), None, None, [], [])
    fit = sr.IMAnnData(raw.x().clone(), None, None, [], [])
    opts = F.PcaOpts(a.n_pc, -1, -1, -1, 0, 0, 0, 0.0, 12345)
    res = F.PipelineResult()
    F.check(lib.srx_pipeline(fit.x().handle, 1e4, a.n_hvg, C.byref(opts), C.byref(res)), ctx.handle)   # warm (graphs, scratch)
    # one pipeline step with the profiler on, on a fresh raw clone
    step = sr.IMAnnData(raw.x().clone(), None, None, [], [])
    ctx.synchronize()
    ctx.prof_enable(0xffffffff)
    ctx.prof_reset()
    F.check(lib.srx_pipeline(step.x().handle, 1e4, a.n_hvg, C.byref(opts), C.byref(res)), ctx.handle)
    ctx.synchronize()
    pipe = by_class(ctx)
    ctx.prof_enable(0)
    step.x().free()
    model = dim_red.PcaModel.from_result(fit)
    dim_red.pca_transform(raw, model, target_sum=1e4, log1p=True)      # warm
    walls, prof = [], None
    for r in range(a.reps):
        ctx.synchronize()
        if r == 0:
            ctx.prof_enable(0xffffffff)
            ctx.prof_reset()
        t0 = time.perf_counter()
        scores = dim_red.pca_transform(raw, model, target_sum=1e4, log1p=True)
        walls.append((time.perf_counter() - t0) * 1e3)
        if r == 0:
            ctx.synchronize()
            prof = by_class(ctx)
            ctx.prof_enable(0)
    print(json.dumps({"shape": [a.cells, a.genes, a.density], "n_hvg": a.n_hvg, "n_pc": a.n_pc,
                      "transform_kernels": prof, "pipeline_same_classes": pipe,
                      "kernel_ratio": round(prof["sum_ms"] / pipe["sum_ms"], 3) if pipe["sum_ms"] else None,
                      "transform_wall_ms": {"min": round(min(walls), 2), "median": round(float(np.median(walls)), 2)},
                      "scores_mb": round(scores.nbytes / 1e6, 1)}))


if __name__ == "__main__":
    main()
