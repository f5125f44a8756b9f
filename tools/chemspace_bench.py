#!/usr/bin/env python3
"""Measurements behind profiles/chemspace_moments.txt: the moments kernel (ops.Moments: fp64 column sums and Gram matrix
of resident rows) against the library route ``z = x - s; z.T @ z`` in fp32 and in fp64, and the projection kernel (ops.rows_project)
against ``(x - s) @ W`` (k = 2) and ``(((x - s) @ W) ** 2).sum(1)`` (k = d, squared norm only), alternating in one process (device
events, 7 repeats after a warm-up of each); then ``chemspace.map`` against the forward-only sweep ``neighbours.embed_all`` of the same
store (host clock around work that ends in a synchronise).  The accuracy of each route's Gram matrix against a float64 reference on the
host is printed next to its time.

    python tools/chemspace_bench.py [--out profiles/chemspace_moments.txt] [--kernel-only]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fragnet_amd import chemspace as cs, neighbours as nb, ops, synth           # noqa: E402
from fragnet_amd.dataset import FlatMolStore                                   # noqa: E402
from fragnet_amd.model import FragNetFineTune                                  # noqa: E402

DEV = "cuda:0"
LINES = []


def say(*a):
    LINES.append(" ".join(str(x) for x in a))
    print(LINES[-1], flush=True)


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(routes, repeats=7):
    for _, fn in routes:
        fn()
    times = {name: [] for name, _ in routes}
    for _ in range(repeats):
        for name, fn in routes:
            times[name].append(timed(fn))
    return {name: np.array(t) for name, t in times.items()}


def verdict(ours, theirs, what):
    if ours.max() < theirs.min():
        return f"ranges disjoint, in favour of the kernel ({np.median(theirs) / np.median(ours):.2f}x by the medians) against {what}"
    if theirs.max() < ours.min():
        return f"ranges disjoint, in favour of {what} ({np.median(ours) / np.median(theirs):.2f}x by the medians): the kernel LOSES"
    return f"ranges overlap with {what} (medians {np.median(ours):.3f} vs {np.median(theirs):.3f} ms)"


def moments_part(N, d):
    g = torch.Generator(device=DEV).manual_seed(N + d)
    x = torch.randn(N, d, device=DEV, generator=g) * 1.5 + 0.75
    s = x[:4096].mean(0)
    out = {}

    def kernel():
        out["kernel"] = ops.Moments(d, DEV).update(x, s).result()[2]

    def torch32():
        z = x - s
        out["torch fp32"] = z.T @ z

    def torch64():
        z = (x - s).double()
        out["torch fp64"] = z.T @ z

    times = alternate((("kernel", kernel), ("torch fp32", torch32), ("torch fp64", torch64)))
    # accuracy against the host: float64 of the same fp32 differences, on a sample of columns (the whole [d, d] on the host takes long at 1 M)
    z = (x - s).cpu().numpy().astype(np.float64)
    cols = np.arange(0, d, 16)
    ref = z.T @ z[:, cols]
    scale = np.abs(z).T @ np.abs(z[:, cols])
    say(f"## moments: N={N} d={d}, rows resident ({N * d * 4 / 2**20:.0f} MiB), {2 * N * d * d / 1e9:.1f} GFLOP as a full product "
        f"(the kernel computes the blocks on and above the diagonal: {d // 64 * (d // 64 + 1) // 2} of {(d // 64) ** 2})")
    for name, t in times.items():
        err = (np.abs(out[name].double().cpu().numpy()[:, cols] - ref) / scale).max()
        say(f"{name:11s} ms: median {np.median(t):8.3f}  min {t.min():8.3f}  max {t.max():8.3f}   {N * d * 4 / (np.median(t) * 1e-3) / 1e9:7.1f} GB/s of "
            f"the rows   max |G - ref| / (|Z|^T |Z|) = {err:.2e}")
    say("kernel vs torch fp32: " + verdict(times["kernel"], times["torch fp32"], "the library's fp32 GEMM (+ the n x d temporary)"))
    say("kernel vs torch fp64: " + verdict(times["kernel"], times["torch fp64"], "the library's fp64 GEMM (the like-for-like route on accuracy)"))


def project_part(N, d):
    g = torch.Generator(device=DEV).manual_seed(N + d + 1)
    x = torch.randn(N, d, device=DEV, generator=g)
    s = x[:4096].mean(0)
    for k, sq_only in ((2, False), (d, True)):
        W = torch.randn(d, k, device=DEV, generator=g).contiguous()

        def kernel():
            ops.rows_project(x, W, s, want_rows=not sq_only, want_sq=sq_only)

        def library():
            o = (x - s) @ W
            if sq_only:
                (o * o).sum(1)

        times = alternate((("kernel", kernel), ("torch", library)))
        say(f"## projection: N={N} d={d} k={k}{' squared norm only' if sq_only else ''} ({2 * N * d * k / 1e9:.1f} GFLOP)")
        for name, t in times.items():
            say(f"{name:11s} ms: median {np.median(t):8.3f}  min {t.min():8.3f}  max {t.max():8.3f}   {N * d * 4 / (np.median(t) * 1e-3) / 1e9:7.1f} GB/s of the rows")
        say("kernel vs torch: " + verdict(times["kernel"], times["torch"], "the library route (x - s) @ W" + (", square, sum" if sq_only else "")))


def end_to_end(n_distinct=2048, copies=64):
    torch.manual_seed(0)
    model = FragNetFineTune().to(DEV)
    store = FlatMolStore.from_records(synth.synth_molecules(n_distinct, seed=5, profile="esol")).to(DEV).replicate(copies)
    say(f"## end to end: default 4-layer gat2 finetune model, store of {len(store)} molecules ({n_distinct} distinct x {copies}) resident, "
        f"batches of 512, k=2, no queries")
    for level in ("mol", "frag"):
        rows = [0]

        def sweep():
            rows[0] = nb.embed_all(model, store, level, 512)[0].shape[0]
            torch.cuda.synchronize()

        def mapped():
            cs.map(model, store, level=level, k=2, batch_size=512)
            torch.cuda.synchronize()

        def fitted():
            cs.fit(model, store, level=level, batch_size=512)
            torch.cuda.synchronize()

        sweep(), mapped(), fitted()
        ts, tm, tf = [], [], []
        for _ in range(3):                               # alternating
            t0 = time.perf_counter(); sweep(); ts.append(time.perf_counter() - t0)            # noqa: E702
            t0 = time.perf_counter(); mapped(); tm.append(time.perf_counter() - t0)           # noqa: E702
            t0 = time.perf_counter(); fitted(); tf.append(time.perf_counter() - t0)           # noqa: E702
        ts, tm, tf = np.array(ts), np.array(tm), np.array(tf)
        say(f"level {level}: {rows[0]} rows; embed_all median {np.median(ts):.3f} s [{ts.min():.3f} .. {ts.max():.3f}]; map median "
            f"{np.median(tm):.3f} s [{tm.min():.3f} .. {tm.max():.3f}] = {(np.median(tm) / np.median(ts) - 1) * 100:+.1f} % (moments per batch, "
            f"the host's eigen-decomposition, two projections, the copies of the results); fit alone median {np.median(tf):.3f} s "
            f"[{tf.min():.3f} .. {tf.max():.3f}] = {(np.median(tf) / np.median(ts) - 1) * 100:+.1f} % (it holds no rows)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="also write the lines to this file")
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chemspace_bench.py measures on the GPU; none found")
    say(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}; FN_MOMENTS_CHUNK {ops.MOMENTS_CHUNK}, FN_MOMENTS_GROUP {ops.MOMENTS_GROUP}")
    for N in (1 << 16, 1 << 20):
        for d in (256, 128):
            moments_part(N, d)
            project_part(N, d)
    if not args.kernel_only:
        end_to_end()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
