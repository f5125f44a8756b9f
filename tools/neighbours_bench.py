#!/usr/bin/env python3
"""Measurements behind profiles/neighbours_topk.txt: the fused similarity + top-k kernel against the library route
``(q @ lib.T).topk(k)`` on a resident library, alternating in one process (device events), and ``neighbours.nearest`` against the
forward-only sweep of the same store (host clock around work that ends in a synchronise), with the peak memory of each.

    python tools/neighbours_bench.py [--out profiles/neighbours_topk.txt] [--kernel-only]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fragnet_amd import neighbours as nb, ops, synth          # noqa: E402
from fragnet_amd.dataset import FlatMolStore                  # noqa: E402
from fragnet_amd.model import FragNetFineTune                 # noqa: E402

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


def peak_of(fn):
    """Peak allocated bytes of one (warmed) call above what was allocated before it."""
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def kernel_part(Q=512, d=256, N=1 << 20, chunk=1 << 16, k=8):
    g = torch.Generator(device=DEV).manual_seed(0)
    q = torch.randn(Q, d, device=DEV, generator=g)
    lib = torch.randn(N, d, device=DEV, generator=g)
    say(f"## kernel: Q={Q} d={d} N={N} in chunks of {chunk}, k={k}, dot; library resident ({N * d * 4 / 2**30:.2f} GiB)")

    def fused():
        tk = ops.TopK(Q, k, "dot", DEV)
        for lo in range(0, N, chunk):
            tk.update(q, lib[lo:lo + chunk], lo)
        return tk.result()

    def library_route():
        best_s = torch.full((Q, k), float("-inf"), device=DEV)
        best_i = torch.full((Q, k), -1, dtype=torch.int64, device=DEV)
        for lo in range(0, N, chunk):
            s, i = (q @ lib[lo:lo + chunk].T).topk(k, dim=1)
            s, i = torch.cat([best_s, s], 1), torch.cat([best_i, i + lo], 1)
            best_s, pick = s.topk(k, dim=1)
            best_i = i.gather(1, pick)
        return best_s, best_i

    routes = (("fused", fused), ("library", library_route))
    peaks = {name: peak_of(fn) for name, fn in routes}
    times = {name: [] for name, _ in routes}
    for _ in range(7):                                   # alternating, one process
        for name, fn in routes:
            times[name].append(timed(fn))
    (fs, fi), (ls, li) = fused(), library_route()
    for name in times:
        t = np.array(times[name])
        say(f"{name:8s} ms per search: median {np.median(t):8.3f}  min {t.min():8.3f}  max {t.max():8.3f}   "
            f"peak memory above the inputs {peaks[name] / 2**20:8.2f} MiB")
    med = np.median(times["fused"]) * 1e-3
    say(f"fused: {2.0 * Q * N * d / med / 1e12:.1f} TFLOP/s fp32 (2 Q N d over the median); a Q x N score matrix would be "
        f"{Q * N * 4 / 2**30:.2f} GiB; indices equal to the library route's: {(fi == li).float().mean().item() * 100:.3f} % "
        f"(max |score difference| {(fs - ls).abs().max().item():.2e})")
    for kk, dd, metric in ((32, 256, "cosine"), (8, 128, "cosine"), (8, 256, "l2")):
        qq, ll = q[:, :dd].contiguous(), lib[:, :dd].contiguous()
        qa = ops.rows_rnorm(qq) if metric == "cosine" else (qq * qq).sum(1)
        la = ops.rows_rnorm(ll) if metric == "cosine" else (ll * ll).sum(1)

        def other():
            tk = ops.TopK(Q, kk, metric, DEV)
            for lo in range(0, N, chunk):
                tk.update(qq, ll[lo:lo + chunk], lo, qa, la[lo:lo + chunk])
        other()
        say(f"fused d={dd} k={kk} {metric}: median {np.median([timed(other) for _ in range(5)]):.3f} ms")
        del ll, qq


def end_to_end(n_distinct=2048, copies=64, n_queries=512, k=8):
    torch.manual_seed(0)
    model = FragNetFineTune().to(DEV)
    store = FlatMolStore.from_records(synth.synth_molecules(n_distinct, seed=5, profile="esol")).to(DEV).replicate(copies)
    queries = FlatMolStore.from_records(synth.synth_molecules(n_queries, seed=6, profile="esol")).to(DEV)
    say(f"## end to end: default 4-layer gat2 finetune model, {n_queries} query molecules, library of {len(store)} molecules "
        f"({n_distinct} distinct x {copies}) resident, batches of 512, k={k}, cosine")
    for level in ("mol", "frag"):
        rows = [0]

        def sweep():
            rows[0] = sum(part.rows.shape[0] for part in nb.embed(model, store, level, 512))
            torch.cuda.synchronize()

        def search():
            rows.append(nb.nearest(model, queries, store, level=level, k=k, metric="cosine", batch_size=512).score.shape[0])
            torch.cuda.synchronize()

        peak_sweep, peak_search = peak_of(sweep), peak_of(search)
        ts, tn = [], []
        for _ in range(3):                               # alternating
            t0 = time.perf_counter(); sweep(); ts.append(time.perf_counter() - t0)          # noqa: E702
            t0 = time.perf_counter(); search(); tn.append(time.perf_counter() - t0)         # noqa: E702
        ts, tn = np.array(ts), np.array(tn)
        say(f"level {level}: {rows[-1]} query rows x {rows[0]} library rows; forward-only sweep median {np.median(ts):.3f} s "
            f"[{ts.min():.3f} .. {ts.max():.3f}] ({len(store) / np.median(ts) / 1e6:.2f} M molecules/s); nearest median {np.median(tn):.3f} s "
            f"[{tn.min():.3f} .. {tn.max():.3f}] = +{(np.median(tn) / np.median(ts) - 1) * 100:.1f} % (its pass over the queries "
            f"included); peak memory sweep {peak_sweep / 2**20:.1f} MiB, nearest {peak_search / 2**20:.1f} MiB "
            f"(a score matrix would be {rows[-1] * rows[0] * 4 / 2**20:.0f} MiB)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="also write the lines to this file")
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("neighbours_bench.py measures on the GPU; none found")
    say(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    kernel_part()
    if not args.kernel_only:
        end_to_end()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
