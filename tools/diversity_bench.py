#!/usr/bin/env python3
"""Measurements behind profiles/diversity_kcenter.txt: greedy k-centre by the fused kernel (ops.KCenter, one launch per
pick) against the library route ``d = ((x - x[c]) ** 2).sum(1); mind = minimum(mind, d); c = mind.argmax()`` on resident rows,
alternating in one process (device events, 7 repeats after a warm-up of each), and ``diversity.select`` against the forward-only sweep
``neighbours.embed_all`` of the same store (host clock around work that ends in a synchronise).

    python tools/diversity_bench.py [--out profiles/diversity_kcenter.txt] [--kernel-only]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fragnet_amd import diversity as dv, neighbours as nb, ops, synth          # noqa: E402
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


def kernel_part(N, d, k=256, repeats=7):
    g = torch.Generator(device=DEV).manual_seed(N + d)
    x = torch.randn(N, d, device=DEV, generator=g)
    out = {}

    def fused():
        kc = ops.KCenter(N, d, "l2", DEV, cap=k).pick(x, k, first=0)
        out["fused"] = kc.result()[0]

    def library_route():
        mind = torch.full((N,), float("inf"), device=DEV)
        c = torch.zeros((), dtype=torch.int64, device=DEV)
        picked = []
        for t in range(k):                               # the pick stays on the device: nothing synchronises here either
            picked.append(c)
            dist = ((x - x[c]) ** 2).sum(1)
            mind = torch.minimum(mind, dist)
            c = mind.argmax()
        out["library"] = torch.stack(picked)

    routes = (("fused", fused), ("library", library_route))
    for _, fn in routes:
        fn()
    times = {name: [] for name, _ in routes}
    for _ in range(repeats):                             # alternating, one process
        for name, fn in routes:
            times[name].append(timed(fn))
    same = (out["fused"] == out["library"]).float().mean().item()
    say(f"## kernel: N={N} d={d} k={k}, squared L2, rows resident ({N * d * 4 / 2**20:.0f} MiB per pass)")
    for name in times:
        t = np.array(times[name])
        per_pick = np.median(t) / k * 1e3
        say(f"{name:8s} ms per {k} picks: median {np.median(t):9.3f}  min {t.min():9.3f}  max {t.max():9.3f}   "
            f"{per_pick:8.2f} us per pick   {N * d * 4 / (per_pick * 1e-6) / 1e9:8.1f} GB/s of the N d 4 bytes of a pick")
    f, l = np.array(times["fused"]), np.array(times["library"])
    say(f"fused range {'BELOW' if f.max() < l.min() else 'NOT below'} the library route's; medians {np.median(l) / np.median(f):.2f}x; "
        f"picks equal to the library route's (whose tie-break and summation order are its own): {same * 100:.1f} %")


def end_to_end(n_distinct=2048, copies=64, k=256):
    torch.manual_seed(0)
    model = FragNetFineTune().to(DEV)
    store = FlatMolStore.from_records(synth.synth_molecules(n_distinct, seed=5, profile="esol")).to(DEV).replicate(copies)
    say(f"## end to end: default 4-layer gat2 finetune model, store of {len(store)} molecules ({n_distinct} distinct x {copies}) resident, "
        f"batches of 512, k={k}, squared L2")
    for level in ("mol", "frag"):
        rows = [0]

        def sweep():
            rows[0] = nb.embed_all(model, store, level, 512)[0].shape[0]
            torch.cuda.synchronize()

        def select():
            dv.select(model, store, k, level=level, batch_size=512)
            torch.cuda.synchronize()

        sweep(), select()
        ts, tn = [], []
        for _ in range(3):                               # alternating
            t0 = time.perf_counter(); sweep(); ts.append(time.perf_counter() - t0)           # noqa: E702
            t0 = time.perf_counter(); select(); tn.append(time.perf_counter() - t0)          # noqa: E702
        ts, tn = np.array(ts), np.array(tn)
        say(f"level {level}: {rows[0]} rows; embed_all median {np.median(ts):.3f} s [{ts.min():.3f} .. {ts.max():.3f}]; select median "
            f"{np.median(tn):.3f} s [{tn.min():.3f} .. {tn.max():.3f}] = +{(np.median(tn) / np.median(ts) - 1) * 100:.1f} % "
            f"({(np.median(tn) - np.median(ts)) / k * 1e6:.1f} us per pick on top of the sweep, the copy of the results included)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="also write the lines to this file")
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("diversity_bench.py measures on the GPU; none found")
    say(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    for N in (1 << 17, 1 << 20):
        for d in (256, 128):
            kernel_part(N, d)
    if not args.kernel_only:
        end_to_end()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
