#!/usr/bin/env python3
"""Measurements behind profiles/device_metrics.txt: one validation pass with ``TrainerFineTune.test`` (a host read per
batch, sklearn per task column) against ``TrainerFineTune.evaluate`` (metrics on the device) on the same loader and model, alternating
in one process (host clock around work that ends in a synchronise); and the pair-count launches alone (device events around a window
of calls) next to ``sklearn.metrics.roc_auc_score`` on the same arrays (host clock).

    python tools/device_metrics_bench.py [--out profiles/device_metrics.txt] [--kernel-only]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fragnet_amd import metrics as M, ops, synth, train       # noqa: E402
from fragnet_amd.dataset import FlatMolStore                  # noqa: E402
from fragnet_amd.model import FragNetFineTune                 # noqa: E402

DEV = "cuda:0"
LINES = []


def say(*a):
    LINES.append(" ".join(str(x) for x in a))
    print(LINES[-1], flush=True)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(t):
    t = np.asarray(t)
    return f"median {np.median(t):9.3f}  [{t.min():9.3f} .. {t.max():9.3f}]"


def validation_pass(n, distinct):
    torch.manual_seed(0)
    model = FragNetFineTune(n_classes=12).to(DEV)
    store = FlatMolStore.from_records(synth.synth_molecules(distinct, seed=11, profile="tox21")).to(DEV)
    if n > distinct:
        store = store.replicate(n // distinct)
    loader = train.StoreLoader(store, 64)
    trainer = train.TrainerFineTune(target_type="clsf")
    say(f"## validation pass: tox21-profile store of {len(store)} molecules ({distinct} distinct), 12 task columns, batches of 64 "
        f"({len(loader)} batches), default 4-layer gat2 finetune model in eval mode")
    routes = (("test", lambda: trainer.test(model, loader)[0]), ("evaluate", lambda: trainer.evaluate(model, loader)["neg_auc"]))

    def forward_only():
        with torch.no_grad():
            model.eval()
            for b in loader:
                model(b)

    scores = {name: fn() for name, fn in routes}          # warm-up of every shape, and the two scores
    forward_only()
    times = {name: [] for name, _ in routes}
    fwd = []
    for _ in range(9):                                    # alternating, one process
        for name, fn in routes:
            times[name].append(clock(fn))
        fwd.append(clock(forward_only))
    for name in times:
        say(f"{name:9s} ms per pass: {spread(times[name])}   score {scores[name]!r}")
    say(f"{'forward':9s} ms per pass: {spread(fwd)}   (the batches' forward passes alone, no read-back, no metric)")
    _, t, p = trainer.test(model, loader)
    from sklearn.metrics import roc_auc_score

    def host_metric():
        for c in range(t.shape[1]):
            ok = t[:, c] > -0.5
            if ok.any() and len(np.unique(t[ok, c])) == 2:
                roc_auc_score(t[ok, c], p[ok, c])

    host = []
    for _ in range(9):
        t0 = time.perf_counter()
        host_metric()
        host.append((time.perf_counter() - t0) * 1e3)
    say(f"{'sklearn':9s} ms per pass: {spread(host)}   (test's 12 roc_auc_score calls alone, host clock)")
    say(f"evaluate / test = {np.median(times['evaluate']) / np.median(times['test']):.3f} (medians); |score difference| "
        f"{abs(scores['test'] - scores['evaluate']):.1e}")


def count_launches(n, c, seed=0):
    rng = np.random.default_rng(seed)
    y = (rng.random((n, c)) < 0.4).astype(np.float32)
    y[rng.random((n, c)) < 0.3] = -1.0
    p = (rng.standard_normal((n, c)) + np.maximum(y, 0)).astype(np.float32)
    pd, yd = torch.as_tensor(p).to(DEV), torch.as_tensor(y).to(DEV)
    ops.pair_concordance(pd, yd, M.CLSF_LABEL_FLOOR)
    torch.cuda.synchronize()
    one = clock(lambda: ops.pair_concordance(pd, yd, M.CLSF_LABEL_FLOOR))
    reps = int(min(2000, max(3, 200.0 / max(one, 1e-3))))             # a window of about 0.2 s
    windows = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            out = ops.pair_concordance(pd, yd, M.CLSF_LABEL_FLOOR)
        b.record()
        torch.cuda.synchronize()
        windows.append(a.elapsed_time(b) / reps)
    counts = out.cpu().numpy()
    from sklearn.metrics import roc_auc_score
    host = []
    for _ in range(3 if n >= 1 << 18 else 7):
        t0 = time.perf_counter()
        aucs = []
        for k in range(c):
            ok = y[:, k] > -0.5
            aucs.append(roc_auc_score(y[ok, k], p[ok, k]))
        host.append((time.perf_counter() - t0) * 1e3)
    pairs = float(n) * n * c
    med = float(np.median(windows))
    say(f"n={n:8d} c={c:2d}: count launches ms per call {spread(windows)} ({reps} calls per window; {pairs / med / 1e9:6.2f} T pair "
        f"updates/s over n^2 c)   sklearn ms {spread(host)}   device / sklearn = {med / np.median(host):7.3f}   "
        f"max |AUC difference| {np.abs(M.concordance_per_column(counts) - np.array(aucs)).max():.1e}")
    return med, float(np.median(host))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="also write the lines to this file")
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("device_metrics_bench.py measures on the GPU; none found")
    say(f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    if not args.kernel_only:
        validation_pass(783, 783)
        validation_pass(8192, 1024)
    say("## pair-count launches alone (ops.pair_concordance: count + combine, device events) against sklearn.metrics.roc_auc_score on the "
        "same arrays (binary labels, 30 % missing; host clock, masking included)")
    for n in (8192, 65536):
        for c in (1, 12):
            count_launches(n, c)
    say("## where the O(n^2) count stops beating sklearn's sort, c = 1")
    crossed = None
    for e in range(17, 21):
        dev_ms, host_ms = count_launches(1 << e, 1)
        if crossed is None and dev_ms > host_ms:
            crossed = 1 << e
    say(f"first measured n at which the device count is slower than sklearn (c = 1): {crossed if crossed else 'none up to 2^20'}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
