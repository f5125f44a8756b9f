#!/usr/bin/env python3
"""Fragment Shapley values on one GPU: one encoder pass per molecule against the floor of a replicated implementation, the two forms of the
coalition read-out against each other, and where a chunk's time goes.

    python tools/fragment_shapley_bench.py [--repeats 5] [--mols 1024] > profiles/frag_shapley_bench.txt

One process, arms alternating, device events around each, min / median / max over the repeats; model: the quick start's (4 layers, 4
heads, FTHead3 128/1024/1024/512, relu); ESOL-profile molecules.
(i)   FEATURE: attribution.fragment_shapley(model, store, exact_max=10), end to end (design, collate, encoder, read-out, head, values to the
      host, reduction).  YARDSTICK: the plain evaluation forward over as many replicated molecules as there are coalition rows, in chunks
      under leave_one_out's row budget, its replica list built outside the timed region, predictions copied to the host once: no mask, no
      reduction -- less than any replicated implementation has to do.
(ii)  fn_pool_cat_coalitions_f32 in its two forms (FN_TUNE_COALITION_STAGED 17: a tile of 64 rows per workgroup, the atom rows of a run of
      >= 16 rows staged in LDS; 0: one workgroup per row and half) on the same rows: all 2^F masks per molecule for F = 2, 6, 10 (groups: atom index % F) over the
      encoder outputs of the first molecules, and the rows of the first chunk of (i).
(iii) The split of the first chunk: encoder pass, read-out, head over the chunk's rows (slices of ops.DENSE_MAX_ROWS), the whole call;
      the rest is host time (design, collate, plan, upload, download, reduction)."""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import fragnet_amd
from fragnet_amd import _lib, attribution as attr, ops, synth
from fragnet_amd.dataset import FlatMolStore
from fragnet_amd.model import FragNetFineTune
from fragnet_amd.plan import _stream_ptr, plan_for

DEV = "cuda:0"
KEY = 34          # FN_TUNE_COALITION_STAGED


def spread(xs):
    return f"min {min(xs):.3f}  median {statistics.median(xs):.3f}  max {max(xs):.3f}"


def timed(fn, n=1):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / n


def alternate(arms, repeats, n=1):
    for fn in arms.values():          # warm-up: code objects, library GEMM selection, allocator
        fn()
        fn()
    ms = {k: [] for k in arms}
    for _ in range(repeats):
        for k, fn in arms.items():
            ms[k].append(timed(fn, n))
    return ms


def read_out_launch(x_atoms, x_frags, plan, bit_d, mol_d, mask_d, out):
    a, f = ops._seg_struct(plan.segs["mol_atoms"]), ops._seg_struct(plan.segs["mol_frags"])
    st = _stream_ptr(out.device)
    return lambda: _lib.call("fn_pool_cat_coalitions_f32", x_atoms.data_ptr(), x_frags.data_ptr(), C.byref(a), C.byref(f), bit_d.data_ptr(),
                             mol_d.data_ptr(), mask_d.data_ptr(), mol_d.shape[0], out.data_ptr(), st)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mols", type=int, default=1024)
    args = ap.parse_args()
    if args.repeats < 5 or args.mols < 1024:
        ap.error("at least 5 repeats on at least 1024 molecules")
    fragnet_amd.prefer_rocblas_for_dense_heads()
    torch.manual_seed(5)
    model = FragNetFineTune(n_classes=1, num_layer=4, drop_ratio=0.1, h1=128, h2=1024, h3=1024, h4=512, act="relu").to(DEV).eval()
    records = synth.synth_molecules(args.mols, seed=4200, profile="esol")
    store = FlatMolStore.from_records(records).to(DEV)
    lens = store._host_lengths()
    off = store._host_offsets()["atom"]
    flat, table = attr._store_fragment_table(store)
    counts = table[3]
    rows = attr.coalition_design(counts, exact_max=10)[2]
    total = int(rows.sum())
    cost = lens["atom"] + lens["edge"]
    replica_chunks = attr.plan_chunks(cost, rows, attr.DEFAULT_MAX_ROWS)
    chunk_mols = [np.concatenate([np.full(r1 - r0, i, dtype=np.int64) for i, r0, r1 in chunk]) for chunk in replica_chunks]

    # ---------------------------------------------------------------------------------------- (i) against the floor
    def feature():
        return attr.fragment_shapley(model, store, exact_max=10)

    def yardstick():
        with torch.no_grad():
            return torch.cat([model(store.collate(m)).reshape(len(m), -1) for m in chunk_mols], 0).cpu()

    ms = alternate({"feature": feature, "yardstick": yardstick}, args.repeats)
    res = feature()
    assert sum(len(m) for m in chunk_mols) == total
    chunks = attr.plan_coalition_chunks(rows, 512, attr.DEFAULT_SHAPLEY_ROWS)
    print(f"(i) {len(store)} ESOL-profile molecules, {int(counts.sum())} fragments (at most {int(counts.max())} per molecule), {total} coalition rows "
          f"({total / len(store):.1f} per molecule), {int(res.exact.sum())} molecules exact; atom + directed-bond rows: {int(cost.sum())} once per "
          f"molecule, {int((cost * rows).sum())} replicated ({(cost * rows).sum() / cost.sum():.1f} x)")
    print(f"ms per run over all molecules, {args.repeats} repeats, arms alternating, device events:")
    print(f"   feature    fragment_shapley, exact_max 10 ({len(chunks)} chunks of <= 512 molecules and <= {attr.DEFAULT_SHAPLEY_ROWS} rows)   {spread(ms['feature'])}")
    print(f"   yardstick  plain forward over the replicated molecules ({len(replica_chunks)} chunks of <= {attr.DEFAULT_MAX_ROWS} rows)   {spread(ms['yardstick'])}")
    f_med, y_med = statistics.median(ms["feature"]), statistics.median(ms["yardstick"])
    print(f"   yardstick / feature (medians): {y_med / f_med:.2f} x; per coalition row: feature {f_med * 1e3 / total:.3f} us, yardstick {y_med * 1e3 / total:.3f} us")

    # ---------------------------------------------------------------------------------------- (ii) the two read-out forms
    print(f"(ii) fn_pool_cat_coalitions_f32, us per launch, {args.repeats} repeats, forms alternating (tiled: FN_TUNE_COALITION_STAGED 17, rows: 0):")

    def two_forms(what, launch, n):
        def form(value):
            def run():
                _lib.call("fn_set_tuning", KEY, value)
                launch()
            return run
        try:
            us = alternate({"tiled": form(17), "rows": form(0)}, args.repeats, n)
        finally:
            _lib.call("fn_set_tuning", KEY, 1)
        t, r = [x * 1e3 for x in us["tiled"]], [x * 1e3 for x in us["rows"]]
        apart = max(t) < min(r) or max(r) < min(t)
        print(f"   {what}, {n} launches per repeat   tiled {spread(t)}   rows {spread(r)}   rows / tiled (medians) "
              f"{statistics.median(r) / statistics.median(t):.2f} x, spreads {'apart' if apart else 'OVERLAP'}")

    for F, M, n in ((2, 512, 200), (6, 512, 50), (10, 128, 10)):
        batch = store.collate(np.arange(M))
        with torch.no_grad():
            x_atoms, x_frags = model.pretrain(batch, edge_outputs=False)[:2]
        plan = plan_for(batch)
        bit = np.concatenate([np.arange(int(off[i + 1] - off[i])) % F for i in range(M)]).astype(np.int8)
        per = np.array([1 << min(F, int(off[i + 1] - off[i])) for i in range(M)], dtype=np.int64)
        first = np.concatenate([[0], np.cumsum(per)])
        mol = np.repeat(np.arange(M, dtype=np.int32), per)
        mask = np.arange(first[-1], dtype=np.int64) - np.repeat(first[:-1], per)
        bit_d, mol_d, mask_d = (torch.from_numpy(x).to(DEV) for x in (bit, mol, mask))
        out = torch.empty(mol.shape[0], 256, device=DEV)
        launch = read_out_launch(x_atoms, x_frags, plan, bit_d, mol_d, mask_d, out)
        two_forms(f"2^F = {1 << F:5d}: {M} molecules, {mol.shape[0]} rows", launch, n)

    # ---------------------------------------------------------------------------------------- (iii) the split of the first chunk
    b, e = chunks[0]
    captured = {}

    def capture(b_, e_, row_mol, row_mask):
        captured["rows"] = (row_mol.copy(), row_mask.copy())
        return np.zeros((row_mol.shape[0], 1), dtype=np.float32)
    attr._shapley_host(counts[b:e], capture, exact_max=10)
    row_mol, row_mask = captured["rows"]
    R = row_mol.shape[0]
    chunk_store = FlatMolStore.from_records(records[b:e]).to(DEV)
    batch = store.collate(np.arange(b, e))
    bits = attr.atom_bits(flat, off, table)[int(off[b]): int(off[e])]
    with torch.no_grad():
        x_atoms, x_frags = model.pretrain(batch, edge_outputs=False)[:2]
        plan = plan_for(batch)
        bit_d, mol_d, mask_d = torch.from_numpy(bits.copy()).to(DEV), torch.from_numpy(row_mol).to(DEV), torch.from_numpy(row_mask.view(np.int64)).to(DEV)
        out = torch.empty(R, 256, device=DEV)
        launch = read_out_launch(x_atoms, x_frags, plan, bit_d, mol_d, mask_d, out)
        two_forms(f"first chunk of (i): {e - b} molecules, {R} rows ({R / (e - b):.1f} per molecule)", launch, 50)

        def head():
            model.fthead.live_rows = None
            return [model.fthead(out[lo: lo + ops.DENSE_MAX_ROWS]) for lo in range(0, R, ops.DENSE_MAX_ROWS)]
        enc = lambda: model.pretrain(batch, edge_outputs=False)
        parts = alternate({"encoder": enc, "read-out": launch, "head": head}, args.repeats, 10)
    call = statistics.median(alternate({"call": lambda: attr.fragment_shapley(model, chunk_store, exact_max=10)}, args.repeats)["call"])
    med = {k: statistics.median(v) for k, v in parts.items()}
    print(f"(iii) first chunk: {e - b} molecules, {R} coalition rows, {-(-R // ops.DENSE_MAX_ROWS)} head slices; ms, {args.repeats} repeats (10 runs per repeat):")
    for k in ("encoder", "read-out", "head"):
        print(f"   {k:9s} {spread(parts[k])}")
    print(f"   whole call on the chunk's molecules alone (median)   {call:.3f}")
    print(f"   host and transfers (call - encoder - read-out - head, medians): {call - sum(med.values()):.3f} ms = {(call - sum(med.values())) / call * 100:.0f} % of the call; "
          f"head / call {med['head'] / call * 100:.0f} %, read-out / call {med['read-out'] / call * 100:.1f} %, encoder / call {med['encoder'] / call * 100:.0f} %")
    return 0


if __name__ == "__main__":
    sys.exit(main())
