#!/usr/bin/env python3
"""Fragment contributions on one GPU: one encoder pass per molecule against the floor of any replicated implementation.

    python tools/fragment_attribution_bench.py [--repeats 5] [--mols 1024] > profiles/frag_attr_bench.txt

Two arms in this one process, alternating, device events around each, min / median / max over the repeats; model: the quick start's
(4 layers, 4 heads, FTHead3 128/1024/1024/512, relu); 1024 ESOL-profile molecules, batch_size 512.
1. FEATURE: attribution.fragment_contributions(model, store), end to end (collate, encoder, read-out, head, results on the host).
2. YARDSTICK: the plain evaluation forward ``model(store.collate(molecule of every replica))`` over the replicated molecules -- one
   encoder pass per fragment, as the reference's ``create_data`` replicates the record -- in chunks under the row budget leave_one_out
   uses (attribution.DEFAULT_MAX_ROWS atom + directed-bond rows), predictions copied to the host once.  It applies no mask and runs
   no unmasked batch: less than any replicated implementation has to do.
Also from the same run: the time of one fn_pool_cat_groups_f32 launch and of one encoder pass on the first chunk of 512 molecules.
Exit status 1 when the feature arm is not faster than the yardstick arm (medians)."""
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

BATCH = 512


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mols", type=int, default=1024)
    args = ap.parse_args()
    if args.repeats < 5 or args.mols < 1024:
        ap.error("at least 5 repeats on at least 1024 molecules")
    fragnet_amd.prefer_rocblas_for_dense_heads()
    torch.manual_seed(5)
    model = FragNetFineTune(n_classes=1, num_layer=4, drop_ratio=0.1, h1=128, h2=1024, h3=1024, h4=512, act="relu").to("cuda:0").eval()
    store = FlatMolStore.from_records(synth.synth_molecules(args.mols, seed=4200, profile="esol")).to("cuda:0")
    lens = store._host_lengths()
    frag_of = store.t["atom_id_frag_id"].cpu().numpy()
    off = store._host_offsets()["atom"]
    counts = np.array([np.unique(frag_of[off[i]: off[i + 1]]).shape[0] for i in range(len(store))], dtype=np.int64)
    chunks = attr.plan_chunks(lens["atom"] + lens["edge"], counts, attr.DEFAULT_MAX_ROWS)
    chunk_mols = [np.concatenate([np.full(r1 - r0, i, dtype=np.int64) for i, r0, r1 in chunk]) for chunk in chunks]

    def feature():
        return attr.fragment_contributions(model, store, batch_size=BATCH)

    def yardstick():
        with torch.no_grad():
            return torch.cat([model(store.collate(m)).reshape(len(m), -1) for m in chunk_mols], 0).cpu()

    arms = {"feature": feature, "yardstick": yardstick}
    for fn in arms.values():                      # warm-up: code objects, library GEMM selection, allocator
        fn()
        fn()
    ms = {k: [] for k in arms}
    for _ in range(args.repeats):
        for k, fn in arms.items():
            ms[k].append(timed(fn))
    res = feature()
    n_rep = int(res.offsets[-1])
    assert n_rep == int(counts.sum()) == sum(len(m) for m in chunk_mols)
    enc_rows = int((lens["atom"] + lens["edge"]).sum())
    rep_rows = int(((lens["atom"] + lens["edge"]) * counts).sum())
    print(f"{len(store)} ESOL-profile molecules, {n_rep} fragment replicas ({n_rep / len(store):.2f} per molecule); atom + directed-bond rows: "
          f"{enc_rows} once per molecule, {rep_rows} replicated ({rep_rows / enc_rows:.2f} x)")
    print(f"ms per run over all molecules, {args.repeats} repeats, arms alternating, device events:")
    print(f"   feature    fragment_contributions, batch_size {BATCH} ({-(-len(store) // BATCH)} chunks)            {spread(ms['feature'])}")
    print(f"   yardstick  plain forward over the replicated molecules ({len(chunks)} chunks of <= {attr.DEFAULT_MAX_ROWS} rows)   {spread(ms['yardstick'])}")
    f_med, y_med = statistics.median(ms["feature"]), statistics.median(ms["yardstick"])
    print(f"   per molecule: feature {f_med * 1e3 / len(store):.2f} us, yardstick {y_med * 1e3 / len(store):.2f} us; yardstick / feature (medians): {y_med / f_med:.2f} x")

    # the read-out launch and the encoder pass of the first chunk, from the same run
    B = min(BATCH, len(store))
    batch = store.collate(np.arange(B))
    with torch.no_grad():
        x_atoms, x_frags = model.pretrain(batch, edge_outputs=False)[:2]
        plan = plan_for(batch)
        groups = [frag_of[off[i]: off[i + 1]] for i in range(B)]
        ids = [np.unique(g) for g in groups]
        atom_group = torch.from_numpy(np.concatenate(groups).astype(np.int64)).to("cuda:0")
        row_mol = torch.from_numpy(np.concatenate([np.arange(B), np.repeat(np.arange(B), [u.shape[0] for u in ids])]).astype(np.int32)).to("cuda:0")
        row_group = torch.from_numpy(np.concatenate([np.full(B, -1, dtype=np.int64)] + ids)).to("cuda:0")
        out = ops.pool_cat_groups(x_atoms, x_frags, plan, atom_group, row_mol, row_group)
        a, f = ops._seg_struct(plan.segs["mol_atoms"]), ops._seg_struct(plan.segs["mol_frags"])
        st = _stream_ptr(out.device)

        def launch():
            _lib.call("fn_pool_cat_groups_f32", x_atoms.data_ptr(), x_frags.data_ptr(), C.byref(a), C.byref(f), atom_group.data_ptr(),
                      row_mol.data_ptr(), row_group.data_ptr(), row_mol.shape[0], out.data_ptr(), st)
        timed(launch, 20)
        k_us = [timed(launch, 200) * 1e3 for _ in range(args.repeats)]
        enc = lambda: model.pretrain(batch, edge_outputs=False)
        timed(enc, 5)
        e_us = [timed(enc, 20) * 1e3 for _ in range(args.repeats)]
    print(f"first chunk: {B} molecules, {row_mol.shape[0]} read-out rows ({B} unmasked + {row_mol.shape[0] - B} replicas)")
    print(f"   fn_pool_cat_groups_f32, us per launch (200 back-to-back launches per repeat)   {spread(k_us)}")
    print(f"   encoder pass (model.pretrain, edge_outputs=False), us per pass (20 per repeat)  {spread(e_us)}")
    print(f"   read-out / encoder pass (medians): {statistics.median(k_us) / statistics.median(e_us) * 100:.1f} %")
    faster = f_med < y_med
    print("verdict: the feature arm is " + ("FASTER than" if faster else "NOT faster than") + " the yardstick arm")
    return 0 if faster else 1


if __name__ == "__main__":
    sys.exit(main())
