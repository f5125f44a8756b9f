"""Hand-built molecule topologies for synth.make_molecule(rng, topology=(n_atoms, bonds, cut)), and what the engine's kernels see of them.

synth.synth_molecules draws valence <= 4 and a handful of fragments: almost every attention row has at most 5 in-edges (12 on the bond
graph) and no molecule crosses a class boundary of the fused fragment tail.  The builders here put rows and molecules ON those boundaries:

  row length (csrc/gat_fwd.inc, gat_bwd_one.inc, gat_bwd_two.inc)   gather tiers 4 / 6 / 8 / 12; the fast path ends at 2 * (32 / heads)
                                                                    in-edges, longer rows take the serial walk
  molecule class (csrc/mol_tail.inc)                                forward LDS path: fragments <= 32 and fragment-graph edges <= 128;
                                                                    backward: fragments <= 24 (32 at eight heads), edges <= 128

``describe`` measures a record with plain loops over its index lists (no code of the package beyond the record itself);
tests/test_topologies_host.py pins the values the GPU tests rely on.
"""
import copy

import numpy as np
import torch

TIERS = (4, 6, 8, 12)                  # source rows gathered per round trip (wide / tier6 / wide8 / wide2)
TAIL_NF_FWD, TAIL_ME = 32, 128         # mol_tail.inc kTailNF, kTailME


def fast_rows(heads):
    """Longest row of the attention kernels' fast path: two edges per lane of a head's 32 / heads lanes."""
    return 2 * (32 // heads)


def tail_nf_bwd(heads):
    """mol_tail.inc tail_bwd_nf<H>()."""
    return 32 if heads == 8 else 24


def star(D, cut_all=False):
    """Centre 0 with D leaves.  Atom-level in-degree of the centre D (+ 1: the self loop the atom level adds), bond-graph in-degree
    2 (D - 1) on the rows of the centre's bonds.  ``cut_all``: D + 1 one-atom fragments, fragment in-degree D, fragment-bond-graph
    in-degree 2 (D - 1)."""
    assert D >= 1
    return D + 1, [(0, i) for i in range(1, D + 1)], [bool(cut_all)] * D


def chain(n, cut=True):
    """n atoms in a row.  Every bond cut: n fragments, 2 (n - 1) fragment-graph edges."""
    assert n >= 2
    return n, [(i, i + 1) for i in range(n - 1)], [bool(cut)] * (n - 1)


def components(sizes):
    """Disjoint chains with every bond cut (size 1: a lone atom).  make_molecule joins every pair of fragments of different components,
    so two components a, b give (a + 1)(b + 1) - 3 connections and a lone first atom plus b, c gives (b + 2)(c + 2) - 6; the
    fragment graph has twice that many edges.  A lone atom must not be the molecule's last atom (the reference rejects that)."""
    sizes = [int(s) for s in sizes]
    assert len(sizes) >= 2 and min(sizes) >= 1 and sizes[-1] >= 2
    bonds, a0 = [], 0
    for s in sizes:
        bonds += [(a0 + i, a0 + i + 1) for i in range(s - 1)]
        a0 += s
    return a0, bonds, [True] * len(bonds)


def two_atoms(cut=False):
    """One bond: the bond graph's two-node special case; cut, the fragment-bond graph's."""
    return 2, [(0, 1)], [bool(cut)]


def _max_count(idx, n):
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    return int(np.bincount(idx, minlength=max(n, 1)).max()) if idx.size else 0


def describe(rec):
    """What the kernels see of one synth.MolRecord.  ``nc``: fragment connections, ``mec``: directed fragment-graph edges (the tail
    kernels' x.mec; = 2 nc except the single-fragment molecule's one (0, 0) edge).  ``in_*``: the longest destination row of each
    attention level as the plan lays it out -- the atom level with its self loop; which row of an index pair is the destination follows
    plan.GraphPlan.from_batch.  ``out_*``: the longest source row (the one-pass backward's source-owner pass walks those)."""
    n, e = int(rec.x_atoms.shape[0]), int(rec.edge_index.shape[1])
    nf, mec = int(rec.n_frags), int(rec.frag_index.shape[1])
    ei, fi = rec.edge_index.numpy(), rec.frag_index.numpy()
    eib, eifb = rec.edge_index_bonds.numpy(), rec.edge_index_fbondg.numpy()
    return dict(
        atoms=n, bonds=e, frags=nf, nc=(mec + 1) // 2, mec=mec, bedges=int(eib.shape[1]), fbedges=int(eifb.shape[1]),
        in_atom=_max_count(ei[1], n) + 1, in_bond=_max_count(eib[0], e), in_frag=_max_count(fi[1], nf), in_fbond=_max_count(eifb[0], mec),
        out_atom=_max_count(ei[0], n) + 1, out_bond=_max_count(eib[1], e), out_frag=_max_count(fi[0], nf), out_fbond=_max_count(eifb[1], mec),
    )


# ---------------------------------------------------------------------------------------------------- the two batches of the GPU tests
# "edges": everything the one-launch plan builder (fn_plan_build_mol) still takes.  Stars whose rows land on both sides of every gather
# tier and of the fast path's end at four and eight heads (16 / 8 in-edges), and on both sides of the fast path's end at two heads on
# the two bond graphs (star(17) / star(18): 32 / 34); chains on both sides of the fused tail's fragment-count classes; the two-atom
# special cases.
#   level        in-degree of the longest row        stars
#   atom         D + 1 (self loop)                   D = 3 .. 13, 15, 16, 17, 18  ->  4 .. 14, 16, 17, 18, 19
#   bond         2 (D - 1): always even              the same stars               ->  4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 28, 30, 32, 34
#   fragment     D                                   cut D = 4 .. 10, 12, 13, 16, 17, 18
#   frag.-bond   2 (D - 1)                           the same cut stars           ->  6, 8, 10, 12, 14, 16, 18, 22, 24, 30, 32, 34
EDGE_STARS = (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 16, 17, 18)
EDGE_CUT_STARS = (4, 5, 6, 7, 8, 9, 10, 12, 13, 16, 17, 18)
EDGE_CHAINS = (12, 24, 25, 32, 33)
# "wide": what pushes the plan to the general builder (fn_plan_build): the fast path's end at one head (64) and at two heads (32) on the
# atom and fragment levels, and at one head on the two bond graphs (star(33) / star(34): 64 / 66).  The component molecules sit here
# too: the fused tail's edge-count class ends at 128 fragment-graph edges, and a molecule with that many has thousands of
# fragment-bond-graph edges (4344 / 4616 / 5472) -- any one of them alone overflows the one-launch builder's 64 KB tile.
WIDE_COMPONENTS = ((1, 5, 8), (3, 16), (8, 8))
WIDE_STARS = (31, 32, 33, 34, 63, 64, 65)
WIDE_CUT_STARS = (31, 32, 33, 34, 63, 64, 65)


def _build(items, seed, pretrain_targets):
    """[(name, MolRecord)] from ``items``: a topology tuple, "ord" (an ordinary synth molecule) or "one" (an ordinary molecule that is one
    fragment), all drawn from one generator."""
    from fragnet_amd import synth
    rng, rng_top = np.random.default_rng(seed), np.random.default_rng(seed + 1)      # topologies from a stream of their own: the same
    out = []                                                                          # molecules with and without pretrain targets
    for name, it in items:
        if it == "ord":
            it = synth.make_topology(rng_top, 6.0, 0.35)
        elif it == "one":
            it = synth.make_topology(rng_top, 5.0, 0.0)
        out.append((name, synth.make_molecule(rng, pretrain_targets=pretrain_targets, topology=it)))
    return out


def edges_batch(pretrain_targets=False, seed=5150):
    """[(name, MolRecord)]: ordinary molecules between the stars (long and short rows share waves), a single-fragment molecule next to
    every chain and two-atom molecule."""
    items = [("ord", "ord")]
    for i, D in enumerate(EDGE_STARS):
        items.append((f"star{D}", star(D)))
        if D in EDGE_CUT_STARS:
            items.append((f"cutstar{D}", star(D, cut_all=True)))
        if i % 2 == 0:
            items.append(("ord", "ord"))
    for n in EDGE_CHAINS:
        items += [(f"chain{n}", chain(n)), ("one", "one")]
    items += [("two", two_atoms()), ("one", "one"), ("two_cut", two_atoms(cut=True)), ("one", "one"), ("ord", "ord")]
    return _build(items, seed, pretrain_targets)


def wide_batch(pretrain_targets=False, seed=6160):
    items = [("ord", "ord")]
    for D in WIDE_STARS:
        items += [(f"star{D}", star(D)), ("ord", "ord")]
        if D in WIDE_CUT_STARS:
            items += [(f"cutstar{D}", star(D, cut_all=True)), ("one", "one")]
    for sizes in WIDE_COMPONENTS:
        items += [("comp" + "_".join(str(s) for s in sizes), components(sizes)), ("one", "one")]
    return _build(items, seed, pretrain_targets)


BATCHES = {"edges": edges_batch, "wide": wide_batch}
CFG = dict(n_classes=1, num_layer=2, drop_ratio=0.0, h1=64, h2=64, h3=64, h4=32, act="relu", edge_features=17)      # + num_heads
LEVELS = ("atom", "bond", "frag", "fbond")


def row_lengths(recs):
    """{level: set of the longest destination-row lengths of the records}, {level: ... source rows}."""
    ds = [describe(r) for _, r in recs]
    return ({lv: {d["in_" + lv] for d in ds} for lv in LEVELS}, {lv: {d["out_" + lv] for d in ds} for lv in LEVELS})


def required_rows(name, heads):
    """{level: row lengths the batch ``name`` must hold for ``heads``}: both sides of every gather tier, and both sides of the fast
    path's end where the batch reaches it (the two bond graphs only have even rows, 2 (D - 1)).  Where the fast path ends below the
    batch's shortest star (the wide batch at four and eight heads) every star row takes the serial walk: its longest rows are required."""
    fast = fast_rows(heads)
    if name == "edges":
        odd = {4, 5, 6, 7, 8, 9, 12, 13} | ({fast, fast + 1} if fast + 1 <= 17 else set())
        even = {4, 6, 8, 10, 12, 14} | ({fast, fast + 2} if fast + 2 <= 34 else set())
    else:
        odd = {fast, fast + 1} if fast >= 32 else {64, 65}
        even = {fast, fast + 2} if fast >= 64 else {124, 126}
    return dict(atom=odd, frag=odd, bond=even, fbond=even)


def collate(recs, pretrain=False):
    from fragnet_amd import data
    return (data.collate_fn_pt if pretrain else data.collate_fn)([r for _, r in recs])


def as_double(batch):
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}


def oracle_finetune(batch, heads, seed=11):
    """The oracle's FragNetFineTune (CFG, ``heads``) on the CPU batch, in float32 and -- from the same weights -- in float64: one
    training step without dropout, MSE loss.  Returns (float32 model, {"f32" | "f64": (logits, {name: gradient})})."""
    from oracle import fragnet_ref as ref
    torch.manual_seed(seed)
    gold = ref.FragNetFineTune(**CFG, num_heads=heads).train()
    res = {}
    for tag, net, b in (("f64", copy.deepcopy(gold).double(), as_double(batch)), ("f32", gold, batch)):
        out = net(b)
        torch.nn.functional.mse_loss(out.view(-1), b["y"]).backward()
        res[tag] = (out.detach(), {n: p.grad.detach() for n, p in net.named_parameters() if p.grad is not None})
    return gold, res


def tail_class(d, heads):
    """(forward, backward) path of the fused fragment tail for a molecule described by ``d``: "lds" or "global"
    (mol_tail.inc: k_tail_fwd / k_tail_bwd class selection; the kernels' x.nc equals x.mec)."""
    fwd = d["frags"] <= TAIL_NF_FWD and d["mec"] <= TAIL_ME
    bwd = d["frags"] <= tail_nf_bwd(heads) and d["mec"] <= TAIL_ME
    return ("lds" if fwd else "global"), ("lds" if bwd else "global")


def assert_batch_claims(name, recs, heads):
    """A batch that lost a boundary case must fail its test, not pass it: the rows of every required length at every level (destination
    and source rows), the tail class of every named molecule, ordinary molecules between the special ones.  Returns the descriptions."""
    ins, outs = row_lengths(recs)
    for lv, want in required_rows(name, heads).items():
        assert want <= ins[lv], f"{name}, {heads} heads, {lv} level: no destination row of {sorted(want - ins[lv])} edges"
        assert want <= outs[lv], f"{name}, {heads} heads, {lv} level: no source row of {sorted(want - outs[lv])} edges"
    ds = {n: describe(r) for n, r in recs}
    cls = {n: tail_class(d, heads) for n, d in ds.items()}
    mid = ("lds", "lds") if heads == 8 else ("lds", "global")           # 25 .. 32 fragments: the backward's tile is smaller below eight heads
    if name == "edges":
        want = {"chain12": ("lds", "lds"), "chain24": ("lds", "lds"), "chain25": mid, "chain32": mid, "chain33": ("global", "global"),
                "cutstar17": ("lds", "lds"), "two": ("lds", "lds"), "two_cut": ("lds", "lds")}
        assert [ds[n]["frags"] for n in ("chain24", "chain25", "chain32", "chain33")] == [24, 25, 32, 33]
    else:
        want = {"comp1_5_8": ("lds", "lds"), "comp3_16": ("global", "global"), "comp8_8": ("global", "global"),
                "cutstar31": mid, "cutstar32": ("global", "global"), "cutstar65": ("global", "global")}
        assert [ds[n]["mec"] for n in ("comp1_5_8", "comp3_16", "comp8_8")] == [128, 130, 156]
        assert (ds["cutstar31"]["frags"], ds["cutstar32"]["frags"]) == (32, 33)
    for n, c in want.items():
        assert cls[n] == c, f"{name}, {heads} heads: {n} is tail class {cls[n]}, the test needs {c}"
    names = [n for n, _ in recs]
    special = [i for i, n in enumerate(names) if n not in ("ord", "one")]
    assert names[0] == "ord" and names[-1] in ("ord", "one")
    assert all(any(names[j] in ("ord", "one") for j in (i - 2, i - 1, i + 1, i + 2) if 0 <= j < len(names)) for i in special)
    for i, n in enumerate(names):                                        # a single-fragment molecule next to each of these
        if n.startswith(("chain", "comp", "two")):
            assert names[i + 1] == "one" and int(recs[i + 1][1].n_frags) == 1, n
    return ds


def plan_row_lengths(plan):
    """{level: set of destination-row lengths} read from a built GraphPlan's row pointers (the rows the kernels walk)."""
    out = {}
    for name, role, ib, sb, items, segs in plan.task_meta:
        if role == 1:
            rp = plan.rowptr[sb: sb + segs + 1].cpu().numpy().astype(np.int64)
            out[name] = set(np.diff(rp).tolist())
    return out
