"""Per-batch graph plan: every destination-sorted CSR the four levels, the atom->fragment sum and
the pooling need, built by ONE fn_plan_build call (5 small kernels) and reused by all layers,
forward and backward.

Which row of each index tensor is the destination follows the reference's unpacking:
``target, source = edge_index_bonds_graph`` / ``edge_index_fbond_graph`` (gat2.py:138,239) but
``source, target = edge_index`` / ``frag_index`` (gat2.py:187,283).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

from . import _lib
from ._lib import CsrTask, GatPlan, ROLE_DST, ROLE_PLAIN, ROLE_SRC


def _stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _require_cuda_i64(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise _lib.FragnetHipError(f"{name} must live on the GPU: fragnet_amd has no CPU path (got {t.device})")
    if t.dtype != torch.int64:
        raise TypeError(f"{name} must be int64, got {t.dtype}")


@dataclass
class Segments:
    """A plain CSR (segment sum / pooling)."""
    rowptr: torch.Tensor      # int32 view [n_seg+1] (global positions)
    perm: torch.Tensor        # int32 view [items]
    pos_base: int
    n_seg: int
    n_items: int
    index: torch.Tensor       # the int64 key (for the gather backward)


MOL_PLAN_ARG_BYTES = 3072      # LDS the one-launch plan builder keeps for its argument block and extents (see GraphPlan._build_mol)


def mol_plan_slice_words(items: int, nodes: int) -> int:
    """LDS words of one CSR task's slice in fn_plan_build_mol's tile (mp_slice_words, csrc/mol_plan.hip)."""
    return 2 * (max(nodes, 1) + 1) + (3 * max(items, 1) + 1) // 2 + 1


def mol_plan_fits(slice_words: int) -> bool:
    """Whether task slices of that many words leave room for the builder's argument block and extents in its 64 KB tile."""
    return slice_words * 4 <= 64 * 1024 - MOL_PLAN_ARG_BYTES


@dataclass
class Level:
    """One attention level: destination CSR + source CSR."""
    c: GatPlan                # ctypes struct handed to the kernels
    n: int
    m: int
    m_real: int
    keep: tuple               # tensors the raw pointers in ``c`` point into


class GraphPlan:
    def __init__(self, specs: List[dict], device, mol_layout: Optional[dict] = None):
        """specs: list of dicts(kind='gat'|'seg', name, ...) -- use GraphPlan.from_batch / .segments_only.
        ``mol_layout`` (molecule-contiguous batches): dict(offsets, n_mols, counts_dev, cap, mod, max_per_mol, hint) and specs that
        carry ``nodes`` / ``items`` (index-space names) -> fn_plan_build_mol, one launch."""
        lib = _lib.load()
        self.device = device
        tasks = (CsrTask * _lib.FN_MAX_TASKS)()
        nt = 0
        layout = []
        keep = []
        for sp in specs:
            if sp["kind"] == "gat":
                dst, src = sp["dst"], sp["src"]
                _require_cuda_i64(dst, sp["name"])
                if not (dst.is_contiguous() and src.is_contiguous()):
                    dst, src = dst.contiguous(), src.contiguous()
                keep += [dst, src]
                m_real = int(dst.numel())
                for role, key, other, partner in ((ROLE_DST, dst, src, nt + 1), (ROLE_SRC, src, dst, nt)):
                    tasks[nt] = CsrTask(key.data_ptr(), other.data_ptr(), m_real, int(sp["n_loops"]), int(sp["n"]),
                                        0, 0, role, partner)
                    nt += 1
                layout.append(("gat", sp["name"], nt - 2, sp))
            else:
                key = sp["key"]
                _require_cuda_i64(key, sp["name"])
                key = key.contiguous()
                keep.append(key)
                tasks[nt] = CsrTask(key.data_ptr(), None, int(key.numel()), 0, int(sp["n_seg"]), 0, 0, ROLE_PLAIN, -1)
                nt += 1
                layout.append(("seg", sp["name"], nt - 1, sp, key))
            if nt > _lib.FN_MAX_TASKS:
                raise ValueError("too many CSR tasks for one plan")
        tot_items, tot_segs = C.c_int64(), C.c_int64()
        _lib.check(lib.fn_plan_layout(tasks, nt, C.byref(tot_items), C.byref(tot_segs)), "fn_plan_layout")
        ti, ts = tot_items.value, tot_segs.value
        # one int32 arena: rowptr | perm | aux_a | aux_b | aux_c | workspace(cursor, tmp, status, block sums)
        ta = max(ti, 1)                 # keep every region non-empty so its pointer is never null
        ws_zeroed = ts + ti + 4 + 2 * (ts // 2048 + 1) + 2                  # FN_PLAN_WS_ZEROED; FN_PLAN_WS = that + ti (never zeroed)
        arena = torch.empty(ts + 1 + 4 * ta + ws_zeroed + ti, dtype=torch.int32, device=device)
        self._arena = arena
        self.rowptr = arena[: ts + 1]
        self.perm = arena[ts + 1: ts + 1 + ta]
        self.aux_a = arena[ts + 1 + ta: ts + 1 + 2 * ta]
        self.aux_b = arena[ts + 1 + 2 * ta: ts + 1 + 3 * ta]
        self.aux_c = arena[ts + 1 + 3 * ta: ts + 1 + 4 * ta]
        ws = arena[ts + 1 + 4 * ta:]
        self._status = ws[ts + ti: ts + ti + 1]
        # regions fn_plan_build needs zeroed: a captured step has its staging launch do it (graphstep, PREZEROED context)
        self.zero_regions = [(self.rowptr.data_ptr(), ts + 1), (ws.data_ptr(), ws_zeroed)]
        self.prezeroed = bool(_PREZEROED)
        if self.prezeroed:
            _BUILT.append(self)
        self.mol_built = False
        if mol_layout is not None and self._build_mol(lib, tasks, nt, specs, mol_layout, ws, device):
            self.mol_built = True
            self.zero_regions = [(self._status.data_ptr(), 1)]      # the one-launch builder only needs a clean status word
        else:
            _lib.check(lib.fn_plan_build(tasks, nt, self.rowptr.data_ptr(), self.perm.data_ptr(), self.aux_a.data_ptr(),
                                         self.aux_b.data_ptr(), self.aux_c.data_ptr(), ws.data_ptr(),
                                         _lib.PLAN_PREZEROED if self.prezeroed else 0, _stream_ptr(device)),
                       "fn_plan_build")
        self._keep = keep
        # (name, role, item_base, seg_base, items, segments) per CSR task: which slices of the arena mean what (tests, tools)
        self.task_meta = [(ent[1], int(tasks[ent[2] + q].role), int(tasks[ent[2] + q].item_base), int(tasks[ent[2] + q].seg_base),
                           int(tasks[ent[2] + q].n_real + tasks[ent[2] + q].n_loops), int(tasks[ent[2] + q].n_seg))
                          for ent in layout for q in range(2 if ent[0] == "gat" else 1)]
        self._sorted = {}
        self.pending = {}           # level name -> raw edge attribute whose sorted copy fn_encoder_forward still has to fill
        self.levels: Dict[str, Level] = {}
        self.segs: Dict[str, Segments] = {}
        for ent in layout:
            if ent[0] == "gat":
                _, name, t0, sp = ent
                d, s = tasks[t0], tasks[t0 + 1]
                m = int(d.n_real + d.n_loops)
                c = GatPlan(self.rowptr.data_ptr() + 4 * d.seg_base, self.perm.data_ptr() + 4 * d.item_base,
                            self.aux_a.data_ptr() + 4 * d.item_base, self.rowptr.data_ptr() + 4 * s.seg_base,
                            self.aux_a.data_ptr() + 4 * s.item_base, self.aux_b.data_ptr() + 4 * s.item_base,
                            self.aux_b.data_ptr() + 4 * d.item_base, self.aux_c.data_ptr() + 4 * d.item_base,
                            int(d.item_base), int(s.item_base), int(d.n_seg), m, int(d.n_real))
                self.levels[name] = Level(c, int(d.n_seg), m, int(d.n_real), (self,))
            else:
                _, name, t0, sp, key = ent
                t = tasks[t0]
                self.segs[name] = Segments(self.rowptr[t.seg_base: t.seg_base + t.n_seg + 1],
                                           self.perm[t.item_base: t.item_base + t.n_real], int(t.item_base),
                                           int(t.n_seg), int(t.n_real), key)

    def _build_mol(self, lib, tasks, nt, specs, layout, ws, device) -> bool:
        """fn_plan_build_mol for a molecule-contiguous batch; False = not applicable (the general builder runs)."""
        off = layout["offsets"]
        if not MOL_PLAN or off is None or not off.is_cuda or off.dtype != torch.int32 or layout.get("max_per_mol") is None:
            return False
        n_mols = layout["n_mols"]
        if off.shape != (len(SPACES), n_mols + 1) or not off.is_contiguous():
            return False
        ml = _lib.MolLayout()
        ml.offsets, ml.n_spaces, ml.n_mols = off.data_ptr(), len(SPACES), n_mols
        counts = layout.get("counts_dev")
        ml.counts_dev = None if counts is None else counts.data_ptr()
        ti = 0
        for sp in specs:
            if "nodes" not in sp:
                return False
            ns, it = SPACES.index(sp["nodes"]), SPACES.index(sp["items"])
            for _ in range(2 if sp["kind"] == "gat" else 1):
                ml.node_space[ti], ml.item_space[ti] = ns, it
                ti += 1
        for s, name in enumerate(SPACES):
            ml.cap[s] = layout["cap"][name]
            ml.pad_mod[s] = max(1, layout["mod"].get(name, 1))
            ml.max_per_mol[s] = layout["max_per_mol"][name]
            ml.pad_hint[s] = layout["hint"].get(name, 0)
        words = 0
        for i in range(nt):       # the LDS tile of csrc/mol_plan.hip: 2 (nodes + 1) + 1.5 items words per task
            items = ml.max_per_mol[ml.item_space[i]] + (ml.max_per_mol[ml.node_space[i]] if tasks[i].n_loops else 0)
            words += mol_plan_slice_words(items, ml.max_per_mol[ml.node_space[i]])
            if items > 65535:
                return False
        # fn_plan_build_mol's tile also holds the argument block and the molecule's extents (2 * FN_MAX_SPACES + kMpArgWords words,
        # csrc/mol_plan.hip:410, about 2.7 KB): the same budget here, with 3 KB set aside for them
        if not mol_plan_fits(words):
            return False             # a molecule too large for the tile: the general builder takes the batch
        self._keep_layout = (off, counts)
        rc = lib.fn_plan_build_mol(tasks, nt, C.byref(ml), self.rowptr.data_ptr(), self.perm.data_ptr(), self.aux_a.data_ptr(),
                                   self.aux_b.data_ptr(), self.aux_c.data_ptr(), ws.data_ptr(),
                                   _lib.PLAN_PREZEROED if self.prezeroed else 0, _stream_ptr(device))
        if rc == _lib.FN_EUNSUPPORTED:
            return False             # "does not fit / not supported" is decided before anything is launched: not applicable, not an error
        _lib.check(rc, "fn_plan_build_mol")
        return True

    def sorted_attr(self, name: str, x: torch.Tensor, defer: bool = False) -> torch.Tensor:
        """Raw edge attribute of level ``name`` permuted into destination-sorted order, once per batch
        (the reference feeds the same edge_attr_bonds / edge_attr_fbonds to every layer, gat2.py:430,433).
        ``defer``: only allocate the buffer and remember ``x`` in ``self.pending[name]``; the caller hands both to
        fn_encoder_forward, which does the permutation inside its prologue launch (engine.py)."""
        key = (name, x.data_ptr(), x._version)
        hit = self._sorted.get(name)
        if hit is not None and hit[0] == key:
            return hit[1]
        lv = self.levels[name]
        if not x.is_cuda or x.dtype != torch.float32:
            raise _lib.FragnetHipError("edge attributes must be float32 GPU tensors")
        x = x.contiguous()
        K = x.shape[1] if x.dim() == 2 else 1
        if x.numel() != lv.m_real * K:
            raise ValueError(f"edge attribute of level {name} has {x.shape[0]} rows, the plan has {lv.m_real} edges")
        out = torch.empty((K, lv.m), dtype=torch.float32, device=x.device)      # [K][m]: a lane's two edges are adjacent
        if defer:
            self.pending[name] = x
        else:
            _lib.call("fn_sort_edge_attr_f32", x.data_ptr(), K, C.byref(lv.c), out.data_ptr(), _stream_ptr(x.device))
        self._sorted[name] = (key, out)
        return out

    def check(self):
        """Synchronising validation: raises if any index was outside its segment range."""
        st = int(self._status.item())
        if st & 1:
            raise IndexError("graph plan: an index tensor holds values outside [0, num_nodes)")
        if st & 2:
            raise IndexError("graph plan: the batch is not molecule-contiguous (an edge joins nodes of different molecules, or "
                             "molecules are interleaved); the fused encoder needs collate_fn's layout (dataset/data.py:877-948)")
        if st & 4:
            raise IndexError("graph plan: a molecule is larger than CollatedBatch.max_per_mol says (fn_plan_build_mol's LDS tile)")

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_batch(cls, batch: Dict[str, torch.Tensor], n_mols: Optional[int] = None, edge_ends: bool = False):
        """Plan for the reference's batch dict.  ``edge_ends`` adds the two CSRs the
        pretrain bond-length head's gather backward needs."""
        dev = batch["x_atoms"].device
        N = batch["x_atoms"].shape[0]
        E = batch["node_features_bonds"].shape[0]
        F = batch["x_frags"].shape[0]
        EF = batch["node_features_fbonds"].shape[0]
        if n_mols is None:
            n_mols = batch_n_mols(batch)
        ei, fi = batch["edge_index"], batch["frag_index"]
        eib, eifb = batch["edge_index_bonds_graph"], batch["edge_index_fbonds"]
        if ei.shape[1] != E:
            raise ValueError("edge_index and node_features_bonds disagree on the number of directed bonds")
        if fi.shape[1] != EF:
            raise ValueError("frag_index and node_features_fbonds disagree on the number of fragment edges")
        # the two molecule-membership CSRs (mol_atoms, mol_frags) are read by the readout (ops.pool_cat: gat2.py:820-823) of
        # every model, and drive the molecule-resident kernels when those are switched on
        specs = [
            dict(kind="gat", name="bond", dst=eib[0], src=eib[1], n=E, n_loops=0, nodes="edge", items="bedge"),
            dict(kind="gat", name="atom", dst=ei[1], src=ei[0], n=N, n_loops=N, nodes="atom", items="edge"),
            dict(kind="gat", name="fbond", dst=eifb[0], src=eifb[1], n=EF, n_loops=0, nodes="fedge", items="fbedge"),
            dict(kind="gat", name="frag", dst=fi[1], src=fi[0], n=F, n_loops=0, nodes="frag", items="fedge"),
            dict(kind="seg", name="a2f", key=batch["atom_to_frag_ids"], n_seg=F, nodes="frag", items="atom"),
            dict(kind="seg", name="mol_atoms", key=batch["batch"], n_seg=n_mols, nodes="mol", items="atom"),
            dict(kind="seg", name="mol_frags", key=batch["frag_batch"], n_seg=n_mols, nodes="mol", items="frag"),
        ]
        if edge_ends:
            specs += [dict(kind="seg", name="edge_src", key=ei[0], n_seg=N, nodes="atom", items="edge"),
                      dict(kind="seg", name="edge_dst", key=ei[1], n_seg=N, nodes="atom", items="edge")]
        contiguous = bool(getattr(batch, "mol_contiguous", False))               # CollatedBatch: collate_fn's layout
        layout = None
        if contiguous and getattr(batch, "offsets", None) is not None and getattr(batch, "max_per_mol", None) is not None:
            cap = {"atom": N, "edge": E, "bedge": eib.shape[1], "frag": F, "fedge": EF, "fbedge": eifb.shape[1], "mol": n_mols}
            pad = getattr(batch, "pad", None) or {}
            layout = dict(offsets=batch.offsets, n_mols=n_mols, counts_dev=batch.get(REAL_MOLS_KEY), cap=cap,
                          mod=pad.get("mod", {}), max_per_mol=batch.max_per_mol, hint=pad.get("hint", {}))
        plan = cls(specs, dev, layout)
        plan.n_mols = n_mols
        plan.mol_contiguous = contiguous
        plan.real_mols = batch.get(REAL_MOLS_KEY)      # int32 [1] on the device when the batch is padded to static shapes
        return plan

    @classmethod
    def gcn_specs(cls, batch: Dict[str, torch.Tensor], n_mols: int) -> List[dict]:
        """The CSR tasks model_version gcn2 reads (gcn2.py:48-65, 187-188): the atom graph with its self loops, the fragment graph,
        the atom -> fragment sum and the two molecule-membership sums of the read-out.  No bond-graph and no fragment-bond-graph task:
        those hold most of a batch's items and this model never looks at them."""
        N, F = batch["x_atoms"].shape[0], batch["x_frags"].shape[0]
        ei, fi = batch["edge_index"], batch["frag_index"]
        return [
            dict(kind="gat", name="atom", dst=ei[1], src=ei[0], n=N, n_loops=N),
            dict(kind="gat", name="frag", dst=fi[1], src=fi[0], n=F, n_loops=0),
            dict(kind="seg", name="a2f", key=batch["atom_to_frag_ids"], n_seg=F),
            dict(kind="seg", name="mol_atoms", key=batch["batch"], n_seg=n_mols),
            dict(kind="seg", name="mol_frags", key=batch["frag_batch"], n_seg=n_mols),
        ]

    @classmethod
    def for_gcn(cls, batch: Dict[str, torch.Tensor], n_mols: Optional[int] = None):
        """The reduced plan of model_version gcn2 (``gcn_specs``), built by the general builder (fn_plan_build)."""
        if n_mols is None:
            n_mols = batch_n_mols(batch)
        plan = cls(cls.gcn_specs(batch, n_mols), batch["x_atoms"].device)
        plan.n_mols = n_mols
        plan.mol_contiguous = bool(getattr(batch, "mol_contiguous", False))
        plan.real_mols = None
        return plan

    @classmethod
    def segments_only(cls, index: torch.Tensor, n_seg: int):
        plan = cls([dict(kind="seg", name="s", key=index, n_seg=n_seg)], index.device)
        return plan


MOL_PLAN = os.environ.get("FRAGNET_MOL_PLAN", "1") != "0"      # molecule-contiguous batches with offsets: fn_plan_build_mol (False / FRAGNET_MOL_PLAN=0: always the general builder; A/B, tests)
_PREZEROED = False      # True only while graphstep captures its step: plans built then skip their zeroing launch
_BUILT = []             # the plans built inside the current prezeroed_plans() context


class prezeroed_plans:
    """Context: plans built inside skip fn_plan_build's zeroing launch; the caller zeroes ``plan.zero_regions`` on the same
    stream before every use (GraphedTrainStep: the staging launch in front of each replay)."""

    def __enter__(self):
        global _PREZEROED
        self._old, _PREZEROED = _PREZEROED, True
        _BUILT.clear()
        return self

    def __exit__(self, *exc):
        global _PREZEROED
        _PREZEROED = self._old
        self.plans = list(_BUILT)
        _BUILT.clear()


SPACES = ("atom", "edge", "bedge", "frag", "fedge", "fbedge", "mol")      # index spaces of a batch (graphstep.COUNT_FIELD)


class CollatedBatch(dict):
    """A batch dict in collate_fn's layout (reference dataset/data.py:877-948): molecules are concatenated, so the atoms,
    directed bonds, fragments, fragment connections and the edges of the four graphs of molecule i are contiguous index ranges.
    data.collate_fn(_pt), FlatMolStore.collate, data.batch_to and StaticBatch return it; same keys and values as the plain
    dict.  The encoder engine runs its molecule-resident kernels (csrc/mol_tail.inc) only for such batches: a hand-built plain
    dict makes no promise about its layout and takes the general per-level kernels.

    Attributes (not dict keys: the key set stays the reference's): ``offsets`` int32 [len(SPACES), B + 1], first index of
    molecule i in each index space -- the collate's cumulative counts; with it (on the batch's device) the graph plan is built
    by one molecule-resident launch (fn_plan_build_mol) instead of four grid-wide passes.  ``max_per_mol``: {space: largest
    extent of one molecule} (python ints; sizes that kernel's LDS tile).  ``pad``: set by StaticBatch, the padding rule of a
    static-shape batch {"cap": {space: n}, "mod": {space: n}, "hint": {space: n}}."""

    mol_contiguous = True
    offsets = None
    max_per_mol = None
    pad = None

    def like(self, items):
        """A batch with the same layout attributes and the given items (moved / re-keyed tensors)."""
        out = type(self)(items)
        out.offsets, out.max_per_mol, out.pad = self.offsets, self.max_per_mol, self.pad
        return out


def mol_offsets(counts: Dict[str, "torch.Tensor"]) -> "torch.Tensor":
    """int32 [len(SPACES), B + 1] from per-molecule counts (int64 tensors [B] per space except "mol")."""
    B = counts["atom"].numel()
    dev = counts["atom"].device
    off = torch.zeros((len(SPACES), B + 1), dtype=torch.int32, device=dev)
    for s, name in enumerate(SPACES):
        if name == "mol":
            off[s] = torch.arange(B + 1, dtype=torch.int32, device=dev)
        else:
            off[s, 1:] = torch.cumsum(counts[name], 0).to(torch.int32)
    return off


PLAN_KEY = "_fragnet_plan"
REAL_MOLS_KEY = "_real_mols"      # StaticBatch: device-side count of the real molecules of a padded batch
REAL_ATOMS_KEY = "_real_atoms"    # StaticBatch.add_count("atom"): device-side count of its real atoms (the masked-atom sampler reads it)
LIVE_MOLS_KEY = "_live_mols"      # StaticBatch: python int, molecule rows >= this are padding in EVERY batch (capacity - slack)
N_MOLS_KEY = "_n_mols"            # factored pair batches (data.collate_fn_*_factored): python int, the molecule count -- y has one entry per PAIR there


def batch_n_mols(batch) -> int:
    """The molecule count of a batch dict: what the batch carries (``N_MOLS_KEY``), else one per entry of ``y``, else (a host
    synchronisation) the largest molecule id."""
    if N_MOLS_KEY in batch:
        return int(batch[N_MOLS_KEY])
    return batch["y"].shape[0] if "y" in batch else int(batch["batch"].max()) + 1


def plan_for(batch: Dict[str, torch.Tensor], edge_ends: bool = False) -> GraphPlan:
    """The plan is cached on the batch dict, so one batch builds it once even if several modules ask."""
    plan = batch.get(PLAN_KEY)
    if plan is None or (edge_ends and "edge_src" not in plan.segs):
        plan = GraphPlan.from_batch(batch, edge_ends=edge_ends)
        batch[PLAN_KEY] = plan
    return plan


GCN_PLAN_KEY = "_fragnet_gcn_plan"


def gcn_plan_for(batch: Dict[str, torch.Tensor]) -> GraphPlan:
    """``GraphPlan.for_gcn`` of the batch, cached on the batch dict under a key of its own (the full plan's key stays the full plan's)."""
    plan = batch.get(GCN_PLAN_KEY)
    if plan is None:
        plan = GraphPlan.for_gcn(batch)
        batch[GCN_PLAN_KEY] = plan
    return plan
