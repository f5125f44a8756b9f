"""The engine's per-block partial sums of the parameter gradients lie row-major (csrc/fn_internal.h: part_at; one contiguous row per
block) and the deferred reduction (csrc/param_grads.hip: rowmajor_sum_32) adds the rows of a column in colmajor_sum_32's order: lane r of
a column's 32 lanes owns rows r, r + 32, .. in four interleaved chains (trips of 128 rows), a remainder loop of 32-row steps, the join
(v + v1) + (v2 + v3), then the xor butterfly.  Its loop edges in the number of partial rows n are therefore 1 (one lane has a row), 32 | 33
(every lane one row | lane 0 a second trip of the remainder loop), 96 | 97 (three remainder trips | the first four-chain trip), 128 | 129.

Tables and who sizes them (tests/launch_geometry_common.py has the block formula):
  part_rd of the atom level   min(ceil(E / 8), key 13) rows: ANY count up to ceil(E / 8) -- the table that lands on every edge exactly
  part_a of a level           nblk of the level's pass under key 23 (one-pass) or key 12 (source pass): ceil(n / 8 r) for some r
  part_a / part_rd of the fragment graph (the molecule-resident tail)   one row per molecule

Reference: the oracle in float64 from the same weights (tests/topologies.py: oracle_finetune), bound |got - ref| <= 1e-4 + 1e-4 |ref|, the
suite's gradient bound.  Two batches of synthetic esol-profile molecules: 3 (E = 120: at most 15 rows; counts it cannot reach fall
back to the largest it can) and 40 (E = 2152: every count up to 269)."""
import pytest
import torch

from tests import launch_geometry_common as G
from tests import topologies as T
from tests.helpers import tuning

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEADS = 4
ATOL = RTOL = 1e-4
COUNTS = (1, 2, 31, 32, 33, 96, 97, 127, 128, 129)
SEEDS = {3: 5, 40: 7}
# attention vectors (a, f: with the edge term's middle block, whose gradient is the column sum of part_rd), edge embeddings
WATCHED = (".a_b", ".a", ".f", ".f_a_b", ".edge_attr_bond_embed.weight", ".edge_attr_bond_embed.bias", ".edge_attr_fbond_embed.weight",
           ".edge_attr_fbond_embed.bias")
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _cpu_batch(n_mols):
    from fragnet_amd import data, synth
    if ("cpu", n_mols) not in _CACHE:
        _CACHE["cpu", n_mols] = data.collate_fn(synth.synth_molecules(n_mols, seed=SEEDS[n_mols], profile="esol"))
    return _CACHE["cpu", n_mols]


def _oracle64(n_mols):
    """(oracle model, float64 logits, float64 gradients) of one training step: computed once, read by every test."""
    if ("f64", n_mols) not in _CACHE:
        gold, res = T.oracle_finetune(_cpu_batch(n_mols), HEADS)
        _CACHE["f64", n_mols] = (gold, res["f64"][0], res["f64"][1])
    return _CACHE["f64", n_mols]


def _model(n_mols):
    from tests.test_gpu_engine_topologies import _model as build
    return build(HEADS, state=_oracle64(n_mols)[0].state_dict())


def _rows(cpu):
    """Rows of the levels whose passes write partial rows, and the atom graph's real edges (= the bond rows)."""
    return dict(bond=int(cpu["node_features_bonds"].shape[0]), atom=int(cpu["x_atoms"].shape[0]),
                fbond=int(cpu["node_features_fbonds"].shape[0]), edges=int(cpu["edge_index"].shape[1]))


def _reachable(n_mols, count):
    """The count itself, or the largest the batch's edge-term table can have."""
    return min(count, -(-_rows(_cpu_batch(n_mols))["edges"] // G.ROWS))


def _setting(count, one_pass=1, tail=1):
    return {G.ONE_BLOCKS: count, G.RD_BLOCKS: count, G.SRC_BLOCKS: count, G.DST_BLOCKS: count, G.BWD_ONE: one_pass, 20: tail}


def partial_row_counts(n_mols, count, tail=1):
    """{table: partial rows} of a backward pass under _setting(count): the launch geometry's own arithmetic."""
    r = _rows(_cpu_batch(n_mols))
    out = {"part_rd[atom]": min(-(-r["edges"] // G.ROWS), count)}
    for lv in ("bond", "atom", "fbond"):
        out[f"part_a[{lv}]"] = G.geometry(r[lv], count)[1]
    if tail:
        out["part_a[frag]"] = out["part_rd[frag]"] = n_mols
    return out


def _watched(want):
    names = [n for n in want if n.endswith(WATCHED)]
    for suffix in WATCHED:
        assert any(n.endswith(suffix) for n in names), f"the reference has no gradient of a parameter {suffix}"
    return names


def _compare(grads, n_mols, what):
    want = _oracle64(n_mols)[2]
    for n in _watched(want):
        got, ref = grads[n].double().cpu(), want[n]
        err = (got - ref).abs()
        print(f"{what} {n}: max|diff| = {float(err.max()):.3e}, max|ref| = {float(ref.abs().max()):.3e}")
        assert bool((err <= ATOL + RTOL * ref.abs()).all()), f"{what} {n}: max|diff| = {float(err.max()):.3e}"


def _step(model, n_mols, setting):
    from fragnet_amd import data
    b = data.batch_to(_cpu_batch(n_mols), DEV)
    model.zero_grad(set_to_none=True)
    with tuning(setting):
        out = model(b)
        torch.nn.functional.mse_loss(out.view(-1), b["y"]).backward()
        torch.cuda.synchronize()
    b["_fragnet_plan"].check()
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


# ----------------------------------------------------------------------------------------------- 1. row-count edges
def test_the_swept_counts_reach_the_reducers_loop_edges():
    """From the geometry's arithmetic: the edge-term table of the 40-molecule batch has exactly every swept count, the tiny batch the
    counts up to 15, and the tail's tables 3 and 40 rows."""
    seen = set()
    for n_mols in SEEDS:
        for c in COUNTS:
            got = partial_row_counts(n_mols, _reachable(n_mols, c))
            assert got["part_rd[atom]"] == _reachable(n_mols, c)
            seen |= set(got.values())
    print(sorted(seen))
    assert {1, 2, 31, 32, 33, 96, 97, 127} <= seen and ({128, 129} & seen)
    assert {3, 40, 15} <= seen
    assert all(partial_row_counts(40, c)["part_rd[atom]"] == c for c in COUNTS)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n_mols", sorted(SEEDS))
def test_gradients_at_partial_row_counts_match_float64(n_mols, count):
    c = _reachable(n_mols, count)
    rows = partial_row_counts(n_mols, c)
    print(rows)
    assert rows["part_rd[atom]"] == c and all(1 <= v <= 4096 for v in rows.values())
    _compare(_step(_model(n_mols), n_mols, _setting(c)), n_mols, f"{n_mols} molecules, {c} rows:")


# ----------------------------------------------------------------------------------------------- 4. two-pass and tail-off paths
@pytest.mark.parametrize("key", [G.BWD_ONE, 20], ids=["two_pass_bwd", "tail_as_separate_launches"])
def test_gradients_on_the_other_engine_paths_match_float64(key):
    """Key 22 = 0: the source pass writes part_a (key 12 sizes it), its launch carries the edge term's blocks.  Key 20 = 0: the fragment
    graph's two passes and its edge term as launches of their own instead of one row per molecule."""
    c = 33
    setting = _setting(c, one_pass=0 if key == G.BWD_ONE else 1, tail=0 if key == 20 else 1)
    assert partial_row_counts(40, c, tail=setting[20])["part_rd[atom]"] == c
    _compare(_step(_model(40), 40, setting), 40, f"key {key} = 0, {c} rows:")


# ----------------------------------------------------------------------------------------------- 2. stale rows
def test_rows_behind_the_written_ones_are_not_read(monkeypatch):
    """One backward workspace for two passes: 129 and more partial rows per table first, then one or two.  The second pass's gradients
    equal, bit for bit, those of the same pass on a workspace filled with NaN -- the reducer reads n rows of the table and nothing
    behind them (the first pass's rows 2 .. 129 lie there)."""
    from fragnet_amd import _lib
    lib = _lib.load()
    real = lib.fn_encoder_backward
    held = {}

    def backward_on_held_workspace(*args):
        args = list(args)
        numel = int(args[-2])
        if "ws" not in held:
            held["ws"] = torch.full((numel,), float("nan"), dtype=torch.float32, device=DEV)
        assert held["ws"].numel() == numel
        args[-3] = held["ws"].data_ptr()
        held["calls"] = held.get("calls", 0) + 1
        return real(*args)

    monkeypatch.setattr(lib, "fn_encoder_backward", backward_on_held_workspace)
    model = _model(40)
    many, few = _setting(129), _setting(1)
    assert min(partial_row_counts(40, 129).values()) > 2 and partial_row_counts(40, 129)["part_rd[atom]"] == 129
    assert {v for k, v in partial_row_counts(40, 1).items() if "frag" not in k} == {1}
    _step(model, 40, many)
    reused = _step(model, 40, few)
    assert held["calls"] == 2
    del held["ws"]
    fresh = _step(model, 40, few)
    assert held["calls"] == 3
    assert set(reused) == set(fresh) and len(fresh) >= 30
    for n in fresh:
        assert torch.isfinite(fresh[n]).all(), n
        assert torch.equal(reused[n], fresh[n]), n
    _compare(fresh, 40, "one row per table:")


# ----------------------------------------------------------------------------------------------- 3. padding path
def test_gradients_of_a_padded_static_batch_match_float64():
    """The 40 molecules staged into static shapes (default margin): the bond level's capacity leaves workgroups whose rows are all
    padding (gat_bwd_one.inc: they write a zero partial row and leave).  Gradients against the float64 oracle of the unpadded batch."""
    from fragnet_amd import data, graphstep, parallel
    gold, _, want = _oracle64(40)
    model = _model(40)
    b = data.batch_to(_cpu_batch(40), DEV)
    opt = parallel.FlatAdam.for_live_parameters(
        model, lambda: torch.nn.functional.mse_loss(model(b).view(-1), b["y"]).backward(), lr=0.0)
    b.pop("_fragnet_plan", None)
    shapes = graphstep.StaticShapes.from_batches([b])
    step = graphstep.GraphedTrainStep(model, opt, shapes, b, loss="regr")
    step(b)
    torch.cuda.synchronize()
    assert step.replays == 1 and step.fallbacks == 0
    step.static.t["_fragnet_plan"].check()
    n_bond, cap_bond = _rows(_cpu_batch(40))["bond"], int(step.static.t["node_features_bonds"].shape[0])
    print(f"bond rows {n_bond}, capacity {cap_bond}")
    assert cap_bond > G.ROWS * -(-n_bond // G.ROWS), "no workgroup of the bond level starts behind the real rows"
    grads = {}
    for name, p in model.named_parameters():
        slot = getattr(p, "_fn_grad_slot", None)
        if slot is not None and name in want:
            flat, off = slot
            grads[name] = flat[off: off + p.numel()].view(p.shape).detach().clone()
    _compare(grads, 40, "padded:")
