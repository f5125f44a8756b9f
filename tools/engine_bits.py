"""Bit fingerprints of the encoder engine: one line per case, the case name and a SHA-256 of every output and of every parameter
gradient.  Run it on two builds of the library and diff the outputs: a change of the engine's HOST code (which launches it
enqueues, with which arguments, in which order) that is meant to leave the arithmetic alone must leave every line alone.

    python tools/engine_bits.py > bits.txt

Cases (24 synthetic molecules, profile esol, fixed Philox offset): every head count, the three model versions, 1 / 2 / 3 / 6
layers (six layers make the deferred-reduction queue flush in mid-pass), training with and without dropout, evaluation with
gradients and under no_grad, the static-shape padded step (padding skip, Adam rider), the masked pass, the attention read-out, the
input-gradient call, single-fragment molecules (with and without their placeholder connection), one molecule, the training
step under the tuning keys that select another path of the host code, and the ways of the encoder's Python front: the input gate
(a batch with keep_atoms, and FragNetPreTrainMasked2), the level-by-level route of the three model versions (use_engine=False),
of FragNetFineTuneViz (training mode; evaluation with use_engine=False) and of a plain model with return_attentions on a layer.

    python tools/engine_bits.py --calls > calls.txt

prints, per case, the fn_* entry points of the library in call order instead (runs of one name as ``name xN``): the host code's
own trace, recorded by wrapping the ctypes functions of ``_lib.load()`` in this process."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from fragnet_amd import _lib, data, graphstep, synth
from fragnet_amd import gradient_attribution as ga
from fragnet_amd import model as M
from fragnet_amd import parallel
from fragnet_amd import viz_model as V

DEV = "cuda:0"
OFFSET = 999
DEFAULTS = {7: 1, 14: 2, 20: 1, 22: 1, 28: 0, 33: 1}


def digest(items):
    """SHA-256 over (name, shape, bytes) of tensors / arrays in the given order; None entries are named too."""
    h = hashlib.sha256()
    for name, t in items:
        h.update(name.encode())
        if t is None:
            h.update(b"<none>")
            continue
        a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        h.update(str(a.shape).encode() + str(a.dtype).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


CALLS = None        # --calls: the names of the library calls since the last report


def record_calls():
    global CALLS
    CALLS = []
    lib = _lib.load()
    for name in _lib.SIGNATURES:
        if name == "fn_last_error":
            continue

        def counted(*a, _fn=getattr(lib, name), _name=name):
            CALLS.append(_name)
            return _fn(*a)
        setattr(lib, name, counted)


def report(name, items):
    torch.cuda.synchronize()
    if CALLS is None:
        print(f"{name:34s} {digest(items)}", flush=True)
        return
    runs = []
    for c in CALLS:
        if runs and runs[-1][0] == c:
            runs[-1][1] += 1
        else:
            runs.append([c, 1])
    print(f"{name:34s} " + " ".join(c if n == 1 else f"{c} x{n}" for c, n in runs), flush=True)
    CALLS.clear()


def net_for(heads=4, layers=3, drop=0.0, cls=M.FragNetFineTune, seed=0):
    torch.manual_seed(seed)
    return cls(n_classes=1, num_layer=layers, num_heads=heads, drop_ratio=drop, h1=32, h2=32, h3=32, h4=32, act="relu",
               fthead="FTHead3").to(DEV)


def encoder_pass(name, net, batch, train=True, grad=True):
    """the encoder's outputs and, with grad, every parameter gradient of sum(mean(out^2)) over the first four"""
    net.train(train)
    net.zero_grad(set_to_none=True)
    net.pretrain.rng.offset = OFFSET
    batch = dict(batch)
    batch.pop("_fragnet_plan", None)
    with torch.set_grad_enabled(grad):
        outs = net.pretrain(batch)
        items = [(f"out{i}", t) for i, t in enumerate(outs)]
        if grad:
            sum(t.square().mean() for t in outs[:4] if t is not None and t.numel()).backward()
            items += [(n, p.grad) for n, p in net.named_parameters()]
    report(name, items)


def graph_step(name, batches, drop):
    """the captured static-shape step of tests/test_graphstep.py (padded batch, Adam in the graph, the head's slice riding)"""
    net = net_for(layers=2, drop=drop, seed=11).train()
    net.pretrain.rng.seed = 5

    def probe():
        torch.nn.functional.mse_loss(net(dict(batches[0])).view(-1), batches[0]["y"]).backward()
    opt = parallel.FlatAdam.for_live_parameters(net, probe, lr=1e-3, eps=1e-4)
    net.pretrain.rng.offset = 0
    shapes = graphstep.StaticShapes.from_batches(batches, margin=0.05)
    step = graphstep.GraphedTrainStep(net, opt, shapes, dict(batches[0]), loss="regr")
    losses = [step(dict(batches[i % len(batches)])).clone() for i in range(3)]
    assert step.replays == 3 and step.fallbacks == 0
    report(name, [(f"loss{i}", l) for i, l in enumerate(losses)] + [("grad", opt.grad), ("flat", opt.flat), ("v", opt.exp_avg_sq)])


def single_fragment_batch(n, strip):
    rng = np.random.default_rng(11)
    mols = [synth.make_molecule(rng, mu=6, p_cut=0.0) for _ in range(n)]
    assert all(int(m.n_frags) == 1 for m in mols)
    b = dict(data.collate_fn(mols))
    if strip:       # without the placeholder connection rows: EF == 0 (tests/test_gpu_attn_readout.py)
        b["frag_index"] = b["frag_index"][:, :0].contiguous()
        b["node_features_fbonds"] = b["node_features_fbonds"][:0].contiguous()
        b["edge_index_fbonds"] = b["edge_index_fbonds"][:, :0].contiguous()
        b["edge_attr_fbonds"] = b["edge_attr_fbonds"][:0].contiguous()
    return data.batch_to(b, DEV)


def main():
    mols = synth.synth_molecules(24, seed=17, profile="esol")
    batch = data.batch_to(data.collate_fn(mols), DEV)

    for heads in (1, 2, 4, 8):
        encoder_pass(f"gat2_heads{heads}", net_for(heads=heads), batch)
    encoder_pass("gat2_lite_heads4", net_for(cls=M.FragNetFineTuneLite), batch)
    encoder_pass("gat2_edge_heads4", net_for(cls=M.FragNetFineTuneEdge), batch)
    encoder_pass("gat2_edge_heads4_dropout", net_for(cls=M.FragNetFineTuneEdge, drop=0.1), batch)
    encoder_pass("gat2_edge_heads1", net_for(heads=1, cls=M.FragNetFineTuneEdge), batch)
    for layers in (1, 2, 3, 6):
        encoder_pass(f"gat2_layers{layers}", net_for(layers=layers), batch)
        encoder_pass(f"gat2_layers{layers}_heads1_dropout", net_for(heads=1, layers=layers, drop=0.1), batch)
    encoder_pass("train_dropout0.1", net_for(drop=0.1), batch)
    encoder_pass("eval_with_grad", net_for(drop=0.1), batch, train=False)
    encoder_pass("eval_no_grad", net_for(drop=0.1), batch, train=False, grad=False)

    gbatches = [data.batch_to(data.collate_fn(synth.synth_molecules(24, seed=61 + i, profile="esol")), DEV) for i in range(3)]
    graph_step("graph_step_padded", gbatches, 0.0)
    graph_step("graph_step_padded_dropout", gbatches, 0.1)

    net = net_for(drop=0.1).eval()
    masked = dict(batch)
    masked.pop("_fragnet_plan", None)
    g = torch.Generator().manual_seed(3)
    for key, rows in (("mask_atoms", "x_atoms"), ("mask_bonds", "node_features_bonds"), ("mask_fbonds", "node_features_fbonds")):
        m = (torch.rand(masked[rows].shape[0] // 2, generator=g) < 0.1).to(torch.uint8).repeat_interleave(2)     # both directed rows
        masked[key] = torch.cat((m, torch.zeros(masked[rows].shape[0] - m.numel(), dtype=torch.uint8))).to(DEV)
    with torch.no_grad():
        report("masked_forward", [(f"out{i}", t) for i, t in enumerate(net.pretrain(masked))] + [("pred", net(masked))])

    viz = V.FragNetFineTuneViz(n_classes=1, edge_features=17, num_layer=3, num_heads=4, drop_ratio=0.1, h1=32, h2=32, h3=32, h4=32, act="relu", fthead="FTHead3")
    viz.load_state_dict(net.state_dict(), strict=True)
    viz = viz.to(DEV).eval()

    def flat(x, prefix="r"):
        if isinstance(x, (tuple, list)):
            return [it for i, v in enumerate(x) for it in flat(v, f"{prefix}.{i}")]
        return [(prefix, x)]
    for name, b in (("readout_forward", batch), ("readout_single_fragment_EF0", single_fragment_batch(6, True))):
        b = dict(b)
        b.pop("_fragnet_plan", None)
        with torch.no_grad():
            report(name, flat(viz(b)))

    res = ga.input_gradients(net_for(), mols, return_gradients=True)
    report("input_gradients", sorted(res.arrays().items()))

    encoder_pass("single_fragment_train", net_for(), single_fragment_batch(6, False))
    encoder_pass("single_molecule_train", net_for(drop=0.1), data.batch_to(data.collate_fn(mols[:1]), DEV))

    # the encoder's Python front: the input gate, and the level-by-level routes
    gated = dict(batch)
    gated["keep_atoms"] = (torch.rand(batch["x_atoms"].shape[0], generator=torch.Generator().manual_seed(5)) < 0.85).to(torch.uint8).to(DEV)
    encoder_pass("keep_train_dropout", net_for(drop=0.1), gated)
    encoder_pass("keep_eval_no_grad", net_for(drop=0.1), gated, train=False, grad=False)
    pt_mols = synth.synth_molecules(12, seed=19, profile="esol", pretrain_targets=True)
    pt_batch = data.batch_to(data.collate_fn_pt(pt_mols), DEV)
    for train in (True, False):
        torch.manual_seed(0)
        pm = M.FragNetPreTrainMasked2(num_layer=2, drop_ratio=0.1, edge_features=17).to(DEV).train(train)
        pm.pretrain.rng.offset = OFFSET
        b = dict(pt_batch)
        b.pop("_fragnet_plan", None)
        with torch.set_grad_enabled(train):
            outs = pm(b)
            items = [(f"out{i}", t) for i, t in enumerate(outs)] + [("keep", pm.last_keep)]
            if train:
                sum(t.square().mean() for t in outs if t is not None).backward()
                items += [(n, p.grad) for n, p in pm.named_parameters()]
        report(f"masked2_{'train_dropout' if train else 'eval'}", items)
    for label, cls in (("gat2", M.FragNetFineTune), ("gat2_lite", M.FragNetFineTuneLite), ("gat2_edge", M.FragNetFineTuneEdge)):
        lv = net_for(drop=0.1, cls=cls)
        lv.pretrain.use_engine = False
        # (the synthetic cnx_attr is 6 wide; the per-level gat2_edge layer checks its Linear(8 -> 128) against the attribute's width)
        wide = dict(batch, cnx_attr=torch.nn.functional.pad(batch["cnx_attr"], (0, 2))) if label == "gat2_edge" else batch
        encoder_pass(f"levels_{label}_train_dropout", lv, wide)
    viz.pretrain.rng.seed = 5
    encoder_pass("viz_levels_train_dropout", viz, batch)
    viz.use_engine = False
    encoder_pass("viz_levels_eval_no_grad", viz, batch, train=False, grad=False)
    viz.use_engine = True
    one = net_for(drop=0.1)
    one.pretrain.layers[1].return_attentions = True
    encoder_pass("levels_return_attentions_layer1", one, batch)

    for key, value in ((22, 0), (14, 0), (7, 0), (20, 0), (20, 2), (33, 0)):
        try:
            _lib.call("fn_set_tuning", key, value)
            encoder_pass(f"train_key{key}={value}", net_for(drop=0.1), batch)
            if key == 22:
                encoder_pass(f"train_6layers_key{key}={value}", net_for(layers=6, drop=0.1), batch)
        finally:
            _lib.call("fn_set_tuning", key, DEFAULTS[key])
    try:
        _lib.call("fn_set_tuning", 28, 1)
        graph_step("graph_step_key28=1", gbatches, 0.1)
    finally:
        _lib.call("fn_set_tuning", 28, DEFAULTS[28])


if __name__ == "__main__":
    if "--calls" in sys.argv[1:]:
        record_calls()
    main()
