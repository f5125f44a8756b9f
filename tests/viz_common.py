"""Shared by the attention read-out tests and tests/golden/make_golden_viz.py: the cases of the fixture attn_readout_b6.npz and the way
the last layer's four ``summed_attn_weights_*`` tensors are taken from any FragNetFineTune-shaped model whose layers have the
reference's ``return_attentions`` switch (the reference itself, the oracle): a forward hook on the last layer."""
import torch

NAMES = ("attn_atoms", "attn_frags", "attn_bonds", "attn_fbonds")
CASES = {"h4": 4, "h2": 2}


def last_layer_readout(model, batch, run):
    """(logits, the four attention tensors) of ``model(batch)`` with the last layer reading its attentions out.  Shared with the
    tests, which take the oracle's read-outs the same way."""
    layer = model.pretrain.layers[-1]
    seen = []

    def hook(_m, _i, out):
        seen.append([t.detach().clone() for t in out[4:]])
        return tuple(out[:4])
    layer.return_attentions = True
    handle = layer.register_forward_hook(hook)
    try:
        with torch.no_grad():
            logits = run(model, batch)
    finally:
        handle.remove()
        layer.return_attentions = False
    assert len(seen) == 1 and len(seen[0]) == 4
    return logits, seen[0]
