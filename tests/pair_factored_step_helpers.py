"""What the captured-FACTORED-pair-step tests share (tests/test_pair_factored_graphstep_host.py, tests/test_gpu_pair_factored_graphstep.py):
factored CDRP / DTA batches over ``synth.pair_records`` whose pair, drug and second-input counts all differ, and the capacities sized
from them.  Test infrastructure only."""
from tests import pair_step_helpers as H

# (pairs M, distinct drugs U, distinct second inputs C): one distinct drug; all pairs distinct; two ordinary ones
SMALL = ((12, 4, 3), (9, 1, 5), (7, 7, 7), (10, 3, 2))
BIG = (20, 4, 3)             # beyond the PAIR capacity only (16 = 12 pairs + 5 %, rounded up to 8): its drugs and second inputs would fit


def factored_batch(kind, M, U, C, seed, device=None):
    from fragnet_amd import data, synth
    recs = synth.pair_records(M, U, C, kind, seed, gene_dim=H.GENE_DIM)
    b = (data.collate_fn_cdrp_factored if kind == "cdrp" else data.collate_fn_dta_factored)(recs)
    return b if device is None else data.batch_to(b, device)


def batches(kind, device=None):
    """(the four small batches, the one beyond the pair capacity, FactoredPairShapes from the small ones at margin 5 %)"""
    from fragnet_amd import graphstep
    small = [factored_batch(kind, M, U, C, 600 + 10 * i, device) for i, (M, U, C) in enumerate(SMALL)]
    big = factored_batch(kind, *BIG, 690, device)
    shapes = graphstep.FactoredPairShapes.from_batches(small, margin=0.05)
    return small, big, shapes
