"""fragnet.model.gat.pretrain_heads -> fragnet_amd.model (reference file: model/gat/pretrain_heads.py)."""
from fragnet_amd.model import FragNetPreTrain, PretrainTask  # noqa: F401


def _outside(name):
    class _Outside:
        def __init__(self, *a, **k):
            # (tests/test_fragnet_aliases.py pins this refusal; the masked models themselves are on the engine since DESIGN section 7l)
            raise NotImplementedError(f"{name} (masked pretraining, pretrain_heads.py:144-) is outside the accelerated FragNet "
                                      f"alias package: use fragnet_amd.model.{name} (scripts/pretrain_gat2.py does, by model_version)")
    _Outside.__name__ = name
    return _Outside


FragNetPreTrainMasked = _outside("FragNetPreTrainMasked")
FragNetPreTrainMasked2 = _outside("FragNetPreTrainMasked2")
