"""fragnet.model.cdrp.model -> fragnet_amd.cdrp (reference file: model/cdrp/model.py)."""
from fragnet_amd.cdrp import CDRPModel, MLP  # noqa: F401
