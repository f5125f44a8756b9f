"""fragnet.model.gcn.gcn2 -> fragnet_amd.gcn (reference file: model/gcn/gcn2.py; its FragNetPreTrain is out of scope)."""
from fragnet_amd.gcn import FragNet, FragNetFineTune, FragNetLayer  # noqa: F401
from fragnet_amd.model import FTHead3, FTHead4  # noqa: F401
