"""fragnet.model.dta.model -> fragnet_amd.dta (reference file: model/dta/model.py)."""
from fragnet_amd.dta import DTAModel, DTAModel2  # noqa: F401
