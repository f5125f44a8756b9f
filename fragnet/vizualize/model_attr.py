"""fragnet.vizualize.model_attr -> fragnet_amd.attr_model (reference file: vizualize/model_attr.py:143-462; ``get_attr_image``'s numbers
come from fragnet_amd.attribution.fragment_contributions, drawing stays with RDKit and the caller)."""
from fragnet_amd.attr_model import FragNetFineTune, FragNetFineTuneBaseViz, FragNetPreTrain, collate_fn, collate_fn_cdrp  # noqa: F401
