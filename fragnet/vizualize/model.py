"""fragnet.vizualize.model -> fragnet_amd.viz_model (reference file: vizualize/model.py:45-280; drawing stays with RDKit and the caller)."""
from fragnet_amd.viz_model import FragNetFineTuneBaseViz, FragNetFineTuneViz, FragNetPreTrainViz, FragNetViz  # noqa: F401
