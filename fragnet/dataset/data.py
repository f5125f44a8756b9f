"""fragnet.dataset.data -> fragnet_amd.data (reference file: dataset/data.py:877-1032, the collate functions; collate_fn_dta: data.py:1035-1109; collate_fn_cdrp: data.py:1112-1187)."""
from fragnet_amd.data import batch_to, collate_fn, collate_fn_cdrp, collate_fn_dta, collate_fn_pt  # noqa: F401
