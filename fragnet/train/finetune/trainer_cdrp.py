"""fragnet.train.finetune.trainer_cdrp -> fragnet_amd.train (reference file: train/finetune/trainer_cdrp.py)."""
from fragnet_amd.train import TrainerFineTuneCDRP as TrainerFineTune  # noqa: F401
