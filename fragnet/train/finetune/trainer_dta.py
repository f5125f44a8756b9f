"""fragnet.train.finetune.trainer_dta -> fragnet_amd.train (reference file: train/finetune/trainer_dta.py)."""
from fragnet_amd.train import TrainerFineTuneDTA as TrainerFineTune  # noqa: F401
