"""Import-path aliases: the names the reference's drivers import from ``fragnet.*`` resolve to the MI355X implementation in
``fragnet_amd`` (nothing of the reference is copied here), so that ``fragnet/train/finetune/finetune_gat2.py`` and
``fragnet/train/pretrain/pretrain_gat2.py`` run against this repository with their import lines unchanged:

    fragnet.model.gat.gat2            FragNet, FragNetFineTune           (finetune_gat2.py:121, pretrain_gat2.py:16)
    fragnet.model.gat.gat2_lite       FragNetFineTune                    (finetune_gat2.py:144)
    fragnet.model.gat.gat2_edge       FragNetFineTune                    (finetune_gat2.py:166)
    fragnet.model.gat.gat2_pretrain   FragNetPreTrain                    (finetune_gat2.py:216)
    fragnet.model.gcn.gcn2            FragNetFineTune, FragNet, FragNetLayer (finetune_gat2.py:102, model_version gcn2)
    fragnet.model.gat.pretrain_heads  FragNetPreTrain, PretrainTask      (pretrain_gat2.py:12)
    fragnet.dataset.data              collate_fn, collate_fn_pt          (finetune_gat2.py:6, pretrain_gat2.py:15)
    fragnet.dataset.dataset           load_pickle_dataset, load_data_parts (finetune_gat2.py:2, pretrain_gat2.py:6)
    fragnet.train.utils               EarlyStopping, TrainerFineTune     (finetune_gat2.py:4,9)
    fragnet.train.pretrain.pretrain_utils   Trainer                      (pretrain_gat2.py:13)
    fragnet.model.cdrp.model          CDRPModel, MLP                     (finetune_cdrp.py:18)
    fragnet.dataset.data              collate_fn_cdrp                    (finetune_cdrp.py:6)
    fragnet.train.finetune.trainer_cdrp     TrainerFineTune              (finetune_cdrp.py:9)
    fragnet.model.dta.model           DTAModel2, DTAModel                (finetune_dta.py:17)
    fragnet.dataset.data              collate_fn_dta                     (finetune_dta.py:6)
    fragnet.train.finetune.trainer_dta      TrainerFineTune              (finetune_dta.py:9)
    fragnet.vizualize.model           FragNetViz, FragNetFineTuneViz, FragNetFineTuneBaseViz, FragNetPreTrainViz (vizualize/viz.py)

Model versions outside the accelerated hot path (masked pretraining heads, gcn.py / gcn3.py / gat v1, DTA's transformer tower; SURVEY.md section 2 rows
10-19) are named here only to fail with a clear message when constructed.
"""
