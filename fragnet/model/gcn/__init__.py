"""fragnet.model.gcn -> fragnet_amd.gcn (model_version gcn2; reference directory: model/gcn/)."""
