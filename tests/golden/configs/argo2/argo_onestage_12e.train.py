# optimizer / schedule settings of configs/argo2/argo_onestage_12e.py (tusen-ai/SST), written by tests/golden/make_argo2_fixtures.py - do not edit
{'fp16': None,
 'lr_config': {'cyclic_times': 1, 'policy': 'cyclic', 'step_ratio_up': 0.1, 'target_ratio': (100, 0.001)},
 'momentum_config': None,
 'optimizer': {'betas': (0.9, 0.999),
               'lr': 1e-05,
               'paramwise_cfg': {'custom_keys': {'norm': {'decay_mult': 0.0}}},
               'type': 'AdamW',
               'weight_decay': 0.05},
 'optimizer_config': {'grad_clip': {'max_norm': 10, 'norm_type': 2}},
 'runner': {'max_epochs': 12, 'type': 'EpochBasedRunner'}}
