{'fp16': None,
 'lr_config': {'cyclic_times': 1, 'policy': 'cyclic', 'step_ratio_up': 0.4, 'target_ratio': (10, 0.0001)},
 'momentum_config': {'cyclic_times': 1,
                     'policy': 'cyclic',
                     'step_ratio_up': 0.4,
                     'target_ratio': (0.8947368421052632, 1)},
 'optimizer': {'lr': 0.0002, 'type': 'AdamW', 'weight_decay': 0.01},
 'optimizer_config': {'grad_clip': {'max_norm': 35, 'norm_type': 2}},
 'runner': {'max_epochs': 12, 'type': 'EpochBasedRunner'}}
