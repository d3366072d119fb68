"""Resolved ``model`` dictionaries of the reference's two Argoverse 2 FSD configs (configs/argo2/argo_onestage_12e.py and
argo_segmentation_pretrain.py) and their train / test pipelines, as Python literals under tests/golden/configs/argo2/:
<name>.model.py in the format of tests/golden/make_config_fixtures.py (the config text read the way mmcv.Config.fromfile reads
it: exec + ``_base_`` merge) and <name>.pipeline.py = dict(train_pipeline=..., test_pipeline=...) in the format of
tests/golden/configs/pipeline/, and <name>.train.py = the optimizer / schedule settings in the format of
tests/golden/configs/train/.  Settings only.  tests/test_argo2_configs.py constructs them on any machine and checks them
against the config text where the reference exists.

    python tests/golden/make_argo2_fixtures.py
"""
import os
import pprint
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
sys.path.insert(0, os.path.join(HERE, '..', '..'))
sys.path.insert(0, HERE)

GROUP = 'argo2'
TRAIN_KEYS = ('fp16', 'lr_config', 'momentum_config', 'optimizer', 'optimizer_config', 'runner')


def main():
    from test_configs_build import load_config, shipped_configs
    out_dir = os.path.join(HERE, 'configs', GROUP)
    os.makedirs(out_dir, exist_ok=True)
    for path in shipped_configs(GROUP):
        name = os.path.splitext(os.path.basename(path))[0]
        cfg = load_config(path)
        with open(os.path.join(out_dir, name + '.model.py'), 'w') as f:
            f.write(f'# resolved `model` of configs/{GROUP}/{name}.py (tusen-ai/SST), written by '
                    'tests/golden/make_argo2_fixtures.py - do not edit\n')
            f.write(pprint.pformat(cfg['model'], width=120, sort_dicts=False) + '\n')
        with open(os.path.join(out_dir, name + '.pipeline.py'), 'w') as f:
            f.write(f'# train / test pipeline of configs/{GROUP}/{name}.py (tusen-ai/SST), written by '
                    'tests/golden/make_argo2_fixtures.py - do not edit\n')
            f.write(pprint.pformat({k: cfg[k] for k in ('train_pipeline', 'test_pipeline')}, width=120, sort_dicts=False))
            f.write('\n')
        # the settings build_training_update reads, in the format of tests/golden/configs/train/
        with open(os.path.join(out_dir, name + '.train.py'), 'w') as f:
            f.write(f'# optimizer / schedule settings of configs/{GROUP}/{name}.py (tusen-ai/SST), written by '
                    'tests/golden/make_argo2_fixtures.py - do not edit\n')
            f.write(pprint.pformat({k: cfg.get(k) for k in TRAIN_KEYS}, width=120) + '\n')
        print(GROUP, name)


if __name__ == '__main__':
    main()
