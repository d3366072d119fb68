"""Resolved ``model`` dictionaries of the reference's shipped SST configs, as Python literals.

/root/reference does not exist on the GPU box, and `bench.py`'s `config_as_is` leg / `--workload sst_center` must build their
models from the config AS SHIPPED.  This script reads the config text the way mmcv.Config.fromfile
does (tests/test_configs_build.load_config: exec + `_base_` merge), takes the `model` entry and writes it with pprint - tuples,
integer keys and all - to tests/golden/configs/<name>.model.py; tests/test_config_fixtures.py checks (in the build container)
that the committed literals still equal what the config files say, and (everywhere) that they construct.
The `model` of every shipped config of the groups in CONSTRUCT_GROUPS goes to tests/golden/configs/<group>/<name>.model.py the
same way: tests/test_configs_build.py constructs them on any machine and checks them against the config text where it exists.

    python tests/golden/make_config_fixtures.py
"""
import os
import pprint
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
sys.path.insert(0, os.path.join(HERE, '..', '..'))

CONFIGS = ['configs/sst_refactor/sst_waymoD5_1x_3class_8heads_v2.py',
           'configs/sst_refactor/sst_waymoD5_1x_3class_centerhead.py',
           'configs/sst_refactor/sst_waymoD1_2x_3class_centerhead.py']
CONSTRUCT_GROUPS = ('fsdv2', 'fsd', 'sst_refactor', 'sst')


def write_model(path, rel, model):
    with open(path, 'w') as f:
        f.write(f'# resolved `model` of {rel} (tusen-ai/SST), written by tests/golden/make_config_fixtures.py - do not edit\n')
        f.write(pprint.pformat(model, width=120, sort_dicts=False))
        f.write('\n')


def main():
    from test_configs_build import REF, load_config, shipped_configs
    out_dir = os.path.join(HERE, 'configs')
    os.makedirs(out_dir, exist_ok=True)
    for rel in CONFIGS:
        cfg = load_config(os.path.join(REF, rel))
        name = os.path.splitext(os.path.basename(rel))[0]
        write_model(os.path.join(out_dir, name + '.model.py'), rel, cfg['model'])
        print(name, 'fp16' in cfg and cfg['fp16'])
    for group in CONSTRUCT_GROUPS:
        os.makedirs(os.path.join(out_dir, group), exist_ok=True)
        for path in shipped_configs(group):
            name = os.path.splitext(os.path.basename(path))[0]
            write_model(os.path.join(out_dir, group, name + '.model.py'), f'configs/{group}/{name}.py', load_config(path)['model'])
            print(group, name)


if __name__ == '__main__':
    main()
