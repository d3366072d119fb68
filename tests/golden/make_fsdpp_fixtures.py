"""Resolved ``model`` dictionary of the reference's shipped FSD++ config (configs/fsdpp/fsdpp_waymoD1_1x_7f_6base.py), as a Python
literal in tests/golden/configs/fsdpp/<name>.model.py - the format of tests/golden/make_config_fixtures.py (the config text read
the way mmcv.Config.fromfile reads it: exec + ``_base_`` merge).  tests/test_fsdpp_configs.py constructs it on any machine and
checks it against the config text where the reference exists.

    python tests/golden/make_fsdpp_fixtures.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
sys.path.insert(0, os.path.join(HERE, '..', '..'))
sys.path.insert(0, HERE)

GROUP = 'fsdpp'


def main():
    from make_config_fixtures import write_model
    from test_configs_build import load_config, shipped_configs
    out_dir = os.path.join(HERE, 'configs', GROUP)
    os.makedirs(out_dir, exist_ok=True)
    for path in shipped_configs(GROUP):
        name = os.path.splitext(os.path.basename(path))[0]
        write_model(os.path.join(out_dir, name + '.model.py'), f'configs/{GROUP}/{name}.py', load_config(path)['model'])
        print(GROUP, name)


if __name__ == '__main__':
    main()
