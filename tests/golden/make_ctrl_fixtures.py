"""Resolved ``model`` dictionaries of the reference's shipped CTRL configs (configs/ctrl/ctrl_{veh_24e,ped_24e,cyc_12e}.py), as
Python literals in tests/golden/configs/ctrl/<name>.model.py - the format of tests/golden/make_config_fixtures.py (the config
text read the way mmcv.Config.fromfile reads it: exec + ``_base_`` merge).  tests/test_tracklet_configs.py constructs them on
any machine and checks them against the config text where the reference exists.

    python tests/golden/make_ctrl_fixtures.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
sys.path.insert(0, os.path.join(HERE, '..', '..'))
sys.path.insert(0, HERE)

GROUP = 'ctrl'


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
