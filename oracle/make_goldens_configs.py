"""Golden record of the reference's shipped training configs: the `model:` section of configs/train/train_MolDiff.yml,
train_MolDiff_simple.yml and train_bondpred.yml (the hyper-parameters a checkpoint carries as ckpt['config'].model), saved as
data to tests/golden/train_configs_model.json so that tests/test_host_logic.py can pin `harness.default_config` against them
on any machine.

    python oracle/make_goldens_configs.py <path of a reference checkout>
"""
import json
import os
import sys

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'train_configs_model.json')
CONFIGS = (('MolDiff', 'train_MolDiff.yml'), ('MolDiff_simple', 'train_MolDiff_simple.yml'), ('bondpred', 'train_bondpred.yml'))


def main(ref):
    rec = {}
    for name, fn in CONFIGS:
        with open(os.path.join(ref, 'configs', 'train', fn)) as f:
            rec[name] = {'file': 'configs/train/' + fn, 'model': yaml.safe_load(f)['model']}
    with open(OUT, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', OUT)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
