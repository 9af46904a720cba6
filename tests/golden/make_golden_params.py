#!/usr/bin/env python3
"""tests/golden/make_golden_params.py -- parameters.txt as the reference's own Config.save writes it (utils/config.py:311-445):
  params/dales_pl/parameters.txt        train_DALES_PseudoLabel.py:44-201 (DALESPLConfig)
  params/vaihingen3d_wl/parameters.txt  train_Vaihingen3D_WeakLabel.py:46-189 (Vaihingen3DWLConfig)
  params/<name>/expected.json           beside each: the value of every attribute the file names, as the saved object held
                                        it (the {epoch: factor} dictionary with its keys as strings, JSON has no integer keys)
Settings-only text.  RUNS ONLY IN THE BUILD CONTAINER, with the import aids of make_golden.py; the two configuration classes
are the reference's, imported from its training scripts (whose `__main__` blocks do not run).  num_classes and dataset_task are
what the dataset's constructor writes into the configuration before the trainer saves it (datasets/DALES_PseudoLabel.py:78-88:
ten label values less one ignored; datasets/Vaihingen3D_WeakLabel.py:78-88: nine, none ignored)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg          # noqa: E402,F401  (import aids, sys.path and the working directory)

from train_DALES_PseudoLabel import DALESPLConfig               # noqa: E402
from train_Vaihingen3D_WeakLabel import Vaihingen3DWLConfig     # noqa: E402

ATTRIBUTE = {'lr_decay_epochs': 'lr_decays', 'contrast_thd[%]': 'contrast_thd'}       # key in the file -> attribute


def write(cls, name, num_classes):
    out = os.path.join(HERE, "params", name)
    os.makedirs(out, exist_ok=True)
    cfg = cls()
    cfg.num_classes = num_classes
    cfg.dataset_task = 'cloud_segmentation'
    cfg.saving_path = out
    cfg.save()
    expected = {}
    with open(os.path.join(out, "parameters.txt")) as f:
        for line in f:
            words = line.split()
            if len(words) >= 2 and words[1] == '=' and words[0] != '#':
                attr = ATTRIBUTE.get(words[0], words[0])
                v = getattr(cfg, attr)
                expected[attr] = {str(k): d for k, d in v.items()} if isinstance(v, dict) else v
    with open(os.path.join(out, "expected.json"), "w") as f:
        json.dump(expected, f, indent=1, sort_keys=True)
        f.write("\n")
    # the reference reads its own file back
    back = cls()
    back.load(out)
    assert back.architecture == cfg.architecture and back.lr_decays == cfg.lr_decays and back.num_layers == cfg.num_layers
    print("wrote", out, len(expected), "keys")


if __name__ == "__main__":
    write(DALESPLConfig, "dales_pl", 9)
    write(Vaihingen3DWLConfig, "vaihingen3d_wl", 9)
