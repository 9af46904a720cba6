"""CPU: Config.save / Config.load against two parameters.txt written by the reference's own Config.save
(tests/golden/params/, made by tests/golden/make_golden_params.py: the DALES pseudo-label and the Vaihingen3D weak-label
configurations) and the attribute values the maker recorded beside them."""
import json
import os

import pytest

from conftest import GOLDEN

FIXTURES = ("dales_pl", "vaihingen3d_wl")


def _fixture(name):
    d = os.path.join(GOLDEN, "params", name)
    with open(os.path.join(d, "expected.json")) as f:
        want = json.load(f)
    want["lr_decays"] = {int(k): v for k, v in want["lr_decays"].items()}
    with open(os.path.join(d, "parameters.txt"), "rb") as f:
        return d, want, f.read()


@pytest.mark.parametrize("name", FIXTURES)
def test_load_gives_the_recorded_values(name):
    from weasal_amd.config import Config
    d, want, _ = _fixture(name)
    cfg = Config()
    assert cfg.load(d) is cfg
    assert len(want) >= 60
    for key, value in want.items():
        got = getattr(cfg, key)
        assert got == value and isinstance(got, bool) == isinstance(value, bool), (key, got, value)
        if isinstance(value, int) and not isinstance(value, bool) and key not in ("in_radius", "grad_clip_norm", "contrast_start",
                                                                                   "contrast_thd", "sub_radius"):
            assert isinstance(got, int), key              # (those five are written with six decimals: floats on the way back)
    assert cfg.saving is True and cfg.saving_path == d
    # the file itself, not its directory
    other = Config().load(os.path.join(d, "parameters.txt"))
    assert {k: getattr(other, k) for k in want} == {k: getattr(cfg, k) for k in want} and other.saving_path == d


@pytest.mark.parametrize("name", FIXTURES)
def test_load_then_save_reproduces_the_file(name, tmp_path):
    from weasal_amd.config import Config
    d, _, text = _fixture(name)
    cfg = Config().load(d)
    cfg.saving_path = str(tmp_path)
    cfg.save()
    assert (tmp_path / "parameters.txt").read_bytes() == text
    # and once more from the copy
    again = Config().load(str(tmp_path))
    (tmp_path / "again").mkdir()
    again.saving_path = str(tmp_path / "again")
    again.save()
    assert (tmp_path / "again" / "parameters.txt").read_bytes() == text


def test_decays_architecture_and_derived_fields_survive():
    from weasal_amd import config as wcfg
    d, want, _ = _fixture("vaihingen3d_wl")
    cfg = wcfg.Config().load(d)
    assert cfg.lr_decays == {i: 0.98 for i in range(1, 1000)} and list(cfg.lr_decays)[:3] == [1, 2, 3]
    assert cfg.architecture == wcfg.Vaihingen3DWLConfig.architecture == want["architecture"]
    assert cfg.num_layers == 3 == want["num_layers"] and cfg.deform_layers == [False] * 3
    assert cfg.augment_symmetries == [True, True, False] and cfg.class_w == [1.0] * 9
    assert (cfg.model_name, cfg.loss_type, cfg.anchor_method, cfg.subsample_labels) == ("KPFCNN_mprm", "region_mprm_loss", "reduced", True)
    d, want, _ = _fixture("dales_pl")
    cfg = wcfg.Config().load(d)
    assert cfg.architecture == wcfg.DALESPLConfig.architecture and cfg.num_layers == 5 and cfg.deform_layers == [False] * 5
    assert cfg.lr_decays == want["lr_decays"] and (cfg.contrast_start, cfg.contrast_thd, cfg.dropout) == (0.0, 10.0, 0.5)


def test_own_configurations_round_trip(tmp_path):
    """save -> load into a plain Config -> save: the same bytes, for the package's own classes (optional keys come and go:
    sub_radius, contrast_start, feature-free `dropout = 0`), a None epoch_steps, a class list and empty lists"""
    from weasal_amd import config as wcfg
    for i, cls in enumerate((wcfg.Config, wcfg.DALESPLConfig, wcfg.Vaihingen3DPLConfig, wcfg.Vaihingen3DWLConfig, wcfg.DALESDeformConfig)):
        a = cls()
        if i == 0:
            a.epoch_steps, a.num_classes, a.lr_decays, a.class_w = None, [4, 5], {}, []
        a.saving_path = str(tmp_path / ("a%d" % i))
        os.makedirs(a.saving_path)
        a.save()
        b = wcfg.Config().load(a.saving_path)
        for key in ("epoch_steps", "num_classes", "lr_decays", "architecture", "num_layers", "deform_layers", "first_features_dim",
                    "modulated", "learning_rate"):
            assert getattr(b, key) == getattr(a, key), (cls.__name__, key)
        b.saving_path = str(tmp_path / ("b%d" % i))
        os.makedirs(b.saving_path)
        b.save()
        assert (tmp_path / ("b%d" % i) / "parameters.txt").read_bytes() == (tmp_path / ("a%d" % i) / "parameters.txt").read_bytes()
    # an optional value set after load is written again
    c = wcfg.Config().load(os.path.join(GOLDEN, "params", "vaihingen3d_wl"))
    c.dropout = 0.5
    c.saving_path = str(tmp_path)
    c.save()
    assert "dropout = 0.500\n" in (tmp_path / "parameters.txt").read_text()
