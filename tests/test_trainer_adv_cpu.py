"""CPU: the FreeLB settings -- command-line flags and their defaults (adv_steps = 0: off), trainer.adv_config's reading of a
config, and the error for an unknown adv_modality."""
import argparse

import pytest


def _parse(argv):
    from meme_challenge_amd.train_template import TrainerTemplate
    parser = argparse.ArgumentParser()
    TrainerTemplate.add_default_argparse(parser)
    return vars(parser.parse_args(argv))


def test_adv_flags_parse_and_default_to_off():
    from meme_challenge_amd.trainer import adv_config
    cfg = _parse([])
    assert cfg['adv_steps'] == 0 and cfg['adv_modality'] == 'both' and cfg['adv_init_mag'] == 0.0
    assert cfg['adv_lr'] > 0 and cfg['adv_max_norm'] > 0
    assert adv_config(cfg).steps == 0
    assert adv_config({}).steps == 0 and adv_config({}).modality == 'both'          # a config without the keys: off
    cfg = _parse(['--adv_steps', '3', '--adv_lr', '0.05', '--adv_max_norm', '0.4', '--adv_init_mag', '0.2', '--adv_modality', 'txt',
                  '--deterministic'])
    adv = adv_config(cfg)
    assert (adv.steps, adv.lr, adv.max_norm, adv.init_mag, adv.modality) == (3, 0.05, 0.4, 0.2, 'txt')
    assert cfg['deterministic'] is True


def test_unknown_adv_modality_is_an_error():
    from meme_challenge_amd.trainer import adv_config
    for ok in ('both', 'txt', 'img'):
        assert adv_config({'adv_steps': 2, 'adv_modality': ok}).modality == ok
    with pytest.raises(ValueError, match='adv_modality'):
        adv_config({'adv_steps': 2, 'adv_modality': 'pos'})
    with pytest.raises(ValueError, match='adv_modality'):
        adv_config(_parse(['--adv_modality', 'image']))          # refused even with adv_steps = 0: a typo does not wait for K > 0
    with pytest.raises(ValueError, match='negative'):
        adv_config({'adv_steps': -1})
