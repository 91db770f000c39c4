"""CPU: the VILLA settings -- command-line flags and their defaults (today's FreeLB behaviour), trainer.adv_config's reading of a
config, and every combination it refuses."""
import argparse

import pytest


def _parse(argv):
    from meme_challenge_amd.train_template import TrainerTemplate
    parser = argparse.ArgumentParser()
    TrainerTemplate.add_default_argparse(parser)
    return vars(parser.parse_args(argv))


def test_villa_flags_parse_and_default_to_todays_behaviour():
    from meme_challenge_amd.trainer import adv_config
    cfg = _parse([])
    assert (cfg['adv_algo'], cfg['adv_kl_weight'], cfg['adv_norm_type']) == ('freelb', 0.0, 'l2')
    adv = adv_config(cfg)
    assert (adv.steps, adv.modality, adv.algo, adv.kl_weight, adv.norm_type) == (0, 'both', 'freelb', 0.0, 'l2')
    cfg = _parse(['--adv_steps', '2', '--adv_algo', 'villa', '--adv_kl_weight', '1.5', '--adv_norm_type', 'linf', '--adv_modality', 'each',
                  '--adv_lr', '0.05', '--adv_max_norm', '0.4', '--adv_init_mag', '0.2'])
    assert adv_config(cfg) == (2, 0.05, 0.4, 0.2, 'each', 'villa', 1.5, 'linf')


def test_adv_config_keeps_its_first_five_fields_and_their_defaults():
    from meme_challenge_amd.trainer import AdvConfig, ADV_MODALITIES, adv_config
    assert AdvConfig._fields == ('steps', 'lr', 'max_norm', 'init_mag', 'modality', 'algo', 'kl_weight', 'norm_type')
    assert ADV_MODALITIES[:3] == ('both', 'txt', 'img') and 'each' in ADV_MODALITIES
    assert adv_config({}) == (0, 0.0, 0.0, 0.0, 'both', 'freelb', 0.0, 'l2')
    adv = adv_config({'adv_steps': 3, 'adv_lr': 0.05, 'adv_max_norm': 0.4, 'adv_init_mag': 0.2, 'adv_modality': 'txt'})
    assert adv[:5] == (3, 0.05, 0.4, 0.2, 'txt') and adv[5:] == ('freelb', 0.0, 'l2')
    adv = adv_config({'adv_steps': 1, 'adv_algo': 'villa', 'adv_kl_weight': 0.5, 'adv_norm_type': 'linf', 'adv_modality': 'each'})
    assert (adv.algo, adv.kl_weight, adv.norm_type, adv.modality) == ('villa', 0.5, 'linf', 'each')
    assert adv_config({'adv_steps': 1, 'adv_algo': 'villa'}).kl_weight == 0.0           # VILLA's clean pass without the KL term
    assert adv_config({'adv_steps': 2, 'adv_norm_type': 'linf'}).norm_type == 'linf'


@pytest.mark.parametrize('config, match', [
    ({'adv_algo': 'pgd'}, 'adv_algo'),
    ({'adv_steps': 2, 'adv_norm_type': 'l1'}, 'adv_norm_type'),
    ({'adv_steps': 2, 'adv_algo': 'villa', 'adv_kl_weight': -0.1}, 'adv_kl_weight'),
    ({'adv_steps': 2, 'adv_kl_weight': 0.5}, 'adv_kl_weight'),                          # FreeLB has no clean pass to pull towards
    ({'adv_steps': 2, 'adv_algo': 'freelb', 'adv_kl_weight': 0.5}, 'adv_kl_weight'),
    ({'adv_algo': 'villa'}, 'adv_steps'),
    ({'adv_steps': 0, 'adv_algo': 'villa', 'adv_kl_weight': 1.0}, 'adv_steps'),
    ({'adv_steps': 2, 'adv_modality': 'each'}, 'each'),
    ({'adv_steps': 2, 'adv_algo': 'villa', 'adv_modality': 'image'}, 'adv_modality'),
    ({'adv_steps': 2, 'adv_algo': 'villa', 'adv_modality': 'pos'}, 'adv_modality'),
])
def test_refused_settings(config, match):
    from meme_challenge_amd.trainer import adv_config
    with pytest.raises(ValueError, match=match):
        adv_config(config)


def test_adv_delta_step_refuses_an_unknown_norm_before_it_touches_the_library():
    from meme_challenge_amd.trainer import adv_delta_step
    with pytest.raises(ValueError, match='norm_type'):
        adv_delta_step(None, None, 0.1, 1.0, norm_type='l1')


def test_adv_rounds_of_every_accepted_algorithm_and_modality():
    from meme_challenge_amd.trainer import ADV_ALGOS, ADV_MODALITIES, adv_config, adv_rounds
    one = {'both': (('txt', 'img'),), 'txt': (('txt',),), 'img': (('img',),)}
    want = {(algo, m): r for algo in ('freelb', 'villa') for m, r in one.items()}
    want[('villa', 'each')] = (('txt',), ('img',))
    accepted = {}
    for algo in ADV_ALGOS:
        for m in ADV_MODALITIES:
            try:
                accepted[(algo, m)] = adv_rounds(adv_config({'adv_steps': 2, 'adv_algo': algo, 'adv_modality': m}))
            except ValueError:
                assert (algo, m) == ('freelb', 'each')
    assert accepted == want
