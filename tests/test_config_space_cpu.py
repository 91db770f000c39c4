"""CPU: the bars and mutations of tests/config_space_ref.py judge what tests/test_config_space_gpu.py needs them to judge.

  1. The float32 oracle stays within 0.05 of every fp32 / fp32x3 bar against the float64 oracle, in eval and in train mode, at
     every configuration: the bars are some 50 x float32 round-off, and what the GPU tests measure against float64 is the kernels'
     error, not the reference's.
  2. Every planted mutation moves at least one gradient tensor by 10 x its bar, at every configuration it applies to (logits alone
     are too weak a witness, so the GPU tests always check gradients).
  3. The same mutations planted in the bf16-rounding oracle break the two-sided bf16 form (some tensor has eh > fac eo + slack):
     the bf16 legs can see them.  Mutations the bf16 form cannot see at these sizes: none.
  4. The Python-side refusals of an illegal (configuration, precision) pair sit behind the library handle
     (UniterModel._ensure_handle), which needs the GPU: they are in the GPU file.
"""
import numpy as np
import pytest
import torch

import config_space_ref as CS


@pytest.mark.parametrize('train', [False, True], ids=['eval', 'train'])
@pytest.mark.parametrize('name', list(CS.CONFIGS))
def test_float32_oracle_is_a_twentieth_of_the_bars(name, train):
    ref = CS.reference_step(name, train)
    f32 = CS.reference_step(name, train, None, 'fp32', torch.float32)
    shares = CS.fp32_shares(f32, ref)
    w = CS.worst(shares)
    print('%s %s: worst share %.4f (%s), logits %.2e' % (name, 'train' if train else 'eval', w[0], w[1],
                                                         np.abs(f32['logits'] - ref['logits']).max()))
    assert w[0] <= 0.05, w
    # the case really has what it is there for: a nonzero loss gradient everywhere but the mask embedding
    zero = [k for k, r in ref.items() if k.startswith('grad/') and not np.abs(r).max() > 0]
    assert zero == ['grad/uniter_model.img_embeddings.mask_embedding.weight'], zero


def test_the_cases_are_the_ones_the_issue_names():
    assert [CS.pieces_for(CS.cfg(n)['intermediate_size']) for n in CS.CONFIGS] == [1, 1, 5, 1, 8]
    assert CS.pieces_for(64) == 1 and CS.pieces_for(128) == 2
    assert sorted(CS.ILLEGAL) == sorted([('h320_i100', 'fp32x3'), ('h320_i100', 'bf16'), ('h64_i96_l1', 'bf16'), ('h128_i32', 'bf16'),
                                         ('h1024_i1056_l1', 'bf16')])
    assert len(CS.LEGAL) == 15
    b = CS.batch('h64_i96_l1')
    assert b['attn_mask'].sum(1).tolist() == [18.0, 9.0, 7.0]


CASES = [(n, mu) for n in CS.CONFIGS for mu in CS.MUTATIONS if CS.applies(mu, n)]


@pytest.mark.parametrize('name,mutation', CASES)
def test_every_mutation_breaks_a_gradient_bar_tenfold(name, mutation):
    ref = CS.reference_step(name, True)
    mut = CS.reference_step(name, True, mutation)
    shares = CS.fp32_shares(mut, ref)
    wg, wl = CS.worst(shares, 'grad/'), shares['logits']
    print('%s %s: gradient %.1f x its bar (%s), logits %.1f x' % (name, mutation, wg[0], wg[1], wl))
    assert wg[0] >= 10.0, (wg, wl)


@pytest.mark.parametrize('name,mutation', CASES)
def test_every_mutation_breaks_the_bf16_form(name, mutation):
    ref = CS.reference_step(name, True)
    orc = CS.reference_step(name, True, None, 'bf16', torch.float32)
    mut = CS.reference_step(name, True, mutation, 'bf16', torch.float32)
    clean, _ = CS.bf16_shares(orc, ref, orc)
    assert CS.worst(clean, 'grad/')[0] <= 1.0            # the unmutated oracle passes its own form (eh = eo)
    shares, _ = CS.bf16_shares(mut, ref, orc)
    wg = CS.worst(shares, 'grad/')
    print('%s %s: bf16 form, gradient share %.1f (%s), logits share %.2f' % (name, mutation, wg[0], wg[1], shares['logits']))
    assert wg[0] > 1.0, wg
