"""Parameter groups and frozen parameters of the fused optimizer step, the parts that are plain values (no GPU, no library): the
group layout a `group_param_func` gives (trainer.group_layout: utils/optim_utils.py:9-30), the flag bytes (trainer.chunk_flag_bytes:
the group index in bits 3-7, frozen tensors 0, the keep bit) and optim_schedule dropping the launches of all-frozen blocks."""
from collections import namedtuple

import pytest

from meme_challenge_amd import trainer as T

NAMES = ['base.embeddings.word_embeddings.weight', 'base.embeddings.LayerNorm.weight', 'base.encoder.layer.0.output.dense.weight',
         'base.encoder.layer.0.output.dense.bias', 'head.weight', 'head.bias']
NAMED = [(n, object()) for n in NAMES]


def _head_base(named):
    return [{'params': [(n, p) for n, p in named if n.startswith('head')], 'lr': 1e-2, 'tag': 'head'},
            {'params': [(n, p) for n, p in named if not n.startswith('head')], 'lr': 1e-3, 'weight_decay': 123.0}]


def test_layout_follows_the_reference_order_and_copies_the_keys():
    out = T.group_layout(NAMED, 0.05, _head_base)
    assert [[n for n, _ in g['params']] for g in out] == [['head.weight'], ['head.bias'],
                                                        [NAMES[0], NAMES[2]], [NAMES[1], NAMES[3]]]
    assert [g['weight_decay'] for g in out] == [0.05, 0.0, 0.05, 0.0]            # the config's, not a group's own 'weight_decay' key
    assert [g['lr'] for g in out] == [1e-2, 1e-2, 1e-3, 1e-3]
    assert out[0]['tag'] == out[1]['tag'] == 'head' and 'tag' not in out[2]
    assert all(p is dict(NAMED)[n] for g in out for n, p in g['params'])         # the parameters themselves, not copies
    # no function: one group of everything, split in two -- the layout FusedAdam always had
    two = T.group_layout(NAMED, 0.05)
    assert len(two) == 2 and set(two[0]) == {'params', 'weight_decay'}
    assert [n for n, _ in two[1]['params']] == [NAMES[1], NAMES[3], NAMES[5]]


@pytest.mark.parametrize('bad, word', [
    (lambda named: None, 'list'),
    (lambda named: [], 'list'),
    (lambda named: [{'lr': 1.0}], 'list'),
    (lambda named: [{'params': [p for _, p in named]}], 'list'),
    (lambda named: [{'params': named}, {'params': named[:1]}], 'twice'),
    (lambda named: [{'params': named[1:]}], 'out'),
    (lambda named: [{'params': named + [('nobody', None)]}], 'no parameter'),
    (lambda named: [{'params': named}] + [{'params': []}] * 16, 'at most 16'),
])
def test_layout_refuses_what_is_no_grouping(bad, word):
    with pytest.raises(T.UniterHipError) as e:
        T.group_layout(NAMED, 0.05, bad)
    assert word in str(e.value)


def test_sixteen_groups_are_accepted():
    out = T.group_layout(NAMED, 0.05, lambda named: [{'params': named}] + [{'params': []}] * 15)
    assert len(out) == 32 == T.MAX_PARAM_GROUPS


def test_flag_bytes_carry_group_frozen_and_keep():
    """a (128), b (64 + 1: two chunks), c (64), d (192), e (64) on chunk boundaries; e receives no gradient"""
    sizes = dict(a=128, b=65, c=64, d=192, e=64)
    offsets = dict(a=0, b=128, c=256, d=320, e=512)
    touched = ['a', 'b', 'c', 'd']
    bits = dict(a=(0, True), b=(1, False), c=(2, True), d=(31, True), e=(3, True))
    got = T.chunk_flag_bytes(9, offsets, sizes, touched, frozen={'c'}, keep={'d'}, group_bits=bits)
    assert got.tolist() == [2, 2, 8 | 1, 8 | 1, 0, 248 | 6, 248 | 6, 248 | 6, 0]
    # the bytes every other entry point takes: by name, no group bits -- what FusedAdam wrote before there were groups
    sizes = {'w.weight': 128, 'w.bias': 64, 'LayerNorm.weight': 64}
    offsets = {'w.weight': 0, 'w.bias': 128, 'LayerNorm.weight': 192}
    assert T.chunk_flag_bytes(4, offsets, sizes, list(sizes), keep={'w.weight'}).tolist() == [6, 6, 1, 1]
    assert T.chunk_flag_bytes(4, offsets, sizes, list(sizes), frozen={'w.weight'}, keep={'w.weight'}).tolist() == [0, 0, 1, 1]
    assert T.chunk_flag_bytes(4, offsets, sizes, []).tolist() == [0, 0, 0, 0]


SW = namedtuple('SW', 'word_split emb_main word_wgs')(True, True, None)
PLAN = ([(0, 128)], [(640, 960), (384, 640), (128, 384)], (640, 832))       # head | embeddings, layer 0, layer 1 | the word table


def test_schedule_drops_all_frozen_blocks_and_keeps_its_default():
    full = T.optim_schedule(960, PLAN, None, False, 256, SW)
    assert [(r.lo, r.hi) for r in full] == [(0, 128), (640, 832), (832, 960), (384, 640), (128, 384)]
    assert T.optim_schedule(960, PLAN, None, False, 256, SW, trainable=None) == full
    assert T.optim_schedule(960, PLAN, None, False, 256, SW, trainable=[(0, 960)]) == full
    # embeddings and layer 0 frozen: their three launches and three events are gone, the others are the launches they were
    live = T.optim_schedule(960, PLAN, None, False, 256, SW, trainable=[(0, 100), (128, 384)])
    assert live == [full[0], full[4]] and [r.event for r in live] == [None, 'block']
    # one trainable tensor inside the embeddings' remainder keeps that launch alone
    assert T.optim_schedule(960, PLAN, None, True, 256, SW, trainable=[(900, 901)]) == \
        [r for r in T.optim_schedule(960, PLAN, None, True, 256, SW) if (r.lo, r.hi) == (832, 960)]
    # without a plan: the one launch, or none
    assert T.optim_schedule(960, None, None, False, 256, SW, trainable=[(5, 6)]) == T.optim_schedule(960, None, None, False, 256, SW)
    assert T.optim_schedule(960, None, None, False, 256, SW, trainable=[]) == []


# ---------------------------------------------------------------------------------------------------------------------------
# the step itself, call by call, under the stand-ins of tests/test_optim_step_cpu.py
# ---------------------------------------------------------------------------------------------------------------------------
def _head_lr(named):
    return [{'params': [e for e in named if e[0].startswith('head')], 'lr': 1e-2},
            {'params': [e for e in named if not e[0].startswith('head')]}]


def _entries(log):
    return [line.split('(')[0] for line in log if line.startswith('uniter_') and not line.startswith('uniter_grad_sumsq')]


def _renumbered(log):
    """the log with its events numbered from 0 (the stand-ins count events across steps)"""
    import re
    seen = {}
    return [re.sub(r'\bev\d+', lambda m: seen.setdefault(m.group(0), 'ev%d' % len(seen)), line) for line in log]


def test_groups_that_differ_send_every_launch_through_the_grouped_entry_point(monkeypatch):
    import test_optim_step_cpu as S
    drive = S.harness(monkeypatch)
    log = drive(init=dict(group_param_func=_head_lr), overlap=True, clip=0.05, lazy=True, mirror=3)
    assert _entries(log) == ['uniter_optim_step_groups'] * 5
    assert all(', 4, 1, 1, ' in line for line in log if line.startswith('uniter_optim_step_groups('))     # four rows, step 1, zero_grads
    assert sum('mirror+' in line and 'pairs+' in line for line in log) == 2                                # the layers' blocks: mirror and pair table
    assert [line for line in log if line.startswith('set_ready_events')] == ['set_ready_events(ev1 ev2 ev3 ev0)']
    # the same grouping with ONE learning rate: the calls of a step without groups, flag bytes included (kind 3 here)
    same = lambda named: [dict(g, lr=1e-3) for g in _head_lr(named)]
    assert _renumbered(drive(cls='FusedSGD', init=dict(group_param_func=same), overlap=True)) == _renumbered(drive(cls='FusedSGD', overlap=True))
    assert _entries(drive(cls='FusedSGD', init=dict(group_param_func=_head_lr))) == ['uniter_optim_step_groups']
    # no row-split update of the word table beside groups
    log = drive(init=dict(group_param_func=_head_lr), rows=True, overlap=True)
    assert 'early_word_update -> False' in log and 'uniter_adam_step_rows' not in _entries(log)


def test_frozen_blocks_are_not_launched_and_the_forward_still_gets_one_event_per_block(monkeypatch):
    import test_optim_step_cpu as S
    drive = S.harness(monkeypatch)
    init = S.Store.__init__

    def frozen_init(self, mirror_pieces):
        init(self, mirror_pieces)
        for n in self.names:
            if 'layer.0' in n or 'embeddings' in n:
                self.params[n].requires_grad = False
    monkeypatch.setattr(S.Store, '__init__', frozen_init)
    log = drive(overlap=True, clip=0.05, armed=True)
    launches = [line for line in log if line.startswith('uniter_adam_step_x3p(')]
    assert [line.split(', ')[0] for line in launches] == ['uniter_adam_step_x3p(flat_params+0', 'uniter_adam_step_x3p(flat_params+512']
    assert any(line.startswith('uniter_grad_sumsq(') for line in log) and not any('combine' in line for line in log)
    # embeddings and layer 0 share an event that the main stream has already passed; layer 1 has its own
    assert 'ev1.record(main)' in log and 'set_ready_events(ev1 ev1 ev0)' in log and log[-1].startswith('pending=ev0 ')


def _freeze(monkeypatch, S, which):
    """the stand-in store with requires_grad cleared on the tensors whose name `which` accepts"""
    init = S.Store.__init__

    def frozen_init(self, mirror_pieces):
        init(self, mirror_pieces)
        for n in self.names:
            if which(n):
                self.params[n].requires_grad = False
    monkeypatch.setattr(S.Store, '__init__', frozen_init)


@pytest.mark.parametrize('overlap', [False, True])
def test_a_frozen_word_table_is_not_updated_by_rows(monkeypatch, overlap):
    """UNITER_ADAM_WORD_ROWS=1 beside frozen embeddings (what freeze_prefix leaves): the row-split launches know no frozen chunk, so
    there is no split -- no mask, no ahead-of-time launch, and no launch of the step reaches into the table (elements 640 .. 832)"""
    import test_optim_step_cpu as S
    drive = S.harness(monkeypatch)
    _freeze(monkeypatch, S, lambda n: 'embeddings' in n)
    log = drive(rows=True, overlap=overlap, clip=0.05)
    assert 'early_word_update -> False' in log and 'uniter_adam_step_rows' not in _entries(log)
    assert not any('rowmask' in line for line in log) and 'noted=False' in log[-1] and 'mask_clear=None' in log[-1]
    starts = [line.split(', ')[0] for line in log if line.startswith('uniter_adam_step_x3p(')]
    assert starts == (['uniter_adam_step_x3p(flat_params+0'] if not overlap else
                      ['uniter_adam_step_x3p(flat_params+%d' % (4 * lo) for lo in (0, 384, 128)])
    if not overlap:         # one launch over everything: the table's chunks carry flag 0
        import torch
        st = S.Store(0)
        opt = T.FusedAdam(st, lr=1e-3)
        st.touched.update(st.names)
        assert torch.count_nonzero(opt._chunk_flags()[640 // 64:]) == 0 and torch.count_nonzero(opt._chunk_flags()[:640 // 64]) == 10


def test_nothing_trainable_in_any_block_clears_the_forward_pass_events(monkeypatch):
    import test_optim_step_cpu as S
    drive = S.harness(monkeypatch)
    _freeze(monkeypatch, S, lambda n: not n.startswith('head'))
    log = drive(overlap=True)
    assert _entries(log) == ['uniter_adam_step_x3p'] and 'set_ready_events()' in log and log[-1].startswith('pending=None ')


def test_only_the_word_table_trainable_still_gates_the_forward_pass(monkeypatch):
    import test_optim_step_cpu as S
    drive = S.harness(monkeypatch)
    _freeze(monkeypatch, S, lambda n: 'word_embeddings' not in n)
    log = drive(overlap=True)
    assert _entries(log) == ['uniter_adam_step_x3p'] and 'ev0.record(side)' in log
    # one (passed) event per block, the word table's own behind them; join() waits for it
    assert 'set_ready_events(ev1 ev1 ev1 ev0)' in log and log[-1].startswith('pending=ev0 ')


@pytest.mark.parametrize('name, cls', [('adam', 'FusedAdam'), ('adamax', 'FusedAdamax'), ('sgd', 'FusedSGD')])
def test_get_optimizer_asks_the_grouping_function_once(monkeypatch, name, cls):
    import test_optim_step_cpu as S
    S.harness(monkeypatch)
    calls = []

    def once(named):
        calls.append([n for n, _ in named])
        return _head_lr(named)
    st = S.Store(0)
    opt = T.get_optimizer(st, dict(optimizer=name, lr=1e-3, beta1=0.9, beta2=0.98, weight_decay=0.01), group_param_func=once)
    assert type(opt).__name__ == cls and calls == [[n for n, _ in st.named_parameters()]]
    assert [g['lr'] for g in opt.param_groups] == [1e-2, 1e-2, 1e-3, 1e-3]
    assert [len(g['params']) for g in opt.param_groups] == [1, 0, 3, 1]
