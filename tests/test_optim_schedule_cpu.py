"""FusedAdam.step's launch schedule is a value (trainer.optim_schedule): which ranges run on which stream, on which grid, behind
which grad_ready wait, and which events the next forward pass gets.  No GPU, no library.

The layout is the smallest with every block kind and a word table that does not fill its bucket: 2 layers, buckets
[head 0..128 | layer 1 128..384 | layer 0 384..640 | embeddings 640..960], word table 640..832 (3 rows of 64)."""
import inspect
import itertools
import os
import re

import pytest

from meme_challenge_amd import trainer
from meme_challenge_amd.trainer import Launch, OptimSwitches, UniterHipError, optim_schedule

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUMEL, WGS = 960, 256
HEAD, LAYER1, LAYER0, EMB, WORD = (0, 128), (128, 384), (384, 640), (640, 960), (640, 832)
PLAN = ([HEAD], [EMB, LAYER0, LAYER1], WORD)                 # _overlap_plan: (head, [embeddings, layer 0, layer 1], word table)
WT = (640, 3, 64, 'uniter_model.embeddings.word_embeddings.weight')         # _word_table: (offset, rows, row length, name)
# the same without a head bucket: [layer 1 0..256 | layer 0 256..512 | embeddings 512..832], word table 512..704
NUMEL_NH = 832
PLAN_NH = ([], [(512, 832), (256, 512), (0, 256)], (512, 704))
WT_NH = (512, 3, 64, WT[3])


def switches(word_split=True, emb_main=True, word_wgs=None):
    return OptimSwitches(overlap_wgs=None, word_rows=False, lazy_zero=True, word_split=word_split, emb_main=emb_main,
                         word_wgs=word_wgs, early_wgs=None)


F = False
LAYERS = [Launch('flat', 384, 640, 'side', 256, None, 'block', F), Launch('flat', 128, 384, 'side', 256, None, 'block', F)]


def test_schedules_record_by_record():
    """Whole schedules, written out from the rules the step has followed since the word table became its own launch (DESIGN.md
    section 4, "The step's tail and head"), not from the function's output."""
    # no overlap: one launch over everything on the caller's stream
    assert optim_schedule(NUMEL, None, None, False, WGS, switches()) == [Launch('flat', 0, 960, 'main', 0, None, None, F)]
    # overlap, UNITER_ADAM_WORD_SPLIT=0: head on the main stream; embeddings (whole chip), layer 0, layer 1 on the side stream
    assert optim_schedule(NUMEL, PLAN, None, False, WGS, switches(word_split=False)) == [
        Launch('flat', 0, 128, 'main', 0, None, None, F), Launch('flat', 640, 960, 'side', 0, None, 'block', F)] + LAYERS
    # overlap, the word table its own launch (side stream, min(2048, 4 x 256) workgroups, the extra event), the embeddings' remainder
    # behind it on the MAIN stream with the embeddings' event
    assert optim_schedule(NUMEL, PLAN, None, False, WGS, switches()) == [
        Launch('flat', 0, 128, 'main', 0, None, None, F), Launch('flat', 640, 832, 'side', 1024, None, 'word', F),
        Launch('flat', 832, 960, 'main', 0, None, 'block', F)] + LAYERS
    # ... with rows updated ahead: the table's launch takes the looked-up rows and the mask is cleared behind it
    assert optim_schedule(NUMEL, PLAN, WT, False, WGS, switches()) == [
        Launch('flat', 0, 128, 'main', 0, None, None, F), Launch('rows', 640, 832, 'side', 1024, None, 'word', True),
        Launch('flat', 832, 960, 'main', 0, None, 'block', F)] + LAYERS
    # with grad_ready (or UNITER_ADAM_EMB_MAIN=0) the remainder goes FIRST on the side stream, the table behind it; every launch
    # waits for its own range on its own stream
    assert optim_schedule(NUMEL, PLAN, None, True, WGS, switches()) == [
        Launch('flat', 0, 128, 'main', 0, (0, 128), None, F), Launch('flat', 832, 960, 'side', 0, (832, 960), 'block', F),
        Launch('flat', 640, 832, 'side', 1024, (640, 832), 'word', F),
        Launch('flat', 384, 640, 'side', 256, (384, 640), 'block', F), Launch('flat', 128, 384, 'side', 256, (128, 384), 'block', F)]
    assert optim_schedule(NUMEL, PLAN, None, False, WGS, switches(emb_main=False))[1:3] == [
        Launch('flat', 832, 960, 'side', 0, None, 'block', F), Launch('flat', 640, 832, 'side', 1024, None, 'word', F)]
    # no overlap, rows updated ahead: in front of the table, its looked-up rows, behind it -- behind ONE wait for the whole buffer
    assert optim_schedule(NUMEL, None, WT, True, WGS, switches()) == [
        Launch('flat', 0, 640, 'main', 0, (0, 960), None, F), Launch('rows', 640, 832, 'main', 0, None, None, F),
        Launch('flat', 832, 960, 'main', 0, None, None, F)]


LAYOUTS = {'plain': (NUMEL, None, WT), 'head': (NUMEL, PLAN, WT), 'no_head': (NUMEL_NH, PLAN_NH, WT_NH)}


@pytest.mark.parametrize('layout,rows,ready,emb_main,word_split',
                         list(itertools.product(LAYOUTS, (False, True), (False, True), (True, False), (True, False))))
def test_schedule_properties(layout, rows, ready, emb_main, word_split):
    numel, plan, wt = LAYOUTS[layout]
    args = (numel, plan, wt if rows else None, ready, WGS, switches(word_split, emb_main))
    if plan is not None and rows and not word_split:
        with pytest.raises(UniterHipError, match='needs the word table as its own optimizer launch'):
            optim_schedule(*args)
        return
    s = optim_schedule(*args)
    # the launches tile [0, numel) exactly once (the rows launch counts as the table's range)
    spans = sorted((r.lo, r.hi) for r in s)
    assert spans[0][0] == 0 and spans[-1][1] == numel and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    table = (wt[0], wt[0] + wt[1] * wt[2])
    assert [(r.lo, r.hi) for r in s if r.kind == 'rows'] == ([table] if rows else [])
    if plan is None:
        # one stream, no events, no grid cap, the mask left to the step's bookkeeping; ONE wait for the whole buffer in front of
        # the first launch (its own range unless rows were updated ahead: then the three launches share it, as they always did)
        assert all((r.stream, r.max_wgs, r.event, r.clear_mask) == ('main', 0, None, False) for r in s)
        assert [r.wait for r in s] == [(0, numel) if ready else None] + [None] * (len(s) - 1)
        assert len(s) == (3 if rows else 1)
        return
    head, blocks, word = plan
    emb, layer0, layer1 = blocks
    inside = lambda r, b: b[0] <= r.lo and r.hi <= b[1]
    # the head stays on the main stream, in front of everything else, without an event
    assert [(r.lo, r.hi) for r in s[:len(head)]] == head
    assert all(r.stream == 'main' and r.event is None and r.max_wgs == 0 for r in s[:len(head)])
    # the side stream sees the embeddings before layer 0 before layer 1
    side = [r for r in s if r.stream == 'side']
    order = [0 if inside(r, emb) else 1 if inside(r, layer0) else 2 if inside(r, layer1) else 3 for r in side]
    assert order == sorted(order) and set(order) == {0, 1, 2}
    # the only launch on the main stream besides the head: the embeddings' remainder, under UNITER_ADAM_EMB_MAIN without grad_ready
    main_rest = [(r.lo, r.hi) for r in s[len(head):] if r.stream == 'main']
    assert main_rest == ([(word[1], emb[1])] if (word_split and emb_main and not ready) else [])
    # events in the forward's order: embeddings, layer 0, layer 1 -- plus the word table's when it is its own launch
    assert [(r.lo, r.hi) for r in s if r.event == 'block'] == [(word[1], emb[1]) if word_split else emb, layer0, layer1]
    assert [(r.lo, r.hi) for r in s if r.event == 'word'] == ([word] if word_split else [])
    assert all(r.event in (None, 'block', 'word') for r in s)
    # a grad_ready wait covers exactly its launch's range (on that launch's stream: tests/test_optim_step_cpu.py)
    assert all(r.wait == ((r.lo, r.hi) if ready else None) for r in s)
    # grids: embeddings 0 (the whole chip), layers the overlap grid, the word table min(2048, 4 x the overlap grid)
    for r in s[len(head):]:
        want = 1024 if (word_split and (r.lo, r.hi) == word) else 0 if inside(r, emb) else WGS
        assert r.max_wgs == want, r
    # the mask is cleared behind the rows launch, and only there
    assert [r.kind for r in s if r.clear_mask] == (['rows'] if rows else [])


def test_word_table_grid():
    word = lambda *a, **kw: [r.max_wgs for r in optim_schedule(*a, **kw) if r.event == 'word']
    assert word(NUMEL, PLAN, None, False, 1024, switches()) == [2048]            # fp32x3's overlap grid: capped at 2048
    assert word(NUMEL, PLAN, None, False, 64, switches()) == [256]
    assert word(NUMEL, PLAN, WT, True, 256, switches(word_wgs=77)) == [77]          # UNITER_ADAM_WORD_WGS
    assert word(NUMEL, PLAN, None, False, 256, switches(word_wgs=0)) == [0]


def test_rows_ahead_errors():
    # the table is not its own launch: switched off, or a table the plan does not know at that offset
    with pytest.raises(UniterHipError, match='UNITER_ADAM_WORD_SPLIT=0 or an unexpected parameter layout'):
        optim_schedule(NUMEL, PLAN, WT, False, WGS, switches(word_split=False))
    with pytest.raises(UniterHipError, match='needs the word table as its own optimizer launch'):
        optim_schedule(NUMEL, (PLAN[0], PLAN[1], None), WT, False, WGS, switches())
    with pytest.raises(UniterHipError, match='needs the word table as its own optimizer launch'):
        optim_schedule(NUMEL, PLAN, (704, 2, 64, WT[3]), False, WGS, switches())


def test_switches_are_read_in_one_place(monkeypatch):
    names = [name for _, name, _ in trainer.OPTIM_SWITCHES]
    assert sorted(names) == ['UNITER_ADAM_EARLY_WGS', 'UNITER_ADAM_EMB_MAIN', 'UNITER_ADAM_OVERLAP_WGS', 'UNITER_ADAM_WORD_ROWS',
                             'UNITER_ADAM_WORD_SPLIT', 'UNITER_ADAM_WORD_WGS', 'UNITER_LAZY_ZERO']
    for name in names:
        monkeypatch.delenv(name, raising=False)
    assert trainer.optim_switches() == OptimSwitches(None, False, True, True, True, None, None)
    for name, value in zip(names, ('512', '1', '0', '0', '0', '96', '48')):
        monkeypatch.setenv(name, value)
    assert trainer.optim_switches() == OptimSwitches(512, True, False, False, False, 96, 48)
    # an empty value: the default for the grid read at construction, refused (int('')) for the grids read at the call, as ever
    monkeypatch.setenv('UNITER_ADAM_OVERLAP_WGS', '')
    assert trainer.optim_switches().overlap_wgs is None
    monkeypatch.setenv('UNITER_ADAM_WORD_WGS', '')
    with pytest.raises(ValueError):
        trainer.optim_switches()
    src = inspect.getsource(trainer)
    assert src.count('os.environ') == 1 and 'os.environ' in inspect.getsource(trainer.optim_switches) and 'getenv' not in src
    with open(os.path.join(REPO, 'INTEGRATION.md')) as f:
        doc = f.read()
    assert not [n for n in names if not re.search(r'`%s\b' % n, doc)]
