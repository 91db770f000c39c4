"""FusedAdam.step and early_word_update, call by call, without a GPU: a stand-in library handle records every entry point's
arguments (pointers as buffer+byte offset, scalars verbatim) and stand-in streams and events record wait_stream, wait_event,
record and the stream each grad_ready wait runs on.  The expected logs are those of the step as it was written before its schedule
became a value (optim_schedule) walked by one executor; tests/tools/optim_step_trace.py compares the same on a GPU.

Layout: [head 0..128 | layer 1 128..384 | layer 0 384..640 | embeddings 640..960], word table 640..832 (3 rows of 64)."""
import contextlib
import ctypes as C
import itertools
import os

import pytest
import torch

from meme_challenge_amd import _lib, trainer


class Stream:
    def __init__(self, log, name, handle):
        self.log, self.name, self.cuda_stream = log, name, handle

    def wait_event(self, ev):
        self.log('%s.wait_event(%s)' % (self.name, ev.tag))

    def wait_stream(self, s):
        self.log('%s.wait_stream(%s)' % (self.name, s.name))


class Store:
    def __init__(self, mirror_pieces):
        sizes = [('head.weight', (2, 64)), ('enc.encoder.layer.1.output.dense.weight', (4, 64)),
                 ('enc.encoder.layer.0.output.dense.weight', (4, 64)), ('enc.embeddings.word_embeddings.weight', (3, 64)),
                 ('enc.embeddings.LayerNorm.bias', (128,))]
        self.names, self.offsets, self.params, off = [], {}, {}, 0
        for n, shape in sizes:
            self.names.append(n)
            self.offsets[n], self.params[n] = off, torch.nn.Parameter(torch.zeros(*shape))
            off += self.params[n].numel()
        self.numel = off
        cuts = [self.offsets[n] for n in self.names[:4]] + [off]
        self.bucket_ranges = list(zip(cuts, cuts[1:]))
        self.flat_params, self.flat_grads = torch.zeros(off), torch.zeros(off)
        self.touched, self.device, self.wgrad_stale = set(), torch.device('cpu'), False
        if mirror_pieces:
            self.mirror, self.mirror_pieces = torch.zeros(mirror_pieces * off, dtype=torch.bfloat16), mirror_pieces
            self.pairs = torch.zeros(off // 64, 2, dtype=torch.int32)

    def pair_src(self):
        return self.pairs if getattr(self, 'mirror_pieces', 1) == 3 else None

    def is_current(self):
        return True

    def param_store(self):
        return self

    def named_parameters(self):
        return list(self.params.items())


def harness(monkeypatch):
    """-> drive(**case): the log of one early_word_update (if rows) and one step of a fresh optimizer under the stand-ins"""
    lines, numbers = [], itertools.count()
    log = lines.append
    main, side = Stream(log, 'main', 1111), Stream(log, 'side', 2222)
    current, bufs, owner = [main], {}, []

    class Event:
        def __init__(self, **kw):
            self.tag, self.cuda_event = 'ev%d' % next(numbers), 0

        def record(self, stream=None):
            log('%s.record(%s)' % (self.tag, (stream or current[-1]).name))

    @contextlib.contextmanager
    def stream_context(s):
        current.append(s)
        try:
            yield
        finally:
            current.pop()

    def where(p):
        if not p or p in (1111, 2222):
            return 'NULL' if not p else 'main' if p == 1111 else 'side'
        for name, t in bufs.items():
            if t is not None and t.data_ptr() <= p < t.data_ptr() + t.numel() * t.element_size():
                return '%s+%d' % (name, p - t.data_ptr())
        return 'unknown'

    class Lib:
        def uniter_grad_sumsq_ws_bytes(self, n):
            return 64

        def __getattr__(self, name):
            def entry(*args):
                opt = owner[-1]
                bufs.update(flags=opt._flags, parts=opt._parts, rowmask=opt._rowmask)
                bufs.update({'row_flags': t for k, t in opt._flags_cache.items() if k[0] == 'rows'})
                pointer = lambda a: a is None or isinstance(a, C.c_void_p) or (isinstance(a, int) and a > 1 << 20)
                shown = [where(a.value if isinstance(a, C.c_void_p) else a) if pointer(a) else repr(a) for a in args]
                log('%s(%s)' % (name, ', '.join(shown)))
                return 0
            return entry

    lib = Lib()
    monkeypatch.setattr(_lib, 'lib', lambda: lib)
    monkeypatch.setattr(_lib, 'shared_stream', lambda device, kind='side': side)
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a: current[-1])
    monkeypatch.setattr(torch.cuda, 'Event', Event)
    monkeypatch.setattr(torch.cuda, 'stream', stream_context)
    for name in ('UNITER_ADAM_OVERLAP_WGS', 'UNITER_ADAM_WORD_ROWS', 'UNITER_LAZY_ZERO', 'UNITER_ADAM_WORD_SPLIT',
                 'UNITER_ADAM_EMB_MAIN', 'UNITER_ADAM_WORD_WGS', 'UNITER_ADAM_EARLY_WGS'):
        monkeypatch.delenv(name, raising=False)

    def drive(**case):
        del lines[:]
        for name, value in case.get('env', {}).items():
            monkeypatch.setenv(name, value)
        st = Store(case.get('mirror', 0))
        opt = getattr(trainer, case.get('cls', 'FusedAdam'))(st, lr=1e-3, weight_decay=1e-2, **case.get('init', {}))
        encoder = type('Encoder', (), dict(
            config=type('Config', (), dict(num_hidden_layers=2)), _side_stream=None, precision='fp32',
            _set_ready_events=lambda self, evs: log('set_ready_events(%s)' % ' '.join(e.tag for e in evs))))()
        owner.append(opt)
        bufs.clear()
        bufs.update(flat_params=st.flat_params, flat_grads=st.flat_grads, exp_avg=opt.exp_avg, exp_avg_sq=opt.exp_avg_sq,
                    sumsq=opt._sumsq, ws=opt._ws, mirror=getattr(st, 'mirror', None), pairs=getattr(st, 'pairs', None))
        if case.get('overlap'):
            opt.overlap_encoder = encoder
        if case.get('lazy'):
            opt.lazy_zero_encoder = encoder
        if case.get('armed'):
            bufs['np_buf'] = opt._np_buf = torch.zeros(32, dtype=torch.float64)
            opt._np_blocks = 32
        if case.get('rows'):
            opt.split_word_rows, opt._word_cache = True, None
            opt.note_tokens(torch.tensor([[1, 2]]))
            log('early_word_update -> %r' % opt.early_word_update())
        st.touched.update(st.names)
        kw = {}
        if case.get('payload'):
            kw['grad_bf16'] = bufs['payload'] = torch.zeros(st.numel, dtype=torch.bfloat16)
        if case.get('ready'):
            kw['grad_ready'] = lambda lo, hi: log('grad_ready(%d, %d) on %s' % (lo, hi, current[-1].name))
        if case.get('pieces'):
            kw['grad_pieces'] = [(0, 384), (384, 640), (640, st.numel)]
        try:
            opt.step(grad_scale=0.5, max_grad_norm=case.get('clip', 0.0), **kw)
        except trainer.UniterHipError as e:
            log('UniterHipError: %s' % e)
        log('pending=%s early=%r noted=%r armed=%r mask_clear=%s stale=%r touched=%d encoder_side=%s' % (
            getattr(opt._pending, 'tag', None), opt._early is not None, opt._rows_noted, opt._np_blocks,
            getattr(opt._rowmask_clear, 'tag', None), st.wgrad_stale, len(st.touched), getattr(encoder._side_stream, 'name', None)))
        return list(lines)
    return drive


CASES = {
    'plain_adam': dict(),
    'plain_adamw_bf16_mirror_clip': dict(init=dict(adamw=True), mirror=1, clip=0.05),
    'plain_sgd_ready_pieces_payload_clip': dict(cls='FusedSGD', ready=True, pieces=True, payload=True, clip=0.05),
    'plain_rows_ready': dict(rows=True, ready=True),
    'plain_rows_payload_refused': dict(rows=True, payload=True),
    'overlap_adam': dict(overlap=True),
    'overlap_adamax_x3_mirror_clip_lazy': dict(cls='FusedAdamax', mirror=3, overlap=True, clip=0.05, lazy=True),
    'overlap_armed_clip': dict(overlap=True, armed=True, clip=0.05),
    'overlap_ready': dict(overlap=True, ready=True),
    'overlap_ready_clip_no_pieces': dict(overlap=True, ready=True, clip=0.05),
    'overlap_rows_clip': dict(overlap=True, rows=True, clip=0.05),
    'overlap_rows_ready_grids': dict(overlap=True, rows=True, ready=True, env={'UNITER_ADAM_WORD_WGS': '96', 'UNITER_ADAM_EARLY_WGS': '48',
                                                                              'UNITER_ADAM_OVERLAP_WGS': '77'}),
    'overlap_rows_no_split_refused': dict(overlap=True, rows=True, env={'UNITER_ADAM_WORD_SPLIT': '0'}),
    'overlap_emb_side_no_lazy': dict(overlap=True, lazy=True, env={'UNITER_ADAM_EMB_MAIN': '0', 'UNITER_LAZY_ZERO': '0'}),
}


def golden_logs():
    logs, name = {}, None
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'optim_step_calls.txt')) as f:
        for line in f.read().splitlines():
            if line.startswith('CASE '):
                name = line[5:]
                logs[name] = []
            elif line:
                logs[name].append(line)
    return logs


@pytest.mark.parametrize('name', sorted(CASES))
def test_step_issues_the_recorded_calls(name, monkeypatch):
    got, want = harness(monkeypatch)(**CASES[name]), golden_logs()[name]
    assert got == want, '\n'.join(['got:'] + got + ['want:'] + want)


def test_waits_run_on_the_stream_of_their_launch(monkeypatch):
    """Every grad_ready wait runs on the stream of the launch behind it, and the side stream joins the main stream in front of
    its first launch -- read off the log itself, whatever the golden file says."""
    log = harness(monkeypatch)(overlap=True, ready=True)
    launches = [k for k, line in enumerate(log) if line.startswith('uniter_adam_step_x3p(')]
    assert len(launches) == 5
    for k in launches:
        assert log[k - 1].startswith('grad_ready(') and log[k - 1].rsplit(' ', 1)[1] == log[k].rstrip(')').rsplit(', ', 1)[1]
    first_side = next(k for k in launches if log[k].endswith(', side)'))
    assert log.index('side.wait_stream(main)') == first_side - 2 and sum(line == 'side.wait_stream(main)' for line in log) == 1
