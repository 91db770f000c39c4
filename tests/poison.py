"""Allocation poisoning for the tests (test infrastructure): inside `Poison`, every `torch.empty` / `torch.empty_like` issued from a
`meme_challenge_amd` module returns a tensor whose bytes are chosen by the test instead of left to the allocator, and that sits
between two guard bands.

The contract it checks: a pass reads no byte of a workspace or output buffer that the same pass did not write first, and
writes nothing outside the sizes it asked for.  A read-before-write then shows as a result that depends on the fill, an overrun as
a broken guard band.

    with Poison('ones') as p:
        ... run the pass ...
    p.sites            # {'model.py:_get_ws:979': 1, ...}: what was poisoned, by call site
    p.broken           # [] -- Poison.__exit__ raises GuardBandError itself unless check=False

Scope: the package modules' global `torch` is replaced by a forwarding proxy whose `empty` / `empty_like` are wrapped (through a
`pytest.MonkeyPatch` of the harness's own, undone at exit); the rest of the process keeps the real functions.  `UniterModel._get_ws` is wrapped as well:
the workspace is the bytes the library asked for less the WS_SLACK bytes uniter_model_ws_bytes adds on top of its plan (the plan
carves from the block's own 256-byte-aligned start, so it needs none of them), and in training not the largest size seen so far:
the block ends where the planned size ends, so that an overrun of a single byte lands in the back guard band.

Layout of one allocation (bytes):  [slack to a 256-byte boundary][front band][payload][back band]; the bands are 4 KiB, 64 KiB
around the model workspace, filled with GUARD; the payload starts on a 256-byte boundary and the back band at its last byte + 1.

Fills: 'zeros' 0x00; 'ones' 0xFF (an fp32 NaN, a bf16 NaN, integer -1, every keep flag set); 'unit' the bytes of fp32 1.0f (finite
and plausible; 0 and 1.0 alternating as bf16): the fill that imitates stale data; 'replay' the payload bytes an earlier Poison
captured at its exit (`Poison(..., capture=True).captured`), call site by call site in allocation order -- where the earlier pass
has no allocation of that site and ordinal, or another size, the site's bytes are repeated or cut to fit, and a site it never saw
gets 'unit'.

With POISON_REPORT=<file> in the environment every Poison appends its call sites and counts to that file at exit (how the list in
DESIGN.md was made)."""
import collections
import os
import sys
import types

import pytest
import torch as _torch

FILLS = ('zeros', 'ones', 'unit', 'replay')
GUARD = 0xC3
BAND, BAND_WS = 4096, 65536
ALIGN = 256
WS_SLACK = 256            # what uniter_model_ws_bytes returns beyond the plan it carved (csrc/model.cpp)
PACKAGE = 'meme_challenge_amd'
_UNIT_WORD = 0x3F800000          # fp32 1.0f


class GuardBandError(AssertionError):
    pass


def package_modules():
    """the modules of the package that have a global `torch`, every one imported first: a module that is first imported inside
    the context (by a function-level import) would otherwise keep the real torch and go unpoisoned without a word"""
    import importlib
    import pkgutil
    import meme_challenge_amd
    for info in pkgutil.iter_modules(meme_challenge_amd.__path__):
        if not info.ispkg:
            try:
                importlib.import_module(PACKAGE + '.' + info.name)
            except ImportError:          # (an optional dependency of a module the tests do not drive)
                pass
    return [m for n, m in sorted(sys.modules.items())
            if (n == PACKAGE or n.startswith(PACKAGE + '.')) and isinstance(m, types.ModuleType)
            and m.__dict__.get('torch') is not None]


def _fill_unit(u8):
    n4 = u8.numel() // 4
    if n4:
        u8[:4 * n4].view(_torch.int32).fill_(_UNIT_WORD)
    for i, byte in enumerate((0x00, 0x00, 0x80, 0x3F)[:u8.numel() - 4 * n4]):
        u8[4 * n4 + i] = byte


class _Record(object):
    __slots__ = ('site', 'base', 'start', 'nbytes', 'band')

    def payload(self):
        return self.base[self.start:self.start + self.nbytes]

    def bands(self):
        return (self.base[self.start - self.band:self.start],
                self.base[self.start + self.nbytes:self.start + self.nbytes + self.band])


class _TorchProxy(object):
    """stands where a package module's global `torch` stood: everything is the real module's, but empty / empty_like"""

    def __init__(self, owner):
        object.__setattr__(self, '_owner', owner)

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        setattr(_torch, name, value)

    def empty(self, *size, **kw):
        return self._owner._empty(size, kw, sys._getframe(1))

    def empty_like(self, t, **kw):
        return self._owner._empty_like(t, kw, sys._getframe(1))


class Poison(object):
    def __init__(self, fill='ones', replay=None, capture=False, check=True):
        if fill not in FILLS:
            raise ValueError('fill must be one of %s' % (FILLS,))
        if fill == 'replay' and not replay:
            raise ValueError("fill 'replay' needs the `captured` of an earlier Poison")
        self._mp = None
        self._fill = fill
        self._replay = replay or {}
        self._capture = capture
        self._check = check
        self.records = []
        self.sites = collections.Counter()          # 'file.py:function:line' -> allocations poisoned
        self.passed_through = collections.Counter() # call sites whose arguments the harness does not rebuild (left to torch)
        self.captured = {}                          # site -> [uint8 tensor per allocation], filled at exit with capture=True
        self.broken = []                            # (site, 'front' | 'back', first broken offset) found at exit
        self._ordinal = collections.Counter()
        self._active = False

    # -- the fill may change between the passes of one context (a trajectory whose fill rotates) --
    @property
    def fill(self):
        return self._fill

    @fill.setter
    def fill(self, fill):
        if fill not in FILLS or (fill == 'replay' and not self._replay):
            raise ValueError('bad fill %r' % (fill,))
        self._fill = fill
        self._ordinal.clear()

    def functions(self):
        """the poisoned call sites without their line numbers: {'model.py:_get_ws', ...}"""
        return {s.rsplit(':', 1)[0] for s in self.sites}

    def count(self, function):
        return sum(n for s, n in self.sites.items() if s.rsplit(':', 1)[0] == function)

    def report(self):
        return '\n'.join('%6d  %s' % (n, s) for s, n in sorted(self.sites.items()))

    # -- context ---------------------------------------------------------------------------------------------------------------
    def __enter__(self):
        proxy = _TorchProxy(self)
        mods = package_modules()
        if not mods:
            raise RuntimeError('no module of %s with a global torch is imported: nothing to poison' % PACKAGE)
        self._mp = mp = pytest.MonkeyPatch()
        for m in mods:
            mp.setattr(m, 'torch', proxy)
        model = sys.modules.get(PACKAGE + '.model')
        if model is not None:
            real = model.UniterModel._get_ws

            def _get_ws(this, nbytes, mode):
                if mode != 0:
                    this._ws_high = 0          # the training workspace: this pass's size, not the largest seen so far
                return real(this, max(nbytes - WS_SLACK, 0), mode)
            mp.setattr(model.UniterModel, '_get_ws', _get_ws)
        self._active = True
        return self

    def __exit__(self, et, ev, tb):
        self._active = False
        self._mp.undo()
        if _torch.cuda.is_available() and any(r.base.is_cuda for r in self.records):
            _torch.cuda.synchronize()
        for r in self.records:
            for side, band in zip(('front', 'back'), r.bands()):
                bad = band != GUARD
                if bool(bad.any()):
                    self.broken.append((r.site, side, int(_torch.nonzero(bad)[0])))
        if self._capture:
            for r in self.records:
                self.captured.setdefault(r.site, []).append(r.payload().clone())
        path = os.environ.get('POISON_REPORT')
        if path:
            with open(path, 'a') as f:
                for s, n in sorted(self.sites.items()):
                    f.write('%s %d\n' % (s, n))
        if et is None and self._check and self.broken:
            raise GuardBandError('guard bands overwritten: %s' % (self.broken[:8],))
        return False

    # -- the wrapped allocators ------------------------------------------------------------------------------------------------
    @staticmethod
    def _site(frame):
        code = frame.f_code
        return '%s:%s:%d' % (os.path.basename(code.co_filename), code.co_name, frame.f_lineno)

    def _empty(self, size, kw, frame):
        site = self._site(frame)
        extra = set(kw) - {'dtype', 'device', 'requires_grad'}
        if extra or not self._active:
            self.passed_through[site] += 1
            return _torch.empty(*size, **kw)
        if len(size) == 1 and isinstance(size[0], (tuple, list, _torch.Size)):
            size = tuple(size[0])
        shape = tuple(int(s) for s in size)
        dtype = kw.get('dtype') or _torch.get_default_dtype()
        device = _torch.device(kw['device']) if kw.get('device') is not None else _torch.empty(0).device
        return self._make(shape, dtype, device, bool(kw.get('requires_grad', False)), site, frame.f_code.co_name == '_get_ws')

    def _empty_like(self, t, kw, frame):
        site = self._site(frame)
        extra = set(kw) - {'dtype', 'device', 'requires_grad'}
        if extra or not self._active:
            self.passed_through[site] += 1
            return _torch.empty_like(t, **kw)
        dtype = kw.get('dtype') or t.dtype
        device = _torch.device(kw['device']) if kw.get('device') is not None else t.device
        # torch.empty_like keeps the strides of a dense source that is not contiguous (a transposed one): ask torch which
        strides = _torch.empty_like(t, dtype=dtype, device='meta').stride()
        return self._make(tuple(t.shape), dtype, device, bool(kw.get('requires_grad', False)), site, False, strides)

    def _make(self, shape, dtype, device, requires_grad, site, is_ws, strides=None):
        numel = 1
        for s in shape:
            numel *= s
        item = _torch.empty(0, dtype=dtype).element_size()
        nbytes = numel * item
        band = BAND_WS if is_ws else BAND
        base = _torch.empty(ALIGN + band + nbytes + band, dtype=_torch.uint8, device=device)
        base.fill_(GUARD)
        r = _Record()
        r.site, r.base, r.nbytes, r.band = site, base, nbytes, band
        r.start = (-base.data_ptr()) % ALIGN + band
        payload = r.payload()
        k = self._ordinal[site]
        self._ordinal[site] += 1
        self._fill_payload(payload, site, k)
        if base.is_cuda:
            # the fill runs on the current stream; the library may first touch the buffer on another one (side / auxiliary stream)
            _torch.cuda.current_stream(base.device).synchronize()
        self.records.append(r)
        self.sites[site] += 1
        out = payload.view(dtype).view(shape) if numel else _torch.empty(shape, dtype=dtype, device=device)
        if numel and strides is not None and tuple(strides) != tuple(out.stride()):
            out = out.as_strided(shape, strides)           # (a permutation of the same numel elements: dense, inside the payload)
        if requires_grad:
            out.requires_grad_(True)
        return out

    def _fill_payload(self, u8, site, k):
        if u8.numel() == 0:
            return
        if self._fill == 'zeros':
            u8.zero_()
        elif self._fill == 'ones':
            u8.fill_(0xFF)
        elif self._fill == 'replay' and self._replay.get(site):
            olds = self._replay[site]
            old = olds[k % len(olds)].to(u8.device)
            n = u8.numel()
            if old.numel() == 0:
                _fill_unit(u8)
            elif old.numel() >= n:
                u8.copy_(old[:n])
            else:
                u8.copy_(old.repeat((n + old.numel() - 1) // old.numel())[:n])
        else:
            _fill_unit(u8)

