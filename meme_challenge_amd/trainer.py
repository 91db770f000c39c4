"""Training-step semantics of the reference trainer on the HIP path.

Mirrors:
  nn.BCEWithLogitsLoss(pos_weight)            train_template.py:64-65
  TrainerTemplate.calculate_loss              train_template.py:95-126
  TrainerTemplate.average_gradients           train_template.py:89-92
  get_optimizer (group_param_func, param-group split, Adam/AdamW/Adamax/SGD) utils/optim_utils.py:9-46
  init_scheduler (warmup / warmup_cosine / step / multi_step)  train_template.py:72-82
  TrainerUniter.{train,eval,test}_iter_step    train_uniter.py:58-81

The optimizer step (gradient averaging, global-norm clip, Adam/AdamW update,
zero_grad) is ONE fused kernel over the flat parameter buffer
(csrc/optim.hip); the gradient norm stays on the device, so a training
iteration needs no host synchronisation (the reference does `.item()` /
`.cpu()` every iteration, train_template.py:121-124).
"""
import contextlib
import ctypes as C
import math
import os
from collections import namedtuple

import torch

from . import _lib
from ._lib import check, ptr, UniterHipError
from .model import CHUNK, ensure_store


# The optimizer's environment variables (member, variable, parse), read by optim_switches() and nowhere else in this file; None = the
# default.  FusedAdam keeps the first two from its construction and reads the others at every call.  INTEGRATION.md lists the names.
_off_if_0 = lambda v: v != '0'
_int = lambda v: None if v is None else int(v)
OPTIM_SWITCHES = (
    ('overlap_wgs', 'UNITER_ADAM_OVERLAP_WGS', lambda v: int(v) if v else None),    # grid of the blocks beside the next forward
    ('word_rows', 'UNITER_ADAM_WORD_ROWS', lambda v: v == '1'),      # the word table's update split by rows (early_word_update)
    ('lazy_zero', 'UNITER_LAZY_ZERO', _off_if_0),           # =0: zero_grad clears the encoder layers' weight gradients too
    ('word_split', 'UNITER_ADAM_WORD_SPLIT', _off_if_0),    # =0: the word table stays inside the embeddings' block
    ('emb_main', 'UNITER_ADAM_EMB_MAIN', _off_if_0),        # =0: the embeddings' remainder goes back on the side stream
    ('word_wgs', 'UNITER_ADAM_WORD_WGS', _int),             # grid of the word table's launch (min(2048, 4 x the overlap grid))
    ('early_wgs', 'UNITER_ADAM_EARLY_WGS', _int),           # grid of early_word_update's launch (the overlap grid)
)
OptimSwitches = namedtuple('OptimSwitches', [member for member, _, _ in OPTIM_SWITCHES])


def optim_switches():
    """The optimizer's switches as the environment states them now."""
    return OptimSwitches(*[parse(os.environ.get(name)) for _, name, parse in OPTIM_SWITCHES])


# --------------------------------------------------------------------------- #
# loss
# --------------------------------------------------------------------------- #
class _LogitsLossFn(torch.autograd.Function):
    """BCE with logits, one launch forward and none backward.  clean_logits None: uniter_bce_logits -> (loss, probs); else
    uniter_bce_kl_logits (a perturbed pass of VILLA) -> (the view terms[0], terms), its gradient scaled by grad_scale."""
    @staticmethod
    def forward(ctx, logits, clean_logits, labels, pos_weight, kl_weight, grad_scale):
        _lib.require_gpu_tensor(logits, torch.float32, 'logits')
        x = logits.reshape(-1).contiguous()
        y = labels.reshape(-1).to(torch.int64).contiguous()
        B = x.numel()
        dlog = torch.empty(B, dtype=torch.float32, device=x.device)
        if clean_logits is None:
            if B != y.numel():
                raise ValueError('logits/labels size mismatch')
            loss = torch.empty((), dtype=torch.float32, device=x.device)
            extra = torch.empty(B, dtype=torch.float32, device=x.device)       # the probabilities
            check(_lib.lib().uniter_bce_logits(ptr(x), ptr(y), float(pos_weight), ptr(loss), ptr(extra),
                                               ptr(dlog), 1.0, B, _lib.cur_stream()), 'uniter_bce_logits')
        else:
            _lib.require_gpu_tensor(clean_logits, torch.float32, 'clean_logits')
            c = clean_logits.detach().reshape(-1).contiguous()
            if B != y.numel() or B != c.numel():
                raise ValueError('logits/clean_logits/labels size mismatch')
            extra = torch.empty(3, dtype=torch.float32, device=x.device)       # [total, bce, kl]
            check(_lib.lib().uniter_bce_kl_logits(ptr(x), ptr(c), ptr(y), float(pos_weight), float(kl_weight), ptr(extra), None,
                                                  ptr(dlog), float(grad_scale), B, _lib.cur_stream()), 'uniter_bce_kl_logits')
            loss = extra[0]                        # (a view: the total needs no launch of its own)
        ctx.save_for_backward(dlog)
        ctx.shape = logits.shape
        ctx.mark_non_differentiable(extra)
        ctx.set_materialize_grads(False)           # no zero tensor for the second output's (absent) gradient
        return loss, extra

    @staticmethod
    def backward(ctx, dloss, _dextra):
        return (_saved_dlogits(ctx, dloss),) + (None,) * 5


def _saved_dlogits(ctx, dloss):
    """The backward of a loss whose forward launch left d loss / d logits in ctx: that tensor, times dloss unless it is
    unit_gradient's"""
    (dlog,) = ctx.saved_tensors
    if dloss is None:
        return None
    unit = _UNIT.get(dlog.device)
    if unit is not None and dloss.data_ptr() == unit.data_ptr():
        return dlog.view(ctx.shape)                # loss.backward(unit_gradient(..)): d loss = 1, nothing to multiply
    return (dlog * dloss).view(ctx.shape)


AUC_SURROGATES = ('logistic', 'hinge2')            # `kind` 0, 1 of uniter_bce_auc_logits
AUC_MAX_BANK = 8192


class ScoreBank(object):
    """The ring buffer of recent (score, label) pairs that uniter_bce_auc_logits reads and pushes into, in device memory:
    `scores` float32 [capacity], `labels` int32 [capacity], `state` int32 {head, fill} -- head the slot the next push starts
    at, fill the number of valid slots (the most recently pushed ones).  Nothing here reads the device but contents()."""

    def __init__(self, capacity, device):
        capacity = int(capacity)
        if not 1 <= capacity <= AUC_MAX_BANK:
            raise ValueError('ScoreBank capacity must lie in [1, %d], got %d' % (AUC_MAX_BANK, capacity))
        self.capacity = capacity
        self.scores = torch.zeros(capacity, dtype=torch.float32, device=device)
        self.labels = torch.zeros(capacity, dtype=torch.int32, device=device)
        self.state = torch.zeros(2, dtype=torch.int32, device=device)

    def reset(self):
        """forget every score: head = fill = 0 (one fill launch, no host read)"""
        self.state.zero_()

    def contents(self):
        """(scores, labels) of the valid slots, oldest first, as host tensors.  Reads on the host: for tests and tools only"""
        head, fill = self.state.tolist()
        idx = (torch.arange(fill) + (head - fill)) % self.capacity
        return self.scores.cpu()[idx], self.labels.cpu()[idx]


class _AucLogitsLossFn(torch.autograd.Function):
    """uniter_bce_auc_logits after _LogitsLossFn's pattern: one launch forward (which also pushes into the bank), none
    backward -> (the view terms[0], terms [total, bce, auc], probs, n_pairs); only the first is differentiable."""
    @staticmethod
    def forward(ctx, logits, labels, pos_weight, auc_weight, bank, kind, margin, grad_scale, push):
        _lib.require_gpu_tensor(logits, torch.float32, 'logits')
        x = logits.reshape(-1).contiguous()
        y = labels.reshape(-1).to(torch.int64).contiguous()
        B = x.numel()
        if B != y.numel():
            raise ValueError('logits/labels size mismatch')
        if bank is not None and bank.scores.device != x.device:
            raise UniterHipError('the score bank lives on %s, the logits on %s' % (bank.scores.device, x.device))
        dlog = torch.empty(B, dtype=torch.float32, device=x.device)
        terms = torch.empty(3, dtype=torch.float32, device=x.device)
        probs = torch.empty(B, dtype=torch.float32, device=x.device)
        n_pairs = torch.empty((), dtype=torch.int32, device=x.device)
        bs, bl, bst, N = (ptr(bank.scores), ptr(bank.labels), ptr(bank.state), bank.capacity) if bank is not None else (None, None, None, 0)
        check(_lib.lib().uniter_bce_auc_logits(ptr(x), ptr(y), float(pos_weight), float(auc_weight), int(kind), float(margin), bs, bl, bst,
                                               N, int(bool(push)), ptr(terms), ptr(n_pairs), ptr(probs), ptr(dlog), float(grad_scale), B,
                                               _lib.cur_stream()), 'uniter_bce_auc_logits')
        loss = terms[0]                            # (a view: the total needs no launch of its own)
        ctx.save_for_backward(dlog)
        ctx.shape = logits.shape
        ctx.mark_non_differentiable(terms, probs, n_pairs)
        ctx.set_materialize_grads(False)
        return loss, terms, probs, n_pairs

    @staticmethod
    def backward(ctx, dloss, *_dextras):
        return (_saved_dlogits(ctx, dloss),) + (None,) * 8


_UNIT = {}


def unit_gradient(device):
    """A cached scalar 1.0 to pass as loss.backward(gradient=...): saves the ones_like fill autograd would launch for the
    root and (recognised by its address in _LogitsLossFn.backward) the multiply by it -- two launch-latency-sized kernels
    in the host-bound stretch between forward and backward."""
    device = torch.device(device)
    t = _UNIT.get(device)
    if t is None:
        t = _UNIT[device] = torch.ones((), dtype=torch.float32, device=device)
    return t


def bce_with_logits_loss(logits, labels, pos_weight=1.0, return_probs=False):
    """BCEWithLogitsLoss(pos_weight=[w]) with mean reduction; labels are cast to
    float as train_template.py:99 does.  Also yields sigmoid(logits)."""
    loss, probs = _LogitsLossFn.apply(logits, None, labels, pos_weight, 0.0, 1.0)
    return (loss, probs) if return_probs else loss


def bce_kl_with_logits_loss(logits, clean_logits, labels, pos_weight, kl_weight, grad_scale=1.0, return_terms=False):
    """The loss of a perturbed pass of VILLA, one launch (uniter_bce_kl_logits): bce_with_logits_loss(logits, labels, pos_weight)
    + kl_weight * mean_b [KL(p||q) + KL(q||p)] with q = sigmoid(logits), p = sigmoid(clean_logits).  Differentiable in `logits`
    only: the clean logits are constants.  The gradient handed back is grad_scale times the loss's (the launch applies the
    1 / K of the K passes itself); the value is not scaled.  return_terms: also the device tensor [total, bce, kl]."""
    if clean_logits is None:
        raise ValueError('bce_kl_with_logits_loss needs the clean logits')
    loss, terms = _LogitsLossFn.apply(logits, clean_logits, labels, pos_weight, kl_weight, grad_scale)
    return (loss, terms) if return_terms else loss


def bce_auc_with_logits_loss(logits, labels, pos_weight, auc_weight, bank=None, surrogate='logistic', margin=1.0, grad_scale=1.0,
                             push=True, return_terms=False, return_probs=False):
    """bce_with_logits_loss(logits, labels, pos_weight) + auc_weight * a pairwise AUROC surrogate, one launch
    (uniter_bce_auc_logits): the mean of l(s_positive - s_negative) over the pairs of the batch's rows with each other and with
    the `bank`'s recent scores (a ScoreBank, or None: the batch alone), l = softplus(-d) ('logistic') or max(0, margin - d)^2
    ('hinge2').  The bank's scores are constants; with push (and a bank) the launch then pushes the batch's logits and labels
    into it.  The gradient handed back is grad_scale times the loss's; the value is not scaled.  return_terms: also the device
    tensor [total, bce, auc]; return_probs: also sigmoid(logits), behind it."""
    if surrogate not in AUC_SURROGATES:
        raise ValueError('surrogate must be one of %s, got %r' % (', '.join(repr(s) for s in AUC_SURROGATES), surrogate))
    loss, terms, probs, _ = _AucLogitsLossFn.apply(logits, labels, pos_weight, auc_weight, bank, AUC_SURROGATES.index(surrogate), margin,
                                                   grad_scale, push)
    out = (loss,) + ((terms,) if return_terms else ()) + ((probs,) if return_probs else ())
    return out if len(out) > 1 else loss


# --------------------------------------------------------------------------- #
# optimizer
# --------------------------------------------------------------------------- #
NO_DECAY = ('bias', 'LayerNorm.bias', 'LayerNorm.weight')      # utils/optim_utils.py:16


def no_decay(name):
    return any(nd in name for nd in NO_DECAY)


Hyper = namedtuple('Hyper', 'lr b1 b2 eps weight_decay step_count adamw')      # in the order the library's entry points take them
# the same stretch of uniter_optim_step_groups' arguments: the table of per-group hyper-parameters (an _lib.OptimGroupC array) in
# the place of the scalars; `rows` repeats it as plain tuples (lr, b1, b2, eps, weight_decay) so that two steps' values compare
GroupHyper = namedtuple('GroupHyper', 'table n_groups step_count')
MAX_PARAM_GROUPS = 32       # bits 3-7 of a chunk's flag byte
Scale = namedtuple('Scale', 'grad_scale max_grad_norm zero_grads')
# One launch of a step.  kind: 'flat' (the flat buffers' range [lo, hi)) or 'rows' (the looked-up rows of the word table [lo, hi));
# stream: 'main' or 'side'; wait: the range that stream waits for through grad_ready in front of the launch, or None; event: None,
# 'block' (for the forward pass's per-block list) or 'word' (the word table's extra event); clear_mask: behind it, on its stream
Launch = namedtuple('Launch', 'kind lo hi stream max_wgs wait event clear_mask')


def group_layout(named, weight_decay, group_param_func=None):
    """utils/optim_utils.py:9-30 on plain values: the (name, parameter) pairs, grouped by `group_param_func` (the pairs -> a list of
    dicts whose 'params' are such pairs; None: one group of everything), each group split into its decay and its no-decay half in
    the reference's order [decay_0, nodecay_0, decay_1, ..], every key other than 'params' / 'weight_decay' copied into both.
    -> the list of dicts, 'params' still (name, parameter) pairs.  Every parameter must be named exactly once."""
    named = list(named)
    if group_param_func is None:
        groups = [{'params': named}]
    else:
        groups = group_param_func(named)
        if not isinstance(groups, (list, tuple)) or not groups or not all(
                isinstance(g, dict) and isinstance(g.get('params'), (list, tuple)) and
                all(isinstance(e, (list, tuple)) and len(e) == 2 and isinstance(e[0], str) for e in g['params']) for g in groups):
            raise UniterHipError("group_param_func must return a non-empty list of dicts whose 'params' are (name, parameter) "
                                 'pairs (utils/optim_utils.py:9-30); got %s' % (type(groups).__name__ if not isinstance(groups, (list, tuple))
                                                                               else 'a list that holds something else'))
        if 2 * len(groups) > MAX_PARAM_GROUPS:
            raise UniterHipError('group_param_func returned %d groups: at most %d (each becomes a decay and a no-decay group, and '
                                 '%d fit the chunk flags)' % (len(groups), MAX_PARAM_GROUPS // 2, MAX_PARAM_GROUPS))
        seen, known = set(), {n for n, _ in named}
        for g in groups:
            for n, _ in g['params']:
                if n in seen:
                    raise UniterHipError('group_param_func names parameter %r twice' % n)
                if n not in known:
                    raise UniterHipError('group_param_func names %r, which is no parameter of the model' % n)
                seen.add(n)
        left = [n for n, _ in named if n not in seen]
        if left:
            raise UniterHipError('group_param_func leaves %d parameter(s) out, the first of them %r' % (len(left), left[0]))
    out = []
    for g in groups:
        extra = {k: v for k, v in g.items() if k not in ('params', 'weight_decay')}
        out.append(dict(extra, params=[(n, p) for n, p in g['params'] if not no_decay(n)], weight_decay=weight_decay))
        out.append(dict(extra, params=[(n, p) for n, p in g['params'] if no_decay(n)], weight_decay=0.0))
    return out


def chunk_flag_bytes(nchunks, offsets, sizes, touched, frozen=(), keep=(), group_bits=None):
    """The optimizer's flag byte per 64-element chunk, from plain values.  offsets / sizes: name -> first element / element count;
    touched: the names that received a gradient; frozen: names that are never updated (byte 0 whatever `touched` says -- neither
    the step nor the norm kernels read or write them); keep: names whose gradient zero_grads leaves alone (+ 4).
    group_bits None: 1 (no weight decay) / 2 (weight decay) by name, as every entry point but uniter_optim_step_groups takes them;
    else name -> (group index, decays): (index << 3) | 2 or 1."""
    host = torch.zeros(nchunks, dtype=torch.uint8)
    for n in touched:
        if n in frozen:
            continue
        o, k = offsets[n] // CHUNK, (sizes[n] + CHUNK - 1) // CHUNK
        if group_bits is None:
            byte = 1 if no_decay(n) else 2
        else:
            index, decays = group_bits[n]
            byte = (index << 3) | (2 if decays else 1)
        host[o:o + k] = byte + (4 if n in keep else 0)
    return host


def optim_schedule(numel, plan, rows_ahead, has_grad_ready, overlap_wgs, sw, trainable=None):
    """The launches of one FusedAdam.step in issue order, from plain values.  plan: _overlap_plan's (head, blocks, word) or None;
    rows_ahead: _word_table's tuple when early_word_update ran for this step, else None; sw: optim_switches(); trainable: the
    element ranges [(lo, hi), ..] that hold parameters the optimizer updates, or None = everything: a launch whose range meets
    none of them is dropped, together with its event (frozen parameters: FusedAdam._trainable_ranges)."""
    if trainable is not None:
        live = lambda r: any(lo < r.hi and r.lo < hi for lo, hi in trainable)
        return [r for r in optim_schedule(numel, plan, rows_ahead, has_grad_ready, overlap_wgs, sw) if live(r)]
    table = rows_ahead and (rows_ahead[0], rows_ahead[0] + rows_ahead[1] * rows_ahead[2])
    if plan is None:            # everything on the caller's stream, behind ONE wait for the whole buffer
        cuts = [0, numel] if not table else sorted({0, numel, *table})
        return [Launch('rows' if (lo, hi) == table else 'flat', lo, hi, 'main', 0, (0, numel) if has_grad_ready and lo == 0 else None,
                       None, False) for lo, hi in zip(cuts, cuts[1:])]
    # The update is HBM-bound, the next forward MFMA-bound: run the encoder's blocks on the side stream in the order the forward
    # needs them (embeddings, layer 0, 1, ..), one event per block; the next uniter_model_forward waits block by block
    head, blocks, word = plan[0], plan[1], plan[2] if sw.word_split else None
    if table and (word is None or word[0] != table[0]):
        raise UniterHipError('FusedAdam.step: early_word_update needs the word table as its own optimizer launch '
                             '(UNITER_ADAM_WORD_SPLIT=0 or an unexpected parameter layout)')
    wait = lambda lo, hi: (lo, hi) if has_grad_ready else None          # each launch waits for the gradients of its own range
    out = [Launch('flat', lo, hi, 'main', 0, wait(lo, hi), None, False) for lo, hi in head]      # pooler / heads: tiny, stay on the main stream
    for k, (lo, hi) in enumerate(blocks):
        if k or word is None:       # the embeddings have the chip to themselves; the layers share it with the forward: its grid
            out.append(Launch('flat', lo, hi, 'side', overlap_wgs if k else 0, wait(lo, hi), 'block', False))
            continue
        # the word table is a launch of its own: the next forward's image branch reads no word embedding and starts behind the
        # block's remainder, beside the table's 0.13 ms (grid: 512 workgroups 4.83, 1024 4.79 ms bf16 step).  With rows updated
        # ahead it takes the looked-up rows, and the mask is cleared behind IT: the next step's note_tokens waits for that
        wgs = sw.word_wgs if sw.word_wgs is not None else min(2048, 4 * overlap_wgs)
        tbl = Launch('rows' if table else 'flat', word[0], word[1], 'side', wgs, wait(*word), 'word', bool(table))
        if sw.emb_main and not has_grad_ready:
            # the remainder on the MAIN stream: in stream order, not behind an event an idle queue picks up 40-150 us late
            out += [tbl, Launch('flat', word[1], hi, 'main', 0, None, 'block', False)]
        else:
            out += [Launch('flat', word[1], hi, 'side', 0, wait(word[1], hi), 'block', False), tbl]
    return out


def ema_weight(decay, steps, warmup=True):
    """The weight w = 1 - d_t of the parameters in the averaging step that follows `steps` earlier ones (a' = a + w (p' - a)):
    d_t = min(decay, (1 + t) / (10 + t)) with warm-up -- the average forgets its start (a copy of the initial weights) at the rate
    the run can afford: w = 0.9, 0.82, 0.75, .. until 1 - decay takes over -- else d_t = decay.  Formed in double; the launch takes
    its fp32 value."""
    d = min(float(decay), (1.0 + steps) / (10.0 + steps)) if warmup else float(decay)
    return 1.0 - d


# state_dict()['state'] in torch's layout, on plain values: `order` = [(name, shape)] of the parameters in param_groups order (None
# in the place of a name: a parameter without state -- frozen), offsets: name -> first element in the flat buffers, `flat`: key ->
# flat tensor.  The keys per rule, in torch's spelling (KIND None / 2 / 3):
STATE_KEYS = {None: ('exp_avg', 'exp_avg_sq'), 2: ('exp_avg', 'exp_inf'), 3: ('momentum_buffer',)}


def _numel(shape):
    return int(math.prod(shape))


def pack_optim_state(order, offsets, flat, keys, step_count):
    """-> {i: {'step': 0-dim fp32 tensor (rules with a counter), key: clone shaped like parameter i}} for every named entry of
    `order`; flat: the flat tensors in the order of `keys`.  Before the first step there is no state (torch's own behaviour)."""
    if step_count < 1:
        return {}
    out = {}
    for i, (name, shape) in enumerate(order):
        if name is None:
            continue
        o, k = offsets[name], _numel(shape)
        entry = {} if keys == STATE_KEYS[3] else {'step': torch.tensor(float(step_count), dtype=torch.float32)}
        for key, buf in zip(keys, flat):
            entry[key] = buf[o:o + k].detach().clone().reshape(shape)
        out[i] = entry
    return out


def unpack_optim_state(state, order, offsets, flat, keys):
    """Copy a torch-layout `state` into the flat tensors (in place, in the order of `keys`) -> the step counter it carries (None:
    the rule has none, or the dict holds no state).  Entries are looked up by index; a parameter without an entry keeps what the
    flat tensors hold; a missing momentum_buffer is zeros (torch leaves it None until the parameter's first gradient).  A count
    or shape mismatch raises ValueError; `step` values that differ raise UniterHipError (ONE counter for every parameter)."""
    if any((not isinstance(i, int)) or i < 0 or i >= len(order) for i in state):
        raise ValueError('optimizer state names parameter(s) %r: this optimizer holds %d' % (sorted(state, key=str)[-1], len(order)))
    steps, copies = set(), []
    for i, entry in state.items():          # everything is checked before anything is written
        name, shape = order[i]
        if name is None:
            if entry:
                raise ValueError('optimizer state holds an entry for parameter %d, which is frozen here' % i)
            continue
        o, k = offsets[name], _numel(shape)
        for key, buf in zip(keys, flat):
            t = entry.get(key)
            if t is None and key != 'momentum_buffer':
                raise ValueError('optimizer state of parameter %d (%s) lacks %r' % (i, name, key))
            if t is not None and tuple(t.shape) != tuple(shape):
                raise ValueError('optimizer state %r of parameter %d (%s) has shape %s, the parameter %s'
                                 % (key, i, name, tuple(t.shape), tuple(shape)))
            copies.append((buf[o:o + k], t))
        if 'step' in entry:
            steps.add(float(entry['step']))
    if len(steps) > 1:
        raise UniterHipError('the optimizer state carries different step counters (%s): the fused step keeps ONE counter for '
                             'every parameter (step_count), as if each had received a gradient in every step'
                             % ', '.join('%g' % v for v in sorted(steps)))
    for dst, t in copies:
        if t is None:
            dst.zero_()
        else:
            dst.copy_(t.detach().reshape(-1).to(dst.dtype))
    return int(steps.pop()) if steps else None


def pack_averaged(order, offsets, avg):
    """top-level 'averaged' of the state dict: {i: clone of the average shaped like parameter i}, frozen parameters left out"""
    return {i: avg[offsets[name]:offsets[name] + _numel(shape)].detach().clone().reshape(shape)
            for i, (name, shape) in enumerate(order) if name is not None}


def unpack_averaged(averaged, order, offsets, avg):
    for i, t in averaged.items():
        if (not isinstance(i, int)) or i < 0 or i >= len(order) or order[i][0] is None:
            raise ValueError("'averaged' names parameter %r, which this optimizer does not average" % (i,))
        name, shape = order[i]
        if tuple(t.shape) != tuple(shape):
            raise ValueError("'averaged' of parameter %d (%s) has shape %s, the parameter %s" % (i, name, tuple(t.shape), tuple(shape)))
        avg[offsets[name]:offsets[name] + _numel(shape)].copy_(t.detach().reshape(-1).to(avg.dtype))


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam (coupled L2) / AdamW over the model's flat buffers.

    ``param_groups`` keeps the reference's layout -- a decay and a no-decay group, or such a pair per group a
    ``group_param_func`` returns (group_layout), each with the keys (``lr``, ..) the function gave it -- so
    LR schedulers written against torch optimizers keep working; the arithmetic is
    one kernel launch, which reads a chunk's hyper-parameters from its group's row once the groups differ
    (uniter_optim_step_groups).  Parameters whose ``requires_grad`` is False when the optimizer is built are never
    read or written.  ``step()`` also performs ``average_gradients`` (``grad_scale``)
    and ``clip_grad_norm_`` (``max_grad_norm``) when asked to, and zeroes the
    gradients (the reference calls ``zero_grad`` right after ``step``).

    FusedAdamax and FusedSGD below are this class with another update rule (``KIND``, uniter_optim_step): everything around the
    arithmetic -- the clip norm, the block-wise overlap with the next forward pass, lazy zeroing, the bf16 gradient payload, the
    weight mirror -- is inherited.
    """

    KIND = None             # None: torch.optim.Adam / AdamW through uniter_adam_step_x3p; 2 / 3: uniter_optim_step's Adamax / SGD
    SECOND_STATE = True     # the rule keeps exp_avg_sq (Adam's second moment, Adamax's infinity norm)

    def __init__(self, model, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3, adamw=False, defaults=None, group_param_func=None, layout=None,
                 ema_decay=None, ema_warmup=True):
        if ema_decay and not 0.0 < float(ema_decay) < 1.0:
            raise ValueError('ema_decay must lie in (0, 1) (0 / None: no averaging), got %r' % (ema_decay,))
        self.model = model
        self.store = model.param_store() if hasattr(model, 'param_store') else ensure_store(model)
        if layout is None:      # (get_optimizer passes the layout it already built: `group_param_func` is called once)
            layout = group_layout(list(model.named_parameters()), weight_decay, group_param_func)
        if defaults is None:
            defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__([dict(g, params=[p for _, p in g['params']]) for g in layout], defaults)
        # per parameter, under the store's names: its param_group and whether that is a decay half; and the frozen ones --
        # requires_grad is read HERE, once, as torch optimizers read their parameter list
        by_id = {id(p): (k, k % 2 == 0) for k, g in enumerate(layout) for _, p in g['params']}
        params = getattr(self.store, 'params', {})
        self._group_of = {n: by_id[id(p)] for n, p in params.items() if id(p) in by_id}
        self._frozen = frozenset(n for n, p in params.items() if not p.requires_grad)
        self.adamw = bool(adamw)
        self.step_count = 0
        st = self.store
        self.exp_avg = torch.zeros_like(st.flat_params)
        self.exp_avg_sq = torch.zeros_like(st.flat_params) if self.SECOND_STATE else None
        self._sumsq = torch.zeros(1, dtype=torch.float64, device=st.device)
        self._parts = None          # per-slice partial sums of the clip norm (data parallel: one per collective)
        # the clip norm taken during the backward pass (attach_norm_hooks): unreduced partial sums per bucket
        self._np_buf = None
        self._np_blocks = 0         # partial sums written by the backward that just ran (0 = not armed)
        self._np_seen = None
        n_ws = _lib.lib().uniter_grad_sumsq_ws_bytes(st.numel)
        self._ws = torch.empty(n_ws, dtype=torch.uint8, device=st.device)
        self._ws_bytes = n_ws
        self._flags_key = None
        self._flags = None
        self._flags_cache = {}      # touched-set -> device flags (multitask training alternates between a few sets)
        # set to the UniterModel to overlap the update with the next forward (see step()); anything
        # else that reads parameters on the current stream must call join() first
        self.overlap_encoder = None
        # set to the UniterModel: zero_grad (fused into step) skips the encoder layers' weight gradients -- four fifths of all
        # parameters -- and the next backward pass writes them with `=` instead of `+=` (uniter_model_set_wgrad_overwrite):
        # 28 instead of 32 bytes per parameter, no read-modify-write in the weight-gradient epilogues.  Until that backward
        # pass those .grad tensors hold the previous step's values (ParamStore.wgrad_stale); the trainers of this package
        # never read them in between (the reference calls zero_grad right after step, train_template.py:105-107)
        self.lazy_zero_encoder = None
        # grid of the blocks that share the chip with the next forward pass.  256 (one workgroup per CU) where the forward's kernels
        # can share a CU with it (fp32, bf16: DESIGN.md section 4 "Streams"); in the fp32x3 mode a persistent 144-KB, 504-of-512-register
        # GEMM workgroup cannot start on a CU while an optimizer workgroup sits there -- the blocks should be OUT OF THE WAY fast, not
        # thin: round 6 measured 9.52 ms (256), 9.42 (512), 9.35 (1024), 9.47 (no overlap at all) per step, bf16 unchanged
        # (profiles/r06_adam_wgs_ab.txt).  UNITER_ADAM_OVERLAP_WGS fixes it for every mode
        sw = optim_switches()
        self._overlap_wgs = sw.overlap_wgs
        self._pending = None
        self._plan_cache = None
        # the word-embedding table's update split by rows (round 6, uniter_adam_step_rows): note_tokens / early_word_update / step
        # (built, bit-identical, and OFF by default: same-box A/B 9.53 ms with and without in fp32x3, 4.39 -> 4.44 ms in bf16 --
        # profiles/r06_word_rows_ab.txt: the 100 us the head of the next forward pass no longer waits for are CU-time the ahead-of-time
        # launch takes from the forward pass it runs beside, and behind the table the next forward's own first kernels bound the head)
        # (Adam / AdamW only: uniter_adam_step_rows knows no other rule, FusedAdamax / FusedSGD never split)
        self.split_word_rows = self.KIND is None and sw.word_rows
        # An exponential moving average of the parameters kept by the step's own launches (uniter_optim_step_avg: 8 bytes per
        # parameter inside the kernel that has the new value in registers; a separate lerp_ pass would have to join() the
        # overlapped update first and stream 12).  avg starts as a copy of the parameters; a parameter a step skips (no gradient,
        # or frozen) keeps its average -- torch.optim.swa_utils would go on averaging it -- so a frozen tensor's average is
        # always the tensor.  averaged_parameters() evaluates and checkpoints on it.  No row-split form of the word table's update
        self.ema_decay = float(ema_decay) if ema_decay else None
        self.ema_warmup = bool(ema_warmup)
        self.avg = st.flat_params.detach().clone() if self.ema_decay else None
        self.avg_steps = 0
        self._exchanged = False
        if self.ema_decay:
            self.split_word_rows = False
        self._rowmask = None        # one byte per row of the table: 1 = a token of the micro-batches since the last step looks it up
        self._rows_noted = False    # every micro-batch since the last step announced its ids (none had a dense table gradient)
        self._early = None          # the rows without a gradient were updated ahead: (the Hyper of that launch, the event behind it)
        self._word_cache = None
        self._rowmask_clear = None  # event behind the mask's clearing (side stream)
        self._rowmask_ready = None  # event behind the mask's last fill (the stream note_tokens ran on)

    @property
    def overlap_workgroups(self):
        if self._overlap_wgs is not None:
            return self._overlap_wgs
        enc = self.overlap_encoder
        return 1024 if (enc is not None and getattr(enc, 'precision', 'fp32') == 'fp32x3') else 256

    @overlap_workgroups.setter
    def overlap_workgroups(self, v):
        self._overlap_wgs = None if v is None else int(v)

    def _overlap_plan(self, enc):
        """(head ranges, [embeddings, layer 0, ..] ranges) in flat-buffer elements, or None when the
        store's buckets are not [head | layer nl-1 .. 0 | embeddings]."""
        if self._plan_cache is None:
            st, nl = self.store, enc.config.num_hidden_layers
            r = list(st.bucket_ranges)
            ok = len(r) in (nl + 1, nl + 2)
            head = r[:len(r) - nl - 1] if ok else []
            blocks = [r[-1]] + r[-2:-2 - nl:-1] if ok else []
            covered = sorted(head + blocks)
            ok = ok and covered[0][0] == 0 and covered[-1][1] == st.numel and \
                all(a[1] == b[0] for a, b in zip(covered, covered[1:]))
            # the word-embedding table, when it opens the embeddings' bucket and does not fill it: its update is a launch of its own
            w = self._find_word_table() if ok else None
            word = (w[1], w[2]) if w is not None and w[1] == blocks[0][0] and w[2] < blocks[0][1] else None
            self._plan_cache = (head, blocks, word) if ok else False
        return self._plan_cache or None

    def _find_word_table(self):
        """(name, offset, end padded to whole chunks) of the word-embedding table in the flat buffers, or None"""
        st = self.store
        name = next((n for n in st.names if n.endswith('embeddings.word_embeddings.weight')), None)
        return None if name is None else (name, st.offsets[name],
                                          st.offsets[name] + (st.params[name].numel() + CHUNK - 1) // CHUNK * CHUNK)

    NORM_BLOCKS = 256           # workgroups (= partial sums) per layer slice, on the side stream beside the input-gradient chain
    NORM_BLOCKS_LAST = 2048     # the embeddings' slice runs alone behind the backward pass: the whole chip
    FUSED_SLOTS = 2048          # fp32x3 / bf16: slots a layer's weight-gradient launch writes itself (one per compute wave: up to 8 x 256)

    def attach_norm_hooks(self, encoder):
        """Take the clip norm (clip_grad_norm_, train_template.py:104) slice by slice DURING the backward pass: the
        encoder's backward schedule announces every bucket of the flat gradient buffer the moment it is final (head,
        layer nl-1 .. 0 on the weight-gradient stream, embeddings on the main stream) and this optimizer reduces the
        bucket into partial sums right there -- on a stream that idles half of each layer anyway.  `step` then only
        joins the partial sums (one 1-workgroup launch) instead of streaming all 440 MB of gradients once more
        behind the backward pass.  Single process only: with a data-parallel exchange attached the norm is that of the
        REDUCED gradients (dp.GradSync.pieces)."""
        if getattr(encoder, '_grad_hook', None) is not None or self._frozen:
            return False         # (frozen parameters: the partial sums cover whole layers; the flag-aware pass takes the norm)
        st = self.store
        nb = len(st.bucket_ranges)
        nl = encoder.config.num_hidden_layers
        if nb not in (nl + 1, nl + 2):
            return False
        first_layer = nb - nl - 1            # index of layer nl-1's bucket (0 when there is no head bucket)
        # partial sums per bucket: [head (optional) | layer 0 .. nl-1 (uniform stride: the fp32x3 backward writes layer l's own
        # partial sums at l * stride, uniter_model_set_norm_partials) | embeddings]
        lstride = max(self.NORM_BLOCKS, self.FUSED_SLOTS)
        head_n = self.NORM_BLOCKS if first_layer == 1 else 0
        self._np_buf = torch.zeros(head_n + nl * lstride + self.NORM_BLOCKS_LAST, dtype=torch.float64, device=st.device)
        layers_view = self._np_buf[head_n:head_n + nl * lstride]
        self._np_blocks, self._np_seen = 0, set()
        lib = _lib.lib()
        state = {'fused': False, 'per_layer': 0}

        def region(k):
            """(offset in doubles, slots) of bucket k's partial sums"""
            if k < first_layer:
                return 0, self.NORM_BLOCKS
            if k == nb - 1:
                return head_n + nl * lstride, self.NORM_BLOCKS_LAST
            layer = nl - 1 - (k - first_layer)
            return head_n + layer * lstride, self.NORM_BLOCKS

        def reduce_bucket(k, stream):
            lo, hi = st.bucket_ranges[k]
            off, n = region(k)
            sp = stream.cuda_stream if stream is not None else _lib.cur_stream()
            check(lib.uniter_grad_sumsq_part(st.flat_grads.data_ptr() + 4 * lo, None, hi - lo,
                                             self._np_buf.data_ptr() + 8 * off, n, sp), 'uniter_grad_sumsq_part')
            self._np_seen.add(k)

        def hook(kind, index, stream):
            if kind == 'begin':
                self._np_seen = set()
                self._np_blocks = 0
                # fp32x3: every layer's weight-gradient launch leaves the layer's share itself (bit-reproducible slots); any other
                # precision: one reduction launch per layer bucket on the weight-gradient stream.  A switch of precision between
                # two backward passes (bench.py's native-fp32 leg) changes which slots are written: clear the stale ones
                per_layer = encoder.norm_partials_per_layer()
                fused = 0 < per_layer <= lstride
                #  the slot COUNT matters too: uniter_sumsq_combine joins the whole buffer, and a launch on a smaller
                # grid (a CU reserve, a capped grid, another batch shape) leaves the larger grid's tail slots behind
                if fused != state['fused'] or (fused and per_layer != state['per_layer']):
                    layers_view.zero_()
                    state['fused'] = fused
                state['per_layer'] = per_layer
                if first_layer == 1:
                    reduce_bucket(0, stream)                 # head / pooler: final before the encoder's backward starts
            elif kind == 'layer':
                if state['fused']:
                    self._np_seen.add(first_layer + (nl - 1 - index))
                else:
                    reduce_bucket(first_layer + (nl - 1 - index), stream)
            elif kind == 'embed':
                reduce_bucket(nb - 1, stream)
                if len(self._np_seen) == nb:
                    self._np_blocks = self._np_buf.numel()   # armed: every bucket of THIS backward is in

        encoder._grad_hook = hook
        encoder._norm_parts = (layers_view, lstride)
        self._norm_hook = hook
        return True

    # -- the word-embedding table, row by row ---------------------------------------------------------------------------
    def _word_table(self):
        """(offset, rows, row length) of the word-embedding table in the flat buffers, or None (no such tensor, a row length
        that is no multiple of the optimizer's 64-element chunks, a frozen table, or the split switched off)."""
        if not self.split_word_rows:
            return None
        if self._word_cache is None:
            w, wt = self._find_word_table(), False
            if w is not None and w[0] not in self._frozen:      # (the row-split launches know no frozen chunk: a frozen table has none)
                V, H = self.store.params[w[0]].shape
                if int(H) % CHUNK == 0 and w[1] % CHUNK == 0:
                    wt = (w[1], int(V), int(H), w[0])
            self._word_cache = wt
        return self._word_cache or None

    def note_tokens(self, input_ids):
        """Once per micro-batch, before its backward pass: the token ids it looks up in the word-embedding table -- the only rows its
        gradient can touch (model/model.py:232-236; padding_idx 0 included: harmless).  None = this micro-batch's table gradient is
        dense (the MLM task's tied decoder): no split this step."""
        wt = self._word_table()
        if wt is None:
            return
        if input_ids is None:
            self._rows_noted = None           # dense until the next step
            return
        if self._rows_noted is None:
            return
        if self._rowmask is None:
            self._rowmask = torch.zeros(wt[1], dtype=torch.uint8, device=self.store.device)
        if self._rowmask_clear is not None:        # (the last step cleared the mask on the side stream, behind its last reader)
            torch.cuda.current_stream().wait_event(self._rowmask_clear)
            self._rowmask_clear = None
        ids = input_ids.reshape(-1)
        self._rowmask.index_fill_(0, ids.clamp(0, wt[1] - 1), 1)
        self._rowmask_ready = torch.cuda.Event()
        self._rowmask_ready.record()
        self._rows_noted = True

    def early_word_update(self, stream=None):
        """Before the backward pass of the micro-batch that steps (every micro-batch since the last step called note_tokens): update the
        rows of the word-embedding table that NO token of them looks up.  Their gradient is zero whatever the backward pass computes, and
        0 x (clip coefficient) = 0: torch.optim.Adam's update of such a row (g = wd p, utils/optim_utils.py:33-40) depends on the
        step number and the learning rate alone -- so 93 % of the table (0.58 of the step's 3.18 GB) leaves the head of the NEXT
        forward pass, whose text branch used to wait for all of it, and streams beside this step's own forward / backward instead.
        `step()` then updates the looked-up rows only (with their gradients, clipped).  Parameters bit-identical to the one-launch
        update.  Returns True when the ahead-of-time launch was issued."""
        if self.KIND is not None:
            raise UniterHipError('%s: the row-split update of the word-embedding table is built for Adam / AdamW only'
                                 % type(self).__name__)
        wt = self._word_table()
        if wt is None or self._rows_noted is not True or self._early is not None:
            return False
        if not self._uniform():
            return False
        h = self._hyper(self.step_count + 1)
        side = stream if stream is not None else self._stream('side')[0]
        # behind the mask's last fill only -- NOT behind everything queued on the current stream: called in front of the forward pass, the
        # launch then runs beside it like one more of the optimizer's blocks (the side stream holds the previous step's update ahead of it)
        if self._rowmask_ready is not None:
            side.wait_event(self._rowmask_ready)
        wgs = optim_switches().early_wgs
        check(_lib.lib().uniter_adam_step_rows(*self._rows_args(wt, h, None, Scale(1.0, 0.0, 0), 0, self.overlap_workgroups if wgs is None
                                                                else wgs, C.c_void_p(side.cuda_stream))), 'uniter_adam_step_rows')
        ev = torch.cuda.Event()
        ev.record(side)
        self._early = (h, ev)
        return True

    def _hyper(self, step_count):
        """The hyper-parameters of step `step_count` (one learning rate; the decay group's weight decay: the chunk flags say where it applies)"""
        g0 = self.param_groups[0]
        return Hyper(float(g0['lr']), *self._rule_args(g0), float(g0['weight_decay']), step_count, int(self.adamw))

    def _uniform(self):
        """Do all parameter groups step with the same hyper-parameters -- one lr, one set of betas / momentum and eps, ONE weight
        decay on the decay halves and none elsewhere?  Then the step is the launch with scalars it always was."""
        gs = self.param_groups
        g0 = gs[0]
        one = (float(g0['lr']), self._rule_args(g0))
        return all((float(g['lr']), self._rule_args(g)) == one and
                   float(g['weight_decay']) == (float(g0['weight_decay']) if k % 2 == 0 else 0.0) for k, g in enumerate(gs))

    def _group_hyper(self, step_count):
        """The table of uniter_optim_step_groups: one row per parameter group, in param_groups' order"""
        gs = self.param_groups
        table = (_lib.OptimGroupC * len(gs))(*[_lib.OptimGroupC(float(g['lr']), *self._rule_args(g), float(g['weight_decay'])) for g in gs])
        return GroupHyper(table, len(gs), step_count)

    def _trainable_ranges(self):
        """Element ranges of the tensors this optimizer updates, or None when nothing is frozen (optim_schedule's `trainable`)"""
        if not self._frozen:
            return None
        st = self.store
        return [(st.offsets[n], st.offsets[n] + st.params[n].numel()) for n in st.names if n not in self._frozen]

    def _stream(self, which, keep=False):
        """(torch stream, its pointer) of 'main', the caller's, or 'side': the encoder's, else the process-wide one (keep: now the encoder's)"""
        s = torch.cuda.current_stream() if which == 'main' else getattr(self.overlap_encoder, '_side_stream', None)
        if s is None:
            s = _lib.shared_stream(self.store.device, 'side')
            if keep:
                self.overlap_encoder._side_stream = s
        return s, C.c_void_p(s.cuda_stream)

    def _rows_args(self, wt, h, sumsq, scale, pass_, max_wgs, stream_ptr):
        """Arguments of uniter_adam_step_rows for the word table `wt`.  pass_ 0: the rows the mask does NOT name, 1: those it names"""
        st, (off, V, H, name) = self.store, wt
        return (st.flat_params.data_ptr() + 4 * off, st.flat_grads.data_ptr() + 4 * off, self.exp_avg.data_ptr() + 4 * off,
                self.exp_avg_sq.data_ptr() + 4 * off, self._row_flags(off, V * H, no_decay(name)).data_ptr(), V * H, sumsq,
                scale.grad_scale, scale.max_grad_norm, *h, scale.zero_grads, self._rowmask.data_ptr(), H, pass_, max_wgs, stream_ptr)

    def _range_args(self, lo, hi, max_wgs, stream_ptr, h, scale, flags, grad_bf16, layers):
        """Arguments of uniter_adam_step_x3p / uniter_optim_step for [lo, hi).  layers: the encoder layers' range when overlapped, or None"""
        st = self.store
        off = lo * 4
        # the bf16 weight mirror (precision 'bf16') is written by the same kernel, on the same stream (precision 'fp32x3': its
        # three bf16 pieces, piece p at mirror + p * numel).  It feeds the encoder LAYERS' dense products only: blocks outside
        # them (the 24 M parameters of the embeddings, the heads) skip its 2 - 6 bytes per parameter
        mirror = getattr(st, 'mirror', None)
        if mirror is not None and layers is not None and not (lo >= layers[0] and hi <= layers[1]):
            mirror = None
        x3 = mirror is not None and getattr(st, 'mirror_pieces', 1) == 3
        dst = st.pair_src() if x3 else None       # fp32x3: the layers' weights go to the mirror in the paired-row layout (the launch walks the mirror's order)
        return (st.flat_params.data_ptr() + off, st.flat_grads.data_ptr() + off,
                (grad_bf16.data_ptr() + lo * 2) if grad_bf16 is not None else None,
                self.exp_avg.data_ptr() + off, (self.exp_avg_sq.data_ptr() + off) if self.exp_avg_sq is not None else None,
                flags.data_ptr() + lo // CHUNK, hi - lo, ptr(self._sumsq),
                scale.grad_scale, scale.max_grad_norm, *h, scale.zero_grads,
                (mirror.data_ptr() + lo * 2) if mirror is not None else None, st.numel if x3 else 0,
                (dst.data_ptr() + 8 * (lo // CHUNK)) if dst is not None else None, lo if dst is not None else 0, max_wgs, stream_ptr)

    def _row_flags(self, off, n, nodecay):
        """chunk flags of the word table for the row-split launches: every chunk on the update path (decay as the tensor's group says)"""
        key = ('rows', off, n, bool(nodecay))
        f = self._flags_cache.get(key)
        if f is None:
            f = torch.full((n // CHUNK,), 1 if nodecay else 2, dtype=torch.uint8, device=self.store.device)
            self._flags_cache[key] = f
        return f

    def _rule_args(self, group):
        """(beta1, beta2, eps) of the launch, from a parameter group"""
        b1, b2 = group['betas']
        return float(b1), float(b2), float(group['eps'])

    def join(self):
        """Make the current stream wait for an overlapped update still running on the side stream."""
        if self._pending is not None:
            torch.cuda.current_stream().wait_event(self._pending)
            self._pending = None

    LAZY_SUFFIXES = ('attention.self.query.weight', 'attention.self.key.weight', 'attention.self.value.weight',
                     'attention.output.dense.weight', 'intermediate.dense.weight', 'output.dense.weight')

    def _chunk_flags(self, lazy=False, grouped=False):
        """grouped: the bytes of uniter_optim_step_groups -- the tensor's parameter group in bits 3-7, and weight decay (2) wherever
        the group's own weight_decay is not 0"""
        st = self.store
        decays = tuple(float(g['weight_decay']) != 0.0 for g in self.param_groups) if grouped else None
        key = (frozenset(st.touched), bool(lazy)) if not grouped else (frozenset(st.touched), bool(lazy), decays)
        if key != self._flags_key:
            flags = self._flags_cache.get(key)
            if flags is None:
                keep = [n for n in st.touched if lazy and '.encoder.layer.' in '.' + n and n.endswith(self.LAZY_SUFFIXES)]
                bits = {n: (k, decays[k]) for n, (k, _) in self._group_of.items()} if grouped else None
                host = chunk_flag_bytes(st.numel // CHUNK, st.offsets, {n: st.params[n].numel() for n in st.touched}, st.touched,
                                        self._frozen, frozenset(keep), bits)
                flags = host.to(st.device)
                if len(self._flags_cache) < 16:
                    self._flags_cache[key] = flags
            self._flags = flags
            self._flags_key = key
        return self._flags

    def grad_norm(self):
        """L2 norm of all gradients touched since the last zero_grad (device tensor)."""
        self._sumsq_range(0, self.store.numel, self._sumsq.data_ptr(), self._chunk_flags(), None)
        return self._sumsq.sqrt()

    def _sumsq_range(self, lo, hi, out_ptr, flags, grad_bf16):
        """sum of squares of the gradients in [lo, hi) -- the bf16 payload's where there is one -- into the double at out_ptr"""
        name, g = ('uniter_grad_sumsq', self.store.flat_grads.data_ptr() + 4 * lo) if grad_bf16 is None else \
            ('uniter_grad_sumsq_bf16', grad_bf16.data_ptr() + 2 * lo)
        check(getattr(_lib.lib(), name)(g, flags.data_ptr() + lo // CHUNK, hi - lo, out_ptr, ptr(self._ws), self._ws_bytes,
                                        _lib.cur_stream()), name)

    def _clip_norm(self, flags, max_grad_norm, grad_ready, grad_bf16, grad_pieces):
        """Leave the squared norm of all gradients in _sumsq when the step clips.  True: it did, and grad_ready is consumed."""
        armed, self._np_blocks = self._np_blocks, 0           # (disarmed on every step, clipping or not)
        if not (max_grad_norm and max_grad_norm > 0):
            return False
        st, lib = self.store, _lib.lib()
        pieces = sorted(grad_pieces) if (grad_ready is not None and grad_pieces) else None
        if pieces is not None and not (pieces[0][0] == 0 and pieces[-1][1] == st.numel and
                                       all(a[1] == b[0] for a, b in zip(pieces, pieces[1:]))):
            pieces = None                     # the slices do not tile the buffer: one pass over all of it
        if armed and grad_ready is None and grad_bf16 is None and not self._frozen:
            # the backward pass left the norm as partial sums (attach_norm_hooks): join them
            check(lib.uniter_sumsq_combine(ptr(self._np_buf), armed, ptr(self._sumsq), _lib.cur_stream()), 'uniter_sumsq_combine')
        elif pieces is None or len(pieces) == 1:
            if grad_ready is not None:
                grad_ready(0, st.numel)
            self._sumsq_range(0, st.numel, self._sumsq.data_ptr(), flags, grad_bf16)
        else:
            if self._parts is None or self._parts.numel() < len(pieces):
                self._parts = torch.zeros(max(16, len(pieces)), dtype=torch.float64, device=st.device)
            for k, (lo, hi) in enumerate(grad_pieces):        # issue order: the early collectives have landed long ago
                grad_ready(lo, hi)
                self._sumsq_range(lo, hi, self._parts.data_ptr() + 8 * k, flags, grad_bf16)
            check(lib.uniter_sumsq_combine(ptr(self._parts), len(pieces), ptr(self._sumsq), _lib.cur_stream()), 'uniter_sumsq_combine')
        return True

    def _execute(self, sched, wt, early_ev, grad_ready, h, scale, flags, grad_bf16, layers, blocks=None, avg_w=None):
        """Issue optim_schedule's launches.  wt: the word table of a 'rows' launch; early_ev: what the main stream waits for first;
        blocks: the plan's blocks when launches may have been dropped from `sched` (frozen parameters), else None; avg_w: the
        average's weight of this step when averaging is on"""
        lib = _lib.lib()
        flat, kind, what = (lib.uniter_adam_step_x3p, (), 'uniter_adam_step') if self.KIND is None else \
            (lib.uniter_optim_step, (self.KIND,), 'uniter_optim_step')
        if isinstance(h, GroupHyper):       # every 'flat' launch with its chunks' own hyper-parameters
            flat, kind, what = lib.uniter_optim_step_groups, (int(self.adamw) if self.KIND is None else self.KIND,), 'uniter_optim_step_groups'
        if avg_w is not None:               # .. and with the average's stream: the same launches through the _avg entry points
            if isinstance(h, GroupHyper):
                flat, what = lib.uniter_optim_step_groups_avg, 'uniter_optim_step_groups_avg'
            else:
                flat, kind, what = lib.uniter_optim_step_avg, (int(self.adamw) if self.KIND is None else self.KIND,), 'uniter_optim_step_avg'
        streams = {'main': self._stream('main')}
        events, by_range = {'block': [], 'word': []}, {}
        for r in sched:
            if r.stream not in streams:         # the first launch on the side stream: behind everything queued on the main stream so far
                streams['side'] = self._stream('side', keep=True)
                streams['side'][0].wait_stream(streams['main'][0])
            s, sp = streams[r.stream]
            if r.wait is not None:
                if r.stream == 'main':
                    grad_ready(*r.wait)
                else:
                    with torch.cuda.stream(s):
                        grad_ready(*r.wait)
            if early_ev is not None and r is sched[0]:
                s.wait_event(early_ev)
            if r.kind == 'rows':
                check(lib.uniter_adam_step_rows(*self._rows_args(wt, h, ptr(self._sumsq), scale, 1, r.max_wgs, sp)), 'uniter_adam_step_rows')
            else:
                args = self._range_args(r.lo, r.hi, r.max_wgs, sp, h, scale, flags, grad_bf16, layers)
                if avg_w is not None:       # (avg, avg_weight) in front of max_workgroups
                    args = args[:-2] + (self.avg.data_ptr() + 4 * r.lo, avg_w) + args[-2:]
                check(flat(*kind, *args), what)
            if r.clear_mask:
                with torch.cuda.stream(s):
                    self._rowmask.zero_()
                self._rowmask_clear = torch.cuda.Event()
                self._rowmask_clear.record(s)
            if r.event is not None:
                ev = torch.cuda.Event()
                ev.record(s)
                events[r.event].append(ev)
                by_range[(r.lo, r.hi)] = ev
        if events['block'] or events['word']:
            # the forward pass gets the blocks' events in its own order and the word table's behind them; join() waits for the last block
            ready = events['block'] + events['word']
            if blocks is not None and len(events['block']) != len(blocks):
                # launches were dropped (frozen blocks): the forward pass still takes one event per block, in its order -- a block
                # without an update gets an event of the main stream, which the forward pass (on that stream) is behind already
                idle = torch.cuda.Event()
                idle.record(streams['main'][0])
                ready = [next((ev for (lo, hi), ev in by_range.items() if b[0] <= lo and hi <= b[1] and ev in events['block']), idle)
                         for b in blocks] + events['word']
            self.overlap_encoder._set_ready_events(ready)
            self._pending = (events['block'] or events['word'])[-1]     # (only the word table trainable: its launch is the last)
        elif blocks is not None:
            self.overlap_encoder._set_ready_events([])      # every block frozen: the forward pass waits for nothing of this step

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0, max_grad_norm=0.0, zero_grads=True, grad_ready=None, grad_bf16=None,
             grad_pieces=None):
        """grad_bf16: optional bf16 tensor holding the gradients to apply (the reduced data-parallel payload, dp.GradSync.comm)
        in place of the fp32 gradient buffer, which is still zeroed.
        grad_ready(lo, hi): optional callable that makes the CURRENT stream wait until flat_grads[lo:hi] is final
        (dp.GradSync.wait_range): each block launch then waits only for the gradient buckets that cover it.  Clipping
        needs the norm of everything: with max_grad_norm > 0 it is reduced slice by slice over `grad_pieces` (the
        collectives' slices in issue order, tiling the buffer) -- wait for one, reduce it into its slot, go on -- so
        that behind the backward only the last collective and the norm of ITS slice are ahead of the update; without
        `grad_pieces` the whole buffer is waited for and reduced in one pass."""
        if closure is not None:
            raise UniterHipError('FusedAdam does not support closures')
        st = self.store
        if not st.is_current():
            raise UniterHipError('model parameters were moved after the optimizer was built')
        if self._exchanged:
            raise UniterHipError('%s.step inside averaged_parameters(): the parameters hold the averaged weights' % type(self).__name__)
        grouped = not self._uniform()
        sw = optim_switches()
        lazy = bool(zero_grads) and self.lazy_zero_encoder is not None and sw.lazy_zero
        flags = self._chunk_flags(lazy, grouped)
        if self._clip_norm(flags, max_grad_norm, grad_ready, grad_bf16, grad_pieces):
            grad_ready = None
        self.step_count += 1
        h = self._group_hyper(self.step_count) if grouped else self._hyper(self.step_count)
        scale = Scale(float(grad_scale), float(max_grad_norm or 0.0), int(bool(zero_grads)))
        enc = self.overlap_encoder
        plan = self._overlap_plan(enc) if enc is not None else None
        layers = (min(b[0] for b in plan[1][1:]), max(b[1] for b in plan[1][1:])) if plan is not None and len(plan[1]) > 1 else None
        # the word table's rows without a gradient were updated ahead (early_word_update): its launch takes the looked-up rows, and
        # without overlap the main stream waits for the ahead-of-time launch (overlapped, both run on the side stream)
        early, self._early = self._early, None
        wt = self._word_table() if early is not None else None
        if early is not None and (wt is None or grouped or early[0] != h or grad_bf16 is not None):
            raise UniterHipError('FusedAdam.step: the word-embedding rows without a gradient were updated ahead (early_word_update) '
                                 'for step %d / lr %g, but this step runs with other hyper-parameters or a bf16 gradient payload'
                                 % (early[0].step_count, early[0].lr))
        trainable = self._trainable_ranges()
        sched = optim_schedule(st.numel, plan, wt, grad_ready is not None, self.overlap_workgroups, sw,
                               **({} if trainable is None else {'trainable': trainable}))
        more = {} if trainable is None or plan is None else {'blocks': plan[1]}
        if self.ema_decay:
            more['avg_w'] = float(ema_weight(self.ema_decay, self.avg_steps, self.ema_warmup))
            self.avg_steps += 1
        self._execute(sched, wt, early[1] if early is not None and plan is None else None, grad_ready, h, scale, flags, grad_bf16, layers,
                      **more)
        if early is not None or self._rows_noted is not False:
            # the row mask belongs to the micro-batches of THIS step: clear it behind its last reader
            if self._rowmask is not None and not (plan is not None and early is not None):
                self._rowmask.zero_()          # (the overlapped path cleared it behind the looked-up rows' launch, on the side stream)
                self._rowmask_clear = None
            self._rows_noted = False
        if zero_grads:
            st.touched.clear()      # flags stay cached: the same set is touched again next step
            if lazy:
                st.wgrad_stale = True

    def zero_grad(self, set_to_none=False):
        self.store.zero_grads()
        self._flags_key = None

    # -- the averaged weights -------------------------------------------------------------------------------------------
    def _exchange(self):
        p, a = self.store.flat_params, self.avg
        with torch.no_grad():
            t = p.detach().clone()
            p.copy_(a)          # in place: the version counter moves, ParamStore.ensure_mirror rebuilds the bf16 / x3 mirror
            a.copy_(t)

    @contextlib.contextmanager
    def averaged_parameters(self):
        """Inside the block the model's parameters ARE the averaged weights (evaluation, the checkpoint's model_state_dict): waits
        for an overlapped update, exchanges the contents of the flat parameter buffer and `avg` in place -- the weight mirror of the
        bf16 / fp32x3 modes is rebuilt at the next forward pass -- and exchanges them back on the way out: the raw weights return
        bit for bit.  Nesting and step() inside the block raise."""
        if self.avg is None:
            raise UniterHipError('averaged_parameters(): this optimizer keeps no average (ema_decay is off)')
        if self._exchanged:
            raise UniterHipError('averaged_parameters() does not nest')
        self.join()
        self._exchange()
        self._exchanged = True
        try:
            yield self
        finally:
            self.join()
            self._exchange()
            self._exchanged = False

    # -- state_dict in torch's layout -----------------------------------------------------------------------------------
    def _state_order(self):
        """[(store name or None (frozen), shape)] of the parameters in param_groups order; the flat tensors and torch's keys"""
        by_id = {id(p): n for n, p in self.store.params.items()}
        order = []
        for g in self.param_groups:
            for p in g['params']:
                n = by_id.get(id(p))
                order.append((None if n is None or n in self._frozen else n, tuple(p.shape)))
        flat = (self.exp_avg, self.exp_avg_sq) if self.SECOND_STATE else (self.exp_avg,)
        return order, flat, STATE_KEYS[self.KIND]

    def state_dict(self):
        """torch.optim's layout: {'state': {i: {'step', 'exp_avg', ..}}, 'param_groups': [..]} with the i-th parameter in param_groups
        order -- loadable by the torch optimizer of the same rule over the same parameters -- plus, with averaging on, top-level
        'averaged' ({i: tensor}) and 'averaged_steps', which torch's loader ignores.  Waits for an overlapped step first."""
        self.join()
        groups = super().state_dict()['param_groups']
        order, flat, keys = self._state_order()
        out = {'state': pack_optim_state(order, self.store.offsets, flat, keys, self.step_count), 'param_groups': groups}
        if self.avg is not None:
            # (inside averaged_parameters() the two buffers are exchanged: the average sits in the parameters' place)
            out['averaged'] = pack_averaged(order, self.store.offsets, self.store.flat_params if self._exchanged else self.avg)
            out['averaged_steps'] = self.avg_steps
        return out

    def load_state_dict(self, state_dict):
        """Takes this class's dicts and those of torch.optim.Adam / AdamW / Adamax / SGD over the same parameters in the same order:
        the moments go into the flat buffers, the hyper-parameters ('initial_lr' included) come from the dict's groups as torch
        takes them, step_count from the entries' `step` (they must agree).  Without 'averaged' while averaging is on, the average
        restarts from the current parameters."""
        self.join()
        if self._exchanged:
            raise UniterHipError('load_state_dict() inside averaged_parameters()')
        groups, state = state_dict['param_groups'], state_dict.get('state', {})
        if len(groups) != len(self.param_groups):
            raise ValueError('loaded state dict has %d parameter groups, this optimizer %d' % (len(groups), len(self.param_groups)))
        for k, (mine, theirs) in enumerate(zip(self.param_groups, groups)):
            if len(mine['params']) != len(theirs['params']):
                raise ValueError('parameter group %d holds %d parameters in the loaded state dict, %d here'
                                 % (k, len(theirs['params']), len(mine['params'])))
        order, flat, keys = self._state_order()
        with torch.no_grad():
            step = unpack_optim_state(state, order, self.store.offsets, flat, keys)
            for mine, theirs in zip(self.param_groups, groups):
                mine.update({k: v for k, v in theirs.items() if k != 'params'})
            if step is not None:
                self.step_count = step
            elif not state:
                self.step_count = 0
            if self.avg is not None:
                if state_dict.get('averaged') is not None:
                    unpack_averaged(state_dict['averaged'], order, self.store.offsets, self.avg)
                    self.avg_steps = int(state_dict.get('averaged_steps', 0))
                else:
                    self.avg.copy_(self.store.flat_params)
                    self.avg_steps = 0


class FusedAdamax(FusedAdam):
    """torch.optim.Adamax (coupled L2; utils/optim_utils.py:36-37) over the flat buffers: FusedAdam's launch with the Adamax rule
    (uniter_optim_step, kind 2).  ``exp_avg_sq`` holds the infinity norm (torch's ``exp_inf``).

    The step counter is the OPTIMIZER's (``step_count``), as in FusedAdam; torch keeps one per parameter.  The two agree as long
    as every parameter receives a gradient from the first step on; a parameter whose first gradient arrives late (a head that
    joins multitask training at step k) gets the GLOBAL bias correction 1 - beta1^step here, torch's starts it at 1 - beta1.

    No row-split update of the word-embedding table (``split_word_rows`` is False whatever UNITER_ADAM_WORD_ROWS says)."""

    KIND = 2

    def __init__(self, model, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, group_param_func=None, layout=None,
                 ema_decay=None, ema_warmup=True):
        super().__init__(model, lr, betas=betas, eps=eps, weight_decay=weight_decay, adamw=False, group_param_func=group_param_func,
                         layout=layout, ema_decay=ema_decay, ema_warmup=ema_warmup)


class FusedSGD(FusedAdam):
    """torch.optim.SGD with momentum, dampening 0, no Nesterov (coupled L2; utils/optim_utils.py:41-43) over the flat buffers:
    FusedAdam's launch with the SGD rule (uniter_optim_step, kind 3).  ``exp_avg`` is the momentum buffer -- zeros before the first
    step, which reproduces torch's ``buf = grad`` exactly -- and there is NO second state: ``exp_avg_sq`` is None, 8 bytes per
    parameter less than Adam in memory and in the step's traffic.  ``momentum = 0`` is plain SGD.

    A parameter without a gradient in a step is skipped, momentum included, as torch skips ``grad is None``.  The rule has no step
    counter of its own; ``step_count`` counts as in FusedAdam.  No row-split update of the word-embedding table."""

    KIND = 3
    SECOND_STATE = False

    def __init__(self, model, lr, momentum=0.0, weight_decay=0.0, group_param_func=None, layout=None, ema_decay=None, ema_warmup=True):
        super().__init__(model, lr, weight_decay=weight_decay, adamw=False,
                         defaults=dict(lr=lr, momentum=momentum, weight_decay=weight_decay), group_param_func=group_param_func,
                         layout=layout, ema_decay=ema_decay, ema_warmup=ema_warmup)

    def _rule_args(self, group):
        return float(group['momentum']), 0.0, 0.0


class TorchOptimizerStep(object):
    """`--optimizer adamax | sgd` (utils/optim_utils.py:36-43) with torch.optim's own update on the views into the flat buffers
    (get_optimizer(.., fused=False)); averaging, global-norm clipping and zero_grad around it follow FusedAdam.step's
    contract so the trainer drives both alike.  Not a fused kernel: the comparison partner of FusedAdamax / FusedSGD."""

    def __init__(self, model, inner):
        self.store = model.param_store() if hasattr(model, 'param_store') else ensure_store(model)
        self.inner = inner
        self.param_groups = inner.param_groups

    def join(self):
        pass

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0, max_grad_norm=0.0, zero_grads=True, grad_ready=None):
        st = self.store
        if grad_ready is not None:
            grad_ready(0, st.numel)
        g = st.flat_grads
        if grad_scale != 1.0:
            g.mul_(grad_scale)
        if max_grad_norm and max_grad_norm > 0:
            g.mul_(torch.clamp(float(max_grad_norm) / (g.norm() + 1e-6), max=1.0))
        idle = [p for n, p in st.params.items() if n not in st.touched]     # no gradient this step: no update, no decay
        for p in idle:
            p.grad = None
        self.inner.step()
        st.reattach_grads(full=True)
        st.mirror_dirty = True
        if zero_grads:
            g.zero_()
            st.touched.clear()

    def zero_grad(self, set_to_none=False):
        self.store.zero_grads()


def get_optimizer(model, config, group_param_func=None, fused=True):
    """utils/optim_utils.py:9-46: the parameter groups -- everything, or what `group_param_func` returns (a list of dicts whose
    'params' are (name, parameter) pairs; every other key, an 'lr' of the group's own above all, is copied), each split into a
    decay and a no-decay group (weight decay off for biases and LayerNorm) -- then the optimizer by name.  All four run as the
    fused HIP step; fused=False runs adamax / sgd as torch.optim's own update (TorchOptimizerStep)."""
    name = config['optimizer']
    ema = dict(ema_decay=config.get('ema_decay') or None, ema_warmup=config.get('ema_warmup', True))
    if ema['ema_decay'] and not fused:
        raise ValueError('ema_decay needs the fused step (the average is kept by its kernel): fused=False keeps none')
    if name in ('adam', 'adamw'):
        return FusedAdam(model, lr=config['lr'], betas=(config['beta1'], config['beta2']),
                         weight_decay=config['weight_decay'], adamw=(name == 'adamw'), group_param_func=group_param_func, **ema)
    if name not in ('adamax', 'sgd'):
        raise ValueError('invalid optimizer %r' % name)
    store = model.param_store() if hasattr(model, 'param_store') else ensure_store(model)
    # ONE layout for the torch optimizer and the fused class: `group_param_func` is called once, with the model's own names as
    # the reference calls it (without one the names only decide decay / no decay, and the store's order is kept)
    named = list(store.params.items()) if group_param_func is None else list(model.named_parameters())
    layout = group_layout(named, config['weight_decay'], group_param_func)
    groups = [dict(g, params=[p for _, p in g['params']]) for g in layout]
    if group_param_func is None:
        layout = None           # (the fused classes order their two groups as the model names its parameters, as they always did)
    if name == 'adamax':             # utils/optim_utils.py:36-37: torch's default betas, the config's are not passed
        inner = torch.optim.Adamax(groups, lr=config['lr'])
    else:                            # :41-43: momentum = beta1
        inner = torch.optim.SGD(groups, lr=config['lr'], momentum=config['beta1'])
    if not fused:
        return TorchOptimizerStep(model, inner)
    # the torch optimizer carries the reference's hyper-parameters (its defaults where the reference passes none)
    d = inner.defaults
    if name == 'adamax':
        return FusedAdamax(model, lr=d['lr'], betas=tuple(d['betas']), eps=d['eps'], weight_decay=config['weight_decay'], layout=layout, **ema)
    return FusedSGD(model, lr=d['lr'], momentum=d['momentum'], weight_decay=config['weight_decay'], layout=layout, **ema)


# --------------------------------------------------------------------------- #
# schedulers (transformers.get_*_schedule_with_warmup restated; train_template.py:72-82)
# --------------------------------------------------------------------------- #
def cosine_warmup_lambda(num_warmup_steps, num_training_steps, num_cycles=0.5):
    def f(step):
        if step < num_warmup_steps:
            return float(step) / float(max(1, num_warmup_steps))
        prog = float(step - num_warmup_steps) / float(max(1, num_training_steps - num_warmup_steps))
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(num_cycles) * 2.0 * prog)))
    return f


def linear_warmup_lambda(num_warmup_steps, num_training_steps):
    def f(step):
        if step < num_warmup_steps:
            return float(step) / float(max(1, num_warmup_steps))
        return max(0.0, float(num_training_steps - step) /
                   float(max(1, num_training_steps - num_warmup_steps)))
    return f


def get_scheduler(optimizer, config, steps_per_epoch):
    optimizer = getattr(optimizer, 'inner', optimizer)        # TorchOptimizerStep wraps a torch optimizer
    total = steps_per_epoch * config['max_epoch']
    kind = config['scheduler']
    if kind == 'step':
        return torch.optim.lr_scheduler.StepLR(optimizer, step_size=config['lr_decay_step'],
                                               gamma=config['lr_decay_factor'])
    if kind == 'multi_step':
        return torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=[5, 10, 15, 25, 40],
                                                    gamma=config['lr_decay_factor'])
    if kind == 'warmup':
        return torch.optim.lr_scheduler.LambdaLR(optimizer, linear_warmup_lambda(config['warmup_steps'], total))
    if kind == 'warmup_cosine':
        return torch.optim.lr_scheduler.LambdaLR(optimizer, cosine_warmup_lambda(config['warmup_steps'], total))
    raise ValueError('unknown scheduler %r' % kind)


# --------------------------------------------------------------------------- #
# the step
# --------------------------------------------------------------------------- #
def sync_step(optimizer, grad_sync, accum, max_grad_norm):
    """average_gradients + clip + optimizer step + zero_grad behind the data-parallel exchange
    (train_template.py:89-92,103-107).  With clipping the norm needs every bucket; without it each
    optimizer block waits only for the buckets that cover it."""
    world, ready, g16, kw = 1, None, None, {}
    if grad_sync is not None and grad_sync.active:
        world = grad_sync.world
        fused = isinstance(optimizer, FusedAdam)
        # bf16 payload + the fused optimizer: the reduced sums are consumed where RCCL left them
        grad_sync.consumer_reads_comm = grad_sync.comm is not None and fused
        if grad_sync.consumer_reads_comm:
            kw['grad_bf16'] = grad_sync.comm
        grad_sync.flush_all()
        if fused:
            ready = grad_sync.wait_range
            if max_grad_norm and max_grad_norm > 0:
                kw['grad_pieces'] = grad_sync.pieces()     # the clip norm, slice by slice as the collectives land
        else:
            grad_sync.finish()
    elif grad_sync is not None:
        world = grad_sync.world
    optimizer.step(grad_scale=1.0 / (accum * world), max_grad_norm=max_grad_norm, zero_grads=True, grad_ready=ready, **kw)



ADV_MODALITIES = ('both', 'txt', 'img', 'each')
ADV_ALGOS = ('freelb', 'villa')
ADV_NORM_TYPES = ('l2', 'linf')
AdvConfig = namedtuple('AdvConfig', 'steps lr max_norm init_mag modality algo kl_weight norm_type')


def adv_config(config):
    """The adversarial settings of a trainer config (adv_steps = 0, the default, switches the adversarial step off):
    adv_steps K, adv_lr (ascent step size), adv_max_norm (radius of the ball, <= 0: none), adv_init_mag (magnitude of the
    random start, 0: start from zero), adv_modality ('both' | 'txt' | 'img': which inputs are perturbed; 'each', VILLA only: the
    text and the regions in a round each), adv_algo ('freelb' | 'villa': VILLA adds the clean pass and the KL consistency term),
    adv_kl_weight (weight of that term, VILLA only), adv_norm_type ('l2' | 'linf': the ball and the ascent step's norm)."""
    adv = AdvConfig(int(config.get('adv_steps', 0) or 0), float(config.get('adv_lr', 0.0) or 0.0),
                    float(config.get('adv_max_norm', 0.0) or 0.0), float(config.get('adv_init_mag', 0.0) or 0.0),
                    config.get('adv_modality', 'both') or 'both', config.get('adv_algo', 'freelb') or 'freelb',
                    float(config.get('adv_kl_weight', 0.0) or 0.0), config.get('adv_norm_type', 'l2') or 'l2')
    if adv.modality not in ADV_MODALITIES:
        raise ValueError("adv_modality must be one of %s, got %r" % (', '.join(repr(m) for m in ADV_MODALITIES), adv.modality))
    if adv.algo not in ADV_ALGOS:
        raise ValueError("adv_algo must be one of %s, got %r" % (', '.join(repr(m) for m in ADV_ALGOS), adv.algo))
    if adv.norm_type not in ADV_NORM_TYPES:
        raise ValueError("adv_norm_type must be one of %s, got %r" % (', '.join(repr(m) for m in ADV_NORM_TYPES), adv.norm_type))
    if adv.steps < 0 or adv.lr < 0 or adv.init_mag < 0:
        raise ValueError('adv_steps, adv_lr and adv_init_mag must not be negative')
    if not adv.kl_weight >= 0:
        raise ValueError('adv_kl_weight must not be negative, got %r' % adv.kl_weight)
    if adv.algo == 'freelb':
        if adv.kl_weight > 0:
            raise ValueError("adv_kl_weight > 0 needs adv_algo='villa': the KL term pulls towards the clean pass, which FreeLB does not run")
        if adv.modality == 'each':
            raise ValueError("adv_modality='each' needs adv_algo='villa'")
    elif adv.steps < 1:
        raise ValueError("adv_algo='villa' needs adv_steps >= 1")
    return adv


AucConfig = namedtuple('AucConfig', 'weight bank surrogate margin')


def auc_config(config):
    """The pairwise AUROC term's settings of a trainer config (auc_weight = 0, the default, switches it off): auc_weight (its
    weight beside BCE), auc_bank (capacity of the bank of recent scores, 0: the batch alone), auc_surrogate ('logistic' |
    'hinge2'), auc_margin (the squared hinge's margin)."""
    auc = AucConfig(float(config.get('auc_weight', 0.0) or 0.0), int(config.get('auc_bank', 0) or 0),
                    config.get('auc_surrogate', 'logistic') or 'logistic', float(config.get('auc_margin', 1.0)))
    if not auc.weight >= 0:
        raise ValueError('auc_weight must not be negative, got %r' % auc.weight)
    if auc.surrogate not in AUC_SURROGATES:
        raise ValueError("auc_surrogate must be one of %s, got %r" % (', '.join(repr(s) for s in AUC_SURROGATES), auc.surrogate))
    if auc.margin != auc.margin:
        raise ValueError('auc_margin is NaN')
    if auc.bank < 0 or auc.bank > AUC_MAX_BANK:
        raise ValueError('auc_bank must lie in [0, %d], got %d' % (AUC_MAX_BANK, auc.bank))
    if auc.bank and auc.bank < int(config.get('batch_size', 0) or 0):
        raise ValueError('auc_bank = %d holds less than one batch (batch_size = %d)' % (auc.bank, config['batch_size']))
    if auc.weight > 0 and config.get('loss_func', 'bce_logits') != 'bce_logits':
        raise ValueError("auc_weight > 0 needs loss_func='bce_logits': the term is part of that loss's launch")
    return auc


def new_score_bank(auc, device):
    """The ScoreBank the AucConfig `auc` asks for, or None: the term is off, or it takes its pairs from the batch alone"""
    return ScoreBank(auc.bank, device) if auc.weight > 0 and auc.bank > 0 else None


def adv_rounds(adv):
    """The rounds of an adversarial micro-batch under the AdvConfig `adv`, each the tuple of the modalities it perturbs together:
    one round, or with adv_modality = 'each' a text round and then an image round"""
    return {'both': (('txt', 'img'),), 'txt': (('txt',),), 'img': (('img',),), 'each': (('txt',), ('img',))}[adv.modality]


def adv_delta_step(delta, grad, step_size, max_norm, norm_type='l2'):
    """One ascent step of a perturbation and its projection, per sample of the leading dimension, in place (step_size = 0
    projects only).  'l2' (uniter_adv_delta_step): delta[b] <- project(delta[b] + step_size * grad[b] / |grad[b]|) onto the L2
    ball of radius max_norm; 'linf' (uniter_adv_delta_step_linf): delta[b] <- clamp(delta[b] + step_size * grad[b] / max|grad[b]|,
    -max_norm, max_norm)."""
    if norm_type not in ADV_NORM_TYPES:
        raise ValueError("norm_type must be one of %s, got %r" % (', '.join(repr(m) for m in ADV_NORM_TYPES), norm_type))
    _lib.require_gpu_tensor(delta, torch.float32, 'delta')
    _lib.require_gpu_tensor(grad, torch.float32, 'grad')
    if delta.shape != grad.shape or not delta.is_contiguous() or not grad.is_contiguous():
        raise UniterHipError('adv_delta_step: delta and grad must be contiguous and of one shape')
    B = delta.shape[0]
    n = delta.numel() // max(B, 1)
    lib = _lib.lib()
    ws_bytes, step, name = ((lib.uniter_adv_delta_ws_bytes, lib.uniter_adv_delta_step, 'uniter_adv_delta_step') if norm_type == 'l2' else
                            (lib.uniter_adv_delta_linf_ws_bytes, lib.uniter_adv_delta_step_linf, 'uniter_adv_delta_step_linf'))
    ws = torch.empty(max(ws_bytes(B, n), 8), dtype=torch.uint8, device=delta.device)
    check(step(ptr(delta), ptr(grad), B, n, float(step_size), float(max_norm), ptr(ws), _lib.cur_stream()), name)
    return delta


class TrainStep(object):
    """`TrainerTemplate.calculate_loss` (train_template.py:95-126) + the forward of
    `TrainerUniter.train_iter_step` (train_uniter.py:67-72).

    With ``adv_steps`` = K > 0 in the config a micro-batch is a FreeLB step (`adv_config`, `_train_iter_adv`): K forward /
    backward passes on the batch (`_adv_passes`) with a perturbation on the word-embedding rows and / or the region features, the
    perturbation taking one normalised ascent step (projected onto the ball of radius ``adv_max_norm``) between two passes.  The
    parameter gradients of the K passes accumulate as micro-batches do and the optimizer step divides by K on top of
    ``gradient_accumulation``.  The logged loss and probabilities are the first (least perturbed) pass's.

    With ``adv_algo`` = 'villa' the micro-batch is a VILLA step instead, the same passes in another frame: a clean pass with
    today's loss (`_clean_pass`), then per round (`adv_rounds`) K perturbed passes whose loss is BCE + ``adv_kl_weight`` x the
    symmetric KL divergence to the clean prediction (`bce_kl_with_logits_loss`, its gradient scaled by 1 / K in the launch), so that the accumulated gradient is
    g_clean + (1 / K) sum_k g_adv,k per round.  ``adv_modality`` = 'each' runs a text round and an image round, each with a
    perturbation of its own; ``adv_norm_type`` chooses the L2 or the L-infinity ball.  The logged loss and probabilities are
    the clean pass's; `last_adv_terms` holds [total, bce, kl] of the last perturbed pass.

    With ``auc_weight`` > 0 (`auc_config`) the loss of the training passes is `bce_auc_with_logits_loss`: BCE plus the pairwise
    AUROC surrogate against the batch and a `ScoreBank` of ``auc_bank`` recent scores, which the same launch pushes into -- the
    plain step, VILLA's clean pass, and FreeLB's K passes (the first of them pushes).  VILLA's perturbed passes keep their BCE +
    KL loss, and `eval_iter` the plain BCE: it never touches the bank.  `last_auc_terms` holds [total, bce, auc].

    Quirk kept on purpose: the modulo test is on the per-epoch iteration index
    starting at 0, so iteration 0 steps immediately with a single micro-batch whose
    gradient is still divided by ``gradient_accumulation``.
    """

    def __init__(self, model, optimizer, scheduler, config, grad_sync=None, auc_bank=None):
        self.model, self.optimizer, self.scheduler, self.config = model, optimizer, scheduler, config
        self.grad_sync = grad_sync          # DP: object with .finish() called before the optimizer step
        self.auc = auc_config(config)       # (before the loss_func check: auc_weight > 0 with another loss is a ValueError)
        if config.get('loss_func', 'bce_logits') != 'bce_logits':
            raise UniterHipError("only loss_func='bce_logits' is built on the HIP path")
        # auc_weight > 0: the training passes' loss is bce_auc_with_logits_loss (_train_loss); the bank of recent scores is the
        # caller's (TrainerTemplate keeps one across epochs) or this step's own.  Each rank of a data-parallel run has its own
        self.auc_bank = auc_bank if (auc_bank is not None or self.auc.weight <= 0) else \
            new_score_bank(self.auc, next(model.parameters()).device)
        self.last_auc_terms = None          # the device tensor [total, bce, auc] of the last training pass that carried the term
        enc = getattr(model, 'uniter_model', None)
        if grad_sync is None and enc is not None and isinstance(optimizer, FusedAdam) and (config.get('max_grad_norm') or 0) > 0:
            optimizer.attach_norm_hooks(enc)        # the clip norm is reduced bucket by bucket during the backward pass
        if enc is not None and isinstance(optimizer, FusedAdam):
            optimizer.lazy_zero_encoder = enc       # zero_grad skips what the next backward pass overwrites anyway
        self.iters = 0
        self.last_loss = None
        self.last_probs = None
        self.adv = adv_config(config)
        if self.adv.steps > 0 and grad_sync is not None:
            # (the exchange's prepare(will_step=...) would have to be held back to the last of the K passes: not built, because it
            # could not be checked without a multi-rank run)
            raise UniterHipError('adv_steps > 0 (FreeLB) is built for the single-process step: not with a data-parallel gradient exchange'
                                 if self.adv.algo == 'freelb' else
                                 "adv_algo='villa' is built for the single-process step: not with a data-parallel gradient exchange")
        self._adv_gen = None
        self.last_adv_delta = None      # (delta_txt, delta_img) after the last adversarial micro-batch's final ascent step
        self.last_adv_terms = None      # VILLA: the device tensor [total, bce, kl] of the last perturbed pass

    def _adv_start(self, batch, shape):
        """delta_0 of one perturbation: uniform in [-1, 1] * adv_init_mag / sqrt(n) per sample (n = its elements per sample;
        adv_norm_type = 'linf': uniform in [-1, 1] * adv_init_mag) from a device generator seeded with the config's seed,
        projected onto the ball; zeros for adv_init_mag = 0"""
        dev = batch['labels'].device
        if self.adv.init_mag <= 0:
            return torch.zeros(shape, dtype=torch.float32, device=dev)
        if self._adv_gen is None or self._adv_gen.device != dev:
            self._adv_gen = torch.Generator(device=dev)
            self._adv_gen.manual_seed(int(self.config.get('seed', 0) or 0) + 0x5EED)
        n = 1
        for d in shape[1:]:
            n *= int(d)
        linf = self.adv.norm_type == 'linf'
        mag = self.adv.init_mag if linf else self.adv.init_mag / n ** 0.5
        delta = (torch.rand(shape, generator=self._adv_gen, dtype=torch.float32, device=dev) * 2 - 1) * mag
        if self.adv.max_norm > 0:
            adv_delta_step(delta, delta, 0.0, self.adv.max_norm, self.adv.norm_type)
        return delta

    def _train_loss(self, logits, labels, push=True):
        """The loss of a training pass on unperturbed or FreeLB-perturbed logits -> (loss, probs): today's launch, or with
        auc_weight > 0 the one that adds the pairwise AUROC term and, with `push`, pushes the logits into the bank"""
        if self.auc.weight <= 0:
            return bce_with_logits_loss(logits, labels, self.config['pos_wt'], return_probs=True)
        loss, self.last_auc_terms, probs = bce_auc_with_logits_loss(
            logits, labels, self.config['pos_wt'], self.auc.weight, bank=self.auc_bank, surrogate=self.auc.surrogate,
            margin=self.auc.margin, push=push, return_terms=True, return_probs=True)
        return loss, probs

    def _clean_pass(self, batch, train=False):
        """forward + the loss -> (logits, loss, probs); the caller runs backward (or none: eval_iter, whose loss is the plain BCE
        whatever the training passes add to it, and which never touches the bank)"""
        preds = self.model(**self.forward_kwargs(batch))
        if train:
            loss, probs = self._train_loss(preds.squeeze(1), batch['labels'])
        else:
            loss, probs = bce_with_logits_loss(preds.squeeze(1), batch['labels'], self.config['pos_wt'], return_probs=True)
        return preds, loss, probs

    def _adv_deltas(self, batch, which, delta0):
        """The perturbations a round starts from, text before image: {'txt': [B, T, H], 'img': [B, R, D]} without the modalities
        the round leaves alone or the batch lacks; from delta0 where it holds one, else the seeded random start"""
        deltas = {}
        for m, key in (('txt', 'input_ids'), ('img', 'img_feat')):
            if m not in which or batch.get(key) is None:
                continue
            if delta0.get(m) is not None:
                deltas[m] = delta0[m].detach().clone().float().contiguous()
            else:
                tail = (self.model.uniter_model.config.hidden_size,) if m == 'txt' else ()
                deltas[m] = self._adv_start(batch, tuple(batch[key].shape) + tail)
        return deltas

    def _adv_passes(self, batch, deltas, loss_fn):
        """K forward / backward passes on the batch under `deltas` (_adv_deltas), which take one ascent step between two passes, in
        place.  loss_fn(logits) -> (loss, what it yields besides).  -> [(loss, the latter)] of the K passes"""
        adv, K, out = self.adv, self.adv.steps, []
        for k in range(K):
            ascend = k < K - 1              # the last pass needs no gradient of the perturbation
            kw = self.forward_kwargs(batch)
            leaves = {m: d.detach().requires_grad_(ascend) for m, d in deltas.items()}      # (each shares its delta's memory)
            if 'txt' in leaves:
                kw['txt_embed_delta'] = leaves['txt']
            if 'img' in leaves:
                kw['img_feat'] = batch['img_feat'] + leaves['img']
            loss, extra = loss_fn(self.model(**kw).squeeze(1))
            loss.backward(unit_gradient(loss.device))
            out.append((loss.detach(), extra))
            if ascend:
                for m, leaf in leaves.items():
                    adv_delta_step(deltas[m], leaf.grad.contiguous(), adv.lr, adv.max_norm, adv.norm_type)
        return out

    def _train_iter_adv(self, batch, stepping, delta0=None):
        """An adversarial micro-batch (class docstring): VILLA's clean pass, then per round (adv_rounds) the K passes.  delta0:
        {'txt': [B, T, H], 'img': [B, R, D]} to start from (either may be missing) instead of the seeded random start; with
        adv_modality = 'each' its 'txt' starts the text round and its 'img' the image round."""
        cfg, adv = self.config, self.adv
        K, villa, labels, pos_wt = adv.steps, adv.algo == 'villa', batch['labels'], cfg['pos_wt']
        if villa:
            preds, loss, probs = self._clean_pass(batch, train=True)
            loss.backward(unit_gradient(loss.device))
            result = loss.detach(), probs
            clean = preds.detach().squeeze(1)       # (no copy: every forward pass returns logits in a tensor of its own)
            # the 1 / K of the round's average sits in the loss launch: the optimizer step's grad_scale stays the plain one
            loss_fn = lambda z: bce_kl_with_logits_loss(z, clean, labels, pos_wt, adv.kl_weight, grad_scale=1.0 / K, return_terms=True)
        else:
            # (auc_weight > 0: a sample enters the bank once per micro-batch -- the first, least perturbed pass pushes, the others do not)
            seen = []

            def loss_fn(z):
                seen.append(1)
                return self._train_loss(z, labels, push=len(seen) == 1)
        final = {}
        for which in adv_rounds(adv):
            deltas = self._adv_deltas(batch, which, delta0 or {})
            if villa and not deltas:        # (nothing to perturb: VILLA has its clean pass; FreeLB's K passes run regardless)
                continue
            passes = self._adv_passes(batch, deltas, loss_fn)
            final.update(deltas)
            if villa:
                self.last_adv_terms = passes[-1][1]
            else:
                result = passes[0]
        self.last_adv_delta = (final.get('txt'), final.get('img'))
        if stepping:
            # FreeLB's K passes were accumulated like K micro-batches: the step's grad_scale carries the extra 1 / K
            sync_step(self.optimizer, None, cfg['gradient_accumulation'] * (1 if villa else K), cfg['max_grad_norm'])
            self.scheduler.step()
        return result

    @staticmethod
    def forward_kwargs(batch):
        return dict(img_feat=batch['img_feat'], img_pos_feat=batch['img_pos_feat'],
                    input_ids=batch['input_ids'], position_ids=batch['position_ids'],
                    attention_mask=batch['attn_mask'], gather_index=batch['gather_index'],
                    output_all_encoded_layers=False, seq_lens=batch.get('seq_lens'))

    def train_iter(self, batch, iters=None, adv_delta0=None):
        if iters is not None:
            self.iters = iters
        cfg = self.config
        accum = cfg['gradient_accumulation']
        stepping = self.iters % accum == 0
        opt = self.optimizer
        if self.grad_sync is None and isinstance(opt, FusedAdam) and opt.split_word_rows:
            # single process: the rows of the word-embedding table this step cannot touch are updated AHEAD, beside this forward pass
            # (FusedAdam.early_word_update); with a gradient exchange the other ranks' tokens are not known here
            opt.note_tokens(batch.get('input_ids'))
            if stepping:
                opt.early_word_update()
        if self.adv.steps > 0:
            self.last_loss, self.last_probs = self._train_iter_adv(batch, stepping, adv_delta0)
            self.iters += 1
            return self.last_loss
        _, loss, probs = self._clean_pass(batch, train=True)
        if self.grad_sync is not None:
            self.grad_sync.prepare(will_step=stepping, token_ids=batch['input_ids'])
        loss.backward(unit_gradient(loss.device))
        if stepping:
            sync_step(self.optimizer, self.grad_sync, accum, cfg['max_grad_norm'])
            self.scheduler.step()
        self.last_loss, self.last_probs = loss.detach(), probs
        self.iters += 1
        return self.last_loss

    @torch.no_grad()
    def eval_iter(self, batch):
        return self._clean_pass(batch)[1:]

    @torch.no_grad()
    def test_iter(self, batch):
        return self.model(**self.forward_kwargs(batch)).squeeze()
