"""MemeUniter: UNITER encoder -> pooler -> Linear(hidden, n_classes)
(mirror of model/meme_uniter.py:6-21)."""
from torch import nn

from .model import UniterModel, HipLinear, ensure_store, pool_head


class MemeUniter(nn.Module):

    def __init__(self, uniter_model: UniterModel, hidden_size: int, n_classes: int):
        super().__init__()
        self.uniter_model = uniter_model
        self.n_classes = n_classes
        self.linear = HipLinear(hidden_size, n_classes)
        # True: the encoder is told that only row 0 of every sample of its output is read (the pooler's input) and that the gradient
        # coming back is zero elsewhere, so its last layer computes those rows only behind the attention (fp32x3 on padded batches;
        # every other mode ignores it).  The other rows of the encoder's output are then exact zeros.  False: every row, as UniterModel
        # alone computes them
        self.head_rows_only = True

    def param_store(self):
        """Flat parameter/gradient storage shared by encoder and head."""
        st = ensure_store(self)
        self.uniter_model._ensure_handle()
        return st

    def forward(self, **kwargs):
        ensure_store(self)
        um = self.uniter_model
        if self.head_rows_only:
            um._head_rows_next = True      # one-shot: the encoder's forward pass hands it to the library and forgets it
        try:
            out = um(**kwargs)
        finally:
            um.__dict__.pop('_head_rows_next', None)      # (a call refused before it reached the library leaves nothing behind)
        # pooler -> linear (model/meme_uniter.py:19-21), one launch each way
        return pool_head(out, self.uniter_model.pooler, self.linear)
