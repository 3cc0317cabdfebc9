"""Shared by the tests of the trainable item table: the torch yardstick of tests/ncf_train_util.py with the table as one more trained
parameter -- autograd through the gathered table rows, clip_grad_norm_ over head and table together, AdamW with the table decaying like
every weight -- and the helpers that lay a head and a table out in the flat buffers of the device entries."""
import numpy as np
import torch

from pmgt_amd.ncf_train import TABLE_KEY
from tests.ncf_train_util import TorchHead


class TorchTableHead(TorchHead):
    """TorchHead whose item table is a parameter, keyed TABLE_KEY in `p` (so it is clipped, stepped and decayed with the head)."""

    def __init__(self, w, table, dtype, lr, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None):
        super().__init__({**w, TABLE_KEY: table}, table, dtype, lr, weight_decay=weight_decay, betas=betas, eps=eps, max_grad_norm=max_grad_norm)
        self.table = self.p[TABLE_KEY]                       # logits() gathers the rows of the parameter


def fit_table_yardstick(w, table, pairs, num_user, num_item, batch_size, epochs, num_ng, seed, lr, max_grad_norm, dtype=torch.float32):
    """tests/ncf_train_util.fit_yardstick with the table trained -> (the mean training loss of every epoch, the largest move of a table entry)."""
    from pmgt_amd.fit_loop import epoch_order
    from pmgt_amd.ncf_train import ng_sample
    head = TorchTableHead(w, table, dtype, lr=lr, max_grad_norm=max_grad_norm)
    means = []
    for epoch in range(epochs):
        users, items, labels = ng_sample(pairs, num_user, num_item, num_ng, seed + epoch)
        order = epoch_order(len(users), seed, epoch)
        users, items, labels = users[order], items[order], labels[order]
        losses = [head.step(users[lo: lo + batch_size], items[lo: lo + batch_size], labels[lo: lo + batch_size])
                  for lo in range(0, len(order), batch_size)]
        means.append(float(np.mean(losses)))
    return means, float((head.table.detach() - torch.as_tensor(np.asarray(table), dtype=dtype)).abs().max())


def flat_buffer(model) -> torch.Tensor:
    """The flat parameter buffer an NcfHeadTrainer moved `model`'s head into, found through the model alone: mlp_user_embeddings.weight is
    the view at offset 0 of it, so the buffer is that parameter's storage."""
    w = model.mlp_user_embeddings.weight
    assert w.storage_offset() == 0
    return torch.empty(0, dtype=torch.float32, device=w.device).set_(w.untyped_storage(), 0, (w.untyped_storage().nbytes() // 4,))
