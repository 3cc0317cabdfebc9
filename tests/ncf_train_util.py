"""Shared by the NcfHeadTrainer / fit_ncf tests: a PMGT_NCF with a seeded head, and the parent's only way to train that head -- the
head's formula in torch (pmgt_amd/pmgt_ncf.py:83-95) on gathered rows, autograd, clip_grad_norm_, torch.optim.AdamW -- as the yardstick."""
import numpy as np
import torch

from tests.test_recommend_cpu import random_head


def make_model(factor, num_layers, kind, user_num, item_num, seed):
    """(PMGT_NCF on the GPU with random_head's weights as its head, those weights as numpy, a seeded item table [item_num, d] numpy)."""
    from oracle import pmgt_oracle as po
    from pmgt_amd.configuration_pmgt import PMGTConfig
    from pmgt_amd.pmgt_ncf import PMGT_NCF
    d = factor << (num_layers - 1)
    cfg = po.default_cfg(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, hidden_size=d, num_attention_heads=4, num_hidden_layers=2,
                         intermediate_size=d, beta=0.5)
    model = PMGT_NCF(user_num=user_num, item_num=item_num, factor_num=factor, num_layers=num_layers, model=kind, config=PMGTConfig(**cfg),
                     dtype="fp32")
    w, table = random_head(factor, num_layers, kind, user_num, item_num, seed)
    sd = model.state_dict()
    with torch.no_grad():
        for k, v in w.items():
            sd[k].copy_(torch.from_numpy(v))
    return model, w, table


class TorchHead:
    """The head over a frozen table on the CPU in `dtype`: parameters keyed like the state_dict, AdamW with the trainer's decay mask."""

    def __init__(self, w, table, dtype, lr, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None):
        self.p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in w.items()}      # (copies: `w` stays as it is)
        self.table = torch.tensor(np.asarray(table), dtype=dtype)
        self.num_layers = sum(1 for k in w if k.startswith("mlp_layers.") and k.endswith(".weight"))
        self.neumf = "gmf_user_embeddings.weight" in w
        self.max_grad_norm = max_grad_norm
        self.opt = torch.optim.AdamW([{"params": [v for k, v in self.p.items() if not k.endswith(".bias")], "weight_decay": weight_decay},
                                      {"params": [v for k, v in self.p.items() if k.endswith(".bias")], "weight_decay": 0.0}],
                                     lr=lr, betas=betas, eps=eps)

    def logits(self, users, items):
        p = self.p
        u, it = torch.as_tensor(users), torch.as_tensor(items)
        x = torch.cat([p["mlp_user_embeddings.weight"][u], self.table[it]], dim=-1)
        for i in range(self.num_layers):
            x = torch.relu(x @ p[f"mlp_layers.{i}.linear.weight"].T + p[f"mlp_layers.{i}.linear.bias"])
        if self.neumf:
            x = torch.cat([p["gmf_user_embeddings.weight"][u] * p["gmf_item_embeddings.weight"][it], x], dim=-1)
        return (x @ p["predict_layer.weight"].T + p["predict_layer.bias"]).view(-1)

    def step(self, users, items, labels) -> float:
        self.opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(self.logits(users, items), torch.as_tensor(labels).to(self.table.dtype))
        loss.backward()
        if self.max_grad_norm:
            torch.nn.utils.clip_grad_norm_(list(self.p.values()), self.max_grad_norm)
        self.opt.step()
        return float(loss.item())


def fit_yardstick(w, table, pairs, num_user, num_item, batch_size, epochs, num_ng, seed, lr, max_grad_norm, dtype=torch.float32):
    """fit_ncf's training loop with TorchHead in place of the device step -> the mean training loss of every epoch."""
    from pmgt_amd.fit_loop import epoch_order
    from pmgt_amd.ncf_train import ng_sample
    head = TorchHead(w, table, dtype, lr=lr, max_grad_norm=max_grad_norm)
    means = []
    for epoch in range(epochs):
        users, items, labels = ng_sample(pairs, num_user, num_item, num_ng, seed + epoch)
        order = epoch_order(len(users), seed, epoch)
        users, items, labels = users[order], items[order], labels[order]
        losses = [head.step(users[lo: lo + batch_size], items[lo: lo + batch_size], labels[lo: lo + batch_size])
                  for lo in range(0, len(order), batch_size)]
        means.append(float(np.mean(losses)))
    return means
