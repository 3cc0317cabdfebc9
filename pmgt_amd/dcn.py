"""The Deep & Cross Network of the reference's click-through experiment (pmgt/dcn/models.py, scripts/run_dcn.sh) as a torch module with
the reference's constructor, state_dict keys, shapes and initialisation, so its checkpoints load with strict=True.  forward() is the torch
restatement of dcn_head.py's formulae (the autograd yardstick of the tests); the device path is dcn_train.py."""
import math

import torch
import torch.nn as nn


class _DeepLayer(nn.Module):
    def __init__(self, in_size: int, out_size: int, dropout: float, use_layer_norm: bool, eps: float):
        super().__init__()
        self.linear = nn.Linear(in_size, out_size)
        self.dropout = nn.Dropout(dropout)
        self.layer_norm = nn.LayerNorm(out_size, eps) if use_layer_norm else nn.Identity()

    def forward(self, x):
        return torch.relu(self.layer_norm(self.dropout(self.linear(x))))


class _CrossLayer(nn.Module):
    """x^(c+1) = LN(x0 (x^(c) . weight) + x0).  `bias` is a parameter of the reference's layer that its forward never reads: it is kept
    for the state_dict, gets no gradient and is never stepped."""

    def __init__(self, size: int, dropout: float, use_layer_norm: bool, eps: float):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(size, 1))
        self.bias = nn.Parameter(torch.empty(size))
        self.dropout = nn.Dropout(dropout)
        self.layer_norm = nn.LayerNorm(size, eps) if use_layer_norm else nn.Identity()
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        bound = 1 / math.sqrt(self.weight.shape[1])          # fan_in of a [size, 1] tensor is 1
        nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x0, x):
        return self.layer_norm(self.dropout(x0 * (x @ self.weight)) + x0)


class _Layers(nn.Module):
    def __init__(self, layers):
        super().__init__()
        self.layers = nn.Sequential(*layers)


class DCN(nn.Module):
    def __init__(self, user_num: int, item_num: int, factor_num: int = 32, deep_net_num_layers: int = 3, cross_net_num_layers: int = 2,
                 emb_dropout: float = 0.0, dropout: float = 0.0, use_layer_norm: bool = False, layer_norm_eps: float = 1e-12):
        super().__init__()
        self.user_num, self.item_num, self.factor_num = int(user_num), int(item_num), int(factor_num)
        self.deep_layers, self.cross_layers = int(deep_net_num_layers), int(cross_net_num_layers)
        self.use_layer_norm, self.layer_norm_eps = bool(use_layer_norm), float(layer_norm_eps)
        emb = factor_num * 2 ** deep_net_num_layers
        self.user_embeddings = nn.Embedding(user_num, emb)
        self.item_embeddings = nn.Embedding(item_num, emb)
        self.emb_dropout = nn.Dropout(emb_dropout)
        self.dropout_p = float(dropout)
        sizes = [2 * emb >> i for i in range(deep_net_num_layers + 1)]
        self.deep_net = _Layers([_DeepLayer(a, b, dropout, use_layer_norm, layer_norm_eps) for a, b in zip(sizes[:-1], sizes[1:])])
        self.cross_net = _Layers([_CrossLayer(2 * emb, dropout, use_layer_norm, layer_norm_eps) for _ in range(cross_net_num_layers)])
        self.output_layer = nn.Linear(2 * emb + sizes[-1], 1)

    def forward(self, inputs):
        users, items = inputs
        x0 = self.emb_dropout(torch.cat([self.user_embeddings(users), self.item_embeddings(items)], dim=-1))
        x = x0
        for layer in self.cross_net.layers:
            x = layer(x0, x)
        h = self.deep_net.layers(x0)
        return self.output_layer(torch.cat([x, h], dim=-1)).view(-1)
