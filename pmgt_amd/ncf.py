"""The stand-alone Neural Collaborative Filtering model of the reference's NCF experiment (pmgt/ncf/models.py, scripts/run_ncf.sh) as a torch
module with the reference's constructor, state_dict keys, shapes and initialisation -- the same random draws in the same order -- so its
checkpoints load with strict=True.  forward() is the torch restatement of ncf_model.py's formulae (the autograd yardstick of the tests); the
device path is ncf_model_train.py.

THE REFERENCE'S QUIRKS, kept as they are:
  * all four embedding tables and the MLP stack exist whatever the kind.  Kind "MLP" never reads the GMF tables; kind "GMF" never reads
    the MLP tables and layers, and its predict_layer is [1, factor_num];
  * GMF_model / MLP_model are assigned as attributes and so become sub-modules: the state_dict of a NeuMF-pre carries GMF_model.* and
    MLP_model.* keys.  Nothing in forward reads them;
  * with MLP_model, only the Linear weights and biases of MLP_layers are copied; its LayerNorm gamma / beta are not;
  * with both, predict_layer = cat(alpha GMF.predict_layer.weight, (1 - alpha) MLP.predict_layer.weight), the biases mixed the same way;
  * emb_dropout acts on the GMF product and on the concatenated [user ; item] MLP input.
MLP_layers is a Sequential of Linear, Dropout, [LayerNorm,] ReLU per layer: the Linear of layer i is MLP_layers.{3i} without LayerNorm and
MLP_layers.{4i} with it, the LayerNorm MLP_layers.{4i+2}."""
import torch
import torch.nn as nn

KINDS = ("MLP", "GMF", "NeuMF-end", "NeuMF-pre")


class NCF(nn.Module):
    def __init__(self, user_num: int, item_num: int, factor_num: int = 32, num_layers: int = 3, emb_dropout: float = 0.0, dropout: float = 0.0,
                 use_layer_norm: bool = False, layer_norm_eps: float = 1e-12, model: str = "NeuMF-end", GMF_model=None, MLP_model=None,
                 alpha: float = 0.5):
        super().__init__()
        if model not in KINDS:
            raise ValueError(f"NCF: model kind {model!r}, expected one of {KINDS}")
        self.user_num, self.item_num, self.factor_num, self.num_layers = int(user_num), int(item_num), int(factor_num), int(num_layers)
        self.use_layer_norm, self.layer_norm_eps = bool(use_layer_norm), float(layer_norm_eps)
        self.dropout, self.model, self.alpha = dropout, model, alpha
        self.GMF_model, self.MLP_model = GMF_model, MLP_model
        d = factor_num << (num_layers - 1)
        self.embed_user_GMF = nn.Embedding(user_num, factor_num)
        self.embed_item_GMF = nn.Embedding(item_num, factor_num)
        self.embed_user_MLP = nn.Embedding(user_num, d)
        self.embed_item_MLP = nn.Embedding(item_num, d)
        self.emb_dropout = nn.Dropout(p=emb_dropout)
        layers = []
        for i in range(num_layers):
            out = d >> i
            layers += [nn.Linear(2 * out, out), nn.Dropout(p=dropout)]
            if use_layer_norm:
                layers.append(nn.LayerNorm(out, eps=layer_norm_eps))
            layers.append(nn.ReLU())
        self.MLP_layers = nn.Sequential(*layers)
        self.predict_layer = nn.Linear(factor_num if model in ("MLP", "GMF") else 2 * factor_num, 1)
        self._init_weight()

    def _init_weight(self) -> None:
        for m in self.modules():                             # (the sub-modules GMF_model / MLP_model included: their Linear biases are zeroed too)
            if isinstance(m, nn.Linear) and m.bias is not None:
                m.bias.data.zero_()
        gmf, mlp = self.GMF_model, self.MLP_model
        with torch.no_grad():
            if gmf is not None:
                self.embed_user_GMF.weight.copy_(gmf.embed_user_GMF.weight)
                self.embed_item_GMF.weight.copy_(gmf.embed_item_GMF.weight)
            else:
                nn.init.normal_(self.embed_user_GMF.weight, std=0.01)
                nn.init.normal_(self.embed_item_GMF.weight, std=0.01)
            if mlp is not None:
                self.embed_user_MLP.weight.copy_(mlp.embed_user_MLP.weight)
                self.embed_item_MLP.weight.copy_(mlp.embed_item_MLP.weight)
                for m1, m2 in zip(self.MLP_layers, mlp.MLP_layers):
                    if isinstance(m1, nn.Linear) and isinstance(m2, nn.Linear):
                        m1.weight.copy_(m2.weight)
                        m1.bias.copy_(m2.bias)
            else:
                nn.init.normal_(self.embed_user_MLP.weight, std=0.01)
                nn.init.normal_(self.embed_item_MLP.weight, std=0.01)
                for m in self.MLP_layers:
                    if isinstance(m, nn.Linear):
                        nn.init.xavier_uniform_(m.weight)
            if gmf is not None and mlp is not None:
                self.predict_layer.weight.copy_(torch.cat([self.alpha * gmf.predict_layer.weight, (1 - self.alpha) * mlp.predict_layer.weight], dim=1))
                self.predict_layer.bias.copy_(self.alpha * gmf.predict_layer.bias + (1 - self.alpha) * mlp.predict_layer.bias)
            else:
                nn.init.kaiming_uniform_(self.predict_layer.weight, a=1, nonlinearity="sigmoid")

    def head(self, user, item_ids, item_embeds):
        """The model on ready item embeddings, PMGT_NCF.head's contract: user [n] and item_ids [n] (for the GMF branch) on the parameters'
        device, item_embeds [n, d] in place of embed_item_MLP(item_ids); kind "GMF" ignores it.  evaluation.rank_users calls this on rows
        gathered from a table of the whole catalogue."""
        parts = []
        if self.model != "MLP":
            parts.append(self.emb_dropout(self.embed_user_GMF(user) * self.embed_item_GMF(item_ids)))
        if self.model != "GMF":
            parts.append(self.MLP_layers(self.emb_dropout(torch.cat((self.embed_user_MLP(user), item_embeds), -1))))
        return self.predict_layer(parts[0] if len(parts) == 1 else torch.cat(parts, -1)).view(-1)

    def forward(self, inputs):
        user, item = inputs
        return self.head(user, item, None if self.model == "GMF" else self.embed_item_MLP(item))
