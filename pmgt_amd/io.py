"""On-disk formats either side of the hot path: the dataset directory the reference's
trainer reads (`node_encoder`, `graph.gpickle`, `visual_init_emb.npy`, `textual_init_emb.npy`;
pmgt/pmgt/trainer.py:30-71,108-135), Lightning-style checkpoints with the reference's key names
(`net.` prefix, pmgt/base_trainer.py:99-110,291-298), the exported `[N, d]` embedding file and its
node -> item remap (pmgt/pmgt/utils.py:15-40).  Host-side glue only: nothing here is on the device path."""
from __future__ import annotations

import os
import pickle
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from .graph import CSRGraph


def _load_encoder(path: str):
    import joblib
    return joblib.load(path)


def relabel_like_reference(graph, classes) -> "object":
    """mapping = {label: i + 2}; nx.relabel_nodes(graph, mapping) (pmgt/pmgt/trainer.py:37-41).  The copy that
    networkx builds re-inserts edges in `graph.edges()` order, which CHANGES the neighbour order of every node —
    and the neighbour order is the `a` array of the sampler's np.random.choice — so the relabel is done by
    networkx itself rather than restated."""
    import networkx as nx
    mapping = {label: i + 2 for i, label in enumerate(classes)}
    return nx.relabel_nodes(graph, mapping)


def load_graph(data_dir: str) -> Tuple[CSRGraph, np.ndarray]:
    """`node_encoder` (joblib'd sklearn LabelEncoder) + `graph.gpickle` (pickled nx.Graph, float `weight` per
    edge) -> CSR with ids 2..N+1 in the reference's adjacency order, and the encoder's classes."""
    enc = _load_encoder(os.path.join(data_dir, "node_encoder"))
    with open(os.path.join(data_dir, "graph.gpickle"), "rb") as f:        # nx.read_gpickle == pickle.load
        g = pickle.load(f)
    classes = np.asarray(enc.classes_)
    if g.number_of_nodes() != len(classes):
        raise ValueError(f"graph has {g.number_of_nodes()} nodes but node_encoder has {len(classes)} classes")
    csr = CSRGraph.from_networkx(relabel_like_reference(g, classes))
    csr.validate()
    return csr, classes


def load_features(data_dir: str, n_nodes: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """`visual_init_emb.npy`, `textual_init_emb.npy`: [N+2, F_m] with rows 0 (<pad>) and 1 (<mask>)
    (notebooks/PMGT.ipynb cell 30; loaded at pmgt/pmgt/trainer.py:114-116)."""
    vis = np.load(os.path.join(data_dir, "visual_init_emb.npy"))
    txt = np.load(os.path.join(data_dir, "textual_init_emb.npy"))
    if vis.shape[0] != txt.shape[0] or (n_nodes is not None and vis.shape[0] != n_nodes + 2):
        raise ValueError(f"feature tables have {vis.shape[0]} / {txt.shape[0]} rows, expected {None if n_nodes is None else n_nodes + 2}")
    return vis, txt


def save_dataset_dir(data_dir: str, graph, classes, visual: np.ndarray, textual: np.ndarray):
    """Writer for the same layout (used by the tests and to stage synthetic datasets)."""
    import joblib
    from sklearn.preprocessing import LabelEncoder
    os.makedirs(data_dir, exist_ok=True)
    enc = LabelEncoder()
    enc.classes_ = np.asarray(classes)
    joblib.dump(enc, os.path.join(data_dir, "node_encoder"))
    with open(os.path.join(data_dir, "graph.gpickle"), "wb") as f:
        pickle.dump(graph, f, pickle.HIGHEST_PROTOCOL)
    np.save(os.path.join(data_dir, "visual_init_emb.npy"), visual)
    np.save(os.path.join(data_dir, "textual_init_emb.npy"), textual)


# ---- checkpoints ---------------------------------------------------------------------------------------------
def to_reference_state_dict(model, prefix: str = "net.") -> Dict[str, torch.Tensor]:
    """state_dict of a `pmgt_amd.models.PMGT` under the keys a Lightning checkpoint of the reference holds
    (`net.bert.…`, `net.nfr_loss.projections.…`, `net.feat_embeddings.{0,1}.weight`, position/role id buffers)."""
    return {prefix + k: v.detach().to("cpu", copy=True) for k, v in model.state_dict().items()}


def save_checkpoint(model, path: str, prefix: str = "net.", **extra):
    torch.save({"state_dict": to_reference_state_dict(model, prefix), **extra}, path)


class _Opaque(dict):
    """Stand-in for any class a checkpoint pickles that is not plain data (Lightning's AttributeDict / AttrDict
    hyper-parameters, callback state objects, ...): keeps items and attributes, runs none of the original code."""

    def __init__(self, *args, **kwargs):
        dict.__init__(self)

    def __setstate__(self, state):
        if isinstance(state, dict):
            self.__dict__.update(state)
        elif isinstance(state, tuple) and len(state) == 2 and isinstance(state[1], dict):
            self.__dict__.update(state[1])

    def __reduce__(self):                       # never re-pickled as the original class
        return (dict, (dict(self),))


class _TolerantUnpickler(pickle.Unpickler):
    """Restricted unpickler for checkpoints written by the reference's Lightning run (pmgt/base_trainer.py:291-298:
    ModelCheckpoint -> {"state_dict", "hyper_parameters", "callbacks", "optimizer_states", ...}).  torch's
    weights_only loader refuses such a file because `hyper_parameters` is an AttributeDict / AttrDict; this one resolves
    ONLY tensor / container reconstruction globals and maps every other global to an inert placeholder, so a real checkpoint
    loads without pytorch_lightning installed and without executing code from the file."""

    _ALLOWED = {
        ("collections", "OrderedDict"), ("collections", "defaultdict"), ("copyreg", "_reconstructor"), ("builtins", "dict"),
        ("builtins", "list"), ("builtins", "tuple"), ("builtins", "set"), ("builtins", "frozenset"), ("builtins", "object"),
        ("builtins", "int"), ("builtins", "float"), ("builtins", "bool"), ("builtins", "str"), ("builtins", "bytes"),
        ("builtins", "complex"), ("builtins", "slice"), ("builtins", "range"),
        ("torch._utils", "_rebuild_tensor_v2"), ("torch._utils", "_rebuild_tensor"), ("torch._utils", "_rebuild_parameter"),
        ("torch._utils", "_rebuild_parameter_with_state"), ("torch", "Size"), ("torch", "device"), ("torch", "dtype"),
        ("torch._tensor", "_rebuild_from_type_v2"), ("torch", "Tensor"), ("torch.nn.parameter", "Parameter"),
        ("numpy", "dtype"), ("numpy", "ndarray"), ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"),
        ("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
    }

    def find_class(self, module, name):
        if (module, name) in self._ALLOWED:
            return super().find_class(module, name)
        if module == "torch" and (name.endswith("Storage") or isinstance(getattr(torch, name, None), torch.dtype)):
            return getattr(torch, name)
        return _Opaque


class _TolerantPickle:            # the `pickle_module` interface torch.load asks for
    Unpickler = _TolerantUnpickler
    __name__ = "pmgt_amd.io._TolerantPickle"

    @staticmethod
    def load(f, **kw):
        return _TolerantUnpickler(f, **kw).load()


def read_checkpoint(path) -> dict:
    """A checkpoint file as plain data.  First torch's weights_only loader (enough for checkpoints written by
    `save_checkpoint`); a file it refuses because it pickles non-tensor classes -- a real Lightning checkpoint of the
    reference -- goes through the restricted tolerant unpickler above (still no code from the file is executed)."""
    try:
        return torch.load(path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError:
        return torch.load(path, map_location="cpu", weights_only=False, pickle_module=_TolerantPickle)


def load_checkpoint(model, path_or_dict, prefix: str = "net.", strict: bool = True):
    """Accepts a Lightning checkpoint ({"state_dict": {"net.…": …}, "hyper_parameters": …, "callbacks": …,
    "optimizer_states": …}), a bare state_dict with or without the prefix, or a path to either; copies the weights into the
    engine's flat buffer and re-uploads the tables."""
    ck = read_checkpoint(path_or_dict) if isinstance(path_or_dict, (str, os.PathLike)) else path_or_dict
    sd = ck.get("state_dict", ck)
    if any(k.startswith(prefix) for k in sd):
        sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    return model.load_state_dict(sd, strict=strict)


# ---- full training checkpoints (weights + optimizer + counters): a superset of save_checkpoint's file, under a Lightning checkpoint's keys --------
FORMAT_VERSION = 1
NO_DECAY = ("bias", "LayerNorm.weight")              # pmgt/base_trainer.py:38
_EMB_ORDER = ("position_embeddings", "role_embeddings", "feat_linear", "attention", "LayerNorm")
_LAYER_ORDER = ("attention.self.query", "attention.self.key", "attention.self.value", "attention.self.ctx_attention",
                "attention.output.dense", "attention.output.LayerNorm", "intermediate.dense", "output.dense", "output.LayerNorm")


def _reference_position(name: str):
    """Sort key of a trainable parameter in the reference's `named_parameters()` order (pmgt/pmgt/models.py:31-47 registers bert, then
    nfr_loss, then the frozen feat_embeddings; inside a module weight comes before bias).  The engine's flat layout groups a layer's
    Q|K|V|C weights and the partial-sum neighbours of the LayerNorms, so its entry order is NOT this order."""
    stem, leaf = name.rsplit(".", 1)
    wb = ("weight", "bias").index(leaf)
    if stem.startswith("bert.embeddings."):
        parts = stem[len("bert.embeddings."):].split(".")
        return (0, 0, _EMB_ORDER.index(parts[0]), int(parts[1]) if parts[0] == "feat_linear" else 0, wb)
    if stem.startswith("bert.encoder.layer."):
        layer, rest = stem[len("bert.encoder.layer."):].split(".", 1)
        return (1, int(layer), _LAYER_ORDER.index(rest), 0, wb)
    if stem.startswith("nfr_loss.projections."):
        return (2, 0, 0, int(stem[len("nfr_loss.projections."):]), wb)
    raise ValueError(f"{name!r} is not a trainable parameter of the reference's PMGT")


def optimizer_param_groups(names) -> Tuple[list, list]:
    """The two groups `get_optimizer` builds (pmgt/base_trainer.py:35-59) over the TRAINABLE parameter names: ([decayed], [not decayed:
    any of "bias", "LayerNorm.weight" in the name]), each in named_parameters() order.  torch.optim.Optimizer.state_dict() numbers the
    parameters by their running index across the groups: group 0 takes 0 .. len - 1, group 1 continues.  The frozen feat_embeddings are
    left out here; a file of the reference lists them at the tail of group 0 (get_optimizer does not filter on requires_grad) with no
    state: optimizer_state_to_flat steps over them."""
    ordered = sorted(names, key=_reference_position)
    nd = lambda n: any(k in n for k in NO_DECAY)
    return [n for n in ordered if not nd(n)], [n for n in ordered if nd(n)]


def flat_to_optimizer_state(entries, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, step: int, lr: float, weight_decay: float,
                            betas=(0.9, 0.999), eps: float = 1e-8, current_lr: Optional[float] = None) -> dict:
    """Flat CPU moments (the engine's layout: `entries` = [{name, offset, numel, shape}]) -> torch.optim.Optimizer.state_dict() form of the
    reference's DenseSparseAdamW: per parameter {"step", "exp_avg", "exp_avg_sq"} (pmgt/optimizers.py:187-201).  current_lr: the rate a
    LambdaLR has written into the groups (then `lr` is their "initial_lr")."""
    by = {e["name"]: e for e in entries}
    decay, no_decay = optimizer_param_groups(by)
    state = {}
    for i, n in enumerate(decay + no_decay):
        e = by[n]
        sl = slice(e["offset"], e["offset"] + e["numel"])
        state[i] = {"step": int(step), "exp_avg": exp_avg[sl].reshape(tuple(e["shape"])).clone(),
                    "exp_avg_sq": exp_avg_sq[sl].reshape(tuple(e["shape"])).clone()}
    groups = []
    for lo, members, wd in ((0, decay, float(weight_decay)), (len(decay), no_decay, 0.0)):
        g = {"params": list(range(lo, lo + len(members))), "weight_decay": wd, "lr": float(lr if current_lr is None else current_lr),
             "betas": tuple(float(b) for b in betas), "eps": float(eps)}
        if current_lr is not None:
            g["initial_lr"] = float(lr)
        groups.append(g)
    return {"state": state, "param_groups": groups}


def optimizer_state_to_flat(entries, opt_state: dict, n_params: int, n_frozen: int = 0):
    """Inverse of flat_to_optimizer_state: (exp_avg, exp_avg_sq, step) with the elements no entry covers (alignment gaps, never
    touched by a step) zero.  n_frozen: how many frozen parameters a file of the reference may list behind the decayed ones in group 0.
    A parameter without state (the reference creates it at the first step that sees a gradient) keeps zero moments."""
    by = {e["name"]: e for e in entries}
    decay, no_decay = optimizer_param_groups(by)
    groups = opt_state["param_groups"]
    if len(groups) != 2:
        raise ValueError(f"optimizer state has {len(groups)} parameter groups, the reference's get_optimizer builds 2")
    ids0, ids1 = list(groups[0]["params"]), list(groups[1]["params"])
    if len(ids0) == len(decay) + n_frozen and n_frozen:
        ids0 = ids0[:len(decay)]
    if len(ids0) != len(decay) or len(ids1) != len(no_decay):
        raise ValueError(f"optimizer state lists {len(groups[0]['params'])} + {len(ids1)} parameters in its groups, this model has "
                         f"{len(decay)} decayed (+ {n_frozen} frozen tables in a file of the reference) + {len(no_decay)} undecayed")
    m, v = torch.zeros(n_params, dtype=torch.float32), torch.zeros(n_params, dtype=torch.float32)
    step = 0
    for idx, n in zip(ids0 + ids1, decay + no_decay):
        st = opt_state["state"].get(idx)
        if not st:
            continue
        e = by[n]
        for buf, key in ((m, "exp_avg"), (v, "exp_avg_sq")):
            t = torch.as_tensor(st[key]).to(torch.float32)
            if t.numel() != e["numel"]:
                raise ValueError(f"optimizer state {idx} ({n}): {key} has {t.numel()} elements, the parameter has {e['numel']}")
            buf[e["offset"]: e["offset"] + e["numel"]] = t.reshape(-1)
        step = max(step, int(st["step"]))
    return m, v, step


def _callback(callbacks: dict, prefix: str) -> Optional[dict]:
    """Lightning keys a callback's state by its class name followed by its arguments (pmgt/base_trainer.py:105-108 looks one up the same way)."""
    for k, v in (callbacks or {}).items():
        if isinstance(k, str) and k.startswith(prefix):
            return v
    return None


def average_model_state(entries, block: dict, prefix: str = "net.") -> dict:
    """The callback state the reference's on_save_checkpoint returns (pmgt/callbacks.py:284-295): {"average_model": swa_state}, swa_state =
    {parameter name: tensor, ..., "models_num": n} (pmgt/utils/train.py:39-50).  The tensors are VIEWS of the block's flat average, so a
    file stores the average once.  An "ema" average carries "n_upd" in place of "models_num"."""
    flat = block["average"]
    count = "models_num" if block["mode"] == "swa" else "n_upd"
    model = {prefix + e["name"]: flat[e["offset"]: e["offset"] + e["numel"]].view(tuple(e["shape"])) for e in entries}
    model[count] = int(block[count])
    return {"average_model": model}


def training_checkpoint(state_dict: Dict[str, torch.Tensor], entries, trainer_sd: dict, epoch: int = 0, callbacks: Optional[dict] = None,
                        fit: Optional[dict] = None, swa_key: str = "StochasticWeightAveraging", prefix: str = "net.", **extra) -> dict:
    """The checkpoint as plain data (pure: CPU tensors in, a dict out).  `state_dict`: the weights under their `net.` keys, what
    save_checkpoint writes; `trainer_sd`: Trainer.state_dict().  Keys of a Lightning checkpoint of the reference, plus the block
    "pmgt_amd" for what that format has no place for.  A trainer that averages its weights adds its `weight_average` block (settings,
    count, flat average) there and, under `swa_key` among the callbacks, the reference's `average_model` state."""
    est, hp = trainer_sd["engine"], trainer_sd["hyper_parameters"]
    steps = int(est["opt_step"])
    current = None
    if hp["schedule"] is not None:
        from .schedule import lr_lambda
        kind, W, T = hp["schedule"]
        current = hp["lr"] * lr_lambda(kind, W, T, hp["lr"])(steps)
    opt = flat_to_optimizer_state(entries, est["exp_avg"], est["exp_avg_sq"], steps, hp["lr"], hp["weight_decay"], hp["betas"], hp["eps"], current)
    sched = []
    if hp["schedule"] is not None:
        sched = [{"base_lrs": [hp["lr"]] * 2, "last_epoch": steps, "_step_count": steps + 1, "verbose": False,
                  "_get_lr_called_within_step": False, "_last_lr": [current] * 2, "lr_lambdas": [None, None]}]
    private = {"format_version": FORMAT_VERSION, "rng_state": dict(est["rng_state"]), "opt_steps": int(trainer_sd["opt_steps"]),
               "options": list(est["options"]), "pipeline_step": int(trainer_sd["pipeline_step"]), "dtype": est["dtype"],
               "n_params": int(est["n_params"]), "config": dict(est["config"]), "hyper_parameters": dict(hp),
               "accumulate_grad_batches": int(trainer_sd["accumulate_grad_batches"]), "fit": fit,
               "step_counters": dict(est.get("step_counters") or {"attempts": 0, "skipped": 0, "skipped_in_a_row": 0})}
    callbacks = dict(callbacks or {})
    block = trainer_sd.get("weight_average")
    if block is not None:      # absent without averaging: the file's structure is what it always was
        private["weight_average"] = dict(block)
        callbacks[swa_key] = average_model_state(entries, block, prefix)
    return {"state_dict": state_dict, "optimizer_states": [opt], "lr_schedulers": sched, "global_step": steps, "epoch": int(epoch),
            "callbacks": callbacks, "pmgt_amd": private, **extra}


def training_state_from_checkpoint(ck: dict, entries, n_params: int, n_frozen: int = 0, prefix: str = "net.") -> dict:
    """A checkpoint (ours, or a Lightning file of the reference as read_checkpoint returns it) -> Trainer.state_dict() layout.  Pure.
    Without the "pmgt_amd" block the weights, the moments and the step count are still there; what the reference does not record comes
    back as None (rng_state, options, dtype) or absent (clip value, schedule, accumulation factor), and Trainer.load_state_dict keeps its
    own for those."""
    sd = ck["state_dict"]
    if any(k.startswith(prefix) for k in sd):
        sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    params = torch.zeros(n_params, dtype=torch.float32)
    for e in entries:
        if e["name"] not in sd:
            raise ValueError(f"checkpoint has no weights for {e['name']!r}")
        t = torch.as_tensor(sd[e["name"]]).to(torch.float32)
        if t.numel() != e["numel"]:
            raise ValueError(f"checkpoint: {e['name']} has shape {tuple(t.shape)}, this model's has {tuple(e['shape'])}")
        params[e["offset"]: e["offset"] + e["numel"]] = t.reshape(-1)
    m, v, step = optimizer_state_to_flat(entries, ck["optimizer_states"][0], n_params, n_frozen)
    pv = ck.get("pmgt_amd")
    if pv is not None:
        if int(pv.get("format_version", 0)) > FORMAT_VERSION:
            raise ValueError(f"checkpoint format version {pv['format_version']} is newer than this library's ({FORMAT_VERSION})")
        eng = dict(n_params=int(pv["n_params"]), dtype=pv["dtype"], config=dict(pv["config"]), rng_state=dict(pv["rng_state"]), options=list(pv["options"]),
                   step_counters=dict(pv.get("step_counters") or {}))       # absent before the guarded step existed: zeros
        out = {"opt_steps": int(pv["opt_steps"]), "pipeline_step": int(pv["pipeline_step"]), "hyper_parameters": dict(pv["hyper_parameters"]),
               "accumulate_grad_batches": int(pv["accumulate_grad_batches"])}
        if pv.get("weight_average") is not None:
            out["weight_average"] = dict(pv["weight_average"])
    else:
        g0 = ck["optimizer_states"][0]["param_groups"][0]
        eng = dict(n_params=n_params, dtype=None, config=None, rng_state=None, options=None)
        hp = {"lr": float(g0.get("initial_lr", g0["lr"])), "weight_decay": float(g0["weight_decay"])}
        if "betas" in g0:
            hp["betas"] = tuple(float(b) for b in g0["betas"])
        if "eps" in g0:
            hp["eps"] = float(g0["eps"])
        out = {"opt_steps": step, "hyper_parameters": hp}
    eng.update(params=params, exp_avg=m, exp_avg_sq=v, opt_step=step)
    out["engine"] = eng
    return out


def atomic_save(obj, path) -> None:
    """torch.save to a temporary name in the same directory, then one rename: a kill at any point leaves the previous file whole."""
    path = os.fspath(path)
    tmp = f"{path}.tmp.{os.getpid()}"
    try:
        torch.save(obj, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)


def _engine_of(model_or_engine):
    return getattr(model_or_engine, "engine", model_or_engine)


def save_training_checkpoint(model_or_engine, trainer, path, prefix: str = "net.", **extra):
    """save_checkpoint's file plus everything a resume needs (training_checkpoint above).  `model_or_engine`: a PMGT module (its
    state_dict, frozen tables and id buffers included, exactly what save_checkpoint writes) or a bare Engine (its trainable entries: the
    frozen tables are the caller's input to set_tables).  Only at an optimizer-step boundary (Trainer.state_dict).  Under data
    parallelism only rank 0 writes -- the replicas are identical -- and the returned dict is None elsewhere."""
    from .parallel import world
    if trainer.world_size > 1 and world()[0] != 0:
        if trainer._micro != 0:
            trainer.state_dict()                   # raises the same error on every rank
        return None
    eng = _engine_of(model_or_engine)
    if eng is not trainer.engine:
        raise ValueError("save_training_checkpoint: the trainer drives another engine than the one passed")
    tsd = trainer.state_dict()
    if model_or_engine is eng:
        sd = {prefix + e["name"]: tsd["engine"]["params"][e["offset"]: e["offset"] + e["numel"]].reshape(tuple(e["shape"])).clone() for e in eng.entries}
    else:
        sd = to_reference_state_dict(model_or_engine, prefix)
    ck = training_checkpoint(sd, eng.entries, tsd, prefix=prefix, **extra)
    atomic_save(ck, path)
    return ck


def load_training_checkpoint(model_or_engine, trainer, path_or_dict, strict: bool = True, prefix: str = "net.") -> dict:
    """Restores weights, moments, counters, RNG state and path options from a file of save_training_checkpoint -- or the weights,
    moments and step count from a Lightning checkpoint of the reference -- through Trainer.load_state_dict (in place; see there for
    `strict`).  Every rank loads.  Returns the checkpoint as read (callbacks, epoch, the "pmgt_amd" block)."""
    ck = read_checkpoint(path_or_dict) if isinstance(path_or_dict, (str, os.PathLike)) else path_or_dict
    eng = _engine_of(model_or_engine)
    if eng is not trainer.engine:
        raise ValueError("load_training_checkpoint: the trainer drives another engine than the one passed")
    trainer.load_state_dict(training_state_from_checkpoint(ck, eng.entries, eng.n_params, eng.n_feats, prefix), strict=strict)
    if model_or_engine is not eng and hasattr(model_or_engine, "set_features"):
        tabs = [ck["state_dict"].get(f"{prefix}feat_embeddings.{i}.weight") for i in range(eng.n_feats)]
        if all(t is not None for t in tabs):
            model_or_engine.set_features(tabs)
    return ck


# ---- exported embeddings ------------------------------------------------------------------------------------------
def save_embeddings(path: str, emb: np.ndarray):
    """[N, d] fp32 in node-id order (pmgt/base_trainer.py:403-405: np.save(args.inference_result_path, predictions))."""
    np.save(path, np.ascontiguousarray(emb, dtype=np.float32))


def load_node_init_emb(item_encoder_path: str, node_encoder_path: str, node_init_emb_path: str, normalize: bool = True) -> np.ndarray:
    """pmgt/pmgt/utils.py:15-40: rows of the exported node embeddings re-indexed by the downstream item encoder;
    items absent from the graph get `np.random.normal` rows (global numpy stream, as in the reference); rows are
    L2-normalised (sklearn `normalize`: zero rows stay zero)."""
    item_encoder = _load_encoder(item_encoder_path)
    node_encoder = _load_encoder(node_encoder_path)
    node_init_emb = np.load(node_init_emb_path)
    item2idx = {item: i for i, item in enumerate(node_encoder.classes_)}
    out = np.empty((len(item_encoder.classes_), node_init_emb.shape[1]), dtype=node_init_emb.dtype)
    for i, item in enumerate(item_encoder.classes_):
        if item in item2idx:
            out[i] = node_init_emb[item2idx[item]]
        else:
            out[i] = np.random.normal(size=node_init_emb.shape[1])
    if normalize:
        nrm = np.sqrt((out.astype(np.float64) ** 2).sum(axis=1, keepdims=True))
        nrm[nrm == 0.0] = 1.0
        out = (out / nrm).astype(out.dtype)
    return out
