"""The inputs and the launches of the bit-pinning test of the pair-head training kernels (test_pair_train_bits_gpu.py; the fixture is
tests/golden/pair_train_bits.json).  Every input of a case comes from ONE seeded numpy generator, in a fixed order (users, items, labels,
then the tensors in slot order), and goes straight into the C entry: the entries of ops/ncf_train.hip, ops/ncf_model_train.hip and
ops/dcn_train.hip.  Nothing is multiplied out on the host, so no BLAS version enters.  torch only holds the device memory.

A case is n pairs (161: five full tiles of 32 and one pair, six 32-pair chunks of the weight role; 1 and 300 on the smallest shape of each
entry) of users drawn from [0, 40) of USER_NUM = 64 and items from [0, 30) of ITEM_NUM = 50: runs of equal ids are certain, and the table
rows 40 .. 63 and 30 .. 49 must stay +0.0.  HASHED, in this order: loss, logits [n], the flat gradient buffer allocated TAIL = 8 floats
longer than the layout, table_grad and d_item where the entry writes them.  Every output is pre-filled with SENTINEL, so an unwritten element
or a store past the end changes the hash; the tail must still hold it.  The workspace is not hashed.

run_case(name) -> (sha256 of the input bytes, sha256 of the output bytes).  Run as a script, it writes the fixture:
    python tests/pair_train_bits_util.py OUT.json
"""
import ctypes as C
import hashlib
import json
import sys
import zlib

import numpy as np

N, USER_NUM, ITEM_NUM, USER_IDS, ITEM_IDS, TAIL = 161, 64, 50, 40, 30, 8
SENTINEL = np.float32(-12345.0)
EPS = 1e-5
RNG_STATE = (1234, 7)                                # the device {seed, step} pair
P_EMB, P_LAYER, P_CROSS = 0.25, (0.5, 0.0, 0.125, 0.25), (0.25, 0.0, 0.5, 0.0, 0.125, 0.25)      # one site of each list is 0 on purpose

_NT_HEADS = [(8, 1, "MLP"), (8, 2, "NeuMF-end"), (16, 3, "MLP"), (32, 3, "NeuMF-end"), (64, 3, "MLP"), (32, 4, "MLP")]      # (factor, layers, kind)
_NT_ENTRIES = ["grad", "table", "dropout-frozen", "dropout-table", "rows-plain", "rows-dropout"]
_NM_SHAPES = [(8, 1), (16, 3), (64, 3), (32, 4)]
_DC_HEADS = [(16, 1, 4, 1), (16, 2, 2, 0), (16, 3, 2, 1), (64, 2, 6, 1), (64, 2, 6, 0)]      # (factor, deep, cross, LN)
_DC_ENTRIES = ["forward", "grad", "dropout", "dropout-nocross"]

CASES = {}
for _f, _l, _k in _NT_HEADS:
    for _e in _NT_ENTRIES:
        CASES[f"ncf_train-{_e}-{_f}-{_l}-{_k}"] = ("ncf_train", _e, _f, _l, _k, N)
for _n in (1, 300):
    for _e in _NT_ENTRIES:
        CASES[f"ncf_train-{_e}-8-1-MLP-n{_n}"] = ("ncf_train", _e, 8, 1, "MLP", _n)
for _k in ("MLP", "NeuMF-end"):
    for _f, _l in _NM_SHAPES:
        for _t in (0, 1):
            for _d in (0, 1):
                CASES[f"ncf_model-ln-{_f}-{_l}-{_k}-items{_t}-{'drop' if _d else 'plain'}"] = ("ncf_model", _f, _l, _k, 1, _t, _d, N)
for _d in (0, 1):
    CASES[f"ncf_model-ln-64-1-GMF-items0-{'drop' if _d else 'plain'}"] = ("ncf_model", 64, 1, "GMF", 1, 0, _d, N)
CASES["ncf_model-noln-16-3-NeuMF-end-items1-drop"] = ("ncf_model", 16, 3, "NeuMF-end", 0, 1, 1, N)      # delegated to ncf_train.hip
for _n in (1, 300):
    for _d in (0, 1):
        CASES[f"ncf_model-ln-8-1-MLP-items1-{'drop' if _d else 'plain'}-n{_n}"] = ("ncf_model", 8, 1, "MLP", 1, 1, _d, _n)
for _f, _l, _c, _ln in _DC_HEADS:
    for _e in _DC_ENTRIES:
        CASES[f"dcn-{_e}-{_f}-{_l}-{_c}-{'ln' if _ln else 'plain'}"] = ("dcn", _e, _f, _l, _c, _ln, N)
for _n in (1, 300):
    for _e in _DC_ENTRIES:
        CASES[f"dcn-{_e}-16-1-4-ln-n{_n}"] = ("dcn", _e, 16, 1, 4, 1, _n)


class _Inputs:
    """Draws arrays from the case's generator in call order and remembers them for the hash."""

    def __init__(self, name: str):
        self.rng = np.random.default_rng([2025, zlib.crc32(name.encode())])
        self.arrays = []

    def keep(self, a):
        a = np.ascontiguousarray(a)
        self.arrays.append(a)
        return a

    def normal(self, shape, scale=1.0, shift=0.0):
        return self.keep((self.rng.standard_normal(shape) * scale + shift).astype(np.float32))

    def pairs(self, n):
        """users, items, labels: the first three draws of every case"""
        users = self.keep(self.rng.integers(0, USER_IDS, n).astype(np.int64))
        items = self.keep(self.rng.integers(0, ITEM_IDS, n).astype(np.int64))
        labels = self.keep((self.rng.random(n) < 0.3).astype(np.float32))
        return users, items, labels

    def sha(self) -> str:
        h = hashlib.sha256()
        for a in self.arrays:
            h.update(a.tobytes())
        return h.hexdigest()


for _name, _spec in CASES.items():                   # the ids of every case but n = 1 repeat, and leave rows of both tables untouched
    _u, _i, _ = _Inputs(_name).pairs(_spec[-1])
    assert _spec[-1] == 1 or (len(set(_u)) < len(_u) and len(set(_i)) < len(_i)), _name
    assert _u.max() < USER_IDS < USER_NUM and _i.max() < ITEM_IDS < ITEM_NUM, _name


def _ncf_slots(F, L, kind, model, ln, table):
    """(slot, shape, role) of the flat layout of pmgt_ncf_train_layout (model False) or pmgt_ncf_model_layout, in slot order; role is
    'table', 'gamma', 'bias' or the fan-in of a weight"""
    mlp, gmf = kind != "GMF", kind != "MLP"
    d, per = F << (L - 1), 4 if model else 2
    slots = [(0, (USER_NUM, d), "table")] if mlp else []
    if gmf:
        slots += [(1, (USER_NUM, F), "table"), (2, (ITEM_NUM, F), "table")]
    for l in range(L if mlp else 0):
        out = d >> l
        slots += [(3 + per * l, (out, 2 * out), 2 * out), (4 + per * l, (out,), "bias")]
        if ln:
            slots += [(5 + per * l, (out,), "gamma"), (6 + per * l, (out,), "bias")]
    wp = 2 * F if mlp and gmf else F
    slots += [(3 + per * 4, (wp,), wp), (4 + per * 4, (1,), "bias")]
    if table:
        slots.append((5 + per * 4, (ITEM_NUM, d), "table"))
    return slots


def _dcn_slots(F, L, Cn, ln):
    E = F << L
    D = 2 * E
    slots = [(0, (USER_NUM, E), "table"), (1, (ITEM_NUM, E), "table")]
    for l in range(L):
        out, inn = D >> (l + 1), D >> l
        slots += [(2 + 4 * l, (out, inn), inn), (3 + 4 * l, (out,), "bias")]
        if ln:
            slots += [(4 + 4 * l, (out,), "gamma"), (5 + 4 * l, (out,), "bias")]
    for c in range(Cn):
        slots.append((18 + 3 * c, (D,), D))
        if ln:
            slots += [(19 + 3 * c, (D,), "gamma"), (20 + 3 * c, (D,), "bias")]
    return slots + [(36, (D + 2 * F,), D + 2 * F), (37, (1,), "bias")]


def _draw_params(x: _Inputs, slots, off, count):
    """The flat parameters: every tensor drawn at its offset, the padding between tensors 0."""
    flat = np.zeros(count, dtype=np.float32)
    end = 0
    for slot, shape, role in slots:
        assert off[slot] >= end, (slot, off[slot], end)
        if role == "table":
            v = x.normal(shape)
        elif role == "gamma":
            v = x.normal(shape, 0.1, 1.0)
        elif role == "bias":
            v = x.normal(shape, 0.1)
        else:
            v = x.normal(shape, 1.0 / np.sqrt(role))
        flat[off[slot]: off[slot] + v.size] = v.reshape(-1)
        end = off[slot] + v.size
    assert end == count and sum(o >= 0 for o in off) == len(slots), (end, count)
    return flat


class _Run:
    """The device buffers of one call: uploads, sentinel-filled outputs, and the hash of what was written."""

    def __init__(self, x: _Inputs, n: int):
        import torch
        self.torch, self.x, self.n, self.held, self.hashed = torch, x, n, [], []
        self.users, self.items, self.labels = (self.up(a) for a in x.pairs(n))

    def up(self, a):
        self.held.append(self.torch.from_numpy(np.ascontiguousarray(a)).cuda())
        return self.held[-1].data_ptr()

    def out(self, *shape, hashed=True):
        t = self.torch.full(shape, float(SENTINEL), dtype=self.torch.float32, device="cuda")
        self.held.append(t)
        if hashed:
            self.hashed.append(t)
        return t

    def workspace(self, nbytes):
        assert nbytes > 0, nbytes
        self.held.append(self.torch.zeros(int(nbytes), dtype=self.torch.uint8, device="cuda"))
        return self.held[-1].data_ptr(), int(nbytes)

    def rng(self):
        self.held.append(self.torch.tensor(RNG_STATE, dtype=self.torch.int64, device="cuda"))
        return self.held[-1].data_ptr()

    def finish(self, rc, grads=None, count=0):
        from pmgt_amd import _lib
        _lib.check(rc)
        self.torch.cuda.synchronize()
        if grads is not None:
            assert (grads[count:].cpu().numpy() == SENTINEL).all(), "the tail behind the gradient buffer was written"
        h = hashlib.sha256()
        for t in self.hashed:
            h.update(t.cpu().numpy().tobytes())
        return self.x.sha(), h.hexdigest()


def _ncf_drop(r: _Run):
    from pmgt_amd import _lib
    return _lib.NcfDropoutC(r.rng(), P_EMB, (C.c_float * 4)(*P_LAYER))


def _ncf_train_case(name, entry, F, L, kind, n):
    from pmgt_amd import _lib
    lib = _lib.hip()
    x = _Inputs(name)
    r = _Run(x, n)
    k, d = _lib.NCF_KINDS.index(kind), F << (L - 1)
    off = (C.c_int64 * _lib.NCF_TRAIN_TENSORS)()
    count = lib.pmgt_ncf_train_layout(F, L, k, USER_NUM, ITEM_NUM, off)
    params = r.up(_draw_params(x, _ncf_slots(F, L, kind, False, False, False), list(off), count))
    rows = entry.startswith("rows")
    item_rows = r.up(x.normal((n, d) if rows else (ITEM_NUM, d)))      # x_item of the rows entry, else the table
    loss, logits, grads = r.out(1), r.out(n), r.out(count + TAIL)
    head = _lib.NcfTrainC(F, L, k, 0, USER_NUM, ITEM_NUM, None if rows else item_rows, params, grads.data_ptr())
    args = (C.byref(head), r.users, r.items, r.labels, n, loss.data_ptr(), logits.data_ptr())
    if entry == "grad":
        ws = r.workspace(lib.pmgt_ncf_train_workspace_bytes(F, L, k, n))
        rc = lib.pmgt_ncf_train_grad(*args, *ws, _lib.stream())
    elif entry == "table":
        ws = r.workspace(lib.pmgt_ncf_train_table_workspace_bytes(F, L, k, n))
        rc = lib.pmgt_ncf_train_grad_table(*args, r.out(ITEM_NUM, d).data_ptr(), *ws, _lib.stream())
    elif entry == "dropout-frozen":
        ws = r.workspace(lib.pmgt_ncf_train_workspace_bytes(F, L, k, n))
        drop = _ncf_drop(r)
        rc = lib.pmgt_ncf_train_grad_dropout(*args, None, C.byref(drop), *ws, _lib.stream())
    elif entry == "dropout-table":
        ws = r.workspace(lib.pmgt_ncf_train_table_workspace_bytes(F, L, k, n))
        drop = _ncf_drop(r)
        rc = lib.pmgt_ncf_train_grad_dropout(*args, r.out(ITEM_NUM, d).data_ptr(), C.byref(drop), *ws, _lib.stream())
    else:
        ws = r.workspace(lib.pmgt_ncf_train_rows_workspace_bytes(F, L, k, n))
        drop = _ncf_drop(r) if entry == "rows-dropout" else None
        rc = lib.pmgt_ncf_train_grad_rows(*args, item_rows, r.out(n, d).data_ptr(), C.byref(drop) if drop else None, *ws, _lib.stream())
    return r.finish(rc, grads, count)


def _ncf_model_case(name, F, L, kind, ln, train_items, dropped, n):
    from pmgt_amd import _lib
    lib = _lib.hip()
    x = _Inputs(name)
    r = _Run(x, n)
    k, d, mlp = _lib.NCF_MODEL_KINDS.index(kind), F << (L - 1), kind != "GMF"
    off = (C.c_int64 * _lib.NCF_MODEL_TENSORS)()
    count = lib.pmgt_ncf_model_layout(F, L, k, ln, train_items, USER_NUM, ITEM_NUM, off)
    params = r.up(_draw_params(x, _ncf_slots(F, L, kind, True, ln and mlp, train_items and mlp), list(off), count))
    loss, logits, grads = r.out(1), r.out(n), r.out(count + TAIL)
    table = table_grad = None                        # a trained table lies in the flat buffers (slot 21), a frozen one is a buffer of its own
    if mlp and train_items:
        table, table_grad = params + 4 * off[21], grads.data_ptr() + 4 * off[21]
    elif mlp:
        table = r.up(x.normal((ITEM_NUM, d)))
    m = _lib.NcfModelC(F, L, k, ln, EPS, train_items, USER_NUM, ITEM_NUM, table, params, grads.data_ptr(), table_grad)
    drop = _ncf_drop(r) if dropped else None
    ws = r.workspace(lib.pmgt_ncf_model_workspace_bytes(F, L, k, ln, train_items, n))
    rc = lib.pmgt_ncf_model_train_grad(C.byref(m), r.users, r.items, r.labels, n, loss.data_ptr(), logits.data_ptr(),
                                       C.byref(drop) if drop else None, *ws, _lib.stream())
    return r.finish(rc, grads, count)


def _dcn_case(name, entry, F, L, Cn, ln, n):
    from pmgt_amd import _lib
    lib = _lib.hip()
    x = _Inputs(name)
    r = _Run(x, n)
    off = (C.c_int64 * _lib.DCN_TENSORS)()
    count = lib.pmgt_dcn_layout(F, L, Cn, ln, USER_NUM, ITEM_NUM, off)
    params = r.up(_draw_params(x, _dcn_slots(F, L, Cn, ln), list(off), count))
    ws = r.workspace(lib.pmgt_dcn_workspace_bytes(F, L, Cn, ln, n))
    if entry == "forward":
        logits = r.out(n)
        head = _lib.DcnHeadC(F, L, Cn, ln, EPS, 0, USER_NUM, ITEM_NUM, params, None)
        return r.finish(lib.pmgt_dcn_forward(C.byref(head), r.users, r.items, n, logits.data_ptr(), *ws, _lib.stream()))
    loss, logits, grads = r.out(1), r.out(n), r.out(count + TAIL)
    head = _lib.DcnHeadC(F, L, Cn, ln, EPS, 0, USER_NUM, ITEM_NUM, params, grads.data_ptr())
    args = (C.byref(head), r.users, r.items, r.labels, n, loss.data_ptr(), logits.data_ptr())
    if entry == "grad":
        rc = lib.pmgt_dcn_train_grad(*args, *ws, _lib.stream())
    else:                                            # every p_cross 0: launch 1 runs its dropout instantiation, launch 2 its plain one
        p_cross = P_CROSS if entry == "dropout" else (0.0,) * 6
        drop = _lib.DcnDropoutC(r.rng(), P_EMB, (C.c_float * 4)(*P_LAYER), (C.c_float * 6)(*p_cross))
        rc = lib.pmgt_dcn_train_grad_dropout(*args, C.byref(drop), *ws, _lib.stream())
    return r.finish(rc, grads, count)


def run_case(name: str):
    spec = CASES[name]
    return {"ncf_train": _ncf_train_case, "ncf_model": _ncf_model_case, "dcn": _dcn_case}[spec[0]](name, *spec[1:])


def record() -> dict:
    return {name: dict(zip(("input", "output"), run_case(name))) for name in CASES}


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with open(sys.argv[1], "w") as f:
        json.dump(record(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", len(CASES), "cases ->", sys.argv[1])
