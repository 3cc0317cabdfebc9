"""The inputs and the launches of the bit-pinning test of the scoring tower (test_score_tower_bits_gpu.py; the fixture is
tests/golden/score_tower_bits.json).  Every input of a case comes from ONE seeded numpy generator, in a fixed order, and goes straight
into the C entry (pmgt_ncf_score, pmgt_ncf_model_score, pmgt_dcn_score_rows + pmgt_dcn_score): Pu and Pi are drawn, not multiplied out,
so no BLAS version enters.  torch only holds the device memory.

Every case is N_USERS = 17 users by N_ITEMS = 70 items (neither a multiple of the tile: 16 or 8 users, 32 items) into rows of
ROW_STRIDE = 72 floats whose two padding columns are pre-filled with SENTINEL: they are part of the hashed output, so a store past the
catalogue changes the hash.

run_case(name) -> (sha256 of the input bytes, sha256 of the output bytes).  Run as a script, it writes the fixture:
    python tests/score_bits_util.py OUT.json
"""
import ctypes as C
import hashlib
import json
import sys
import zlib

import numpy as np

N_USERS, N_ITEMS, ROW_STRIDE, USER_NUM = 17, 70, 72, 23
SENTINEL = np.float32(-12345.0)
EPS = 1e-5

_NCF_SHAPES = [(8, 1, "MLP"), (8, 2, "NeuMF-end"), (16, 3, "MLP"), (32, 3, "NeuMF-end"), (64, 3, "MLP")]      # (factor, layers, kind)
_DCN_SHAPES = [(16, 1, 4, True), (16, 2, 2, False), (16, 3, 2, True), (64, 2, 6, True), (64, 2, 6, False)]       # (factor, deep, cross, LN)
CASES = {f"ncf_score-{f}-{l}-{k}": ("ncf", f, l, k) for f, l, k in _NCF_SHAPES}
CASES.update({f"ncf_model_score-ln-{f}-{l}-{k}": ("ncf_model", f, l, k) for f, l, k in _NCF_SHAPES + [(64, 1, "GMF")]})
CASES.update({f"dcn_score-{f}-{l}-{c}-{'ln' if ln else 'plain'}": ("dcn", f, l, c, ln) for f, l, c, ln in _DCN_SHAPES})


class _Inputs:
    """Draws fp32 arrays from the case's generator in call order and remembers them for the hash."""

    def __init__(self, name: str):
        self.rng = np.random.default_rng([2024, zlib.crc32(name.encode())])
        self.arrays = []

    def keep(self, a):
        a = np.ascontiguousarray(a)
        self.arrays.append(a)
        return a

    def normal(self, shape, scale=1.0, shift=0.0):
        return self.keep((self.rng.standard_normal(shape) * scale + shift).astype(np.float32))

    def users(self):
        return self.keep(self.rng.integers(0, USER_NUM, N_USERS).astype(np.int64))

    def sha(self) -> str:
        h = hashlib.sha256()
        for a in self.arrays:
            h.update(a.tobytes())
        return h.hexdigest()


def _run(launch, inputs: _Inputs, held):
    """Upload is done by the caller (`held` keeps the device tensors alive); launch(out_ptr) calls the entry -> the two hashes."""
    import torch

    from pmgt_amd import _lib
    out = torch.full((N_USERS, ROW_STRIDE), float(SENTINEL), dtype=torch.float32, device="cuda")
    _lib.check(launch(out.data_ptr()))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    del held
    assert (got[:, N_ITEMS:] == SENTINEL).all(), "the padding columns were written"
    return inputs.sha(), hashlib.sha256(got.tobytes()).hexdigest()


def _ncf_case(name, entry, factor, layers, kind):
    import torch

    from pmgt_amd import _lib
    lib = _lib.hip()
    x = _Inputs(name)
    mlp, gmf = kind != "GMF", kind != "MLP"
    d = factor << (layers - 1)
    dev = lambda a: torch.from_numpy(a).cuda()
    held = []

    def up(a):
        held.append(dev(a))
        return held[-1].data_ptr()
    model = entry == "ncf_model"
    h = _lib.NcfModelHeadC() if model else _lib.NcfHeadC()
    h.factor_num, h.num_layers, h.user_num = factor, layers, USER_NUM
    h.kind = (_lib.NCF_MODEL_KINDS if model else _lib.NCF_KINDS).index(kind)
    if model:
        h.use_layer_norm, h.layer_norm_eps = 1, EPS
    pu = pi = 0
    if mlp:
        pu, pi = up(x.normal((N_USERS, d))), up(x.normal((N_ITEMS, d)))
        for i in range(layers):
            m, k = d >> i, d >> (i - 1) if i else 0
            if i:
                h.weight[i], h.bias[i] = up(x.normal((m, k), 1.0 / np.sqrt(k))), up(x.normal((m,), 0.1))
            if model:
                h.gamma[i], h.beta[i] = up(x.normal((m,), 0.1, 1.0)), up(x.normal((m,), 0.1))
    h.predict_weight = up(x.normal((factor * (2 if mlp and gmf else 1),), 1.0 / np.sqrt(factor)))
    h.predict_bias = up(x.normal((1,), 0.1))
    if gmf:
        h.gmf_user, h.gmf_item = up(x.normal((USER_NUM, factor))), up(x.normal((N_ITEMS, factor)))
    users = up(x.users())
    fn = lib.pmgt_ncf_model_score if model else lib.pmgt_ncf_score
    return _run(lambda out: fn(C.byref(h), pu, pi, users, N_USERS, N_ITEMS, out, ROW_STRIDE, _lib.stream()), x, held)


def _dcn_case(name, factor, deep, cross, ln):
    import torch

    from pmgt_amd import _lib
    from pmgt_amd.dcn_head import ITEM_KEY, USER_KEY, dcn_layout
    lib = _lib.hip()
    x = _Inputs(name)
    E = factor << deep
    layout, count = dcn_layout(factor, deep, cross, ln, USER_NUM, N_ITEMS)
    flat = np.zeros(count, dtype=np.float32)
    for key, (off, shape) in layout.items():
        if key.endswith("layer_norm.weight"):
            v = x.normal(shape, 0.1, 1.0)
        elif len(shape) == 2:
            v = x.normal(shape, 1.0 / np.sqrt(shape[1] if shape[1] > 1 else shape[0]))
        else:
            v = x.normal(shape, 0.1)
        flat[off: off + v.size] = v.reshape(-1)
    pu_h, pi_h = x.normal((N_USERS, E)), x.normal((N_ITEMS, E))
    consts_h = x.normal((2 * _lib.DCN_MAX_CROSS,), 0.1)
    users_h = x.users()
    off = layout[USER_KEY][0]
    user_table = flat[off: off + USER_NUM * E].reshape(USER_NUM, E)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    flat_d, pu, pi, consts, users, gathered = dev(flat), dev(pu_h), dev(pi_h), dev(consts_h), dev(users_h), dev(user_table[users_h])
    head = _lib.DcnHeadC(factor, deep, cross, int(ln), EPS, 0, USER_NUM, N_ITEMS, flat_d.data_ptr(), None)
    item_off = layout[ITEM_KEY][0]
    user_rows = torch.empty(N_USERS, _lib.DCN_SCORE_ROW_STRIDE, dtype=torch.float32, device="cuda")
    item_rows = torch.empty(N_ITEMS, _lib.DCN_SCORE_ROW_STRIDE, dtype=torch.float32, device="cuda")
    _lib.check(lib.pmgt_dcn_score_rows(C.byref(head), gathered.data_ptr(), N_USERS, 0, user_rows.data_ptr(), _lib.stream()))
    _lib.check(lib.pmgt_dcn_score_rows(C.byref(head), flat_d.data_ptr() + 4 * item_off, N_ITEMS, 1, item_rows.data_ptr(), _lib.stream()))
    held = [flat_d, pu, pi, consts, users, gathered, user_rows, item_rows]
    return _run(lambda out: lib.pmgt_dcn_score(C.byref(head), pu.data_ptr(), pi.data_ptr(), user_rows.data_ptr(), item_rows.data_ptr(),
                                               consts.data_ptr(), users.data_ptr(), N_USERS, N_ITEMS, out, ROW_STRIDE, _lib.stream()), x, held)


def run_case(name: str):
    spec = CASES[name]
    if spec[0] == "dcn":
        return _dcn_case(name, *spec[1:])
    return _ncf_case(name, *spec)


def record() -> dict:
    return {name: dict(zip(("input", "output"), run_case(name))) for name in CASES}


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with open(sys.argv[1], "w") as f:
        json.dump(record(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", len(CASES), "cases ->", sys.argv[1])
