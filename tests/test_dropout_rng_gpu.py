"""The device's counter-based RNG against its numpy restatement (tests/dropout_util.py), bit for bit: the dropout keep decisions of
csrc/common.h (pmgt_op_dropout_keep: make_drop_key + drop_keep4), the NFR masking draws (pmgt_op_nfr_generate -> nfr_generate) and the
compact row list of the last layer (pmgt_op_build_need_rows -> build_need_rows).  Integer work: every comparison is exact.  The restated
masks are what test_dropout_ops_gpu.py and test_dropout_oracle_gpu.py hand to their fp64 / oracle references."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dropout_util as du

pytestmark = pytest.mark.gpu

SEEDS = [0, (1 << 32) + 12345, -(1 << 63) + 77]          # what every test engine uses; above 2^32; top bit set (as int64)
STEPS = [0, 1, (1 << 32) + 5]
L_LAYERS = 4


def _lib_():
    from pmgt_amd import _lib
    return _lib, _lib.hip()


def P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def device_keep(H, _lib, rng, p, site, rows, cols):
    out = torch.full((rows, cols), 7, dtype=torch.uint8, device="cuda")
    _lib.check(H.pmgt_op_dropout_keep(P(rng), p, site, rows, cols, P(out), stream()))
    return out.cpu().numpy()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("step", STEPS)
def test_keep_bytes_equal_the_restatement_for_every_engine_site(seed, step):
    """Every site id the engine uses (layer -1 .. L-1, kinds 0 .. 4), p in {0.1, 0.2, 0.25, 0.5, 1e-6, 0}, column counts that are not
    multiples of 4 (the attention shapes of test_attention_fwd_bwd); seeds / steps through an int64 tensor as the engine passes them."""
    _lib, H = _lib_()
    rng = torch.tensor([seed, step], dtype=torch.int64, device="cuda")
    shapes = [(67, 33), (40, 17), (50, 6), (9, 256)]
    n = 0
    for layer in range(-1, L_LAYERS):
        for kind in range(5):
            site = du.site_id(layer, kind)
            for p in (0.1, 0.2, 0.25, 0.5, 1e-6, 0.0):
                rows, cols = shapes[n % len(shapes)]
                n += 1
                got = device_keep(H, _lib, rng, p, site, rows, cols)
                want = du.keep(seed, step, site, rows, cols, p)
                assert set(np.unique(got)) <= {0, 1}
                assert np.array_equal(got.astype(bool), want), (layer, kind, p, rows, cols)
                if p == 0.0 or p == 1e-6:
                    assert got.all()                                  # p = 0: off; p = 1e-6: (thr >> 16) == 0, the 16-bit decision keeps all
                elif rows * cols > 2000:
                    assert abs(got.mean() - (1 - (du.drop_threshold(p) >> 16) / 65536)) < 0.04


@pytest.mark.parametrize("rows,cols,p", [((1 << 20) + 3, 6, 0.1), ((1 << 20) + 3, 33, 0.25), (70001, 256, 0.1), (4099, 1024, 0.5), (1, 1, 0.2)])
def test_keep_bytes_at_large_row_counts(rows, cols, p):
    _lib, H = _lib_()
    seed, step = SEEDS[1], 7
    rng = torch.tensor([seed, step], dtype=torch.int64, device="cuda")
    site = du.site_id(2, du.SITE_A2)
    got = device_keep(H, _lib, rng, p, site, rows, cols)
    assert np.array_equal(got.astype(bool), du.keep(seed, step, site, rows, cols, p))
    # p = 0 needs no rng at all
    assert device_keep(H, _lib, None, 0.0, site, min(rows, 100), cols).all()


@pytest.mark.parametrize("S", [2, 9, 32, 64])
@pytest.mark.parametrize("n_nodes", [3, 7252, 10 ** 6])
def test_nfr_generate_equals_the_restatement(S, n_nodes):
    _lib, H = _lib_()
    B = 41
    rs = np.random.RandomState(S + n_nodes % 97)
    ids = rs.randint(2, n_nodes + 2, size=(B, S)).astype(np.int64)
    for b in range(B):                                  # padded tails (id 0), some sequences with the target alone
        ids[b, 1 + (b * 5) % S:] = 0
    ids[3] = rs.randint(2, n_nodes + 2, size=S)
    d_ids = torch.from_numpy(ids).cuda()
    for seed, step, rr, mr in [(0, 0, 0.02, 0.16), (0, 1, 0.02, 0.16), (SEEDS[1], 5, 0.3, 0.5), (SEEDS[2], STEPS[2], 0.9, 0.9), (0, 2, 0.0, 1.0)]:
        rng = torch.tensor([seed, step], dtype=torch.int64, device="cuda")
        masked = torch.full((B, S), -9, dtype=torch.int64, device="cuda")
        tgt = torch.full((B, S), -9, dtype=torch.int64, device="cuda")
        _lib.check(H.pmgt_op_nfr_generate(P(d_ids), B, S, n_nodes, rr, mr, P(rng), P(masked), P(tgt), stream()))
        m, t = masked.cpu().numpy(), tgt.cpu().numpy()
        wm, wt = du.nfr_device_masks(ids, n_nodes, seed, step, rr, mr)
        assert np.array_equal(m, wm) and np.array_equal(t, wt), (seed, step, rr, mr)
        # the definition itself, on the device's output
        assert np.array_equal(m[:, 0], ids[:, 0]) and (t[:, 0] == -1).all()
        pad = ids == 0
        assert (m[pad] == 0).all() and (t[pad] == -1).all()
        hit = t >= 0
        assert (m[hit] == 1).all() and ((t[hit] >= 2) & (t[hit] < n_nodes + 2)).all()
        changed = ~hit & (m != ids)
        assert ((m[changed] >= 2) & (m[changed] < n_nodes + 2)).all()
        if mr == 1.0:
            live = ~pad
            live[:, 0] = False
            assert np.array_equal(hit, live) and np.array_equal(t[hit], ids[hit])     # random_ratio 0: targets are the original ids


@pytest.mark.parametrize("B,Pn,S,n_nfr", [(4, 7, 8, 0), (4, 7, 8, 1), (4, 7, 8, 28), (5, 0, 16, 9), (64, 130, 32, 300), (64, 130, 32, 64 * 31),
                                          (3, 2, 1, 0)])
def test_build_need_rows_equals_the_definition(B, Pn, S, n_nfr):
    """rows = CLS rows of the B targets, of the P pairs, then the NFR rows in their given order; count = B + P + n; inv = the inverse map,
    -1 elsewhere.  nfr_count 0 / 1 / full, P = 0, and B * S beyond one 256-thread block."""
    _lib, H = _lib_()
    n_tokens = (2 * B + Pn) * S
    cap = B + Pn + B * max(S - 1, 1)
    rs = np.random.RandomState(B + S + n_nfr)
    # masked positions live in the third group of sequences (the masked copy of the targets), never at position 0
    cand = np.array([(B + Pn + b) * S + s for b in range(B) for s in range(1, S)], dtype=np.int64)
    nfr = np.sort(rs.choice(cand, size=n_nfr, replace=False)) if n_nfr else np.zeros(0, dtype=np.int64)
    nfr_buf = torch.full((max(B * max(S - 1, 1), 1),), -5, dtype=torch.int64, device="cuda")
    nfr_buf[:n_nfr] = torch.from_numpy(nfr).cuda()
    cnt = torch.tensor([n_nfr], dtype=torch.int32, device="cuda")
    rows = torch.full((cap,), -7, dtype=torch.int64, device="cuda")
    count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    inv = torch.full((n_tokens,), 12345, dtype=torch.int32, device="cuda")
    _lib.check(H.pmgt_op_build_need_rows(B, Pn, S, P(nfr_buf), P(cnt), P(rows), P(count), P(inv), n_tokens, stream()))
    want = du.need_rows(B, Pn, S, nfr)
    assert int(count.item()) == B + Pn + n_nfr == want.size
    got = rows.cpu().numpy()
    assert np.array_equal(got[:want.size], want) and (got[want.size:] == -7).all()
    winv = np.full(n_tokens, -1, dtype=np.int32)
    winv[want] = np.arange(want.size)
    assert np.array_equal(inv.cpu().numpy(), winv)
    # without the inverse map
    rows.fill_(-7)
    _lib.check(H.pmgt_op_build_need_rows(B, Pn, S, P(nfr_buf), P(cnt), P(rows), P(count), None, 0, stream()))
    assert np.array_equal(rows.cpu().numpy()[:want.size], want)
