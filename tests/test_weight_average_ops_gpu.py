"""The weight-averaging kernels through their C entries (pmgt_amd/ops/weight_average.hip: pmgt_weight_average_update, pmgt_weight_swap).

Bounds.  Everything is bit-exact (== on the raw 32-bit words): the update is two fp32 products and one fp32 sum, each rounded once and
never fused, which tests/weight_average_util.py restates in numpy; the swap moves words; the prepare lane computes one fp64 division
and rounds to fp32 once per weight, as the host series pmgt_amd.averaging.ema_decay does.  Both buffers sit between 64-element canaries
that must survive, and the parameter side of an update is never written.  Sizes: the scalar tail alone (1, 2, 3), one group, a group and
a tail, one 256-lane block of groups less / exactly / more (1023 / 1024 / 1025 elements), a quarter of it (255 / 256 / 257) and four
blocks plus one element; base offsets: 16-byte aligned (the 16-byte form) and one element past it (the scalar form)."""
import ctypes as C

import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd import averaging as av
from tests import weight_average_util as wu
from tests.test_rowops_gpu import H, P, check, stream

pytestmark = pytest.mark.gpu

CANARY_BITS = 0x7FC12345          # a NaN with a payload: an arithmetic pass over it would not keep it


class Guarded:
    """n words between canaries, `shift` elements past a 16-byte boundary."""

    def __init__(self, values_u32: np.ndarray, shift: int = 0):
        self.n, self.lo = len(values_u32), wu.CANARY + shift
        host = np.full(self.n + 2 * wu.CANARY + shift, CANARY_BITS, dtype=np.uint32)
        host[self.lo: self.lo + self.n] = values_u32
        self.buf = torch.from_numpy(host.view(np.int32)).cuda()
        assert self.buf.data_ptr() % 16 == 0

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + 4 * self.lo)

    def words(self):
        return self.buf.cpu().numpy().view(np.uint32)[self.lo: self.lo + self.n]

    def canaries_intact(self):
        w = self.buf.cpu().numpy().view(np.uint32)
        return bool((w[:self.lo] == CANARY_BITS).all() and (w[self.lo + self.n:] == CANARY_BITS).all())


def ema_cfg(state, decay=0.999, warmup=True, skip_flag=None):
    return _lib.AvgStepC(1, int(warmup), decay, P(state), P(skip_flag), 0.0, 0.0)


def read_state(state):
    st = state.cpu()
    return dict(n_upd=int(st[0]), skip=int(st.view(torch.int32)[2]), w_old=st.view(torch.float32)[3].numpy().copy(),
                w_new=st.view(torch.float32)[4].numpy().copy(), rest=st.view(torch.int32)[5:].tolist())


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", wu.OP_SIZES)
def test_avg_apply_is_the_restatement_bit_for_bit(n, shift):
    avg0, p0 = wu.special_inputs(n, seed=100 + n)
    # by value: swa_step at models_num = 3
    a, p = Guarded(avg0.view(np.uint32), shift), Guarded(p0.view(np.uint32), shift)
    w_old, w_new = av.swa_weights(3)
    cfg = _lib.AvgStepC(0, 0, 0.0, None, None, float(w_old), float(w_new))
    check(H().pmgt_weight_average_update(a.ptr(), p.ptr(), n, C.byref(cfg), stream()))
    torch.cuda.synchronize()
    want = wu.swa_step_np(avg0, p0, 3)
    assert np.array_equal(a.words(), want.view(np.uint32))
    assert np.array_equal(p.words(), p0.view(np.uint32)) and a.canaries_intact() and p.canaries_intact()
    # from the device state: the update that follows 5 applied ones, decay 0.999 with warm-up -> d = 6 / 15
    a2 = Guarded(avg0.view(np.uint32), shift)
    state = torch.tensor([5, 0, 0, 0], dtype=torch.int64, device="cuda")
    cfg2 = ema_cfg(state)
    check(H().pmgt_weight_average_update(a2.ptr(), p.ptr(), n, C.byref(cfg2), stream()))
    torch.cuda.synchronize()
    wo, wn = av.ema_weights(5)
    assert wo == np.float32(6 / 15) and wn == np.float32(1.0 - 6 / 15)
    assert np.array_equal(a2.words(), wu.avg_apply_np(avg0, p0, wo, wn).view(np.uint32))
    assert np.array_equal(p.words(), p0.view(np.uint32)) and a2.canaries_intact() and p.canaries_intact()
    st = read_state(state)
    assert (st["n_upd"], st["skip"], st["rest"]) == (6, 0, [0, 0, 0]) and st["w_old"] == wo and st["w_new"] == wn


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", wu.OP_SIZES)
def test_swap_moves_raw_words_and_is_its_own_inverse(n, shift):
    rng = np.random.RandomState(7 + n)
    x0 = rng.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    y0 = rng.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    nan_payloads = np.array([0x7FC00001, 0xFFC00002, 0x7F800001, 0xFF80FFFF, 0x7F800000, 0x80000000, 0x00000001], dtype=np.uint32)
    k = min(n, len(nan_payloads))
    if k:
        x0[n - k:] = nan_payloads[:k]                  # quiet and signalling NaNs with payloads, Inf, -0, a denormal
        y0[:k] = nan_payloads[::-1][:k]
    x, y = Guarded(x0, shift), Guarded(y0, shift)
    check(H().pmgt_weight_swap(x.ptr(), y.ptr(), n, stream()))
    torch.cuda.synchronize()
    assert np.array_equal(x.words(), y0) and np.array_equal(y.words(), x0) and x.canaries_intact() and y.canaries_intact()
    check(H().pmgt_weight_swap(x.ptr(), y.ptr(), n, stream()))
    torch.cuda.synchronize()
    assert np.array_equal(x.words(), x0) and np.array_equal(y.words(), y0) and x.canaries_intact() and y.canaries_intact()


@pytest.mark.parametrize("decay,warmup", [(0.999, True), (0.5, True), (0.999, False)])
def test_prepare_lane_counts_and_writes_the_series(decay, warmup):
    """40 updates of a 5-element average: after update k the device state holds the fp32 weights of ema_decay(k) and the count k + 1, and
    the average is the restatement's.  Then a skip flag of 1.0: count, weights and average untouched, the skip word set; a flag of 0.0
    clears it and applies."""
    n = 5
    avg0, p0 = wu.special_inputs(n, seed=3)
    a, p = Guarded(avg0.view(np.uint32)), Guarded(p0.view(np.uint32))
    state = torch.zeros(4, dtype=torch.int64, device="cuda")
    cfg = ema_cfg(state, decay, warmup)
    want = avg0
    for k in range(40):
        check(H().pmgt_weight_average_update(a.ptr(), p.ptr(), n, C.byref(cfg), stream()))
        st = read_state(state)
        d = av.ema_decay(k, decay, warmup)
        assert st["n_upd"] == k + 1 and st["skip"] == 0
        assert st["w_old"] == np.float32(d) and st["w_new"] == np.float32(1.0 - d), (k, st, d)
        want = wu.avg_apply_np(want, p0, np.float32(d), np.float32(1.0 - d))
    assert np.array_equal(a.words(), want.view(np.uint32)) and a.canaries_intact()
    before = read_state(state)
    flag = torch.tensor([1.0], device="cuda")
    cfg_skip = ema_cfg(state, decay, warmup, flag)
    check(H().pmgt_weight_average_update(a.ptr(), p.ptr(), n, C.byref(cfg_skip), stream()))
    st = read_state(state)
    assert st["n_upd"] == 40 and st["skip"] == 1 and st["w_old"] == before["w_old"] and st["w_new"] == before["w_new"]
    assert np.array_equal(a.words(), want.view(np.uint32)) and np.array_equal(p.words(), p0.view(np.uint32))
    flag.zero_()
    check(H().pmgt_weight_average_update(a.ptr(), p.ptr(), n, C.byref(cfg_skip), stream()))
    st = read_state(state)
    d = av.ema_decay(40, decay, warmup)
    assert st["n_upd"] == 41 and st["skip"] == 0 and st["w_old"] == np.float32(d)
    assert np.array_equal(a.words(), wu.avg_apply_np(want, p0, np.float32(d), np.float32(1.0 - d)).view(np.uint32))
    assert a.canaries_intact() and p.canaries_intact()


def test_bad_arguments_are_refused():
    x, y = Guarded(np.arange(8, dtype=np.uint32)), Guarded(np.arange(8, 16, dtype=np.uint32))
    state = torch.zeros(4, dtype=torch.int64, device="cuda")
    L = H()
    swa = _lib.AvgStepC(0, 0, 0.0, None, None, 0.5, 0.5)

    def refused(rc, word):
        return rc == -2 and word in L.pmgt_last_error().decode()
    assert refused(L.pmgt_weight_average_update(None, y.ptr(), 8, C.byref(swa), stream()), "NULL buffer")
    assert refused(L.pmgt_weight_average_update(x.ptr(), None, 8, C.byref(swa), stream()), "NULL buffer")
    assert refused(L.pmgt_weight_average_update(x.ptr(), y.ptr(), 8, None, stream()), "NULL cfg")
    assert refused(L.pmgt_weight_average_update(x.ptr(), y.ptr(), -1, C.byref(swa), stream()), "negative")
    assert refused(L.pmgt_weight_average_update(x.ptr(), y.ptr(), 8, C.byref(_lib.AvgStepC(2, 0, 0.0, None, None, 0.5, 0.5)), stream()), "unknown mode")
    for decay in (1.0, -0.25, 1.5, float("nan")):
        assert refused(L.pmgt_weight_average_update(x.ptr(), y.ptr(), 8, C.byref(ema_cfg(state, decay)), stream()), "outside [0, 1)")
    assert refused(L.pmgt_weight_average_update(x.ptr(), y.ptr(), 8, C.byref(_lib.AvgStepC(1, 1, 0.9, None, None, 0.0, 0.0)), stream()), "NULL device state")
    assert refused(L.pmgt_weight_swap(None, y.ptr(), 8, stream()), "NULL buffer")
    assert refused(L.pmgt_weight_swap(x.ptr(), None, 8, stream()), "NULL buffer")
    assert refused(L.pmgt_weight_swap(x.ptr(), y.ptr(), -3, stream()), "negative")
    assert refused(L.pmgt_weight_swap(x.ptr(), x.ptr(), 8, stream()), "the same")
    torch.cuda.synchronize()
    assert np.array_equal(x.words(), np.arange(8, dtype=np.uint32)) and np.array_equal(y.words(), np.arange(8, 16, dtype=np.uint32))
    assert int(state[0]) == 0 and L.pmgt_abi_version() == 4
