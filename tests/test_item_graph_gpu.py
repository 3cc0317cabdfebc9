"""build_item_graph(impl="device") against item_graph_host, EXACTLY: indptr, indices, counts, items and the 64 bits of every weight, over
the shapes where the kernels take another path (a wave's row, a workgroup's row, a long user, the dense fallback), the named edge cases,
the forced fallback, and determinism."""
import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd.item_graph import ItemGraphKernels, build_item_graph, device_csrs, item_graph_host, synthetic_interactions

pytestmark = pytest.mark.gpu


def same_bits(x, y):
    assert x.graph.n_nodes == y.graph.n_nodes
    assert np.array_equal(x.graph.indptr, y.graph.indptr)
    assert np.array_equal(x.graph.indices, y.graph.indices)
    assert np.array_equal(x.counts, y.counts)
    assert np.array_equal(x.items, y.items) and np.array_equal(x.node_of_item, y.node_of_item)
    assert np.array_equal(x.graph.weights.view(np.uint64), y.graph.weights.view(np.uint64))


def check(pairs, num_item, min_count, **kw):
    """device == host, or both refuse with the same words -> the device result or None"""
    try:
        want = item_graph_host(pairs, num_item, min_count)
    except ValueError as e:
        with pytest.raises(ValueError) as got:
            build_item_graph(pairs, num_item, min_count, impl="device", **kw)
        assert str(got.value) == str(e) and "no edge" in str(e)
        return None
    got = build_item_graph(pairs, num_item, min_count, impl="device", **kw)
    same_bits(got, want)
    got.graph.validate()
    return got


@pytest.mark.parametrize("min_count", [1, 3])
@pytest.mark.parametrize("num_user", [1, 5, 67, 400])
@pytest.mark.parametrize("num_item", [2, 63, 64, 65, 300, 1000])
def test_equals_the_numpy_yardstick_exactly(num_item, num_user, min_count):
    n_pairs = min(4 * num_item * num_user, 12 * max(num_item, num_user))
    pairs = synthetic_interactions(num_user, num_item, n_pairs, seed=num_item + 7 * num_user)
    got = check(pairs, num_item, min_count)
    if num_user >= 67 or (num_user == 5 and num_item <= 65):
        assert got is not None                                           # (these shapes do have edges: the comparison ran)


def test_one_item_co_reviewed_with_every_other_item():
    """the longest row: item 0 shares three users with each other item, the other items share none among themselves"""
    n = 700
    pairs = np.array([(3 * j + k, i) for j in range(1, n) for k in range(3) for i in (0, j)], dtype=np.int64)
    got = check(pairs, n, 3)
    assert got.graph.degree(2) == n - 1 and (np.diff(got.graph.indptr)[3:] == 1).all()
    assert (got.counts == 3).all()


def test_one_user_who_reviewed_every_item():
    """the largest expansion, and a user whom a whole wave walks"""
    n = 500
    rest = synthetic_interactions(40, n, 900, seed=1)
    pairs = np.concatenate([np.stack([np.full(n, 99), np.arange(n)], 1), rest]).astype(np.int64)
    got = check(pairs, n, 1)
    assert got.graph.n_nodes == n and (np.diff(got.graph.indptr)[2:] == n - 1).all()
    check(pairs, n, 2)
    check(pairs, n, 3)


def test_the_default_table_overflows_into_the_fallback():
    """more distinct neighbours than a workgroup's table holds at the default slot count"""
    n = 4 * _lib.ITEM_GRAPH_MAX_SLOTS + 300
    rest = synthetic_interactions(30, n, 3000, seed=2)
    pairs = np.concatenate([np.stack([np.full(n, 31), np.arange(n)], 1), rest]).astype(np.int64)
    got = check(pairs, n, 2)
    assert len(got.fallback_items) == n                                  # every row has n - 1 neighbours
    again = check(pairs, n, 2)                                           # the scratch rows were left clean
    assert np.array_equal(again.fallback_items, got.fallback_items)


def test_items_without_interaction_and_the_last_item():
    n = 130
    pairs = synthetic_interactions(50, n - 1, 1500, seed=5)
    pairs = pairs[pairs[:, 1] != 17]                                     # item 17 has no interaction at all
    top = np.array([(u, n - 1) for u in range(6)] + [(u, 3) for u in range(6)], dtype=np.int64)      # item n - 1, with item 3
    got = check(np.concatenate([pairs, top]), n, 3)
    assert got.node_of_item[17] == -1 and got.node_of_item[n - 1] == got.graph.n_nodes + 1


def test_no_edge_is_refused_from_the_device_too():
    one = np.array([[0, 0], [1, 0], [2, 0]], dtype=np.int64)
    with pytest.raises(ValueError, match="largest count seen is 0"):
        build_item_graph(one, 1, 1, impl="device")                      # num_item = 1
    singles = np.stack([np.arange(40), np.arange(40)], 1).astype(np.int64)
    assert check(singles, 40, 1) is None                                 # all singletons
    with pytest.raises(ValueError, match=r"min_count = 3 users \(the largest count seen is 2\)"):
        build_item_graph(np.array([[0, 0], [0, 1], [1, 0], [1, 1]], dtype=np.int64), 4, 3, impl="device")
    with pytest.raises(ValueError, match="largest count seen is 0"):
        build_item_graph(np.zeros((0, 2), dtype=np.int64), 4, 1, impl="device")


@pytest.mark.parametrize("min_count", [1, 3])
def test_forced_fallback_with_sixteen_slots(min_count):
    n = 300
    pairs = synthetic_interactions(400, n, 12000, seed=9)
    got = check(pairs, n, min_count, slots=16)
    assert len(got.fallback_items) > n // 2                              # most rows have more than 48 distinct neighbours
    plain = check(pairs, n, min_count)
    assert len(plain.fallback_items) == 0
    same_bits(got, plain)
    # the flags are a function of the row: more than 3 * slots distinct neighbours, from the host's count at min_count 1
    full = item_graph_host(pairs, n, 1)
    distinct = np.zeros(n, dtype=np.int64)
    distinct[full.items] = np.diff(full.graph.indptr)[2:]
    assert np.array_equal(got.fallback_items, np.nonzero(distinct > 48)[0])
    mid = check(pairs, n, min_count, slots=64)                           # between: some rows on each path
    assert np.array_equal(mid.fallback_items, np.nonzero(distinct > 192)[0])


@pytest.mark.parametrize("slots", [16, 32, 64, 256])
def test_every_slot_count_on_sparse_and_dense_rows(slots):
    """tables shorter than a wave (16, 32), one chunk (64) and several; sparse rows stay with their wave, dense ones go to the workgroup"""
    sparse = synthetic_interactions(700, 1000, 4000, seed=12)
    assert check(sparse, 1000, 1, slots=slots) is not None
    keys = torch.unique(torch.from_numpy(sparse[:, 0] * 1000 + sparse[:, 1]).cuda())
    work = device_csrs(keys, 1000)["work"].cpu().numpy()
    assert ((work > 0) & (work <= slots // 4 * 3)).sum() > 100 and (work > slots // 4 * 3).sum() > 10     # both schedules ran
    assert check(sparse, 1000, 2, slots=slots) is not None
    dense = synthetic_interactions(600, 1000, 20000, seed=4)
    same_bits(check(dense, 1000, 3, slots=slots), check(dense, 1000, 3))


def test_determinism_and_device_resident_pairs():
    n = 1000
    pairs = synthetic_interactions(600, n, 20000, seed=4)
    first = check(pairs, n, 3)
    same_bits(build_item_graph(pairs, n, 3, impl="device"), first)      # a second call
    rs = np.random.RandomState(0)
    same_bits(build_item_graph(pairs[rs.permutation(len(pairs))], n, 3, impl="device"), first)
    same_bits(build_item_graph(np.concatenate([pairs[::2], pairs]), n, 3, impl="device"), first)
    same_bits(build_item_graph(torch.from_numpy(pairs).cuda(), n, 3), first)
    same_bits(build_item_graph(torch.from_numpy(pairs), n, 3, device="cuda:0", slots=32), first)
    with pytest.raises(ValueError, match="item 1000 outside"):
        build_item_graph(torch.tensor([[0, 1000], [1, 2]]).cuda(), n, 3)
    with pytest.raises(ValueError, match="negative"):
        build_item_graph(torch.tensor([[0, 1], [-1, 2]]).cuda(), n, 3)


def test_the_raw_entries_refuse_and_leave_the_scratch_clean():
    n = 200
    pairs = synthetic_interactions(100, n, 4000, seed=6)
    keys = torch.unique(torch.from_numpy(pairs[:, 0] * n + pairs[:, 1]).cuda())
    k = ItemGraphKernels(device_csrs(keys, n), n, 2, slots=16)
    words = k.count().cpu().numpy().view(np.uint32)
    torch.cuda.synchronize()
    assert int(k.scratch.abs().max()) == 0 and (words >> 31).any()
    want = item_graph_host(pairs, n, 2)
    deg = np.zeros(n, dtype=np.int64)
    deg[want.items] = np.diff(want.graph.indptr)[2:]
    assert np.array_equal(words & 0x7FFFFFFF, deg)
    assert int(k.max_count.item()) == int(item_graph_host(pairs, n, 1).counts.max())
    lib, front = k.lib, k._front()
    tail = (k.deg_flags.data_ptr(), k.max_count.data_ptr(), k.scratch.data_ptr(), k.scratch_rows, _lib.stream())
    for at, bad in ((9, 8), (9, 24), (9, 2048), (8, 0), (5, 0), (5, 2 ** 31 - 1), (7, 0), (6, 0), (0, 0)):      # slots, min_count, num_item, n_pairs, n_users, NULL
        args = list(front)
        args[at] = bad
        assert lib.pmgt_item_graph_count(*args, *tail) == -2, (at, bad)
    assert lib.pmgt_item_graph_count(*front, tail[0], tail[1], tail[2], 0, tail[4]) == -2
    assert lib.pmgt_item_graph_count(*front, tail[0], tail[1], tail[2] + 4, tail[3], tail[4]) == -2      # misaligned scratch
    assert lib.pmgt_item_graph_count(*front, tail[0], 0, tail[2], tail[3], tail[4]) == -2
    row_ptr = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    node = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = torch.zeros(8, dtype=torch.int32, device="cuda")
    assert lib.pmgt_item_graph_fill(*front, k.deg_flags.data_ptr(), row_ptr.data_ptr(), node.data_ptr(), 0, out.data_ptr(), out.data_ptr(),
                                    k.scratch.data_ptr(), k.scratch_rows, _lib.stream()) == -2      # total < 1
    assert lib.pmgt_item_graph_fill(*front, k.deg_flags.data_ptr(), 0, node.data_ptr(), 4, out.data_ptr(), out.data_ptr(),
                                    k.scratch.data_ptr(), k.scratch_rows, _lib.stream()) == -2
    torch.cuda.synchronize()
    assert int(out.abs().max()) == 0
    assert lib.pmgt_item_graph_default_slots() in (16, 32, 64, 128, 256, 512, 1024)
