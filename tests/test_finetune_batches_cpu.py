"""finetune_batches: the batches of one fine-tuning epoch -- ng_sample's pairs in epoch_order's order, one sampled context per pair -- on a
synthetic graph of 40 nodes and 12 users.  A pure function of its arguments; no GPU."""
import numpy as np
import pytest

from pmgt_amd.datasets import MCNSampler
from pmgt_amd.finetune import finetune_batches
from pmgt_amd.fit_loop import epoch_order
from pmgt_amd.graph import synthetic_graph
from pmgt_amd.pair_train import ng_sample

N_ITEMS, N_USERS, S, BATCH, NUM_NG, SEED = 40, 12, 6, 16, 2, 7


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(1)
    pairs = np.unique(np.stack([rng.integers(0, N_USERS, size=35), rng.integers(0, N_ITEMS, size=35)], 1), axis=0)
    return MCNSampler(synthetic_graph(N_ITEMS, 160, seed=4), max_ctx_neigh=S - 1), pairs


def epoch(data, e, **kw):
    sampler, pairs = data
    args = dict(batch_size=BATCH, num_ng=NUM_NG, seed=SEED, epoch=e)
    args.update(kw)
    return list(finetune_batches(pairs, sampler, N_USERS, N_ITEMS, **args))


def cat(batches, k):
    return np.concatenate([b[k] for b in batches])


def test_same_arguments_same_arrays_another_epoch_other_draws(data):
    a, b, c = epoch(data, 0), epoch(data, 0), epoch(data, 1)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert all(np.array_equal(u, v) for u, v in zip(x, y))
    # the sampler's own sequential stream is not what the contexts come from: drawing from it in between changes nothing
    data[0].context(5)
    for x, y in zip(a, epoch(data, 0)):
        assert all(np.array_equal(u, v) for u, v in zip(x, y))
    # one thread or many: the streams are per pair
    for x, y in zip(a, epoch(data, 0, threads=1)):
        assert all(np.array_equal(u, v) for u, v in zip(x, y))
    neg = lambda bs: np.sort(cat(bs, 1)[cat(bs, 2) == 0])
    assert not np.array_equal(neg(a), neg(c))                # other negatives ...
    pos_a, pos_c = cat(a, 2) == 1, cat(c, 2) == 1
    ctx_a = cat(a, 3)[pos_a][np.lexsort((cat(a, 1)[pos_a], cat(a, 0)[pos_a]))]
    ctx_c = cat(c, 3)[pos_c][np.lexsort((cat(c, 1)[pos_c], cat(c, 0)[pos_c]))]
    assert ctx_a.shape == ctx_c.shape and np.array_equal(ctx_a[:, 0], ctx_c[:, 0]) and not np.array_equal(ctx_a, ctx_c)      # ... and other contexts of the same positives


def test_every_pair_has_its_own_context_headed_by_its_item(data):
    for b in epoch(data, 0) + epoch(data, 3):
        users, items, labels, node_ids, mask = b
        n = len(users)
        assert users.dtype == items.dtype == node_ids.dtype == np.int64 and labels.dtype == mask.dtype == np.float32
        assert items.shape == labels.shape == (n,) and node_ids.shape == mask.shape == (n, S)
        assert np.array_equal(node_ids[:, 0], items + 2)
        assert (mask[:, 0] == 1).all() and set(np.unique(mask)) <= {0.0, 1.0}
        assert ((node_ids >= 2) | (mask == 0)).all() and node_ids.max() < N_ITEMS + 2
    # the same item twice in an epoch draws two contexts (a stream per position, not per item)
    b = epoch(data, 0)
    items, ctx = cat(b, 1), cat(b, 3)
    twice = [i for i in np.unique(items) if (items == i).sum() >= 2]
    assert twice and any(len({tuple(r) for r in ctx[items == i]}) >= 2 for i in twice)


def test_pairs_labels_and_negatives_are_ng_samples_in_epoch_order(data):
    _, pairs = data
    for e in (0, 2):
        users, items, labels = ng_sample(pairs, N_USERS, N_ITEMS, NUM_NG, SEED + e)
        order = epoch_order(len(users), SEED, e)
        b = epoch(data, e)
        assert np.array_equal(cat(b, 0), users[order]) and np.array_equal(cat(b, 1), items[order]) and np.array_equal(cat(b, 2), labels[order])


def test_the_last_batch_is_short_and_no_pair_is_lost(data):
    _, pairs = data
    total = len(pairs) * (1 + NUM_NG)
    assert total % BATCH != 0
    b = epoch(data, 0)
    assert [len(x[0]) for x in b] == [BATCH] * (total // BATCH) + [total % BATCH]
    got = np.stack([cat(b, 0), cat(b, 1)], 1)[cat(b, 2) == 1]
    assert np.array_equal(np.unique(got, axis=0), pairs) and len(got) == len(pairs)
    # another batch size cuts the same sequence elsewhere: pair q keeps its context
    c = epoch(data, 0, batch_size=5)
    assert np.array_equal(cat(b, 3), cat(c, 3)) and np.array_equal(cat(b, 4), cat(c, 4))
    with pytest.raises(ValueError, match="batch_size"):
        epoch(data, 0, batch_size=0)
