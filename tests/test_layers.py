"""hbx.layers: how CoinReplay, CoinSession and EpochSession split a run of messages into engine
calls that hold each (row, sender) position once."""
from collections import Counter

from hbbft_amd.hbx import layers

KEYS = [(0, 1), (2, 2), (0, 1), (1, 0), (0, 1), (2, 2), (3, 3), (1, 0), (0, 1)]


def test_layers_partition_the_indices_in_order():
    got = layers(KEYS)
    assert sorted(i for layer in got for i in layer) == list(range(len(KEYS)))
    for layer in got:
        assert layer == sorted(layer)
        assert len({KEYS[i] for i in layer}) == len(layer)
    assert len(got) == max(Counter(KEYS).values())


def test_layer_L_holds_the_Lth_occurrences():
    seen = Counter()
    want = {}
    for i, key in enumerate(KEYS):
        want.setdefault(seen[key], []).append(i)
        seen[key] += 1
    assert layers(KEYS) == [want[L] for L in range(len(want))]
    assert layers(KEYS) == [[0, 1, 3, 6], [2, 5, 7], [4], [8]]


def test_layers_of_nothing_and_of_distinct_keys():
    assert layers([]) == []
    assert layers(iter("abc")) == [[0, 1, 2]]
