"""The shared comparators of tests/gallery_support.py must not pass silently: each one fails on the smallest difference it exists to
catch.  The host-packed allow words equal gallery_mask_ref.pack_words with the requested tail, and ShardPair.to_global is the row
mapping the shard references state.  No GPU."""

import numpy as np
import pytest
import torch

import gallery_mask_ref as MR
import gallery_shard_graph_ref as SG
from gallery_support import ShardPair, same_bits, same_values, words_tensor

CPU = torch.device("cpu")


def _pair():
    return torch.tensor([[0.5, 0.0, -1.0]]), torch.tensor([[4, 2, 7]])


def test_same_bits_tells_the_zeros_apart_and_sees_one_row():
    vals, rows = _pair()
    same_bits((vals, rows), (vals.clone().numpy(), rows.clone().numpy()))
    minus = vals.clone()
    minus[0, 1] = -0.0
    assert torch.equal(minus, vals)  # (equal as values: only the bit patterns differ)
    with pytest.raises(AssertionError):
        same_bits((minus, rows), (vals.numpy(), rows.numpy()))
    other = rows.clone()
    other[0, 2] = 8
    with pytest.raises(AssertionError):
        same_bits((vals, other), (vals.numpy(), rows.numpy()))


def test_same_values_sees_one_value_one_row_and_one_pid():
    vals, rows = _pair()
    pids = torch.arange(10) * 3
    same_values((vals, rows), (vals.clone(), rows.clone()), "equal")
    same_values((vals, rows, pids[rows]), (vals.clone(), rows.clone()), "equal, pids", pids)
    nudged = vals.clone()
    nudged[0, 0] = torch.nextafter(vals[0, 0], torch.tensor(1.0))
    with pytest.raises(AssertionError):
        same_values((nudged, rows), (vals, rows), "value")
    other = rows.clone()
    other[0, 0] = 5
    with pytest.raises(AssertionError):
        same_values((vals, other), (vals, rows), "row")
    with pytest.raises(AssertionError):
        same_values((vals, rows, pids[other]), (vals, rows), "pid", pids)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65])
def test_words_tensor_equals_pack_words_with_the_requested_tail(n):
    nw = (n + 31) // 32
    tail = nw * 32 - n
    top = (np.arange(n) & 31) == min(31, n - 1)  # the highest bit a word of this length can hold
    if n >= 32:
        assert int(words_tensor(top, CPU)[0]) == -(1 << 31)  # bit 31 alone: uint32 0x80000000 wraps to the lowest int32
    for allow in (np.random.RandomState(n).rand(n) < 0.5, top, np.ones(n, dtype=bool)):
        want = MR.pack_words(torch.from_numpy(allow))
        for src in (allow, torch.from_numpy(allow)):
            got = words_tensor(src, CPU)
            assert got.dtype == torch.int32 and torch.equal(MR.words_as_int64(got), want)
        # extra: words of all ones behind the named ones
        got = words_tensor(allow, CPU, extra=3)
        assert got.shape == (nw + 3,) and torch.equal(MR.words_as_int64(got[:nw]), want) and got[nw:].tolist() == [-1, -1, -1]
        # garbage: the named bits unchanged, every tail bit set; with a seed bit n set and the bits above it the seed's draws
        low = (1 << (32 - tail)) - 1
        ones = MR.words_as_int64(words_tensor(allow, CPU, garbage=True))
        drawn = MR.words_as_int64(words_tensor(allow, CPU, garbage=True, seed=n))
        for got in (ones, drawn):
            assert torch.equal(got[:-1], want[:-1]) and int(got[-1]) & low == int(want[-1])
        assert int(ones[-1]) >> (32 - tail) == (1 << tail) - 1
        if tail:
            draws = np.random.RandomState(n).randint(0, 2, size=tail)
            draws[0] = 1
            assert [(int(drawn[-1]) >> (32 - tail + i)) & 1 for i in range(tail)] == draws.tolist()
        else:
            assert torch.equal(drawn, want)


def test_to_global_at_the_part_boundaries():
    S = 32
    empty = (torch.zeros(1, 256), torch.zeros(0, 256), torch.zeros(0, dtype=torch.int64), True)
    pair = ShardPair(CPU, empty, S)
    rows = torch.tensor([-1, 0, S - 1, S, S + 1, 2 * S - 1, 2 * S, 3 * S + 2])
    want = [-1, 0, S - 1, SG.SHARD_STRIDE, SG.SHARD_STRIDE + 1, SG.SHARD_STRIDE + S - 1, 2 * SG.SHARD_STRIDE, 3 * SG.SHARD_STRIDE + 2]
    assert pair.to_global(rows).tolist() == want
    assert pair.to_global(rows.to(torch.int32)).tolist() == want  # (the graph's int32 lists)
    assert [(r // S) * SG.SHARD_STRIDE + r % S for r in rows.tolist()[1:]] == want[1:]
