"""evaluation._Collected alone, on CPU tensors (.cpu() is then a no-op: the cutting of the one carrier is what is under test): every
column comes back as torch.cat of its own pieces, bit for bit, in the dtype and shape stated, as an array of its own."""
import numpy as np
import pytest
import torch

from samplenet_amd.evaluation import _Collected, _need_added


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _columns(B, g):
    """one batch of B items: {key: (tensor, dtype fetch() is to return)}"""
    value = torch.randn(B, generator=g)
    value[0], value[B // 2] = -0.0, float("nan")
    count = torch.randint(0, 2 ** 24, (B,), generator=g, dtype=torch.int32)
    count[0] = 2 ** 24 - 1  # the largest integer the float32 carrier is trusted with
    return {"value": (value, np.float64),
            "count": (count, np.int64),
            "twist": (torch.randn(B, 7, generator=g), np.float64),
            "cloud": (torch.randn(B, 16, 3, generator=g), np.float32),
            "batch_loss": (torch.randn(1, generator=g), np.float64),
            ("x", 8): (torch.randn(B, 8, generator=g), np.float32),
            ("x", 16): (torch.randint(-5, 5, (B, 16, 2), generator=g, dtype=torch.int64), np.int64),
            "empty": (torch.zeros(B, 0), np.int64)}


@pytest.mark.parametrize("batches", [(5, 4, 3), (1,)])
def test_fetch_returns_every_column_as_the_cat_of_its_pieces(batches):
    g = torch.Generator().manual_seed(7)
    got, pieces = _Collected(), {}
    for B in batches:
        for key, (t, dtype) in _columns(B, g).items():
            got.put(key, t, dtype)
            pieces.setdefault(key, (dtype, []))[1].append(t)
    assert got
    out = got.fetch()
    assert set(out) == set(pieces)
    n = sum(batches)
    assert out["value"].shape == (n,) and out["twist"].shape == (n, 7) and out["cloud"].shape == (n, 16, 3)
    assert out["batch_loss"].shape == (len(batches),) and out["x", 8].shape == (n, 8) and out["x", 16].shape == (n, 16, 2)
    assert out["empty"].shape == (n, 0)
    for key, (dtype, ps) in pieces.items():
        want = torch.cat(ps).numpy().astype(dtype)  # (exact: float32 -> float64, and integers below 2^24)
        a = out[key]
        assert a.dtype == dtype and a.shape == want.shape and a.flags.c_contiguous, key
        assert np.array_equal(_bits(a), _bits(want)), key
        assert a.base is None and a.flags.owndata, key  # (no view of the carrier)
    keys = list(out)
    for i, u in enumerate(keys):
        for v in keys[i + 1:]:
            assert not np.shares_memory(out[u], out[v]), (u, v)
    assert out["count"][0] == 2 ** 24 - 1


def test_on_device_keeps_the_dtype_put():
    got = _Collected()
    got.put("labels", torch.tensor([2 ** 24 + 1, 3], dtype=torch.int32), np.int64)
    got.put("labels", torch.tensor([4], dtype=torch.int32), np.int64)
    assert torch.equal(got.on_device("labels"), torch.tensor([2 ** 24 + 1, 3, 4], dtype=torch.int32))


def test_an_empty_collector_is_what_the_nothing_added_helper_refuses():
    got = _Collected()
    assert not got and got.fetch() == {}
    with pytest.raises(RuntimeError, match=r"^SomeEvaluator\.result: nothing was added$"):
        _need_added(got, "SomeEvaluator")
    got.put("a", torch.zeros(1), np.float64)
    assert _need_added(got, "SomeEvaluator") is got
