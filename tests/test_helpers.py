"""The comparison helpers themselves (CPU): a NaN on the side under test must
never read as agreement, wherever it sits."""
import numpy as np
import pytest
import torch

from helpers import rel_err, worst_err


def test_rel_err_equal_and_empty():
    a = np.array([1.0, -2.0, 0.0, 3.5])
    assert rel_err(a, a.copy()) == 0.0
    assert rel_err(torch.tensor([1.0, 2.0]), torch.tensor([1.0, 2.0])) == 0.0
    assert rel_err(np.zeros((0,)), np.zeros((0,))) == 0.0
    assert rel_err(torch.zeros(0, 3), torch.zeros(0, 3)) == 0.0


def test_rel_err_normwise():
    assert rel_err(np.array([1.0, 10.5]), np.array([1.0, 10.0])) == pytest.approx(0.05)


@pytest.mark.parametrize("pos", [0, 2, 4])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_rel_err_nonfinite_in_a_is_inf(pos, bad):
    b = np.arange(5, dtype=np.float64)
    a = b.copy()
    a[pos] = bad
    assert rel_err(a, b) == float("inf")
    assert rel_err(torch.from_numpy(a).float(), torch.from_numpy(b).float()) == float("inf")


def test_rel_err_all_nan_is_inf():
    assert rel_err(np.full(4, np.nan), np.ones(4)) == float("inf")


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_worst_err_keeps_a_nan(where):
    good = np.array([1.0, 2.0, 3.0])
    nan = np.array([1.0, np.nan, 3.0])
    keys = ["p", "q", "r"]
    at = {"first": "p", "middle": "q", "last": "r"}[where]
    pairs = {k: ((nan if k == at else good * (1 + 1e-7)), good) for k in keys}
    worst, key = worst_err(pairs)
    assert worst == float("inf") and key == at
    # the aggregate the training tests used before: max() drops a NaN
    assert not worst <= 1e-5


def test_worst_err_equal_empty_and_order():
    a = np.array([1.0, -4.0])
    assert worst_err({"x": (a, a.copy()), "y": (a * 2, a * 2)}) == (0.0, "x")
    assert worst_err({"e": (np.zeros(0), np.zeros(0))}) == (0.0, "e")
    assert worst_err({}) == (0.0, None)
    worst, key = worst_err({"x": (a, a), "y": (np.array([1.0, -4.4]), a), "z": (np.array([1.2, -4.0]), a)})
    assert key == "y" and worst == pytest.approx(0.1)


def test_worst_err_nan_reference_is_inf():
    """A NaN on the reference side makes rel_err NaN: not a pass either."""
    a = np.array([1.0, 2.0])
    worst, key = worst_err({"x": (a, a), "y": (a, np.array([1.0, np.nan]))})
    assert worst == float("inf") and key == "y"
