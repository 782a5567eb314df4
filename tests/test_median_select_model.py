"""CPU: the model of k_median's bin search (tests/models/median_select_model.py) that supplies the preconditions of
tests/test_gpu_median_edges.py — it finds the median of arbitrary norm sets, and its rounds are bounded as its docstring says."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "models"))
import median_select_model as msm  # noqa: E402
sys.path.insert(0, HERE)
import median_edge_cases as mec  # noqa: E402


def test_a_third_round_always_has_shift_zero():
    """Norm patterns lie in [0, 0x7f800000]; a round with shift s leaves a range of at most 2^s - 1."""
    worst = msm.shift_of(0x7F800000)
    assert worst == 20 and all(msm.shift_of(r) <= worst for r in (1 << np.arange(31)).tolist() + [0x7F800000, 2047, 2048])
    second = max(msm.shift_of(r) for s in range(1, worst + 1) for r in ((1 << s) - 1, 1 << (s - 1)))
    assert second == 9
    assert all(msm.shift_of((1 << s) - 1) == 0 for s in range(0, second + 1))


@pytest.mark.parametrize("seed", range(6))
def test_select_finds_the_median_of_random_norms(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 5000))
    kind = seed % 3
    if kind == 0:
        v = rng.uniform(0.0, 10.0 ** rng.integers(-3, 6), size=n)
    elif kind == 1:
        v = rng.choice(rng.uniform(0.5, 1.5, size=7), size=n)             # heavy ties
    else:
        v = np.concatenate([rng.uniform(1.0, 1.0001, size=n), [0.0, np.inf, 1e-30]])
    bits = v.astype(np.float32).view(np.uint32)
    rounds, exact, value, nties = msm.select(bits)
    want = np.sort(bits)[::-1][bits.size // 2]
    assert value == int(want) and nties == int((bits == want).sum())
    assert 1 <= len(rounds) <= 3 and exact == (rounds[-1]["shift"] == 0)
    assert all(r["inbin"] > msm.K_MED_DIRECT for r in rounds[:-1]) and (exact or rounds[-1]["inbin"] <= msm.K_MED_DIRECT)
    assert rounds[-1]["rem"] < rounds[-1]["inbin"]
    if exact:
        assert rounds[-1]["inbin"] == nties


@pytest.mark.parametrize("inbin", [255, 256, 257])
def test_boundary_construction(inbin):
    bits = mec.boundary_bits(inbin)
    assert bits.size == 1200 and np.unique(bits).size == bits.size - 2
    rounds, exact, value, nties = msm.select(bits)
    assert rounds[0]["inbin"] == inbin and len(rounds) == (1 if inbin <= 256 else 2) and not exact
