"""`bench.py --dump-outputs DIR`: the step's result as DIR/<name>.npy, float32 / float64, at most 64 MiB in all (rows
of larger arrays sampled with a fixed seed).  The helpers are exercised here on host tensors; no GPU."""
import os
from typing import NamedTuple, Optional

import numpy as np
import torch

import bench


class _Result(NamedTuple):
    logz: torch.Tensor
    logz64: torch.Tensor
    posterior: Optional[torch.Tensor]
    beta_me: Optional[torch.Tensor]


def _arrays():
    g = torch.Generator().manual_seed(0)
    r = _Result(torch.randn(7, generator=g), torch.randn(7, generator=g, dtype=torch.float64),
                torch.rand(5000, generator=g), None)
    return bench.host_outputs(r, torch.tensor([3.5], dtype=torch.float64))


def test_host_outputs_keeps_float64_and_skips_missing():
    a = _arrays()
    assert sorted(a) == ["logz", "logz64", "posterior", "sum_logz"]
    assert a["logz"].dtype == np.float32 and a["posterior"].dtype == np.float32
    assert a["logz64"].dtype == np.float64 and a["sum_logz"].dtype == np.float64 and a["sum_logz"].tolist() == [3.5]


def test_dump_writes_everything_under_the_cap(tmp_path):
    a = _arrays()
    bench.dump_outputs(str(tmp_path), a)
    for k, v in a.items():
        got = np.load(tmp_path / f"{k}.npy")
        assert got.dtype == v.dtype and np.array_equal(got, v)


def test_dump_samples_the_same_rows_past_the_cap(tmp_path):
    a = _arrays()
    cap = 4096 * len(a) + 8000  # room for the headers and ~8 kB of data: the posterior cannot be kept whole
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), a, cap=cap)
    total = sum(os.path.getsize(tmp_path / "one" / f) for f in os.listdir(tmp_path / "one"))
    assert total <= cap
    p1, p2 = np.load(tmp_path / "one" / "posterior.npy"), np.load(tmp_path / "two" / "posterior.npy")
    assert 0 < p1.size < a["posterior"].size and np.array_equal(p1, p2)
    assert np.isin(p1, a["posterior"]).all()
