"""bench.py --dump-outputs, host side: file types, the fixed seeded sample of a large array, the size limit."""
import os

import numpy as np
import pytest
import torch


def test_dump_outputs_types_sample_and_limit(tmp_path):
  import bench
  big = torch.arange(bench.DUMP_CAP + 1000, dtype=torch.float32)
  stats = {'loss': torch.tensor(1.5), 'losses': {'data': torch.tensor(0.25)}, 'grad_norms': {'NerfMLP_0/Dense_0': torch.tensor(2.0)}}
  arrays = {'params': big, 'half': torch.ones(5, 3, dtype=torch.bfloat16), 'rng': torch.tensor([-7, 2**31 - 1], dtype=torch.int32),
            'step': 25, 'dbl': np.array([1.0 + 2.0**-40]), **bench._flatten('stats', stats, {})}
  a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
  bench.dump_outputs(a, arrays)
  bench.dump_outputs(b, arrays)
  names = sorted(os.listdir(a))
  assert names == ['dbl.npy', 'half.npy', 'params.npy', 'rng.npy', 'stats.grad_norms.NerfMLP_0.Dense_0.npy', 'stats.loss.npy',
                   'stats.losses.data.npy', 'step.npy']
  for n in names:
    x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
    assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), n
  p = np.load(os.path.join(a, 'params.npy'))
  # the sample: DUMP_CAP values of the array itself at sorted, seeded flat indices (arange: value == index)
  idx = np.sort(np.random.default_rng(0).integers(0, big.numel(), bench.DUMP_CAP))
  assert p.dtype == np.float32 and p.shape == (bench.DUMP_CAP,) and np.array_equal(p, idx.astype(np.float32))
  assert np.load(os.path.join(a, 'half.npy')).shape == (5, 3)
  r = np.load(os.path.join(a, 'rng.npy'))
  assert r.dtype == np.float64 and r.tolist() == [-7.0, 2.0**31 - 1]           # integers exactly
  assert np.load(os.path.join(a, 'dbl.npy'))[0] == 1.0 + 2.0**-40              # doubles are not rounded to float32
  assert float(np.load(os.path.join(a, 'step.npy'))) == 25.0
  assert sum(os.path.getsize(os.path.join(a, n)) for n in names) <= 64 << 20


def test_dump_outputs_refuses_more_than_64_mb(tmp_path):
  import bench
  assert bench.DUMP_LIMIT == 64 << 20
  one = torch.zeros(bench.DUMP_CAP)
  with pytest.raises(AssertionError):
    bench.dump_outputs(str(tmp_path / 'c'), {f'a{i}': one for i in range(bench.DUMP_LIMIT // (4 * bench.DUMP_CAP) + 1)})
