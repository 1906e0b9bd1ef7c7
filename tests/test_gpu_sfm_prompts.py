"""nerf_hugs_amd.hugs' SfM prompt selection (csrc/hugs_sfmpoints.hip) against HuGS/generate_static_mask.py:81-107, :293-336 restated
in numpy float64 / plain torch on the CPU.  Decisions are compared exactly (kept index lists, neighbour indices); every case first
asserts, on the CPU, that no distance lies within 1e-4 relative of a decision, so a last-bit difference of torch's own CPU kernels
cannot matter."""
import numpy as np
import pytest
import torch

from tests.test_cpu_sfm_colmap import write_model

pytestmark = pytest.mark.gpu
MARGIN = 1e-4


def _observations(m, seed=0):
  """COLMAP-like: camera 840 x 1297 -> image 415 x 640 (factors 0.494..., no integer), some keypoints outside the camera frame on
  every side, a fifth without a 3-D point, track lengths 2..9."""
  rng = np.random.default_rng(seed)
  xys = rng.uniform([-150, -100], [1450, 940], (m, 2))
  track_len = np.where(rng.random(m) < 0.2, -1, rng.integers(2, 10, m)).astype(np.int32)
  return xys, track_len, (840, 1297), (415, 640)


def _ref_filter(xys, track_len, cam, size, thr):
  (cam_h, cam_w), (h, w) = cam, size
  pts = [[np.clip(xy[0] * (w / cam_w), 0, w), np.clip(xy[1] * (h / cam_h), 0, h)]
         for xy, t in zip(xys, track_len) if thr == 0 or (t != -1 and t >= thr)]
  return torch.tensor(pts, dtype=torch.float32).reshape(-1, 2)


@pytest.mark.parametrize('thr', [0, 5])
@pytest.mark.parametrize('m', [1, 257, 1000])
def test_filter(m, thr):
  from nerf_hugs_amd import hugs
  xys, track_len, cam, size = _observations(m, seed=m)
  if m == 1:
    xys, track_len = np.array([[1300., -2.]]), np.array([7], np.int32)
  ref = _ref_filter(xys, track_len, cam, size, thr)
  if m > 1:
    assert (ref[:, 0] == 0).any() and (ref[:, 0] == size[1]).any() and (ref[:, 1] == 0).any() and (ref[:, 1] == size[0]).any()
    assert (thr == 0) == (len(ref) == m)
  got = hugs.sfm_feature_points(xys, track_len, cam, size, thr)
  assert got.dtype == torch.float32 and got.is_cuda and torch.equal(got.cpu(), ref)      # bit for bit


def _pairwise(p):
  p = p.double()
  return torch.linalg.norm(p[:, None] - p[None], dim=-1)


def _ref_same(p, thr=0.1):
  """:88-94 as the loop it is, in float64."""
  p, kept = p.double().numpy(), [0]
  for i in range(1, len(p)):
    if np.sqrt(((p[i] - p[kept])**2).sum(-1)).min() >= thr:
      kept.append(i)
  return kept


def _same_case(n):
  if n == 'chain':      # dependency depth n: only the index-order walk finishes it
    return torch.stack([torch.arange(300) * 0.06 + 3, torch.full((300,), 7.)], -1).float()
  rng = np.random.default_rng(n)
  base = rng.uniform(0, 400, (n, 2)).astype(np.float32)
  p = base[np.repeat(np.arange(n), rng.integers(1, 5, n))[:n]]      # each distinct point 1-4 times
  return torch.from_numpy(p[rng.permutation(n)] if n > 1 else p)


@pytest.mark.parametrize('n', [1, 2, 64, 65, 1030, 'chain'])
def test_delete_same_points(n):
  from nerf_hugs_amd import hugs
  p = _same_case(n)
  d = _pairwise(p)
  assert ((d - 0.1).abs() > MARGIN * 0.1).all()
  ref = _ref_same(p)
  stats = {}
  kept, index = hugs.delete_same_points(p.cuda(), stats=stats)
  assert index.dtype == torch.int32 and index.cpu().tolist() == ref and torch.equal(kept.cpu(), p[ref])
  if n == 'chain':
    assert ref == list(range(0, 300, 2)) and stats['walked'] > 0
  elif n != 1:
    assert len(ref) < len(p) and stats['walked'] == 0 and stats['rounds'] <= 4


def _outlier_case(n):
  g = torch.Generator().manual_seed(n)
  far = torch.tensor([[500., 500.], [-400., 300.], [900., -700.]])[:max(1, min(3, n - 2))]
  p = torch.cat([torch.randn(n - len(far), 2, generator=g) * 5 + 50, far])
  return p[torch.randperm(n, generator=g)].contiguous()


@pytest.mark.parametrize('n', [2, 3, 130, 1025])
def test_delete_outlier_points(n):
  from nerf_hugs_amd import hugs
  p = _outlier_case(n)
  d = _pairwise(p)[~torch.eye(n, dtype=torch.bool)].reshape(n, n - 1)      # :103-106 in float64
  thr, mins = d.mean() + 3.0 * d.std(), d.min(-1).values
  if n == 2:
    ref = []                                                              # std = 0, mean = d, d < d is false
  else:
    assert ((mins - thr).abs() > MARGIN * thr).all()
    ref = torch.nonzero(mins < thr).flatten().tolist()
    assert n < 100 or 0 < n - len(ref) <= 3
  kept, index = hugs.delete_outlier_points(p.cuda())
  assert index.cpu().tolist() == ref and torch.equal(kept.cpu(), p[ref].reshape(-1, 2))
  again = hugs.delete_outlier_points(p.cuda())
  assert torch.equal(again[0], kept) and torch.equal(again[1], index)
  one = p[:1].cuda()
  assert torch.equal(hugs.delete_outlier_points(one)[0], one)             # n < 2: unchanged


def _nearest_case(n, k):
  """Uniform points, redrawn where a row's k + 1 smallest distances come closer than the margin."""
  g = torch.Generator().manual_seed(100 * n + k)
  p = torch.rand(n, 2, generator=g) * 1000
  for _ in range(20):
    d, order = _pairwise(p).sort(dim=-1, stable=True)
    head = d[:, :min(k + 1, n)]
    bad = ((head[:, 1:] - head[:, :-1]) <= MARGIN * head[:, 1:]).any(-1)
    if not bad.any():
      return p, order[:, :min(k, n)]
    p[bad] = torch.rand(int(bad.sum()), 2, generator=g) * 1000
  raise AssertionError('no draw with separated distances')


@pytest.mark.parametrize('n,k', [(5, 2), (5, 8), (300, 3), (1025, 8), (70, 32)])
def test_nearest_points(n, k):
  from nerf_hugs_amd import hugs
  p, ref = _nearest_case(n, k)
  out, index = hugs.nearest_points(p.cuda(), k, return_index=True)
  assert tuple(out.shape) == (n, min(k, n), 2) and out.dtype == torch.float32
  assert torch.equal(index.cpu().long(), ref) and torch.equal(out.cpu(), p[ref])
  assert torch.equal(hugs.nearest_points(p.cuda(), k), out)


def test_nearest_points_refuses_k_over_32():
  from nerf_hugs_amd import hugs
  with pytest.raises(ValueError):
    hugs.nearest_points(torch.zeros(40, 2, device='cuda'), 33)


@pytest.mark.parametrize('outliers', [False, True])
@pytest.mark.parametrize('per_mask', [1, 3])
def test_select_sfm_prompts(per_mask, outliers):
  from nerf_hugs_amd import hugs
  xys, track_len, cam, size = _observations(600, seed=5)
  xys[300:] = xys[:300]                                  # the same keypoint twice, as COLMAP lists it per orientation
  cfg = hugs.SegmentConfig(sfm_delete_outlier_points=outliers, sfm_points_per_mask=per_mask)
  ref = hugs.delete_same_points(hugs.sfm_feature_points(xys, track_len, cam, size, 5))[0]
  assert 0 < len(ref) < 300
  if outliers:
    ref = hugs.delete_outlier_points(ref)[0]
  ref = hugs.nearest_points(ref, 3) if per_mask > 1 else ref[:, None]
  got = hugs.select_sfm_prompts(xys, track_len, cam, size, cfg)
  assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (len(ref), per_mask, 2) and torch.equal(got, ref)


def test_select_sfm_prompts_edges(tmp_path):
  from nerf_hugs_amd import hugs
  xys, track_len, cam, size = _observations(100, seed=6)
  none = hugs.select_sfm_prompts(xys, track_len, cam, size, hugs.SegmentConfig(sfm_point_count_threshold=10))
  assert tuple(none.shape) == (0, 1, 2) and none.dtype == torch.float32
  with pytest.raises(ValueError, match='cluster'):
    hugs.select_sfm_prompts(xys, track_len, cam, size, hugs.SegmentConfig(sfm_cluster_num=2))
  some = hugs.select_sfm_prompts(xys, track_len, cam, size, hugs.SegmentConfig(sfm_cluster_num=10**6))      # >= n: disabled (:319)
  assert some.shape[0] > 2 and tuple(some.shape[1:]) == (1, 2)
  # COLMAP files -> prompts: image c_002 of the written model keeps the observations with tracks 5, 6 and 9
  cfg = hugs.SegmentConfig(sfm_points_per_mask=2)
  got = hugs.sfm_prompts_from_colmap(str(write_model(tmp_path)), 'c_002', (420, 640), cfg)
  ref = hugs.select_sfm_prompts(*hugs.sfm_observations(str(tmp_path), 'c_002'), (420, 640), cfg)
  assert tuple(got.shape) == (3, 2, 2) and torch.equal(got, ref)
  assert torch.equal(got[:, 0].cpu(), _ref_filter(np.array([[1., 2.], [7., 8.], [9., 10.]]), [5, 6, 9], (840, 1297), (420, 640), 5))
