"""nerf_hugs_amd.hugs (csrc/hugs_staticmask.hip) against plain restatements of HuGS/generate_static_mask.py:110-145,239-275,344-407
in numpy float64 / CPU torch, written out below.  Shapes and the seams they cross:
  37x53    smaller than every tile (64x16 labelling, 64x32 box, 256-pixel logit chunk) in at least one direction, odd extents, H*W odd
           (the scalar logit loads);
  130x257  several tiles / workgroups in both directions with ragged right and bottom edges; H*W = 2 mod 4 (scalar loads again);
  40x52    H*W a multiple of 4 but not of 256: the 16-byte logit loads with a ragged last chunk (SfM test only)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(37, 53), (130, 257)]
ULP = lambda t: float(np.spacing(np.float32(t)))


def _box(m, k, mode):
  """k x k box sums of a 0/1 map, padded by reflection ('reflect'), zeros (0) or ones (1)."""
  p = np.pad(m, k // 2, mode='reflect') if mode == 'reflect' else np.pad(m, k // 2, constant_values=mode)
  return np.lib.stride_tricks.sliding_window_view(p, (k, k)).sum((-1, -2))


def fill_gap_ref(m, k, mode='reflect'):      # :110-125 (mode 0: the smoothing of :391-397)
  k += k % 2 == 0
  return ((_box(m, k, mode) / k**2 + m) >= 0.5).astype(np.float64)


def erode_ref(m, k):                         # :400-407: the minimum over the window, the border never erodes
  return (_box(m, k, 1) == k * k).astype(np.float64)


def labels_ref(seg, S):
  """:243-259 as written (sequential, whole-image rewrite on a merge), then each new label renamed S + its smallest pixel index."""
  a = seg.astype(np.int64).copy()
  H, W = a.shape
  index = S
  for i, j in zip(*np.nonzero(seg < 0)):     # (row-major, like range(height*width) with the `continue`)
    nb = [a[y, x] for y, x in ((i - 1, j), (i, j - 1), (i - 1, j - 1)) if y >= 0 and x >= 0 and a[y, x] >= S]
    nb = np.unique(nb)
    if len(nb) == 0:
      a[i, j] = index
      index += 1
    else:
      a[i, j] = nb[0]
      for other in nb[1:]:
        a[a == other] = nb[0]
  flat = a.ravel().copy()
  vals, first = np.unique(flat, return_index=True)
  for v, f in zip(vals, first):
    if v >= S:
      flat[a.ravel() == v] = S + f
  return flat.reshape(H, W).astype(np.int32)


def intersect_ref(coarse, labels):           # :128-145, threshold 0.5, fine masks = the label classes
  _, inv = np.unique(labels, return_inverse=True)
  inv = inv.ravel()
  area, inter = np.bincount(inv), np.bincount(inv, coarse.ravel())
  return (inter / area >= 0.5)[inv].reshape(labels.shape).astype(np.float64)


def sfm_ref(logits, iou, c, thr=0.):         # :360-374 with segment_anything's calculate_stability_score, CPU torch
  keep = torch.ones(len(iou), dtype=torch.bool)
  if c.sfm_pred_iou_thresh > 0:
    keep &= iou > c.sfm_pred_iou_thresh
  inter = (logits > (thr + c.sfm_stability_score_offset)).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
  union = (logits > (thr - c.sfm_stability_score_offset)).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
  if c.sfm_stability_score_thresh > 0:
    keep &= (inter / union) >= c.sfm_stability_score_thresh
  return keep.numpy(), (logits[keep] > thr).sum(0).numpy()


@functools.lru_cache(maxsize=None)
def _images(shape, levels=False):
  rng = np.random.default_rng(shape[0])
  if levels:    # residual exactly one of four levels: ties at the order statistics (cum. 0.8 < q = 0.85 < 0.9), mean 0.2 between levels
    v = rng.choice(np.float32([0, .25, .5, .75]), size=shape, p=[.5, .3, .1, .1])
    return np.repeat(v[..., None], 3, -1), np.zeros(shape + (3,), np.float32)
  gt = rng.random(shape + (3,), dtype=np.float32)
  return np.clip(gt + 0.1 * rng.standard_normal(shape + (3,)).astype(np.float32) ** 3, 0, 1), gt


@functools.lru_cache(maxsize=None)
def _seg(shape, kind):
  """(seg, S, labels_ref).  'noise': 55 % uncovered, just above the site-percolation threshold of this neighbourhood, so components
  wind across many tile borders; 'pairs': diagonal pairs (must merge) and anti-diagonal pairs (must not), inside a tile and across
  the tile corner at row 16 / column 64 where the image has one."""
  H, W = shape
  rng = np.random.default_rng(H + 1)
  yy, xx = np.mgrid[:H, :W]
  seg = ((yy // 9) * ((W + 10) // 11) + xx // 11).astype(np.int32)
  S = int(seg.max()) + 1
  if kind == 'noise':
    seg[rng.random(shape) < 0.55] = -1
  elif kind == 'pairs':
    for y, x in [(3, 3), (4, 4), (3, 10), (4, 9), (15, 20), (16, 21), (15, 30), (16, 29), (15, 63), (16, 64), (31, 64), (32, 63)]:
      if x < W:
        seg[y, x] = -1
  elif kind == 'uncovered':
    seg[:] = -1
  return seg, S, labels_ref(seg, S)


@functools.lru_cache(maxsize=None)
def _logits(shape, n):
  """n logit planes a * (g - c): sharp ones (a = 40) are stable, soft ones (a = 0.7) are not; plane 0 is sharp with a high IoU (n = 1:
  one kept), every fourth plane is below every threshold (0 / 0)."""
  rng = np.random.default_rng(n)
  g = torch.from_numpy(_box(rng.standard_normal((shape[0] + 6, shape[1] + 6)), 7, 0)[3:-3, 3:-3] / 7).float()
  a = torch.tensor([40. if i % 3 == 0 else 0.7 for i in range(n)])
  lg = a[:, None, None] * (g[None] - torch.from_numpy(rng.uniform(-1, 1, n)).float()[:, None, None])
  lg[3::4] = -10.
  iou = torch.from_numpy(rng.uniform(0.7, 1., n)).float()
  iou[0] = 0.95
  return lg.contiguous(), iou


@pytest.mark.parametrize('shape,levels,q', [(SHAPES[0], False, 0.93), (SHAPES[1], False, 0.95), (SHAPES[1], True, 0.85)])
def test_residual_masks(shape, levels, q):
  """Residual and thresholds against float64.  Bound: 4 x the error of the same arithmetic in CPU fp32 (torch), and never below half an
  fp32 ulp of the value, which is what storing any result in fp32 costs.  Measured on an MI355X (device / CPU fp32): see
  profiles/staticmask.txt."""
  from nerf_hugs_amd import hugs
  pred, gt = _images(shape, levels)
  res, base, upper, thr = (t.cpu().numpy() for t in hugs.residual_masks(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), q))
  want = np.abs(pred.astype(np.float64) - gt).mean(-1)
  cpu = (torch.from_numpy(pred) - torch.from_numpy(gt)).abs().mean(-1)
  e_cpu, e_dev = np.abs(cpu.numpy() - want).max(), np.abs(res - want).max()
  print(f'{shape} residual: max err device {e_dev:.3e}, CPU fp32 {e_cpu:.3e}')
  assert e_dev <= 4 * max(e_cpu, ULP(want.max()) / 2)
  r64, r32 = res.astype(np.float64), torch.from_numpy(res)
  for i, (t_ref, t_cpu) in enumerate([(r64.mean(), float(r32.mean())), (np.quantile(r64, q), float(torch.quantile(r32.flatten(), q)))]):
    tol = 4 * max(abs(t_cpu - t_ref), ULP(t_ref) / 2)
    print(f'{shape} threshold {i}: ref {t_ref:.9f} device err {abs(thr[i] - t_ref):.3e}, CPU fp32 err {abs(t_cpu - t_ref):.3e}')
    assert abs(thr[i] - t_ref) <= tol
    if not levels:
      assert np.count_nonzero(np.abs(r64 - t_ref) <= tol) == 0, 'a pixel sits within the tolerance of a threshold: change the seed'
  t_base, t_upper = r64.mean(), np.quantile(r64, q)
  assert np.array_equal(base, r64 <= t_base) and np.array_equal(upper, (r64 <= t_base) | (r64 <= t_upper))
  if levels:
    assert t_upper in (0.5, 0.75) and 0 < base.mean() < upper.mean() < 1


@pytest.mark.parametrize('shape', SHAPES + [(40, 52)])
def test_sfm_accumulate(shape):
  """N = 1 (one kept), 5 (all dropped: low IoU, unstable or empty), 67 (mixed, past one 64-mask word); then 5 + 67 as two batches."""
  from nerf_hugs_amd import hugs
  cfg = hugs.SegmentConfig()
  total = np.zeros(shape, np.int64)
  both = hugs.SfmAccumulator(*shape)
  for n in (1, 5, 67):
    lg, iou = _logits(shape, n)
    if n == 5:
      iou = torch.minimum(iou, torch.tensor([0.5, 1., 1., 1., 0.5]))      # planes 0 and 4 fail on IoU, 1 and 2 are soft, 3 is empty
    keep, count = sfm_ref(lg, iou, cfg)
    assert keep.sum() == {1: 1, 5: 0}.get(n, keep.sum()) and (n < 67 or 0 < keep.sum() < n)
    acc = hugs.SfmAccumulator(*shape).add(lg.cuda(), iou.cuda())
    assert np.array_equal(acc.kept[0].cpu().numpy(), keep) and np.array_equal(acc.count.cpu().numpy(), count)
    assert np.array_equal(acc.mask().cpu().numpy(), fill_gap_ref((count >= 1).astype(np.float64), 5))
    if n > 1:
      both.add(lg.cuda(), iou.cuda())
      total += count
  assert np.array_equal(both.count.cpu().numpy(), total)
  assert not hugs.SfmAccumulator(*shape).mask().any()


@pytest.mark.parametrize('kind', ['noise', 'pairs', 'covered', 'uncovered'])
@pytest.mark.parametrize('shape', SHAPES)
def test_labels_and_intersect(shape, kind):
  from nerf_hugs_amd import hugs
  seg, S, want = _seg(shape, kind)
  labels = hugs.label_uncovered(torch.from_numpy(seg).cuda(), S)
  assert labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy(), want)
  if kind == 'pairs':                         # S from seg.max() + 1 (the last segment is still visible in this map)
    assert np.array_equal(hugs.label_uncovered(torch.from_numpy(seg).cuda()).cpu().numpy(), want)
  coarse = fill_gap_ref((np.random.default_rng(7).random(shape) < 0.38).astype(np.float64), 3)       # ~half set, clumped
  got = hugs.intersect_masks(torch.from_numpy(coarse).cuda(), labels, S)
  assert np.array_equal(got.cpu().numpy(), intersect_ref(coarse, want))


@pytest.mark.parametrize('shape', SHAPES)
def test_box_stages(shape):
  from nerf_hugs_amd import hugs
  m = (np.random.default_rng(3).random(shape) < 0.45).astype(np.float64)
  m[:, -1] = m[0] = 1                         # set pixels on the borders the paddings differ at
  d = torch.from_numpy(m).cuda()
  for k in (4, 5):
    assert np.array_equal(hugs.fill_gap(d, k).cpu().numpy(), fill_gap_ref(m, k))
  assert np.array_equal(hugs.smooth(d, 7).cpu().numpy(), fill_gap_ref(m, 7, 0))
  dense = fill_gap_ref(m, 5)                  # mostly set: an erosion of the sparse map would be empty
  assert np.array_equal(hugs.erode(torch.from_numpy(dense).cuda(), 5).cpu().numpy(), erode_ref(dense, 5))
  assert 0 < erode_ref(dense, 5).mean() < dense.mean()


def test_refusals():
  from nerf_hugs_amd import hugs
  with pytest.raises(ValueError, match='3 <= H'):
    hugs.fill_gap(torch.zeros(2, 8, device='cuda'))
  hugs.check_image_size(4096, 4096)
  with pytest.raises(ValueError, match='2\\^24'):
    hugs.check_image_size(4097, 4096)
  with pytest.raises(ValueError, match='erode_kernel_size'):
    hugs.erode(torch.zeros(8, 8, device='cuda'), 4)


def test_end_to_end():
  """generate_static_mask = the reference stages composed on the device's residual; a second call is bitwise equal."""
  from nerf_hugs_amd import hugs
  shape, cfg = SHAPES[1], hugs.SegmentConfig()
  pred, gt = _images(shape)
  seg, S, labels = _seg(shape, 'noise')
  lg, iou = _logits(shape, 67)

  def run():
    sfm = hugs.SfmAccumulator(*shape, config=cfg).add(lg.cuda(), iou.cuda())
    return hugs.generate_static_mask(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(seg).cuda(), sfm, cfg)

  out = run()
  assert list(out) == ['residual', 'residual_mask_base', 'residual_mask_upper', 'sfm_mask', 'sfm_residual_mask', 'labels', 'static_mask']
  assert all(torch.equal(a, b) for a, b in zip(out.values(), run().values()))
  got = {k: v.cpu().numpy() for k, v in out.items()}
  r64 = got['residual'].astype(np.float64)
  base = (r64 <= r64.mean()).astype(np.float64)
  upper = np.maximum(base, r64 <= np.quantile(r64, cfg.residual_quantile_upper))
  sfm_mask = fill_gap_ref((sfm_ref(lg, iou, cfg)[1] >= 1).astype(np.float64), 5)
  combined = ((sfm_mask + base) * upper >= 0.5).astype(np.float64)
  static = erode_ref(intersect_ref(fill_gap_ref(combined, cfg.smooth_kernel_size, 0), labels), cfg.erode_kernel_size)
  want = {'residual_mask_base': base, 'residual_mask_upper': upper, 'sfm_mask': sfm_mask, 'sfm_residual_mask': combined, 'labels': labels,
          'static_mask': static}
  for k, v in want.items():
    assert np.array_equal(got[k], v), k
  assert got['static_mask'].dtype == np.float32 and 0 < static.mean() < 1
