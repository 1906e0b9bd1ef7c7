"""nerf_hugs_amd.hugs.SamPointDecoder (csrc/hugs_samdecode.hip) and SfmAccumulator.add_lowres / add_points against the float64
restatement in tests/sam_decoder_ref.py.  Weights come from a seeded generator; nothing is downloaded.

test_predict: the HIP path may differ from float64 by at most 4x what the same restatement in float32 on the CPU differs by (a
different fp32 summation order through ~10 chained reductions).  Measured on an MI355X, max abs error (CPU float32 | HIP):
  (1,1) lowres 4.02e-6 | 3.86e-6, iou 3.66e-7 | 2.17e-7      (3,1) lowres 4.51e-6 | 3.95e-6, iou 3.71e-7 | 5.95e-7
  (2,3) lowres 4.65e-6 | 4.11e-6, iou 7.55e-7 | 5.17e-7      (9,1) lowres 5.28e-6 | 4.19e-6, iou 7.61e-7 | 5.22e-7
("SAM point decoder"); the test prints both numbers for every case."""
import pytest
import torch

from tests import sam_decoder_ref as R

pytestmark = pytest.mark.gpu

SIZE = (300, 200)      # (H, W) of the image the prompts of test_predict live in


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
  from nerf_hugs_amd import hugs
  w = R.make_weights(0)
  path = tmp_path_factory.mktemp('sam') / 'sam_random.pth'
  torch.save(w, path)
  emb = torch.randn(256, 64, 64, generator=torch.Generator().manual_seed(1))
  dec = hugs.SamPointDecoder.from_checkpoint(str(path)).set_image(emb.cuda(), SIZE)
  return w, {k: v.double() for k, v in w.items()}, emb, dec


def _prompts(n, p, size, seed):
  g = torch.Generator().manual_seed(seed)
  pts = torch.rand(n, p, 2, generator=g) * torch.tensor([size[1], size[0]], dtype=torch.float32)
  return pts, torch.randint(0, 2, (n, p), generator=g, dtype=torch.int32)


# a single prompt; an odd count at the HuGS default P; T = 9 tokens; one prompt more than the kernels' chunk of 8
@pytest.mark.parametrize('n,p', [(1, 1), (3, 1), (2, 3), (9, 1)])
def test_predict(setup, n, p):
  w32, w64, emb, dec = setup
  pts, labels = _prompts(n, p, SIZE, 10 * n + p)
  h_in, w_in = R.input_size(*SIZE)
  coords = pts * torch.tensor([w_in / SIZE[1], h_in / SIZE[0]], dtype=torch.float32)      # apply_coords, as predict does it
  ref = R.decode(w64, emb, coords, labels)
  cpu = R.decode(w32, emb, coords, labels)
  got = dec.predict(pts.cuda(), labels.cuda())
  for name, r, c, g in zip(('lowres', 'iou'), ref, cpu, got):
    assert g.shape == r.shape and g.dtype == torch.float32
    e_cpu, e_hip = float((c.double() - r).abs().max()), float((g.cpu().double() - r).abs().max())
    print(f'{name} N={n} P={p}: |ref| max {float(r.abs().max()):.3g}, CPU float32 err {e_cpu:.3e}, HIP err {e_hip:.3e}')
    assert e_hip <= 4 * e_cpu, (name, e_hip, e_cpu)


def test_missing_keys_are_listed(setup):
  from nerf_hugs_amd import hugs
  w = dict(setup[0])
  del w['mask_decoder.iou_token.weight']
  with pytest.raises(ValueError, match='iou_token'):
    hugs.SamPointDecoder(w)


def _smooth_lowres(n, seed):
  """[n,3,256,256] float32 logits within +-4: 4 tanh(sharpness x two low-frequency waves); every fifth mask has soft edges (a
  wide band between thr - off and thr + off: unstable), the others sharp ones."""
  g = torch.Generator().manual_seed(seed)
  y, x = torch.meshgrid(torch.arange(256.) / 256, torch.arange(256.) / 256, indexing='ij')
  f = torch.rand(n, 3, 2, 2, 1, 1, generator=g) * 1.5 + 0.3
  ph = torch.rand(n, 3, 2, 1, 1, generator=g) * 6.28
  sharp = torch.where(torch.arange(3 * n) % 5 == 2, 1.5, 30.).reshape(n, 3, 1, 1)
  return (4 * torch.tanh(sharp * torch.sin(6.28 * (f[:, :, :, 0] * y + f[:, :, :, 1] * x) + ph).sum(2))).contiguous()


IOU = torch.tensor([[0.95, 0.60, 0.90], [0.70, 0.75, 0.30], [0.85, 0.99, 0.99], [0.50, 0.93, 0.10], [0.97, 0.20, 0.96]])


@pytest.mark.parametrize('highest', [True, False])
@pytest.mark.parametrize('size,in_size', [((37, 53), (715, 1024)), ((300, 200), (1024, 683))])
def test_add_lowres(size, in_size, highest):
  from nerf_hugs_amd import hugs
  assert R.input_size(*size) == in_size
  c = hugs.SegmentConfig(sfm_use_highest_iou=highest)
  lowres, thr, off = _smooth_lowres(len(IOU), 1), 0., c.sfm_stability_score_offset
  full = R.postprocess(lowres.double(), in_size, size)                    # [N,3,H,W] float64
  if highest:
    sel = torch.argmax(IOU, -1)
    logits, iou = full[torch.arange(len(IOU)), sel], IOU[torch.arange(len(IOU)), sel]
  else:
    logits, iou = full.flatten(0, 1), IOU.flatten()
  stab = (logits > thr + off).sum((-1, -2)) / (logits > thr - off).sum((-1, -2))
  assert (iou - c.sfm_pred_iou_thresh).abs().min() >= 0.01 and (stab - c.sfm_stability_score_thresh).abs().min() >= 0.01
  keep = (iou > c.sfm_pred_iou_thresh) & (stab >= c.sfm_stability_score_thresh)
  assert keep.any() and not keep.all() and (stab[iou > c.sfm_pred_iou_thresh] < c.sfm_stability_score_thresh).any()
  count = (logits[keep] > thr).sum(0)
  near = torch.stack([(logits - t).abs() < 1e-4 for t in (thr, thr + off, thr - off)]).any(0).any(0)
  assert float(near.float().mean()) < 0.01
  acc = hugs.SfmAccumulator(*size, config=c).add_lowres(lowres.cuda(), IOU.cuda(), in_size, thr)
  assert torch.equal(acc.kept[0].cpu().bool(), keep)
  assert torch.equal(acc.count.cpu()[~near].long(), count[~near])


def test_add_points_is_predict_then_add_lowres(setup):
  from nerf_hugs_amd import hugs
  _, _, emb, _ = setup
  size = (48, 64)
  w = R.make_weights(0)
  dec = hugs.SamPointDecoder(w).set_image(emb.cuda(), size)
  # (random weights draw soft-edged masks that no stability threshold keeps: that rule is off here, the IoU rule at its default)
  c = hugs.SegmentConfig(sfm_seg_batch_size=2, sfm_stability_score_thresh=0.)
  pts = _prompts(5, 1, size, 3)[0].cuda()
  a = hugs.SfmAccumulator(*size, config=c).add_points(dec, pts)
  b = hugs.SfmAccumulator(*size, config=c)
  for i in range(0, 5, 2):
    b.add_lowres(*dec.predict(pts[i:i + 2]), dec.input_size)
  assert [len(k) for k in a.kept] == [2, 2, 1] and int(a.count.sum()) > 0
  assert torch.equal(a.count, b.count) and all(torch.equal(x, y) for x, y in zip(a.kept, b.kept))
