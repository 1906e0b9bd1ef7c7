"""nerf_hugs_amd.hugs.SamMaskGenerator / MaskSet (csrc/hugs_samamg.hip) against the restatement in tests/sam_amg_ref.py: the five
stages one by one, then generate() against the stages called by hand."""
import numpy as np
import pytest
import torch

from tests import sam_amg_ref as A
from tests import sam_decoder_ref, sam_encoder_ref
from tests.test_gpu_sam_decoder import IOU

pytestmark = pytest.mark.gpu


def _blobs(seed=1):
  """[5,3,256,256] elliptical blobs 4 tanh(sharp (1 - d)); every fifth candidate has soft edges (unstable)."""
  g = torch.Generator().manual_seed(seed)
  c = torch.rand(5, 3, 2, 1, 1, generator=g) * 0.6 + 0.05
  r = torch.rand(5, 3, 2, 1, 1, generator=g) * 0.12 + 0.04
  y, x = torch.meshgrid(torch.arange(256.) / 256, torch.arange(256.) / 256, indexing='ij')
  d = (((y - c[:, :, 0]) / r[:, :, 0])**2 + ((x - c[:, :, 1]) / r[:, :, 1])**2).sqrt()
  sharp = torch.where(torch.arange(15) % 5 == 2, 1.5, 30.).reshape(5, 3, 1, 1)
  return (4 * torch.tanh(sharp * (1 - d))).contiguous()


# whole images (W under a word; several words, rows ending mid-word); an inner crop at an odd bit offset whose four sides lie
# away from the image's, so the crop-edge rule fires
@pytest.mark.parametrize('size,box', [((37, 53), (0, 0, 53, 37)), ((300, 200), (0, 0, 200, 300)), ((300, 200), (30, 40, 170, 260))])
def test_candidates(size, box):
  from nerf_hugs_amd import hugs
  cfg = hugs.SamAmgConfig()
  lowres, pts = _blobs(), torch.rand(5, 2, generator=torch.Generator().manual_seed(2)) * torch.tensor([box[2] - box[0], box[3] - box[1]])
  ref, lo, hi = (A.candidates(lowres, IOU, pts, box, size, cfg.pred_iou_thresh, cfg.stability_score_thresh, shift=s) for s in (0., -1e-4, 1e-4))
  keep, scanned = ref['keep'], ref['iou_ok']
  assert (IOU.flatten() - cfg.pred_iou_thresh).abs().min() >= 0.01
  assert (ref['stability'][scanned] - cfg.stability_score_thresh).abs().min() >= 0.01
  assert keep.any() and not keep.all()
  if box[0] > 0:      # each rule alone rejects a candidate the other two pass
    ok = [ref['iou_ok'], ref['stab_ok'], ref['edge_ok']]
    assert all((~ok[i] & ok[i - 1] & ok[i - 2]).any() for i in range(3))
  assert torch.equal(lo['boxes'][keep], ref['boxes'][keep]) and torch.equal(hi['boxes'][keep], ref['boxes'][keep])
  near = ((ref['logits'][scanned, None] - torch.tensor([0., 1., -1.]).reshape(1, 3, 1, 1)).abs() < 1e-4).any(1)      # [scanned, ch, cw]
  assert float(near.float().mean()) < 0.01
  near_full = torch.zeros((int(scanned.sum()), *size), dtype=torch.bool)
  near_full[:, box[1]:box[3], box[0]:box[2]] = near
  near_kept = near_full[keep[scanned]]
  ms = hugs.MaskSet(*size)
  n = hugs.SamMaskGenerator(None, None, cfg).add_candidates(ms, lowres.cuda(), IOU.cuda(), pts.cuda(), box)
  assert n == len(ms) == int(keep.sum())                                   # the keep flags: slots in candidate order carry ...
  assert torch.equal(ms.boxes.cpu().long(), ref['boxes'][keep])            # ... each kept candidate's own box,
  assert torch.equal(ms.points.cpu(), ref['points'][keep])                 # point,
  assert torch.equal(ms.iou.cpu(), IOU.flatten()[keep])                    # and IoU
  assert torch.equal(ms.crop_boxes.cpu().long(), torch.tensor(box).expand(n, 4))
  assert float((ms.stability.cpu().double() - ref['stability'][keep]).abs().max()) < 0.01
  got = ms.to_masks().cpu()
  assert torch.equal(got[~near_kept], ref['masks'][keep][~near_kept])
  assert bool(((ms.area.cpu() - ref['area'][keep]).abs() <= near_kept.sum((-1, -2))).all())
  assert torch.equal(ms.area.cpu().long(), got.sum((-1, -2)))


# a single box, a full tile of 64, one past it, several tiles; two or three distinct scores
@pytest.mark.parametrize('k,levels', [(1, 2), (64, 2), (65, 3), (200, 3)])
def test_nms(k, levels):
  from nerf_hugs_amd import hugs
  g = torch.Generator().manual_seed(k)
  xy, wh = torch.randint(0, 150, (k, 2), generator=g), torch.randint(1, 60, (k, 2), generator=g)
  boxes = torch.cat([xy, xy + wh], 1).int()
  scores = torch.randint(0, levels, (k,), generator=g).float() / 4
  ref = A.nms(boxes, scores, 0.3)
  assert k == 1 or 1 < len(ref) < k
  rank, order = hugs.stable_rank(scores.cuda())
  assert order.tolist() == torch.sort(scores, descending=True, stable=True).indices.tolist() and rank[order.long()].tolist() == list(range(k))
  keep, count = hugs.box_nms(boxes.cuda(), scores.cuda(), 0.3)
  assert keep[:int(count)].tolist() == ref
  assert hugs.stable_rank((scores * 4).int().cuda())[1].tolist() == order.tolist()      # the int32 keys


def _region_masks(h, w):
  """Hand-built masks on an h x w canvas, anchored at its far corner so a row of (64, 129) ends mid-word."""
  m = torch.zeros((8, h, w), dtype=torch.bool)
  y, x = h - 32, w - 40
  m[0, y:y + 30, x:x + 38] = True                                  # 7 x 7 = 49 hole (filled), 5 x 10 = 50 hole (kept)
  m[0, y + 3:y + 10, x + 3:x + 10] = False
  m[0, y + 15:y + 20, x + 20:x + 30] = False
  m[1, y:y + 12, x:x + 12] = True                                  # a hole joined to the outside only through a diagonal
  m[1, y + 1:y + 5, x + 1:x + 5] = False
  m[1, y, x] = False
  m[2, 2:12, 2:12] = True                                          # 100; a 49 island (removed) and a 50 island (kept)
  m[2, 20:27, 2:9] = True
  m[2, y + 20:y + 25, x:x + 10] = True
  m[3, 5:15, 5:15] = True                                          # a 1-pixel island on a diagonal bridge: one component, kept
  m[3, 15, 15] = True
  m[4, 1:4, 1:5], m[4, 10:14, 20:23], m[4, y:y + 2, x:x + 3] = True, True, True      # only small islands: 12, 12, 6 -> the first
  m[5, 8:20, 30:50] = True                                         # untouched
  m[6, 0:12, w - 14:w] = True                                      # a small hole on the image border
  m[6, 0:3, w - 8:w - 4] = False
  m[7, :, 1:6] = True                                              # the outside left of a full-height band is h < 50 pixels
  return m


@pytest.mark.parametrize('size', [(40, 70), (64, 129)])
def test_small_regions(size):
  from nerf_hugs_amd import hugs
  masks = _region_masks(*size)
  clean, changed, keep = A.postprocess_small_regions(masks, 50, 0.7)
  assert changed.tolist() == [1, 0, 1, 0, 1, 0, 1, int(size[0] < 50)] and int(clean[4].sum()) == 12 and bool(clean[4, 1, 1])
  ms = hugs.MaskSet.from_masks(masks.cuda())
  assert torch.equal(ms.boxes.cpu().long(), A.mask_boxes(masks)) and torch.equal(ms.to_masks().cpu(), masks)
  got, got_changed = ms.clean_small_regions(50, max_bytes=3 * 8 * (size[0] * size[1] + 6))      # chunks of three masks
  assert torch.equal(got.to_masks().cpu(), clean) and got_changed.tolist() == changed.tolist()
  assert torch.equal(got.boxes.cpu().long(), A.mask_boxes(clean)) and torch.equal(got.area.cpu().long(), clean.sum((-1, -2)))
  assert ms.remove_small_regions(50, 0.7).tolist() == keep
  final = torch.where(changed[keep].bool()[:, None, None], clean[keep], masks[keep])
  assert torch.equal(ms.to_masks().cpu(), final) and torch.equal(ms.boxes.cpu().long(), A.mask_boxes(final))


@pytest.mark.parametrize('size', [(37, 53), (64, 129)])
def test_paint(size):
  from nerf_hugs_amd import hugs
  h, w = size
  m = torch.zeros((5, h, w), dtype=torch.bool)
  m[0, 2:20, 3:30], m[1, 10:16, 10:22], m[2, 12:18, 16:28] = True, True, True      # 1 and 2: equal areas, overlapping each other and 0
  m[3, 5:h, w - 20:w], m[4, 0:4, 0:w] = True, True                                  # up to the last column; a full-width strip
  seg_ref, s_ref = A.paint(m)
  assert int(m[1].sum()) == int(m[2].sum()) and bool((seg_ref < 0).any())
  seg, s = hugs.MaskSet.from_masks(m.cuda()).label_map()
  assert s == s_ref and seg.dtype == torch.int32 and torch.equal(seg.cpu(), seg_ref)
  g = torch.Generator().manual_seed(0)
  out = hugs.generate_static_mask(torch.rand(h, w, 3, generator=g).cuda(), torch.rand(h, w, 3, generator=g).cuda(), seg, num_segments=s)
  assert tuple(out['static_mask'].shape) == size and int(out['labels'].max()) >= s


def _same(a, b):
  return len(a) == len(b) and all(torch.equal(getattr(a, f), getattr(b, f)) for f in a.FIELDS)


def test_generate_is_the_stages_in_order():
  from nerf_hugs_amd import hugs
  size = (30, 36)      # (every crop side lies within 20 pixels of an image side: the crop-edge rule, which drops the crop-filling masks
                       # random weights draw from every inner crop of a larger image, never fires; test_candidates covers it)
  w = {**sam_encoder_ref.make_weights(128, 2, 2, (1,), seed=128), **sam_decoder_ref.make_weights(0)}
  image = torch.randint(0, 256, (*size, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).numpy()
  resize = lambda crop, hw: np.asarray(torch.nn.functional.interpolate(torch.from_numpy(crop.copy()).permute(2, 0, 1)[None].float(), hw,
                                                                       mode='bilinear')[0].permute(1, 2, 0).round().byte())
  boxes, layers = hugs.amg_crop_boxes(size, 1, 512 / 1500)
  assert boxes == [[0, 0, 36, 30], [0, 0, 23, 20], [0, 10, 23, 30], [13, 0, 36, 20], [13, 10, 36, 30]] and layers == [0, 1, 1, 1, 1]
  grids = hugs.amg_point_grids(4, 1, 2)
  assert [g.shape for g in grids] == [(16, 2), (4, 2)] and grids[1].tolist() == [[.25, .25], [.75, .25], [.25, .75], [.75, .75]]
  # the IoU threshold: the middle of the widest gap in the middle half of the CPU reference's predictions for the whole image
  in_size = sam_decoder_ref.input_size(*size)
  emb = sam_encoder_ref.encode(w, torch.from_numpy(resize(image, in_size)))
  pts0 = torch.from_numpy(grids[0] * [[size[1], size[0]]]).float()
  coords = pts0 * torch.tensor([in_size[1] / size[1], in_size[0] / size[0]])
  iou = sam_decoder_ref.decode(w, emb, coords[:, None], torch.ones(16, 1, dtype=torch.int32))[1].flatten().sort().values
  gap = (iou[13:37] - iou[12:36])
  thr = float((iou[12:36] + gap / 2)[gap.argmax()])
  print(f'IoU predictions {float(iou[0]):.4f} .. {float(iou[-1]):.4f}, threshold {thr:.5f} in a gap of {float(gap.max()):.2e}')
  assert float(gap.max()) > 1e-4
  cfg = hugs.SamAmgConfig(points_per_side=4, points_per_batch=6, stability_score_thresh=0., pred_iou_thresh=thr, min_mask_region_area=20)
  gen = hugs.SamMaskGenerator(hugs.SamImageEncoder(w), hugs.SamPointDecoder(w), cfg, resize)
  got = gen.generate(image)
  by_hand, per_crop = hugs.MaskSet(*size), []
  for box, layer in zip(boxes, layers):
    x0, y0, x1, y1 = box
    crop = image[y0:y1, x0:x1]
    gen.decoder.set_image_from(gen.encoder, torch.from_numpy(resize(crop, sam_decoder_ref.input_size(y1 - y0, x1 - x0))).cuda(), (y1 - y0, x1 - x0))
    pts, start, scanned = torch.from_numpy(grids[layer] * [[x1 - x0, y1 - y0]]).float().cuda(), len(by_hand), 0
    for i in range(0, len(pts), 6):
      scanned += gen.add_candidates(by_hand, *gen.decoder.predict(pts[i:i + 6, None]), pts[i:i + 6], box)
    by_hand.nms(by_hand.iou[start:], cfg.box_nms_thresh, start)
    per_crop.append((scanned, len(by_hand) - start))
  print('candidates kept / after NMS per crop:', per_crop)
  crops = by_hand.crop_boxes.clone()
  by_hand.nms(1. / ((crops[:, 2] - crops[:, 0]) * (crops[:, 3] - crops[:, 1])).float(), cfg.crop_nms_thresh)
  n_cross = len(by_hand)
  by_hand.remove_small_regions(20, 0.7)
  print(f'{len(crops)} masks after the crops, {n_cross} after the cross-crop NMS, {len(by_hand)} after the clean-up')
  assert 0 < per_crop[0][0] < 48 and sum(n > 0 for _, n in per_crop) >= 2
  assert len(torch.unique(by_hand.crop_boxes, dim=0)) >= 2
  assert _same(got, by_hand)
  seg, s = got.label_map()
  assert s == len(got) and int(seg.max()) == s - 1
