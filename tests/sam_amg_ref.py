"""A plain restatement of what segment_anything's SamAutomaticMaskGenerator does around the decoder (amg.py / automatic_mask_generator.py)
and of the painting loop of HuGS/generate_static_mask.py:237-242, in float64 / integer torch.  A helper for
tests/test_gpu_sam_amg.py, not a test."""
import numpy as np
import scipy.ndimage
import torch

from tests import sam_decoder_ref


def mask_boxes(masks):
  """batched_mask_to_box: [K,H,W] bool -> [K,4] (x0, y0, x1, y1), zeros for an empty mask."""
  out = torch.zeros((len(masks), 4), dtype=torch.int64)
  for k, m in enumerate(masks):
    ys, xs = torch.nonzero(m, as_tuple=True)
    if len(ys):
      out[k] = torch.stack([xs.min(), ys.min(), xs.max(), ys.max()])
  return out


def candidates(lowres, iou, points, crop_box, size, iou_thresh, stab_thresh, thr=0., off=1., shift=0.):
  """_process_batch after the decoder, for logits shifted by `shift`.  Returns a dict: the [M] decisions 'iou_ok', 'stab_ok',
  'edge_ok' and 'keep', 'stability', the float64 'logits' [M,ch,cw], and for all M candidates the uncropped 'masks' [M,H,W],
  'boxes', 'points', 'area'."""
  x0, y0, x1, y1 = crop_box
  ch, cw = y1 - y0, x1 - x0
  logits = sam_decoder_ref.postprocess(lowres.double(), sam_decoder_ref.input_size(ch, cw), (ch, cw)).flatten(0, 1) + shift
  iou = iou.flatten()
  stab = (logits > thr + off).sum((-1, -2)) / (logits > thr - off).sum((-1, -2))
  masks = torch.zeros((len(iou), *size), dtype=torch.bool)
  masks[:, y0:y1, x0:x1] = logits > thr
  offset = torch.tensor([x0, y0, x0, y0])
  boxes = mask_boxes(masks[:, y0:y1, x0:x1]) + offset
  near_crop = (boxes - torch.tensor(crop_box)).abs() <= 20
  near_image = (boxes - torch.tensor([0, 0, size[1], size[0]])).abs() <= 20
  d = {'iou_ok': iou > iou_thresh, 'stab_ok': stab >= stab_thresh, 'edge_ok': ~(near_crop & ~near_image).any(1), 'stability': stab,
       'logits': logits, 'masks': masks, 'boxes': boxes, 'area': masks.sum((-1, -2)),
       'points': points.float().repeat_interleave(3, 0) + offset[:2].float()}
  d['keep'] = d['iou_ok'] & d['stab_ok'] & d['edge_ok']
  return d


def nms(boxes, scores, thr):
  """torchvision.ops.nms as a greedy loop over the stable descending score order, float32 like torchvision's kernel."""
  b = boxes.float()
  area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
  order = torch.sort(scores, descending=True, stable=True).indices.tolist()
  keep, dead = [], set()
  for n, i in enumerate(order):
    if i in dead:
      continue
    keep.append(i)
    for j in order[n + 1:]:
      w = (torch.minimum(b[i, 2], b[j, 2]) - torch.maximum(b[i, 0], b[j, 0])).clamp(min=0)
      h = (torch.minimum(b[i, 3], b[j, 3]) - torch.maximum(b[i, 1], b[j, 1])).clamp(min=0)
      if w * h / (area[i] + area[j] - w * h) > thr:
        dead.add(j)
  return keep


def remove_small_regions(mask, min_area, holes):
  """amg.remove_small_regions with scipy's 8-connected labels (numbered by their first pixel in raster order, so argmax takes
  the first of the largest) for cv2.connectedComponentsWithStats."""
  regions, n = scipy.ndimage.label(mask ^ holes, structure=np.ones((3, 3)))
  sizes = np.bincount(regions.ravel(), minlength=n + 1)[1:]
  small = [i + 1 for i, s in enumerate(sizes) if s < min_area]
  if not small:
    return mask, False
  fill = [0] + small
  if not holes:
    fill = [i for i in range(n + 1) if i not in fill] or [int(np.argmax(sizes)) + 1]
  return np.isin(regions, fill), True


def postprocess_small_regions(masks, min_area, thr):
  """-> (cleaned masks [K,H,W], changed [K], the surviving indices in order)."""
  clean, changed = [], []
  for m in masks.numpy():
    m, c0 = remove_small_regions(m, min_area, True)
    m, c1 = remove_small_regions(m, min_area, False)
    clean.append(torch.from_numpy(m))
    changed.append(int(c0 or c1))
  clean, changed = torch.stack(clean), torch.tensor(changed)
  return clean, changed, nms(mask_boxes(clean), 1. - changed, thr)


def paint(masks):
  """generate_static_mask.py:237-242."""
  order = sorted(range(len(masks)), key=lambda i: int(masks[i].sum()), reverse=True)
  seg = torch.full(masks.shape[1:], -1, dtype=torch.int32)
  for index, i in enumerate(order):
    seg[masks[i]] = index
  return seg, len(masks)
