"""HuGS static masks on the device: HuGS/generate_static_mask.py from the point where SAM has run (csrc/hugs_staticmask.hip).

The caller brings, as device tensors,
  pred, gt  [H,W,3] fp32 in [0,1]: a train view rendered by the partially trained model and its ground truth;
  seg       [H,W] int32: the label map of generate_static_mask.py:239-242 (SamAutomaticMaskGenerator's segments sorted by area
            descending and painted in that order, labels 0..S-1, -1 where no segment covers the pixel);
  and, for the SfM branch, batches of logits [N,H,W] fp32 and iou [N] fp32: predictor.predict_torch(..., return_logits=True)
  for the SfM feature points after the highest-IoU selection of :352-355.
generate_static_mask returns what :269-407 compute; 'static_mask' is the content of static_masks/<name>.png, which
internal/loaders.py reads back for `withmask` training.  Masks are [H,W] fp32 0/1 tensors like the reference's.

Not here: SAM itself, the COLMAP point filtering / K-means that choose the prompts (:293-343), the visualisation panels.
intersect_threshold is a rational (numerator, denominator): the kernels compare inter * den >= num * area in integers."""
import dataclasses
import fractions

import torch

from . import _lib

MAX_KERNEL = 15


@dataclasses.dataclass
class SegmentConfig:
  """The post-SAM fields of generate_static_mask.py:17-59 with their defaults."""
  sfm_pred_iou_thresh: float = 0.8
  sfm_stability_score_offset: float = 1.0
  sfm_stability_score_thresh: float = 0.92
  residual_quantile_upper: float = 0.95
  smooth_kernel_size: int = 7
  erode_kernel_size: int = 5


def check_image_size(height, width):
  """ValueError unless 3 <= H, W and H * W <= 2^24 (every count is exact in fp32 and int32).  Allocates nothing."""
  _ws_bytes(0, height, width, 0)


def _ws_bytes(what, height, width, n):
  size = _lib.call('hugs_sm_ws_bytes', what, height, width, n)
  if size < 0:
    raise ValueError(_lib.lib().cdll.hugs_last_error().decode())
  return size


def _ws(what, height, width, n, device):
  return torch.empty(_ws_bytes(what, height, width, n) // 4 + 1, dtype=torch.int32, device=device)


def _mask(m):
  """An [H,W] (or [H,W,1]) mask as a contiguous fp32 plane."""
  if m.dim() == 3 and m.shape[-1] == 1:
    m = m[..., 0]
  if m.dim() != 2:
    raise ValueError(f'mask must be [H,W], got {tuple(m.shape)}')
  check_image_size(*m.shape)
  return m.to(torch.float32).contiguous()


def _odd(size, name):
  size = int(size)
  if size < 0 or size > MAX_KERNEL or (size and size % 2 == 0):
    raise ValueError(f'{name} must be 0 or an odd size up to {MAX_KERNEL}, got {size}')
  return max(size, 1)      # 0 disables the stage: a 1 x 1 box is the identity


def residual_masks(pred, gt, quantile_upper=0.95):
  """:269-275.  Returns (residual, mask_base, mask_upper, thresholds) with thresholds = [mean, quantile] on the device."""
  if pred.shape != gt.shape or pred.dim() != 3 or pred.shape[-1] != 3:
    raise ValueError(f'pred and gt must both be [H,W,3], got {tuple(pred.shape)} and {tuple(gt.shape)}')
  h, w = pred.shape[:2]
  ws = _ws(0, h, w, 0, pred.device)
  pred, gt = pred.to(torch.float32).contiguous(), gt.to(torch.float32).contiguous()
  residual, base, upper = (torch.empty((h, w), dtype=torch.float32, device=pred.device) for _ in range(3))
  thr = torch.empty(2, dtype=torch.float32, device=pred.device)
  _lib.call('hugs_sm_residual', h, w, pred, gt, quantile_upper, residual, base, upper, thr, ws)
  return residual, base, upper, thr


def fill_gap(mask, kernel_size=5):
  """:110-125: mask | (box_k(mask) >= 0.5) with reflect padding; an even size is bumped by one like the reference's."""
  kernel_size = int(kernel_size)
  if kernel_size % 2 == 0:
    kernel_size += 1
  mask = _mask(mask)
  out = torch.empty_like(mask)
  _lib.call('hugs_sm_box', *mask.shape, 0, mask, None, None, kernel_size, 1, 0, None, out)
  return out


def smooth(mask, kernel_size=7):
  """:391-397: mask | (box_k(mask) >= 0.5) with zero padding; 0 disables."""
  k = _odd(kernel_size, 'smooth_kernel_size')
  mask = _mask(mask)
  out = torch.empty_like(mask)
  _lib.call('hugs_sm_box', *mask.shape, 0, mask, None, None, k, 0, 0, None, out)
  return out


def erode(mask, kernel_size=5):
  """:400-407: cv2.erode with a k x k rectangle and OpenCV's default border (nothing outside the image erodes); 0 disables."""
  k = _odd(kernel_size, 'erode_kernel_size')
  mask = _mask(mask)
  out = torch.empty_like(mask)
  _lib.call('hugs_sm_box', *mask.shape, 0, mask, None, None, k, 2, 1, None, out)
  return out


class SfmAccumulator:
  """:344-377: add() once per batch of point-prompted SAM masks, mask() = fill_gap(count >= 1, 5).  `count` is the [H,W] int32
  map of kept masks over each pixel; `kept` lists the keep decisions of every batch (device int32 tensors)."""

  def __init__(self, height, width, config=None, device='cuda'):
    check_image_size(height, width)
    self.config = config if config is not None else SegmentConfig()
    self.count = torch.zeros((height, width), dtype=torch.int32, device=device)
    self.kept = []

  def add(self, logits, iou, mask_threshold=0.):
    h, w = self.count.shape
    if logits.dim() != 3 or tuple(logits.shape[1:]) != (h, w) or tuple(iou.shape) != (logits.shape[0],):
      raise ValueError(f'logits must be [N,{h},{w}] and iou [N], got {tuple(logits.shape)} and {tuple(iou.shape)}')
    n = logits.shape[0]
    if n == 0:
      return self
    c = self.config
    keep = torch.empty(n, dtype=torch.int32, device=self.count.device)
    _lib.call('hugs_sm_sfm_add', n, h, w, logits.to(torch.float32).contiguous(), iou.to(torch.float32).contiguous(),
              c.sfm_pred_iou_thresh, mask_threshold, c.sfm_stability_score_offset, c.sfm_stability_score_thresh, self.count, keep,
              _ws(1, h, w, n, self.count.device))
    self.kept.append(keep)
    return self

  def mask(self):
    out = torch.empty(self.count.shape, dtype=torch.float32, device=self.count.device)
    _lib.call('hugs_sm_box', *self.count.shape, 1, self.count, None, None, 5, 1, 0, None, out)
    return out


def label_uncovered(seg, num_segments=None):
  """:243-259: every pixel no segment covers (seg < 0) gets the label num_segments + (smallest linear pixel index of its connected
  component of uncovered pixels; neighbours: up, down, left, right, up-left, down-right).  num_segments defaults to seg.max() + 1
  (a host read; pass it to stay asynchronous)."""
  if seg.dim() != 2:
    raise ValueError(f'seg must be [H,W], got {tuple(seg.shape)}')
  check_image_size(*seg.shape)
  seg = seg.to(torch.int32).contiguous()
  if num_segments is None:
    num_segments = max(int(seg.max()) + 1, 0)
  labels = torch.empty_like(seg)
  _lib.call('hugs_sm_label', *seg.shape, num_segments, seg, labels)
  return labels


def _ratio(threshold):
  if isinstance(threshold, (tuple, list)):
    num, den = (int(v) for v in threshold)
  else:
    f = fractions.Fraction(threshold).limit_denominator(1 << 20)
    num, den = f.numerator, f.denominator
  return num, den


def _select_erode(coarse, labels, num_segments, threshold, k):
  h, w = labels.shape
  tab = _ws(2, h, w, num_segments, labels.device)
  out = torch.empty((h, w), dtype=torch.float32, device=labels.device)
  num, den = _ratio(threshold)
  _lib.call('hugs_sm_label_hist', h, w, num_segments, labels, coarse, tab)
  _lib.call('hugs_sm_select_erode', h, w, labels, tab, num_segments + h * w, num, den, k, out)
  return out


def intersect_masks(coarse_mask, labels, num_segments, intersect_threshold=(1, 2)):
  """:128-145 for fine masks that partition the image, given as the label map of label_uncovered: the union of the labels l
  with #(coarse & l) / #l >= intersect_threshold, compared as integers (num, den); a float is taken as the nearest ratio with
  a denominator up to 2^20, 0.5 exactly)."""
  coarse_mask = _mask(coarse_mask)
  if labels.shape != coarse_mask.shape:
    raise ValueError(f'labels {tuple(labels.shape)} and coarse mask {tuple(coarse_mask.shape)} differ in shape')
  return _select_erode(coarse_mask, labels.to(torch.int32).contiguous(), int(num_segments), intersect_threshold, 1)


def generate_static_mask(pred, gt, seg, sfm=None, config=None, num_segments=None):
  """:239-407 for one image.  sfm: an SfmAccumulator that has seen the image's batches, or None (no SfM points: an all-zero SfM
  mask, :312).  Returns the dict of [H,W] tensors 'residual', 'residual_mask_base', 'residual_mask_upper', 'sfm_mask',
  'sfm_residual_mask' (:386, before the smoothing), 'labels' (int32) and 'static_mask'."""
  config = config if config is not None else SegmentConfig()
  ks, ke = _odd(config.smooth_kernel_size, 'smooth_kernel_size'), _odd(config.erode_kernel_size, 'erode_kernel_size')
  residual, base, upper, _ = residual_masks(pred, gt, config.residual_quantile_upper)
  h, w = residual.shape
  if sfm is not None and tuple(sfm.count.shape) != (h, w):
    raise ValueError(f'the SfM accumulator is {tuple(sfm.count.shape)}, the image {(h, w)}')
  sfm_mask = sfm.mask() if sfm is not None else torch.zeros_like(base)
  combined, smoothed = torch.empty_like(base), torch.empty_like(base)
  _lib.call('hugs_sm_box', h, w, 2, sfm_mask, base, upper, ks, 0, 0, combined, smoothed)
  if num_segments is None:
    num_segments = max(int(seg.max()) + 1, 0)
  labels = label_uncovered(seg, num_segments)
  static = _select_erode(smoothed, labels, num_segments, (1, 2), ke)
  return {'residual': residual, 'residual_mask_base': base, 'residual_mask_upper': upper, 'sfm_mask': sfm_mask,
          'sfm_residual_mask': combined, 'labels': labels, 'static_mask': static}


def write_static_mask(path, mask):
  """static_masks/<name>.png as generate_static_mask.py:415-418 writes it: the mask on three channels, 0 / 255."""
  from .internal import utils
  utils.save_img_u8(mask.reshape(*mask.shape[:2], 1).expand(-1, -1, 3), path)
