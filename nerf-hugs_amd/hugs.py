"""HuGS static masks on the device: HuGS/generate_static_mask.py from the point where SAM has run (csrc/hugs_staticmask.hip).

The caller brings, as device tensors,
  pred, gt  [H,W,3] fp32 in [0,1]: a train view rendered by the partially trained model and its ground truth;
  seg       [H,W] int32: the label map of generate_static_mask.py:239-242 (SamAutomaticMaskGenerator's segments sorted by area
            descending and painted in that order, labels 0..S-1, -1 where no segment covers the pixel);
  and, for the SfM branch, batches of logits [N,H,W] fp32 and iou [N] fp32: predictor.predict_torch(..., return_logits=True)
  for the SfM feature points after the highest-IoU selection of :352-355.
generate_static_mask returns what :269-407 compute; 'static_mask' is the content of static_masks/<name>.png, which
internal/loaders.py reads back for `withmask` training.  Masks are [H,W] fp32 0/1 tensors like the reference's.

SamPointDecoder + SfmAccumulator.add_points run that SfM loop (:344-374) from the image embedding (csrc/hugs_samdecode.hip);
SamImageEncoder computes that embedding from the resized image (:338, csrc/hugs_samencode.hip).

SamMaskGenerator computes `seg` itself: segment_anything's SamAutomaticMaskGenerator around those two (:193-201, :237-242;
csrc/hugs_samamg.hip), with its masks bit-packed on the device in a MaskSet.

select_sfm_prompts / sfm_prompts_from_colmap choose the points add_points takes (:293-336, csrc/hugs_sfmpoints.hip): COLMAP's
observations of the image filtered by track length, delete_same_points, delete_outlier_points, nearest_points.

Not here: box and mask prompts, RLE output, the K-means reduction of the prompts (:319-326: sfm_cluster_num stays disabled, see
select_sfm_prompts), the visualisation panels.  The PIL resize of the generator's crops is host image I/O (a replaceable callable).
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
  sfm_seg_batch_size: int = 128
  sfm_use_highest_iou: bool = True
  sfm_point_count_threshold: int = 5
  sfm_delete_outlier_points: bool = False
  sfm_cluster_num: int = -1
  sfm_points_per_mask: int = 1


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

  def add_lowres(self, lowres, iou, input_size, mask_threshold=0.):
    """:352-374 on the mask decoder's own output: lowres [N,3,256,256] logits and iou [N,3] (SamPointDecoder.predict),
    input_size = (h_in, w_in) of the resized image inside the 1024 square.  The full-resolution logits are never materialised."""
    h, w = self.count.shape
    n = lowres.shape[0]
    if tuple(lowres.shape) != (n, 3, 256, 256) or tuple(iou.shape) != (n, 3):
      raise ValueError(f'lowres must be [N,3,256,256] and iou [N,3], got {tuple(lowres.shape)} and {tuple(iou.shape)}')
    if n == 0:
      return self
    c = self.config
    keep = torch.empty(n if c.sfm_use_highest_iou else 3 * n, dtype=torch.int32, device=self.count.device)
    _lib.call('hugs_sm_sfm_add_lowres', n, h, w, int(input_size[0]), int(input_size[1]), lowres.to(torch.float32).contiguous(),
              iou.to(torch.float32).contiguous(), c.sfm_pred_iou_thresh, mask_threshold, c.sfm_stability_score_offset,
              c.sfm_stability_score_thresh, int(bool(c.sfm_use_highest_iou)), self.count, keep,
              torch.empty(12 * n, dtype=torch.int32, device=self.count.device))
    self.kept.append(keep)
    return self

  def add_points(self, decoder, points, labels=None):
    """:344-374: the SfM feature points [N,P,2] (xy in original pixels) in batches of sfm_seg_batch_size through
    decoder.predict and add_lowres.  decoder: a SamPointDecoder whose set_image has seen this image."""
    if tuple(decoder.original_size) != tuple(self.count.shape):
      raise ValueError(f'the decoder holds an image of {tuple(decoder.original_size)}, the accumulator is {tuple(self.count.shape)}')
    step = int(self.config.sfm_seg_batch_size)
    for i in range(0, points.shape[0], step):
      lowres, iou = decoder.predict(points[i:i + step], None if labels is None else labels[i:i + step])
      self.add_lowres(lowres, iou, decoder.input_size)
    return self

  def mask(self):
    out = torch.empty(self.count.shape, dtype=torch.float32, device=self.count.device)
    _lib.call('hugs_sm_box', *self.count.shape, 1, self.count, None, None, 5, 1, 0, None, out)
    return out


MAX_SFM_POINTS = 65536       # the all-pairs stages (csrc/hugs_sfmpoints.hip)
MAX_NEAREST = 32
_SAME_ROUNDS_PER_READ, _SAME_MAX_ROUNDS = 4, 16


def _sfp_ws(what, n, device):
  size = _lib.call('hugs_sfp_ws_bytes', what, n)
  if size < 0:
    raise ValueError(_lib.lib().cdll.hugs_last_error().decode())
  return torch.empty(size // 4 + 1, dtype=torch.int32, device=device)


def _points(points):
  if points.dim() != 2 or points.shape[-1] != 2:
    raise ValueError(f'points must be [n,2], got {tuple(points.shape)}')
  return points.to(torch.float32).contiguous()


def _kept(n, device):
  return (torch.empty((n, 2), dtype=torch.float32, device=device), torch.empty(n, dtype=torch.int32, device=device),
          torch.zeros(1, dtype=torch.int32, device=device))


def sfm_feature_points(xys, track_len, camera_size, image_size, point_count_threshold=5, device='cuda'):
  """:296-309.  xys [m,2] float64 (COLMAP keypoints in camera pixels), track_len [m] int32 (the length of the keypoint's 3-D point
  track, -1 without a 3-D point), camera_size and image_size (height, width).  Keeps observation i iff the threshold is 0 or
  track_len[i] >= threshold, and returns [n,2] float32 on the device in input order: clip(x * (W / cam_w), 0, W), clip(y * (H /
  cam_h), 0, H) in float64, rounded once -- bit for bit what the reference's numpy + torch.tensor(..., float32) gives."""
  xys = torch.as_tensor(xys, dtype=torch.float64).to(device).contiguous()
  track_len = torch.as_tensor(track_len).to(device, torch.int32).contiguous()
  m = track_len.shape[0]
  if xys.dim() != 2 or tuple(xys.shape) != (m, 2):
    raise ValueError(f'xys must be [m,2] and track_len [m], got {tuple(xys.shape)} and {tuple(track_len.shape)}')
  (cam_h, cam_w), (h, w) = (int(v) for v in camera_size), (int(v) for v in image_size)
  if m == 0:
    return torch.empty((0, 2), dtype=torch.float32, device=xys.device)
  ws = _sfp_ws(0, m, xys.device)
  out, _, count = _kept(m, xys.device)
  # (the binding keeps float64 tensors away from the fp32 kernels; this entry reads doubles, so it gets the same bytes as int64)
  _lib.call('hugs_sfp_filter', m, xys.view(torch.int64), track_len, int(point_count_threshold), cam_h, cam_w, h, w, out, count, ws)
  return out[:int(count)]


def delete_same_points(points, distance_threshold=0.1, stats=None):
  """:81-94, the reference's greedy loop exactly: point 0 is kept and point i is kept iff no kept j < i is closer than the
  threshold (fp32 distances, the threshold rounded to fp32; dropped points suppress nobody).  Returns (the kept points in input
  order, their former indices int32).  The device decides in rounds -- every undecided point whose closer predecessors are all
  decided -- and the host reads the undecided count every few rounds; a dependency chain deeper than 16 rounds is finished by a
  walk in index order.  stats: a dict that receives 'rounds' (rounds run until nothing was undecided) and 'walked' (points left
  to the walk)."""
  points = _points(points)
  n = points.shape[0]
  if n == 0:
    return points, torch.empty(0, dtype=torch.int32, device=points.device)
  ws = _sfp_ws(1, n, points.device)
  rounds, left = 0, n
  while left and rounds < _SAME_MAX_ROUNDS:
    _lib.call('hugs_sfp_same_rounds', n, points, distance_threshold, rounds, _SAME_ROUNDS_PER_READ, ws)
    rounds += _SAME_ROUNDS_PER_READ
    left = int(ws[rounds])
  out, index, count = _kept(n, points.device)
  _lib.call('hugs_sfp_same_finish', n, points, distance_threshold, rounds, out, index, count, ws)
  if stats is not None:
    undecided = ws[:rounds + 1].tolist()
    stats['rounds'] = undecided.index(0) if 0 in undecided else rounds
    stats['walked'] = left
  count = int(count)
  return out[:count], index[:count]


def delete_outlier_points(points, std_coefficient=3.0):
  """:97-107: keeps the points whose distance to the nearest other point is < mean + std_coefficient * std over all n (n - 1)
  pairwise distances (fp32 distances; the moments and the comparison in float64, summed in a fixed order).  Returns (the kept
  points in input order, their former indices int32).  Two points are both dropped, as in the reference (std = 0, d < d is
  false); with fewer than two the reference fails on an empty min, here the input comes back unchanged."""
  points = _points(points)
  n = points.shape[0]
  if n < 2:
    return points, torch.arange(n, dtype=torch.int32, device=points.device)
  out, index, count = _kept(n, points.device)
  _lib.call('hugs_sfp_outliers', n, points, std_coefficient, out, index, count, _sfp_ws(2, n, points.device))
  count = int(count)
  return out[:count], index[:count]


def nearest_points(points, k, return_index=False):
  """:331-333 with input_points = feature_points: [n, min(k, n), 2], each point followed by its nearest others in ascending
  distance (with return_index also their indices [n, min(k, n)] int32).  Equal distances go lower index first -- the reference's
  argsort is unstable there, so its order among exact ties (and whether a duplicate precedes the point itself) is unspecified.
  k <= 32."""
  points = _points(points)
  n, k = points.shape[0], int(k)
  if not 1 <= k <= MAX_NEAREST:
    raise ValueError(f'nearest_points: k = {k} outside 1..{MAX_NEAREST}')
  k = min(k, n)
  out = torch.empty((n, k, 2), dtype=torch.float32, device=points.device)
  index = torch.empty((n, k), dtype=torch.int32, device=points.device)
  if n:
    _lib.call('hugs_sfp_nearest', n, k, points, out, index)
  return (out, index) if return_index else out


def select_sfm_prompts(xys, track_len, camera_size, image_size, config=None, device='cuda'):
  """:293-336 for one image: sfm_feature_points (config.sfm_point_count_threshold), delete_same_points, delete_outlier_points when
  config.sfm_delete_outlier_points, then nearest_points for config.sfm_points_per_mask > 1.  Returns the prompts [N,P,2] float32
  on the device for SfmAccumulator.add_points ([0,1,2] when no point survives the filter).
  sfm_cluster_num: <= 0 or >= the number of points is "disabled" (:319).  0 < sfm_cluster_num < n raises ValueError: at :325 the
  reference assigns the unique cluster INDICES (an argsort over the cluster axis) to input_points, not points, so that path
  cannot produce [n,1,2] prompts, and no shipped config enables it; K-means is not built."""
  config = config if config is not None else SegmentConfig()
  points = sfm_feature_points(xys, track_len, camera_size, image_size, config.sfm_point_count_threshold, device)
  if points.shape[0] == 0:
    return points.reshape(0, 1, 2)
  points, _ = delete_same_points(points)
  if config.sfm_delete_outlier_points:
    points, _ = delete_outlier_points(points)
  if 0 < config.sfm_cluster_num < points.shape[0]:
    raise ValueError(f'sfm_cluster_num = {config.sfm_cluster_num} with {points.shape[0]} points: the reference\'s K-means path '
                     '(generate_static_mask.py:319-326) yields cluster indices instead of points and is not supported; leave it <= 0')
  if config.sfm_points_per_mask > 1 and points.shape[0]:
    return nearest_points(points, config.sfm_points_per_mask)
  return points.unsqueeze(1)


def read_sfm_model(colmap_dir):
  """The parts of a COLMAP sparse model the prompts need, read once for all images: (cameras, images with their 2-D observations,
  track length per 3-D point)."""
  import os
  from .internal import colmap
  return (colmap.read_cameras_binary(os.path.join(colmap_dir, 'cameras.bin')),
          colmap.read_images_points2D(os.path.join(colmap_dir, 'images.bin')),
          colmap.read_points3D_track_lengths(os.path.join(colmap_dir, 'points3D.bin')))


def sfm_observations(model, image_name):
  """Host side of :294-303.  model: a COLMAP directory or read_sfm_model's tuple; image_name: the image file's stem (:212).
  Returns numpy (xys float64 [m,2], track_len int32 [m] with -1 where the keypoint has no 3-D point, (cam_h, cam_w))."""
  import os
  import numpy as np
  cameras, images, tracks = read_sfm_model(model) if isinstance(model, (str, os.PathLike)) else model
  by_stem = {os.path.splitext(os.path.basename(name))[0]: iid for iid, (name, _, _, _) in images.items()}
  if image_name not in by_stem:
    raise ValueError(f'no image with the stem {image_name!r} in the COLMAP model')
  _, camera_id, xys, ids = images[by_stem[image_name]]
  track_len = np.array([tracks[int(p)] if p != -1 else -1 for p in ids], dtype=np.int32).reshape(-1)
  cam = cameras[camera_id]
  return xys, track_len, (int(cam['height']), int(cam['width']))


def sfm_prompts_from_colmap(model, image_name, image_size, config=None, device='cuda'):
  """COLMAP files to prompts: sfm_observations + select_sfm_prompts.  image_size = (H, W) of pred / gt."""
  xys, track_len, camera_size = sfm_observations(model, image_name)
  return select_sfm_prompts(xys, track_len, camera_size, image_size, config, device)


def _sam_keys():
  """The segment_anything checkpoint keys SamPointDecoder reads, in the order the kernels' packed buffer holds them: each entry
  is (key(s), packer); a linear weight [out,in] is stored transposed, [in][out]."""
  pe, md = 'prompt_encoder.', 'mask_decoder.'
  tr = md + 'transformer.'
  flat = lambda t: t.reshape(-1)
  lin_t = lambda t: t.t().reshape(-1)
  cat_t = lambda *ts: torch.cat([t.t() for t in ts], 1).reshape(-1)
  ks = [((pe + 'pe_layer.positional_encoding_gaussian_matrix',), flat)]
  ks += [((k,), flat) for k in (pe + 'point_embeddings.0.weight', pe + 'point_embeddings.1.weight', pe + 'not_a_point_embed.weight',
                                pe + 'no_mask_embed.weight', md + 'iou_token.weight', md + 'mask_tokens.weight')]

  def t2i(a, norm):
    return [((a + 'q_proj.weight',), lin_t), ((a + 'q_proj.bias',), flat), ((a + 'k_proj.weight', a + 'v_proj.weight'), cat_t),
            ((a + 'k_proj.bias', a + 'v_proj.bias'), lambda k, v: torch.cat([k, v])),
            ((a + 'k_proj.weight',), lambda k: torch.cat([k.t(), torch.zeros_like(k.t())], 1).reshape(-1)),      # keys of pos alone
            ((a + 'out_proj.weight',), lin_t), ((a + 'out_proj.bias',), flat), ((norm + '.weight',), flat), ((norm + '.bias',), flat)]

  for i in range(2):
    l = f'{tr}layers.{i}.'
    sa, ia = l + 'self_attn.', l + 'cross_attn_image_to_token.'
    ks += [((sa + 'q_proj.weight', sa + 'k_proj.weight'), cat_t), ((sa + 'q_proj.bias', sa + 'k_proj.bias'), lambda q, k: torch.cat([q, k])),
           ((sa + 'v_proj.weight',), lin_t), ((sa + 'v_proj.bias',), flat), ((sa + 'out_proj.weight',), lin_t), ((sa + 'out_proj.bias',), flat),
           ((l + 'norm1.weight',), flat), ((l + 'norm1.bias',), flat)]
    ks += t2i(l + 'cross_attn_token_to_image.', l + 'norm2')
    ks += [((l + 'mlp.lin1.weight',), lin_t), ((l + 'mlp.lin1.bias',), flat), ((l + 'mlp.lin2.weight',), lin_t), ((l + 'mlp.lin2.bias',), flat),
           ((l + 'norm3.weight',), flat), ((l + 'norm3.bias',), flat)]
    for p in 'qkv':
      ks += [((f'{ia}{p}_proj.weight',), lin_t), ((f'{ia}{p}_proj.bias',), flat)]
    ks += [((ia + 'out_proj.weight',), lin_t), ((ia + 'out_proj.bias',), flat), ((l + 'norm4.weight',), flat), ((l + 'norm4.bias',), flat)]
  ks += t2i(tr + 'final_attn_token_to_image.', tr + 'norm_final_attn')
  up = md + 'output_upscaling.'
  sub = lambda t: t.permute(0, 2, 3, 1).reshape(-1)             # ConvTranspose2d [Cin,Cout,2,2] -> [Cin][sub-pixel][Cout]
  ks += [((up + '0.weight',), sub), ((up + '0.bias',), flat), ((up + '1.weight',), flat), ((up + '1.bias',), flat),
         ((up + '3.weight',), sub), ((up + '3.bias',), flat)]
  hy = [f'{md}output_hypernetworks_mlps.{m}.layers.' for m in range(4)]
  for j in range(3):
    ks += [(tuple(f'{h}{j}.weight' for h in hy), lambda *ts: torch.stack([t.t() for t in ts]).reshape(-1)),
           (tuple(f'{h}{j}.bias' for h in hy), lambda *ts: torch.cat(ts))]
  for j in range(3):
    ks += [((f'{md}iou_prediction_head.layers.{j}.weight',), lin_t), ((f'{md}iou_prediction_head.layers.{j}.bias',), flat)]
  return ks


_ENC_GRID, _ENC_WINDOW = 64, 14


def _sam_enc_config(weights):
  """(D, depth, heads, global flags) read from the image_encoder.* tensors; ValueError naming the key for an unsupported shape."""
  ie = 'image_encoder.'
  nums = [int(k[len(ie) + 7:].split('.')[0]) for k in weights if k.startswith(ie + 'blocks.')]
  depth = max(nums) + 1 if nums else 0
  need = [ie + 'pos_embed'] + [f'{ie}blocks.{i}.attn.rel_pos_{a}' for i in range(depth) for a in 'hw']
  missing = [k for k in need if k not in weights]
  if missing or not depth:
    raise ValueError(f'SamImageEncoder: the weights lack {sorted(missing) or [ie + "blocks.0.*"]}')
  pos = weights[ie + 'pos_embed']
  if pos.dim() != 4 or tuple(pos.shape[:3]) != (1, _ENC_GRID, _ENC_GRID) or pos.shape[-1] % 32:
    raise ValueError(f'SamImageEncoder: {ie}pos_embed must be [1,64,64,D] with D a multiple of 32, got {tuple(pos.shape)}')
  dim, hd = int(pos.shape[-1]), int(weights[ie + 'blocks.0.attn.rel_pos_h'].shape[-1])
  if hd not in (64, 80) or dim % hd:
    raise ValueError(f'SamImageEncoder: {ie}blocks.0.attn.rel_pos_h has head size {hd} (64 or 80, dividing D = {dim})')
  flags = []
  for i in range(depth):
    rows = {a: tuple(weights[f'{ie}blocks.{i}.attn.rel_pos_{a}'].shape) for a in 'hw'}
    for a, shape in rows.items():      # no rel-pos interpolation: the tables have 2 G - 1 rows for G = 64 (global) or 14 (window)
      if shape not in ((2 * _ENC_GRID - 1, hd), (2 * _ENC_WINDOW - 1, hd)) or shape != rows['h']:
        raise ValueError(f'SamImageEncoder: {ie}blocks.{i}.attn.rel_pos_{a} must be [127,{hd}] or [27,{hd}] like rel_pos_h, got {shape}')
    flags.append(int(rows['h'][0] == 2 * _ENC_GRID - 1))
  return dim, depth, dim // hd, flags


def _sam_enc_keys(depth, flags):
  """The image_encoder.* keys SamImageEncoder reads, in the order the kernels' packed buffer holds them (as _sam_keys)."""
  ie = 'image_encoder.'
  flat = lambda t: t.reshape(-1)
  lin_t = lambda t: t.t().reshape(-1)
  conv_t = lambda t: t.permute(2, 3, 1, 0).reshape(-1)      # [out,in,kh,kw] -> [(kh, kw, in)][out]: the loaders' K order
  ks = [((ie + 'patch_embed.proj.weight',), conv_t), ((ie + 'patch_embed.proj.bias',), flat), ((ie + 'pos_embed',), flat)]
  for i in range(depth):
    b = f'{ie}blocks.{i}.'
    width, off = (256, 128) if flags[i] else (64, 32)

    def rel(h, w, width=width, off=off):      # [hd][width]: rel_pos_h^T from column 0, rel_pos_w^T from column off, zeros between
      out = torch.zeros(h.shape[1], width)
      out[:, :h.shape[0]], out[:, off:off + w.shape[0]] = h.t(), w.t()
      return out.reshape(-1)

    ks += [((b + 'norm1.weight',), flat), ((b + 'norm1.bias',), flat), ((b + 'attn.qkv.weight',), lin_t), ((b + 'attn.qkv.bias',), flat),
           ((b + 'attn.rel_pos_h', b + 'attn.rel_pos_w'), rel), ((b + 'attn.proj.weight',), lin_t), ((b + 'attn.proj.bias',), flat),
           ((b + 'norm2.weight',), flat), ((b + 'norm2.bias',), flat), ((b + 'mlp.lin1.weight',), lin_t), ((b + 'mlp.lin1.bias',), flat),
           ((b + 'mlp.lin2.weight',), lin_t), ((b + 'mlp.lin2.bias',), flat)]
  nk = ie + 'neck.'
  ks += [((nk + '0.weight',), conv_t), ((nk + '1.weight',), flat), ((nk + '1.bias',), flat),
         ((nk + '2.weight',), conv_t), ((nk + '3.weight',), flat), ((nk + '3.bias',), flat)]
  return ks


class SamImageEncoder:
  """segment_anything's Sam.preprocess + ImageEncoderViT as fp32 HIP kernels (csrc/hugs_samencode.hip): the
  predictor.set_image(sam_image) of generate_static_mask.py:338 after ResizeLongestSide(1024).apply_image (the PIL resize is
  host image I/O and stays the caller's).  `weights`: a dict of tensors under the checkpoint's key names; width, depth, heads
  and which blocks attend globally are read from the image_encoder.* shapes (vit_b, vit_l and vit_h all qualify)."""

  def __init__(self, weights, device='cuda'):
    import ctypes
    self.dim, self.depth, self.heads, flags = _sam_enc_config(weights)
    keys = _sam_enc_keys(self.depth, flags)
    missing = [k for names, _ in keys for k in names if k not in weights]
    if missing:
      raise ValueError(f'SamImageEncoder: the weights lack {sorted(set(missing))}')
    self.device = torch.device(device)
    self.global_flags = (ctypes.c_int * self.depth)(*flags)      # (a host array: the library reads it while enqueueing)
    self.packed = torch.cat([pack(*(torch.as_tensor(weights[k]).detach().to('cpu', torch.float32) for k in names)).contiguous()
                             for names, pack in keys]).to(self.device)
    size = _lib.call('hugs_sam_enc_ws_bytes', self.dim, self.depth, self.heads)
    if size < 0:
      raise ValueError(_lib.lib().cdll.hugs_last_error().decode())
    self.ws = torch.empty(size // 4, dtype=torch.float32, device=self.device)

  @classmethod
  def from_checkpoint(cls, path, device='cuda'):
    """A segment_anything checkpoint (sam_vit_*.pth), a local file; only the image encoder's keys are read."""
    return cls(torch.load(path, map_location='cpu', weights_only=True), device)

  def encode(self, image):
    """image [h_in, w_in, 3]: RGB in 0..255, uint8 or float32, max(h_in, w_in) <= 1024.  Returns the embedding [256,64,64] fp32."""
    import ctypes
    if image.dim() != 3 or image.shape[-1] != 3 or not 1 <= max(image.shape[:2]) <= 1024:
      raise ValueError(f'image must be [h,w,3] with h, w <= 1024, got {tuple(image.shape)}')
    if image.dtype != torch.uint8:
      image = image.to(torch.float32)
    image = image.to(self.device).contiguous()
    out = torch.empty((256, _ENC_GRID, _ENC_GRID), dtype=torch.float32, device=self.device)
    _lib.call('hugs_sam_enc_encode', self.dim, self.depth, self.heads, self.packed, self.packed.numel(),
              ctypes.addressof(self.global_flags), image, int(image.dtype == torch.uint8), image.shape[0], image.shape[1], self.ws, out)
    return out


class SamPointDecoder:
  """segment_anything's prompt encoder (points only) and mask decoder with multimask output as fp32 HIP kernels
  (csrc/hugs_samdecode.hip): predictor.predict_torch(points, labels, multimask_output=True, return_logits=True) of
  generate_static_mask.py:346-351 up to the low-resolution logits.  set_image takes the ViT image encoder's [256,64,64]
  embedding, from SamImageEncoder.encode (set_image_from does both) or from a stack of the caller's.  `weights`: a dict of tensors
  under the checkpoint's key names (all SAM sizes share this decoder);
  ln_eps: the eps of the transformer's LayerNorms (1e-5 in segment_anything, 1e-6 in the transformers port)."""
  MAX_POINTS = 10

  def __init__(self, weights, device='cuda', ln_eps=1e-5):
    keys = _sam_keys()
    missing = [k for names, _ in keys for k in names if k not in weights]
    if missing:
      raise ValueError(f'SamPointDecoder: the weights lack {sorted(set(missing))}')
    self.device, self.ln_eps = torch.device(device), float(ln_eps)
    self.packed = torch.cat([pack(*(torch.as_tensor(weights[k]).detach().to('cpu', torch.float32) for k in names)).contiguous()
                             for names, pack in keys]).to(self.device)
    self.state = self.original_size = self.input_size = None

  @classmethod
  def from_checkpoint(cls, path, device='cuda', ln_eps=1e-5):
    """A segment_anything checkpoint (sam_vit_*.pth), a local file; only the prompt encoder's and mask decoder's keys are read."""
    return cls(torch.load(path, map_location='cpu', weights_only=True), device, ln_eps)

  def set_image(self, embedding, original_size):
    """embedding: the image encoder's output [256,64,64] (or [1,256,64,64]) for the image resized as ResizeLongestSide(1024)
    does; original_size = (H, W).  Computes everything that depends on the image alone."""
    if embedding.dim() == 4 and embedding.shape[0] == 1:
      embedding = embedding[0]
    if tuple(embedding.shape) != (256, 64, 64):
      raise ValueError(f'embedding must be [256,64,64], got {tuple(embedding.shape)}')
    h, w = (int(v) for v in original_size)
    check_image_size(h, w)
    scale = 1024. / max(h, w)
    self.original_size, self.input_size = (h, w), (int(h * scale + 0.5), int(w * scale + 0.5))
    self.state = torch.empty(_lib.call('hugs_sam_ws_bytes', 0, 1) // 4, dtype=torch.float32, device=self.device)
    _lib.call('hugs_sam_set_image', self.packed, self.packed.numel(), embedding.to(self.device, torch.float32).contiguous(), self.state)
    return self

  def set_image_from(self, encoder, image, original_size):
    """set_image(encoder.encode(image), original_size): encoder a SamImageEncoder, image the resized RGB image [h_in,w_in,3]."""
    return self.set_image(encoder.encode(image), original_size)

  def predict(self, points, labels=None):
    """points [N,P,2]: xy in pixels of the original image; labels [N,P]: 1 foreground (the default), 0 background.
    Returns (lowres [N,3,256,256] logits, iou [N,3])."""
    if self.state is None:
      raise ValueError('SamPointDecoder.predict before set_image')
    if points.dim() != 3 or points.shape[-1] != 2 or not 1 <= points.shape[1] <= self.MAX_POINTS:
      raise ValueError(f'points must be [N,P,2] with 1 <= P <= {self.MAX_POINTS}, got {tuple(points.shape)}')
    n, p = points.shape[:2]
    if labels is None:
      labels = torch.ones((n, p), dtype=torch.int32, device=self.device)
    if tuple(labels.shape) != (n, p):
      raise ValueError(f'labels must be [{n},{p}], got {tuple(labels.shape)}')
    (h, w), (h_in, w_in) = self.original_size, self.input_size
    scale = torch.tensor([w_in / w, h_in / h], dtype=torch.float32, device=self.device)      # apply_coords
    coords = (points.to(self.device, torch.float32) * scale).contiguous()
    lowres = torch.empty((n, 3, 256, 256), dtype=torch.float32, device=self.device)
    iou4 = torch.empty((n, 4), dtype=torch.float32, device=self.device)
    if n:
      ws = torch.empty(_lib.call('hugs_sam_ws_bytes', n, p) // 4, dtype=torch.float32, device=self.device)
      _lib.call('hugs_sam_predict', n, p, coords, labels.to(self.device, torch.int32).contiguous(), self.packed, self.packed.numel(),
                self.ln_eps, self.state, ws, lowres, iou4)
    return lowres, iou4[:, 1:].contiguous()


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


@dataclasses.dataclass
class SamAmgConfig:
  """SamAutomaticMaskGenerator's fields: HuGS's values (generate_static_mask.py:19-36) where HuGS sets them, segment_anything's
  defaults for the rest."""
  points_per_side: int = 64
  pred_iou_thresh: float = 0.8
  stability_score_thresh: float = 0.9
  crop_n_layers: int = 1
  crop_n_points_downscale_factor: int = 2
  min_mask_region_area: int = 50
  points_per_batch: int = 64
  stability_score_offset: float = 1.0
  box_nms_thresh: float = 0.7
  crop_nms_thresh: float = 0.7
  crop_overlap_ratio: float = 512 / 1500


def amg_crop_boxes(size, n_layers=1, overlap_ratio=512 / 1500):
  """segment_anything's generate_crop_boxes for an image of size (H, W): ([x0, y0, x1, y1] per crop, the whole image first,
  and each crop's layer index)."""
  import itertools
  import math
  h, w = (int(v) for v in size)
  boxes, layers = [[0, 0, w, h]], [0]
  for layer in range(int(n_layers)):
    n = 2**(layer + 1)
    overlap = int(overlap_ratio * min(h, w) * (2 / n))
    crop_w, crop_h = (int(math.ceil((overlap * (n - 1) + side) / n)) for side in (w, h))
    xs, ys = ([int((c - overlap) * i) for i in range(n)] for c in (crop_w, crop_h))
    for x0, y0 in itertools.product(xs, ys):
      boxes.append([x0, y0, min(x0 + crop_w, w), min(y0 + crop_h, h)])
      layers.append(layer + 1)
  return boxes, layers


def amg_point_grids(points_per_side=64, n_layers=1, downscale=2):
  """segment_anything's build_all_layer_point_grids: per layer an [n * n, 2] float64 numpy array of (x, y) in [0, 1], row-major."""
  import numpy as np
  grids = []
  for layer in range(int(n_layers) + 1):
    n = int(points_per_side / (downscale**layer))
    offset = 1 / (2 * n)
    side = np.linspace(offset, 1 - offset, n)
    grids.append(np.stack([np.tile(side[None, :], (n, 1)), np.tile(side[:, None], (1, n))], -1).reshape(-1, 2))
  return grids


def _amg_ws(what, height, width, n, device):
  size = _lib.call('hugs_amg_ws_bytes', what, height, width, n)
  if size < 0:
    raise ValueError(_lib.lib().cdll.hugs_last_error().decode())
  return torch.empty(size // 8 + 1, dtype=torch.int64, device=device)


def stable_rank(keys):
  """keys [K] float32 or int32 on the device -> (rank, order) int32: rank[i] = #{j : key_j > key_i or (key_j == key_i and j < i)},
  the stable descending order (the lower index first among equals), and its inverse order[rank[i]] = i."""
  if keys.dim() != 1 or keys.dtype not in (torch.float32, torch.int32):
    raise ValueError(f'keys must be [K] float32 or int32, got {tuple(keys.shape)} {keys.dtype}')
  keys = keys.contiguous()
  rank, order = torch.empty_like(keys, dtype=torch.int32), torch.empty_like(keys, dtype=torch.int32)
  if len(keys):
    _lib.call('hugs_amg_rank', len(keys), keys, int(keys.dtype == torch.int32), rank, order)
  return rank, order


def box_nms(boxes, scores, iou_threshold):
  """torchvision.ops.nms for integer boxes [K,4] (x0, y0, x1, y1 <= 4096) with a stable score order: returns (keep, count), keep
  [K] int32 holding the surviving indices in descending score order in its first `count` (a device int32 [1]) entries."""
  boxes = boxes.to(torch.int32).contiguous()
  k = boxes.shape[0]
  keep, count = torch.empty(k, dtype=torch.int32, device=boxes.device), torch.zeros(1, dtype=torch.int32, device=boxes.device)
  if k:
    _, order = stable_rank(scores)
    _lib.call('hugs_amg_nms', k, boxes, order, iou_threshold, keep, count, _amg_ws(1, 3, 3, k, boxes.device))
  return keep, count


class MaskSet:
  """SamAutomaticMaskGenerator's MaskData on the device.  masks_bits [K,H,ceil(W/64)] int64: bit l of word c of a row is pixel
  64 c + l; boxes [K,4] int32 (x0, y0, x1, y1 with inclusive maxima, batched_mask_to_box); iou, stability [K] float32; area [K]
  int32; points [K,2] float32; crop_boxes [K,4] int32.  The attributes are views of the first `len` rows of growing buffers."""
  FIELDS = {'masks_bits': (torch.int64, None), 'boxes': (torch.int32, 4), 'iou': (torch.float32, 0), 'stability': (torch.float32, 0),
            'area': (torch.int32, 0), 'points': (torch.float32, 2), 'crop_boxes': (torch.int32, 4)}

  def __init__(self, height, width, capacity=0, device='cuda'):
    check_image_size(height, width)
    if max(height, width) > 4096:
      raise ValueError(f'MaskSet: image {height} x {width} has a side over 4096')
    self.height, self.width, self.words, self.device, self.len = int(height), int(width), (int(width) + 63) // 64, torch.device(device), 0
    self._buf = {name: self._new(name, 0) for name in self.FIELDS}
    self.reserve(capacity)

  def _new(self, name, rows):
    dtype, cols = self.FIELDS[name]
    shape = (rows, self.height, self.words) if cols is None else ((rows, cols) if cols else (rows,))
    return torch.zeros(shape, dtype=dtype, device=self.device)

  def __len__(self):
    return self.len

  def __getattr__(self, name):
    if name in MaskSet.FIELDS:
      return self._buf[name][:self.len]
    raise AttributeError(name)

  def reserve(self, rows):
    """Room for `rows` masks; the buffers at least double when they grow."""
    have = self._buf['iou'].shape[0]
    if rows > have:
      for name, old in self._buf.items():
        self._buf[name] = self._new(name, max(rows, 2 * have))
        self._buf[name][:self.len] = old[:self.len]
    return self

  @classmethod
  def from_masks(cls, masks, iou=None, stability=None, points=None, crop_boxes=None):
    """masks: [K,H,W] bool on the device; boxes and areas are computed, the other fields default to zeros (crop_boxes: the image)."""
    if masks.dim() != 3 or masks.dtype != torch.bool:
      raise ValueError(f'masks must be [K,H,W] bool, got {tuple(masks.shape)} {masks.dtype}')
    k, h, w = masks.shape
    self = cls(h, w, k, masks.device)
    self.len = k
    if k:
      _lib.call('hugs_amg_pack', k, h, w, 0, masks.contiguous(), self._buf['masks_bits'])
      _lib.call('hugs_amg_mask_stats', k, h, w, self._buf['masks_bits'], self._buf['boxes'], self._buf['area'])
      self._buf['crop_boxes'][:] = torch.tensor([0, 0, w, h], dtype=torch.int32, device=masks.device)
      for name, value in (('iou', iou), ('stability', stability), ('points', points), ('crop_boxes', crop_boxes)):
        if value is not None:
          self._buf[name][:k] = value.to(masks.device)
    return self

  def to_masks(self):
    out = torch.empty((self.len, self.height, self.width), dtype=torch.bool, device=self.device)
    if self.len:
      _lib.call('hugs_amg_pack', self.len, self.height, self.width, 1, out, self._buf['masks_bits'])
    return out

  def _filter(self, start, keep, count, changed=None, alt=None):
    """MaskData.filter(keep) on rows start..len: row start + j becomes row start + keep[j], taken from alt[name] where changed."""
    k = self.len - start
    for name, buf in self._buf.items():
      src = buf[start:self.len]
      dst = torch.empty_like(src)
      _lib.call('hugs_amg_gather', k, src[0].numel() * src.element_size() // 4, keep, count, changed, src,
                alt.get(name) if alt else None, dst)
      buf[start:self.len] = dst
    self.len = start + int(count)

  def nms(self, scores, iou_threshold, start=0):
    """batched_nms + MaskData.filter on the masks from `start` on (scores [len - start]): the survivors, in descending score
    order (stable), replace them.  Returns their former indices relative to `start`."""
    if self.len == start:
      return torch.empty(0, dtype=torch.int32, device=self.device)
    keep, count = box_nms(self._buf['boxes'][start:self.len], scores, iou_threshold)
    self._filter(start, keep, count)
    return keep[:self.len - start]

  def clean_small_regions(self, min_area, max_bytes=1 << 28):
    """remove_small_regions(mode='holes') then (mode='islands') on every mask.  Returns (a MaskSet of the cleaned masks with their
    boxes and areas, changed [K] int32: 1 where a pass found a region under min_area).  The union-find workspace stays under
    max_bytes by running the masks in chunks."""
    out = MaskSet(self.height, self.width, self.len, self.device)
    out.len = k = self.len
    changed = torch.zeros(k, dtype=torch.int32, device=self.device)
    if k:
      for name in ('iou', 'stability', 'points', 'crop_boxes'):
        out._buf[name][:k] = self._buf[name][:k]
      chunk = max(1, min(k, max_bytes // (8 * (self.height * self.width + 6))))
      _lib.call('hugs_amg_small_regions', k, self.height, self.width, int(min_area), self._buf['masks_bits'], self._buf['boxes'],
                out._buf['masks_bits'], changed, chunk, _amg_ws(2, self.height, self.width, chunk, self.device))
      _lib.call('hugs_amg_mask_stats', k, self.height, self.width, out._buf['masks_bits'], out._buf['boxes'], out._buf['area'])
    return out, changed

  def remove_small_regions(self, min_area, nms_thresh):
    """postprocess_small_regions: clean every mask, NMS on the cleaned boxes with score 1 - changed, and the survivors that
    changed take their cleaned mask, box and area.  Returns the survivors' former indices."""
    if not self.len:
      return torch.empty(0, dtype=torch.int32, device=self.device)
    clean, changed = self.clean_small_regions(min_area)
    keep, count = box_nms(clean.boxes, 1 - changed, nms_thresh)
    self._filter(0, keep, count, changed, {n: clean._buf[n][:self.len] for n in ('masks_bits', 'boxes', 'area')})
    return keep[:self.len]

  def label_map(self):
    """generate_static_mask.py:237-242: (seg [H,W] int32, S): seg = the rank by area (descending, stable) of the smallest mask
    covering the pixel, -1 where none does; the `seg`, `num_segments` of generate_static_mask."""
    seg = torch.empty((self.height, self.width), dtype=torch.int32, device=self.device)
    boxes, area = torch.empty((self.len, 4), dtype=torch.int32, device=self.device), torch.empty(self.len, dtype=torch.int32, device=self.device)
    if self.len:
      _lib.call('hugs_amg_mask_stats', self.len, self.height, self.width, self._buf['masks_bits'], boxes, area)
    _, order = stable_rank(area)
    _lib.call('hugs_amg_paint', self.len, self.height, self.width, self._buf['masks_bits'], boxes, order, seg)
    return seg, self.len


def _pil_resize(image, size):
  """ResizeLongestSide.apply_image's resize: Pillow bilinear to size = (h, w)."""
  import numpy as np
  from PIL import Image
  return np.array(Image.fromarray(image).resize((size[1], size[0]), Image.BILINEAR))


class SamMaskGenerator:
  """segment_anything's SamAutomaticMaskGenerator (binary masks) on a SamImageEncoder and a SamPointDecoder:
  generate_static_mask.py:193-201 and the generate() of :237.  resize(crop [h,w,3] uint8 numpy, (h_in, w_in)) -> [h_in,w_in,3] uint8
  numpy is host image I/O; the default is Pillow's bilinear resize, what ResizeLongestSide.apply_image does."""

  def __init__(self, encoder, decoder, config=None, resize=None):
    self.encoder, self.decoder = encoder, decoder
    self.config = config if config is not None else SamAmgConfig()
    self.resize = resize if resize is not None else _pil_resize

  @classmethod
  def from_checkpoint(cls, path, config=None, device='cuda', resize=None):
    """A segment_anything checkpoint (sam_vit_*.pth), a local file: the encoder and the decoder are built from the one dict."""
    weights = torch.load(path, map_location='cpu', weights_only=True)
    return cls(SamImageEncoder(weights, device), SamPointDecoder(weights, device), config, resize)

  def add_candidates(self, mask_set, lowres, iou, points, crop_box, mask_threshold=0.):
    """_process_batch after the decoder: lowres [N,3,256,256], iou [N,3] (SamPointDecoder.predict for the crop), points [N,2] xy in
    crop pixels, crop_box (x0, y0, x1, y1).  Appends the kept candidates to mask_set in candidate order; returns how many."""
    n = lowres.shape[0]
    if tuple(lowres.shape) != (n, 3, 256, 256) or tuple(iou.shape) != (n, 3) or tuple(points.shape) != (n, 2):
      raise ValueError(f'lowres [N,3,256,256], iou [N,3], points [N,2]: got {tuple(lowres.shape)}, {tuple(iou.shape)}, {tuple(points.shape)}')
    if n == 0:
      return 0
    c, m = self.config, mask_set
    x0, y0, x1, y1 = (int(v) for v in crop_box)
    scale = 1024. / max(y1 - y0, x1 - x0)
    h_in, w_in = int((y1 - y0) * scale + 0.5), int((x1 - x0) * scale + 0.5)
    m.reserve(m.len + 3 * n)
    b, kept = m._buf, torch.zeros(1, dtype=torch.int32, device=m.device)
    _lib.call('hugs_amg_candidates', n, m.height, m.width, x0, y0, x1, y1, h_in, w_in, lowres.to(torch.float32).contiguous(),
              iou.to(torch.float32).contiguous(), points.to(m.device, torch.float32).contiguous(), c.pred_iou_thresh, c.stability_score_thresh,
              c.stability_score_offset, mask_threshold, m.len, b['iou'].shape[0], b['masks_bits'], b['boxes'], b['iou'], b['stability'],
              b['area'], b['points'], b['crop_boxes'], kept, _amg_ws(0, y1 - y0, x1 - x0, n, m.device))
    m.len += int(kept)
    return int(kept)

  def process_crop(self, mask_set, image, crop_box, grid):
    """_process_crop: image [H,W,3] uint8 numpy, grid [P,2] in [0,1] (amg_point_grids).  Appends the crop's masks after its NMS."""
    x0, y0, x1, y1 = crop_box
    crop = image[y0:y1, x0:x1]
    ch, cw = crop.shape[:2]
    scale = 1024. / max(ch, cw)
    resized = self.resize(crop, (int(ch * scale + 0.5), int(cw * scale + 0.5)))
    self.decoder.set_image_from(self.encoder, torch.as_tensor(resized).to(self.decoder.device), (ch, cw))
    points = torch.as_tensor(grid * [[cw, ch]]).to(self.decoder.device, torch.float32)
    start, step = mask_set.len, int(self.config.points_per_batch)
    for i in range(0, len(points), step):
      lowres, iou = self.decoder.predict(points[i:i + step, None, :])
      self.add_candidates(mask_set, lowres, iou, points[i:i + step], crop_box)
    mask_set.nms(mask_set.iou[start:], self.config.box_nms_thresh, start)
    return mask_set

  def generate(self, image):
    """image: the original [H,W,3] uint8 image (numpy or tensor).  Returns the MaskSet of SamAutomaticMaskGenerator.generate, in
    its order; .label_map() of it is the (seg, num_segments) of generate_static_mask."""
    import numpy as np
    image = np.ascontiguousarray(image.cpu().numpy() if isinstance(image, torch.Tensor) else image)
    if image.ndim != 3 or image.shape[-1] != 3 or image.dtype != np.uint8:
      raise ValueError(f'image must be [H,W,3] uint8, got {image.shape} {image.dtype}')
    c = self.config
    boxes, layers = amg_crop_boxes(image.shape[:2], c.crop_n_layers, c.crop_overlap_ratio)
    grids = amg_point_grids(c.points_per_side, c.crop_n_layers, c.crop_n_points_downscale_factor)
    masks = MaskSet(*image.shape[:2], device=self.decoder.device)
    for box, layer in zip(boxes, layers):
      self.process_crop(masks, image, box, grids[layer])
    if len(boxes) > 1 and masks.len:
      cb = masks.crop_boxes
      masks.nms(1. / ((cb[:, 2] - cb[:, 0]) * (cb[:, 3] - cb[:, 1])).to(torch.float32), c.crop_nms_thresh)
    if c.min_mask_region_area > 0:
      masks.remove_small_regions(c.min_mask_region_area, max(c.box_nms_thresh, c.crop_nms_thresh))
    return masks


def write_static_mask(path, mask):
  """static_masks/<name>.png as generate_static_mask.py:415-418 writes it: the mask on three channels, 0 / 255."""
  from .internal import utils
  utils.save_img_u8(mask.reshape(*mask.shape[:2], 1).expand(-1, -1, 3), path)
