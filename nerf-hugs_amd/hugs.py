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

Not here: SAM's automatic mask generator, box and mask prompts, the PIL resize, the COLMAP point filtering / K-means that choose the prompts
(:293-343), the visualisation panels.
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


def write_static_mask(path, mask):
  """static_masks/<name>.png as generate_static_mask.py:415-418 writes it: the mask on three channels, 0 / 255."""
  from .internal import utils
  utils.save_img_u8(mask.reshape(*mask.shape[:2], 1).expand(-1, -1, 3), path)
