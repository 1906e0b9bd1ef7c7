"""Image metrics and colour helpers (reference MipNeRF360/internal/image.py).

`MetricHarness` (image.py:127-141) runs on the device: the squared error and dm_pix's SSIM are HIP kernels
(csrc/hugs_image.hip).  sRGB transfer curves (:48-67) and `downsample` (:70-79) are elementwise tensor code;
`color_correct` (:82-124) is the reference's float64 host least squares (`np.linalg.lstsq`), kept as the yardstick;
`color_correct_device` is the same fit on the device in float64 (csrc/hugs_colorcc.hip), which eval.py uses.
`LpipsAlex` is the reference's third metric (metrics.py:30-34,61, nerfacto/eval.py:58-60: LPIPS on AlexNet features) in fp32 on
the device (csrc/hugs_lpips.hip), from weight files the user already has."""
import math

import numpy as np
import torch

from .. import _lib as L


def mse_to_psnr(mse):
  """Compute PSNR given an MSE (we assume the maximum pixel value is 1)."""
  return -10. / math.log(10.) * torch.log(mse)


def psnr_to_mse(psnr):
  return torch.exp(-0.1 * math.log(10.) * psnr)


def ssim_to_dssim(ssim):
  return (1 - ssim) / 2


def dssim_to_ssim(dssim):
  return 1 - 2 * dssim


_EPS = float(np.finfo(np.float32).eps)


def linear_to_srgb(linear, eps=None):
  """Assumes `linear` is in [0, 1], see https://en.wikipedia.org/wiki/SRGB (image.py:48-56)."""
  eps = _EPS if eps is None else eps
  srgb0 = 323 / 25 * linear
  srgb1 = (211 * torch.clamp(linear, min=eps) ** (5 / 12) - 11) / 200
  return torch.where(linear <= 0.0031308, srgb0, srgb1)


def srgb_to_linear(srgb, eps=None):
  """image.py:59-67."""
  eps = _EPS if eps is None else eps
  linear0 = 25 / 323 * srgb
  linear1 = torch.clamp((200 * srgb + 11) / 211, min=eps) ** (12 / 5)
  return torch.where(srgb <= 0.04045, linear0, linear1)


def downsample(img, factor):
  """Area downsample img (factor must evenly divide img height and width) (image.py:70-79)."""
  sh = img.shape
  if not (sh[0] % factor == 0 and sh[1] % factor == 0):
    raise ValueError(f'Downsampling factor {factor} does not evenly divide image shape {tuple(sh[:2])}')
  img = img.reshape((sh[0] // factor, factor, sh[1] // factor, factor) + tuple(sh[2:]))
  return img.mean((1, 3))


def color_correct(img, ref, num_iters=5, eps=0.5 / 255):
  """Warp `img` to match the colors in `ref` (image.py:82-124): per channel a quadratic + linear + bias fit on the
  unsaturated pixels, re-solved num_iters times.  numpy float64 on the host, like eval.py:131-136 feeds it."""
  img = np.asarray(img.detach().cpu() if torch.is_tensor(img) else img, np.float64)
  ref = np.asarray(ref.detach().cpu() if torch.is_tensor(ref) else ref, np.float64)
  if img.shape[-1] != ref.shape[-1]:
    raise ValueError(f'img\'s {img.shape[-1]} and ref\'s {ref.shape[-1]} channels must match')
  nc = img.shape[-1]
  x = img.reshape(-1, nc)
  r = ref.reshape(-1, nc)
  ok = lambda z: (z >= eps) & (z <= 1 - eps)
  mask0 = ok(x)
  for _ in range(num_iters):
    cols = [x[:, c:c + 1] * x[:, c:] for c in range(nc)] + [x, np.ones_like(x[:, :1])]
    a = np.concatenate(cols, -1)
    warp = []
    for c in range(nc):
      m = mask0[:, c] & ok(x[:, c]) & ok(r[:, c])
      w = np.linalg.lstsq(np.where(m[:, None], a, 0), np.where(m, r[:, c], 0), rcond=-1)[0]
      assert np.all(np.isfinite(w))
      warp.append(w)
    x = np.clip(a @ np.stack(warp, -1), 0, 1)
  return x.reshape(img.shape)


def color_correct_device(img, ref, num_iters=5, eps=0.5 / 255):
  """`color_correct` (image.py:82-124) on the device: `img`, `ref` are CUDA tensors [..., nc] (float32 or float64, nc <= 4),
  the result is a float64 CUDA tensor of the same shape.  The fit runs in float64 like the host form (eval.py:121-123
  casts the images up), through fp64-MFMA normal equations and a Jacobi pseudo-inverse (csrc/hugs_colorcc.hip)."""
  if not (torch.is_tensor(img) and img.is_cuda and torch.is_tensor(ref) and ref.is_cuda):
    raise L.HugsError('image.color_correct_device: inputs must be on the GPU (no CPU fallback)')
  if img.shape[-1] != ref.shape[-1]:
    raise ValueError(f'img\'s {img.shape[-1]} and ref\'s {ref.shape[-1]} channels must match')
  if img.shape != ref.shape:
    raise ValueError(f'shape mismatch {tuple(img.shape)} vs {tuple(ref.shape)}')
  nc = img.shape[-1]
  x = img.detach().to(torch.float64).contiguous()
  r = ref.detach().to(torch.float64).contiguous()
  npix = x.numel() // max(nc, 1)
  ws = torch.empty(max(L.call('hugs_color_correct_ws_bytes', npix, nc) // 8, 1), dtype=torch.float64, device=x.device)
  out = torch.empty_like(x)
  L.call('hugs_color_correct', npix, nc, num_iters, eps, x, r, out, ws)
  return out


def _dev_f32(x, device):
  t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
  return t.to(device=device, dtype=torch.float32).contiguous()


def mse(a, b):
  """mean((a - b)^2) as a 0-d device tensor."""
  if not (torch.is_tensor(a) and a.is_cuda):
    raise L.HugsError('image.mse: inputs must be on the GPU (no CPU fallback)')
  if a.shape != b.shape:
    raise ValueError(f'shape mismatch {tuple(a.shape)} vs {tuple(b.shape)}')
  ws = torch.empty(1024, dtype=torch.float32, device=a.device)
  out = torch.empty(1, dtype=torch.float32, device=a.device)
  L.call('hugs_mse', a.numel(), a, b, ws, out)
  return out[0]


def ssim(a, b, max_val=1.0, filter_sigma=1.5, k1=0.01, k2=0.03):
  """dm_pix.ssim(a, b) for [H, W, C] images (filter_size 11), as a 0-d device tensor."""
  if not (torch.is_tensor(a) and a.is_cuda):
    raise L.HugsError('image.ssim: inputs must be on the GPU (no CPU fallback)')
  if a.shape != b.shape or a.dim() != 3:
    raise ValueError(f'ssim takes two [H, W, C] images, got {tuple(a.shape)} and {tuple(b.shape)}')
  h, w, c = a.shape
  nbytes = L.lib().cdll.hugs_ssim_ws_bytes(h, w, c)
  ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=a.device)
  out = torch.empty(1, dtype=torch.float32, device=a.device)
  L.call('hugs_ssim', h, w, c, a, b, max_val, filter_sigma, k1, k2, ws, out)
  return out[0]


# AlexNet `features` as torchvision defines it: (Cin, Cout, kernel), and where the weights sit in the two state dicts
_ALEX = ((3, 64, 11), (64, 192, 5), (192, 384, 3), (384, 256, 3), (256, 256, 3))
_ALEX_KEYS = tuple((f'features.{i}.weight', f'features.{i}.bias') for i in (0, 3, 6, 8, 10))      # torchvision alexnet
_LIN_KEYS = tuple(f'lin{i}.model.1.weight' for i in range(5))                                      # the lpips package's alex.pth


class LpipsAlex:
  """LPIPS with AlexNet features, `LearnedPerceptualImagePatchSimilarity(normalize=True, net_type='alex')` of the
  reference (metrics.py:30-34,61, nerfacto/eval.py:58-60), as fp32 HIP kernels.  `conv_weights` / `conv_biases` /
  `lin_weights` are five tensors each, in torch's [Cout, Cin, kh, kw] / [Cout] / [C] (or [1, C, 1, 1]) shapes; they are
  repacked once into the [kh*kw*Cin][Cout] order the kernels read."""

  def __init__(self, conv_weights, conv_biases, lin_weights, device='cuda'):
    self.device = torch.device(device)
    if not (len(conv_weights) == len(conv_biases) == len(lin_weights) == 5):
      raise ValueError('LpipsAlex takes five conv weights, five biases and five lin vectors')
    parts = []
    for (cin, cout, k), w, b, lin in zip(_ALEX, conv_weights, conv_biases, lin_weights):
      w, b, lin = (torch.as_tensor(t).detach().to('cpu', torch.float32) for t in (w, b, lin))
      if tuple(w.shape) != (cout, cin, k, k) or b.numel() != cout or lin.numel() != cout:
        raise ValueError(f'LpipsAlex: expected a [{cout}, {cin}, {k}, {k}] conv with {cout} biases and lin weights, got '
                         f'{tuple(w.shape)}, {tuple(b.shape)}, {tuple(lin.shape)}')
      w = w.permute(2, 3, 1, 0)                                    # [kh, kw, Cin, Cout]
      if cin == 3:
        w = torch.cat([w, torch.zeros(k, 1, cin, cout)], 1)        # conv1: a twelfth, zero tap per kernel row
      parts += [w.reshape(-1), b.reshape(-1), lin.reshape(-1)]
    self.packed = torch.cat(parts).contiguous().to(self.device)

  @classmethod
  def from_files(cls, alexnet_path, lin_path, device='cuda'):
    """`alexnet_path`: torchvision's AlexNet state dict; `lin_path`: the lpips package's alex.pth.  Local files only."""
    alex = torch.load(alexnet_path, map_location='cpu', weights_only=True)
    lin = torch.load(lin_path, map_location='cpu', weights_only=True)
    for name, sd, keys in (('alexnet', alex, [k for p in _ALEX_KEYS for k in p]), ('lin', lin, list(_LIN_KEYS))):
      missing = [k for k in keys if k not in sd]
      if missing:
        raise ValueError(f'LpipsAlex.from_files: {name} state dict lacks {missing}; keys found: {sorted(sd)}')
    return cls([alex[w] for w, _ in _ALEX_KEYS], [alex[b] for _, b in _ALEX_KEYS], [lin[k] for k in _LIN_KEYS], device)

  def __call__(self, a, b, return_layers=False):
    """[H, W, 3] device tensors in [0, 1] -> LPIPS as a 0-d device tensor; with `return_layers` also the five layer means
    (a [5] tensor) and the five per-pixel distance maps."""
    if not (torch.is_tensor(a) and a.is_cuda and torch.is_tensor(b) and b.is_cuda):
      raise L.HugsError('image.LpipsAlex: inputs must be on the GPU (no CPU fallback)')
    if a.shape != b.shape or a.dim() != 3 or a.shape[-1] != 3:
      raise ValueError(f'LpipsAlex takes two [H, W, 3] images, got {tuple(a.shape)} and {tuple(b.shape)}')
    h, w, _ = a.shape
    a, b = a.detach().to(torch.float32).contiguous(), b.detach().to(torch.float32).contiguous()
    nbytes = L.call('hugs_lpips_alex_ws_bytes', h, w)
    ws = torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=a.device)
    out = torch.empty(6, dtype=torch.float32, device=a.device)
    sizes, hh, ww = [], (h - 7) // 4 + 1, (w - 7) // 4 + 1
    for i in range(5):
      if i in (1, 2):
        hh, ww = (hh - 3) // 2 + 1, (ww - 3) // 2 + 1
      sizes.append((hh, ww))
    maps = None
    if return_layers and nbytes > 0:        # (a refused size: the call below raises before it touches anything)
      maps = torch.empty(sum(y * x for y, x in sizes), dtype=torch.float32, device=a.device)
    L.call('hugs_lpips_alex', h, w, a, b, self.packed, self.packed.numel(), ws, out, maps)
    if not return_layers:
      return out[0]
    return out[0], out[1:], [m.reshape(s) for m, s in zip(maps.split([y * x for y, x in sizes]), sizes)]


class MetricHarness:
  """A helper class for evaluating several error metrics (image.py:127-141); with an `LpipsAlex` also 'lpips'."""

  def __init__(self, device='cuda', lpips=None):
    self.device = torch.device(device)
    self.lpips = lpips

  def __call__(self, rgb_pred, rgb_gt, name_fn=lambda s: s):
    a, b = _dev_f32(rgb_pred, self.device), _dev_f32(rgb_gt, self.device)
    out = {name_fn('psnr'): float(mse_to_psnr(mse(a, b))), name_fn('ssim'): float(ssim(a, b))}
    if self.lpips is not None:
      out[name_fn('lpips')] = float(self.lpips(a, b))
    return out
