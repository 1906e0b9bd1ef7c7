"""A plain PyTorch restatement of segment_anything's Sam.preprocess + ImageEncoderViT (64 x 64 token grid, windows of 14,
decomposed relative-position attention, the 256-channel neck), in the dtype of the weights it is given (the tests run it in
float64 and, for the tolerance, in float32 on the CPU).  A helper for tests/test_gpu_sam_encoder.py, not a test.  Keys are those
of a segment_anything checkpoint.

Pinned once (`python -m tests.sam_encoder_ref`, CPU, float64, D 32, 2 heads, one windowed + one global block, a (683, 1024) uint8
image) against transformers.models.sam.modeling_sam.SamVisionEncoder with the keys mapped (to_transformers):
  max |encode - SamVisionEncoder| = 4.4e-15 with |out| max 5.28.
The same run confirms that the two terms the HIP path can get wrong move the output far more than the GPU test's tolerance
(4 x the float32 error, ~1e-5): zeroing the rel_pos tables moves it by 1.17, masking the pad keys of the windows by 1.08."""
import math

import torch
import torch.nn.functional as F

IE = 'image_encoder.'
GRID, WINDOW = 64, 14
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


def make_weights(D, depth, heads, global_blocks, seed=0):
  """A checkpoint-shaped dict of float32 tensors from a seeded generator: linear / conv weights scaled by 1/sqrt(fan_in), small
  biases, LayerNorm gains near 1, and NON-ZERO rel_pos tables of scale 1/sqrt(hd) (the bias q . r is then of unit scale; the
  checkpoints' zero initialisation would hide the term)."""
  g = torch.Generator().manual_seed(seed)
  rn = lambda *s: torch.randn(*s, generator=g)
  hd = D // heads
  w = {IE + 'pos_embed': rn(1, GRID, GRID, D), IE + 'patch_embed.proj.weight': rn(D, 3, 16, 16) / math.sqrt(768),
       IE + 'patch_embed.proj.bias': 0.1 * rn(D)}

  def lin(name, cin, cout):
    w[name + '.weight'], w[name + '.bias'] = rn(cout, cin) / math.sqrt(cin), 0.1 * rn(cout)

  def norm(name, c):
    w[name + '.weight'], w[name + '.bias'] = 1 + 0.1 * rn(c), 0.1 * rn(c)

  for i in range(depth):
    b = f'{IE}blocks.{i}.'
    side = GRID if i in global_blocks else WINDOW
    norm(b + 'norm1', D), lin(b + 'attn.qkv', D, 3 * D), lin(b + 'attn.proj', D, D), norm(b + 'norm2', D)
    lin(b + 'mlp.lin1', D, 4 * D), lin(b + 'mlp.lin2', 4 * D, D)
    w[b + 'attn.rel_pos_h'], w[b + 'attn.rel_pos_w'] = rn(2 * side - 1, hd) / math.sqrt(hd), rn(2 * side - 1, hd) / math.sqrt(hd)
  w[IE + 'neck.0.weight'] = rn(256, D, 1, 1) / math.sqrt(D)
  norm(IE + 'neck.1', 256)
  w[IE + 'neck.2.weight'] = rn(256, 256, 3, 3) / math.sqrt(9 * 256)
  norm(IE + 'neck.3', 256)
  return w


def attention_core(q, k, v, rel_pos_h, rel_pos_w, G, mask_pad_keys=None):
  """q, k, v [B, heads, G*G, hd] -> softmax((q hd^-1/2) k^T + rel-pos bias of the UNSCALED q) v.  mask_pad_keys: [B, G*G] bool of
  keys to exclude (only the pinning run's what-if uses it)."""
  B, heads, _, hd = q.shape
  ar = torch.arange(G, device=q.device)
  idx = ar[:, None] - ar[None, :] + G - 1
  Rh, Rw = rel_pos_h[idx], rel_pos_w[idx]                    # [G(q), G(k), hd]
  out = torch.empty_like(q)
  step = 1024                                                # query rows per chunk: the global score tensor is never whole
  for r0 in range(0, G * G, step):
    qc = q[:, :, r0:r0 + step]
    s = (qc * hd ** -0.5) @ k.transpose(-1, -2)
    rows = torch.arange(r0, min(r0 + step, G * G), device=q.device)
    rel_h = torch.einsum('bnqc,qkc->bnqk', qc, Rh[rows // G])
    rel_w = torch.einsum('bnqc,qkc->bnqk', qc, Rw[rows % G])
    s = (s.reshape(B, heads, -1, G, G) + rel_h[..., :, None] + rel_w[..., None, :]).reshape(B, heads, -1, G * G)
    if mask_pad_keys is not None:
      s = s.masked_fill(mask_pad_keys[:, None, None, :], float('-inf'))
    out[:, :, r0:r0 + step] = torch.softmax(s, -1) @ v
  return out


def _attention(w, b, y, heads, mask_pad_keys=None):
  """y [B, G, G, D] -> [B, G, G, D]"""
  B, G, _, D = y.shape
  qkv = F.linear(y.reshape(B, G * G, D), w[b + 'attn.qkv.weight'], w[b + 'attn.qkv.bias']).reshape(B, G * G, 3, heads, D // heads)
  q, k, v = qkv.permute(2, 0, 3, 1, 4)                       # each [B, heads, G*G, hd]
  out = attention_core(q, k, v, w[b + 'attn.rel_pos_h'], w[b + 'attn.rel_pos_w'], G, mask_pad_keys)
  return F.linear(out.transpose(1, 2).reshape(B, G, G, D), w[b + 'attn.proj.weight'], w[b + 'attn.proj.bias'])


def preprocess(image, dt):
  """[h, w, 3] in 0..255 -> [1, 3, 1024, 1024]: (x - mean) / std, then zero padding at the bottom and right."""
  x = (image.to(dt) - torch.tensor(MEAN, dtype=dt, device=image.device)) / torch.tensor(STD, dtype=dt, device=image.device)
  h, wd = x.shape[:2]
  return F.pad(x.permute(2, 0, 1)[None], (0, 1024 - wd, 0, 1024 - h))


def encode(w, image, mask_pad_keys=False):
  """image [h, w, 3] RGB in 0..255 (uint8 or float, on the weights' device), max(h, w) <= 1024 -> the embedding [256, 64, 64]."""
  dt = w[IE + 'pos_embed'].dtype
  D = w[IE + 'pos_embed'].shape[-1]
  heads = D // w[IE + 'blocks.0.attn.rel_pos_h'].shape[1]
  x = F.conv2d(preprocess(image, dt), w[IE + 'patch_embed.proj.weight'], w[IE + 'patch_embed.proj.bias'], stride=16)
  x = x.permute(0, 2, 3, 1) + w[IE + 'pos_embed']            # [1, 64, 64, D]
  i = 0
  while f'{IE}blocks.{i}.norm1.weight' in w:
    b = f'{IE}blocks.{i}.'
    y = F.layer_norm(x, (D,), w[b + 'norm1.weight'], w[b + 'norm1.bias'], 1e-6)
    if w[b + 'attn.rel_pos_h'].shape[0] == 2 * GRID - 1:
      y = _attention(w, b, y, heads)
    else:
      nw, side = 5, 5 * WINDOW
      real = F.pad(torch.ones(GRID, GRID, dtype=torch.bool, device=x.device), (0, side - GRID, 0, side - GRID))
      y = F.pad(y, (0, 0, 0, side - GRID, 0, side - GRID))   # zero padding AFTER the norm: a pad token's qkv is the bias
      cut = lambda t: t.reshape(nw, WINDOW, nw, WINDOW, -1).permute(0, 2, 1, 3, 4).reshape(nw * nw, WINDOW, WINDOW, -1)
      pad_keys = ~cut(real[..., None]).reshape(nw * nw, WINDOW * WINDOW) if mask_pad_keys else None
      y = _attention(w, b, cut(y), heads, pad_keys)
      y = y.reshape(nw, nw, WINDOW, WINDOW, D).permute(0, 2, 1, 3, 4).reshape(1, side, side, D)[:, :GRID, :GRID]
    x = x + y
    y = F.layer_norm(x, (D,), w[b + 'norm2.weight'], w[b + 'norm2.bias'], 1e-6)
    x = x + F.linear(F.gelu(F.linear(y, w[b + 'mlp.lin1.weight'], w[b + 'mlp.lin1.bias'])), w[b + 'mlp.lin2.weight'], w[b + 'mlp.lin2.bias'])
    i += 1
  ln2d = lambda t, name: F.layer_norm(t.permute(0, 2, 3, 1), (256,), w[name + '.weight'], w[name + '.bias'], 1e-6).permute(0, 3, 1, 2)
  x = ln2d(F.conv2d(x.permute(0, 3, 1, 2), w[IE + 'neck.0.weight']), IE + 'neck.1')
  return ln2d(F.conv2d(x, w[IE + 'neck.2.weight'], padding=1), IE + 'neck.3')[0]


def to_transformers(w):
  """The same tensors under the names of transformers' SamVisionEncoder."""
  ren = (('blocks.', 'layers.'), ('norm1.', 'layer_norm1.'), ('norm2.', 'layer_norm2.'), ('patch_embed.proj.', 'patch_embed.projection.'),
         ('neck.0.', 'neck.conv1.'), ('neck.1.', 'neck.layer_norm1.'), ('neck.2.', 'neck.conv2.'), ('neck.3.', 'neck.layer_norm2.'))
  out = {}
  for k, v in w.items():
    k = k[len(IE):]
    for a, b in ren:
      k = k.replace(a, b)
    out[k] = v
  return out


def _pin():
  from transformers import SamVisionConfig
  from transformers.models.sam.modeling_sam import SamVisionEncoder
  w = {k: v.double() for k, v in make_weights(32, 2, 2, (1,), 0).items()}
  image = torch.randint(0, 256, (683, 1024, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
  cfg = SamVisionConfig(hidden_size=32, num_hidden_layers=2, num_attention_heads=2, global_attn_indexes=[1], mlp_dim=128)
  enc = SamVisionEncoder(cfg).double().eval()
  enc.load_state_dict(to_transformers(w))
  with torch.no_grad():
    theirs = enc(preprocess(image, torch.float64)).last_hidden_state[0]
  ours = encode(w, image)
  print(f'max |encode - SamVisionEncoder| = {float((ours - theirs).abs().max()):.3e}, |out| max {float(ours.abs().max()):.3g}')
  zero = {k: torch.zeros_like(v) if 'rel_pos' in k else v for k, v in w.items()}
  print(f'zeroed rel_pos tables move the output by {float((encode(zero, image) - ours).abs().max()):.3e}')
  print(f'masked pad keys move the output by {float((encode(w, image, mask_pad_keys=True) - ours).abs().max()):.3e}')


if __name__ == '__main__':
  _pin()
